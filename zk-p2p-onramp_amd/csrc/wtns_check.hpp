// `wtns check`: does a witness satisfy every constraint of its .r1cs, and if not, which ones fail
// (later snarkjs' `wtns check <circuit.r1cs> <witness.wtns>`, circom_tester's checkConstraints; recalled,
// unpinned: the reference pins snarkjs 0.4.22, which has neither).  The zkey holds A and B only, so this is
// the one place that reads C.  Load: r1cs_parse.cpp's CSR uploaded once, coefficients converted once, rows
// classified by length.  Check: the witness by a plain copy (or a prover's staged slot in place), one
// sparse matrix-vector product in Fr over A, B and C with the comparison, a fail bitmap, its scan.
#pragma once
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>

#include "../../include/zkp_amd.h"
#include "r1cs_parse.hpp"

namespace zkp {

class Prover;

// ms of the calling thread's last wtns_check / WitnessChecker call (zkp_wtns_check_timings)
struct CheckTimings {
  double parse_ms = 0;    // r1cs -> CSR and the row classification (host)
  double upload_ms = 0;   // CSR upload + coefficient conversion
  double copy_ms = 0;     // witness host -> device (0 for a staged check)
  double kernel_ms = 0;   // witness scan, both constraint kernels, the bitmap's scan, the result's copy back
  double total_ms = 0;    // host wall of the call
};
CheckTimings& check_timings();

class WitnessChecker {
 public:
  // csr from parse_r1cs_or_throw (a malformed r1cs fails there, before any device work)
  WitnessChecker(int device, R1csCsr&& csr, double parse_ms);
  ~WitnessChecker();
  // a .wtns file: ZKP_ERR_FORMAT / _CURVE (parse_wtns), ZKP_ERR_WITNESS_LENGTH as the prover words it
  void check(const uint8_t* wtns, size_t len, zkp_check_result* res, std::string& msg);
  // the witness zkp_witness_stage left in a prover's slot, read in place
  void check_staged(Prover& p, int dev_index, int slot, zkp_check_result* res, std::string& msg);
  uint32_t n_wires() const { return n_wires_; }
  uint32_t n_public() const { return n_public_; }
  uint32_t n_constraints() const { return n_constraints_; }
  uint64_t n_terms() const { return n_terms_; }
  uint32_t n_long() const { return n_long_; }        // constraints on the wavefront-per-constraint kernel
  uint32_t long_terms() const { return long_terms_; }  // the term count they start at (0: none)
  int device() const { return dev_; }

 private:
  struct Dev;  // the HIP side (wtns_check.hip)
  void run(const uint32_t* d_wit, bool copied, zkp_check_result* res, std::string& msg);
  int dev_;
  uint32_t n_wires_ = 0, n_public_ = 0, n_constraints_ = 0, n_long_ = 0, long_terms_ = 0;
  uint64_t n_terms_ = 0;
  std::unique_ptr<Dev> d_;
  std::mutex mu_;  // one check at a time
};

// parse_r1cs with its status as a ZkpError; *parse_ms (nullable) receives the host time
R1csCsr parse_r1cs_or_throw(const uint8_t* r1cs, size_t len, double* parse_ms);

// header checks of a witness against a parsed r1cs, before any device work (the one-shot zkp_wtns_check)
void check_wtns_header(const R1csCsr& csr, const uint8_t* wtns, size_t len);

// total terms (A + B + C) from which a constraint takes the wavefront-per-constraint kernel;
// ZKP_WTNS_CHECK_LONG=<terms> at load overrides it (0: every constraint on the short path)
uint32_t check_long_terms();

}  // namespace zkp
