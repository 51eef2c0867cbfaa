// A circom .r1cs v1 read straight into ONE CSR over 3 * nConstraints rows for `wtns check`
// (wtns_check.hip): row 3c + m is matrix m (0 A, 1 B, 2 C) of constraint c.  Host only: this header and
// r1cs_parse.cpp include nothing of HIP, so the CPU suite builds them alone with a host compiler and the
// sanitizers and feeds them corrupted files (tools/hosttest/wtns_check_emu.cpp).  No exceptions: a status
// and a message.  (zkey_new.hip keeps its own reader, which builds a vector per linear combination.)
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/zkp_amd.h"

namespace zkp {

struct R1csCsr {
  uint32_t n_wires = 0, n_pub_out = 0, n_pub_in = 0, n_prv_in = 0, n_constraints = 0;
  uint64_t n_labels = 0;
  std::vector<uint32_t> rowptr;  // 3 * n_constraints + 1
  std::vector<uint32_t> col;     // a wire per term, every one < n_wires
  std::vector<uint32_t> val;     // 8 LE words per term: the coefficient in standard form, reduced below r
  uint64_t n_terms() const { return col.size(); }
  uint32_t n_public() const { return n_pub_out + n_pub_in; }
};

// The layout of oracle/binfile.py write_r1cs (sections 1 header and 2 constraints; others are skipped).
// Every length is bounded by the bytes that are there before it is used; allocations are bounded by the
// file's size.  An empty linear combination, a zero coefficient and a repeated wire are legal.
// ZKP_ERR_FORMAT: bad magic / version, a truncated section, a wire index >= nWires, more than 2^32 - 1
// terms, bytes left over in the constraints section.  ZKP_ERR_CURVE: n8 != 32 or a prime other than r.
zkp_status parse_r1cs(const uint8_t* buf, size_t len, R1csCsr& out, std::string& err);

}  // namespace zkp
