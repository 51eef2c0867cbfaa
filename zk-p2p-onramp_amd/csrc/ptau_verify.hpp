// `snarkjs powersoftau verify <ptau>`, the point sections (reference call site
// circuit/scripts/generate_keys_phase1.sh:16; commented out as too slow in
// generate_keys_phase2_groth16.sh:3 and generate_keys_phase2_plonk.sh:3): every point of sections 2-6
// and 12-15 on its curve, every G2 point in the subgroup of order r, the singular points, the powers
// by pair sums, the Lagrange sections against the tau sections (ptau_verify.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "host_ec.hpp"
#include "prover.hpp"

namespace zkp {

// ms of one ptau_verify_sections: device time (HIP events) unless marked host
struct PtauVerifyTimings {
  double total_ms = 0;      // host wall
  double parse_ms = 0;      // host: sections, sizes, singular points
  double upload_ms = 0;     // host wall of the section uploads (they overlap the checks)
  double check_ms = 0;      // k_check_points, every section
  double subgroup_ms = 0;   // k_g2_subgroup, sections 3, 6, 13
  double coeffs_ms = 0;     // k_rlc_coeffs
  double ntt_ms = 0;        // the Lagrange scalars: per level widen, inverse NTT, fold into s
  double plan_ms = 0;       // base conversion + every MsmPlan::build
  double acc_pairs_ms = 0;  // accumulate + finish of the pair sums (129-bit)
  double acc_lag_ms = 0;    // ... of the Lagrange side (129-bit, 2N - 1 points, four vectors)
  double acc_tau_ms = 0;    // ... of the tau side (255-bit, N points, four vectors)
  double fold_ms = 0;       // host: msm_fold of every chunk sum
  double pairing_ms = 0;    // host: the same-ratio checks
  size_t chunks = 0;
  // ptau_verify only (host): every contribution's checks; the first challenge hash (its own thread, beside
  // the rest); the next-challenge hash over the uncompressed sections
  double contributions_ms = 0, first_challenge_ms = 0, next_challenge_ms = 0;
};

// the sections of a ptau with the sizes its power gives (section 7 only present and >= 4 bytes)
struct PtauFile {
  uint32_t power = 0, ceremony_power = 0;
  bool lagrange = false;  // sections 12-15
  Section sec[16];
  size_t N() const { return (size_t)1 << power; }
  static bool is_g2(int id) { return id == 3 || id == 6 || id == 13; }
  size_t points(int id) const { return sec[id].len / (is_g2(id) ? 128 : 64); }
};
// Throws ZkpError on a malformed file (ZKP_ERR_FORMAT naming the section, ZKP_ERR_CURVE); host only.
PtauFile parse_ptau(const uint8_t* ptau, size_t len);

constexpr uint64_t SUBGROUP_NO_BAD = ~uint64_t(0);

// zkey-layout G2 points (128 bytes each, on the curve): *n_bad of them are neither all-zero nor of
// order r; *first_bad: the smallest such index (SUBGROUP_NO_BAD if none)
void g2_subgroup_check(int device, const uint8_t* points, size_t n, uint64_t* n_bad, uint64_t* first_bad);
// the same over n points already in HBM (as uploaded), queued on st: bad[0] += the bad points,
// bad[1] = min(bad[1], base + i) over them (points_bad_reset sets 0 and ~0)
void g2_subgroup_resident(const uint32_t* d_points, size_t n, uint64_t base, unsigned long long* bad, hipStream_t st);

// A = sum_{i < n-1} r_i P_i and B = sum_{i < n-1} r_i P_(i+1), r_i = coefficient first_index + i of
// rlc_coeffs(seed32); zkey-layout points, every one canonical and on its curve (else ZKP_ERR_INVALID_ARG).
// n <= 1: two infinities.
struct PairSums {
  host::Jac<host::Fq> a1 = host::Jac<host::Fq>::inf(), b1 = host::Jac<host::Fq>::inf();
  host::Jac<host::Fq2> a2 = host::Jac<host::Fq2>::inf(), b2 = host::Jac<host::Fq2>::inf();
};
PairSums rlc_pairs(int device, bool g2, const uint8_t* seed32, uint64_t first_index, const uint8_t* points, size_t n);

// The verdict on the point sections of a ptau and its message ("OK", or the first failing check).
// seed32: the coefficient seed (nullptr: 32 bytes from the OS CSPRNG).  Throws ZkpError on a malformed file.
bool ptau_verify_sections(int device, const uint8_t* ptau, size_t len, const uint8_t* seed32, std::string& msg);
PtauVerifyTimings& ptau_verify_timings();  // of the last call on this thread

// `snarkjs powersoftau verify <ptau>`: the contribution chain of section 7 (host, mpc.cpp), the ties of the
// last contribution to the sections, ptau_verify_sections, and the next-challenge hash when power =
// ceremonyPower; verdict and message as above.
bool ptau_verify(int device, const uint8_t* ptau, size_t len, const uint8_t* seed32, std::string& msg);

}  // namespace zkp
