// `snarkjs zkey verify` (reference gate: circuit/scripts/generate_keys_phase2_groth16.sh:26,
// circuit/server-scripts/generate_keys_phase2_groth16.sh:56, generate_chunked_keys_phase2_groth16.sh:68,
// zk-email-verify-circuits/scripts/compile.js:109), restated from oracle/mpc.py zkey_verify: the
// transcript chain, header, csHash and section compares on the host (mpc.cpp), the two random linear
// combinations over the L (8) and H (9) sections of the key and of the initial key on the GPU
// (zkey_verify.hip).
//
// The linear combinations: with coefficients r_i, S_old = sum r_i old_i and S_new = sum r_i new_i must
// satisfy e(S_old, delta2_key) = e(S_new, delta2_init).  The verifier draws the r_i, so they are
// uniform 128-bit values: a section that is not the initial one times delta_init / delta passes with
// probability <= 2^-128, and the MSM runs ceil(129 / c) windows instead of ceil(255 / c).
//
// The H check.  A key that `zkey import bellman` wrote (zkey_bellman.hpp) carries an H section that differs from
// the one a direct contribution writes by a multiple of (w^j)_j, n = 2^p the domain and w = Fr.w[p]: the
// direction of the point B_(n-1) that an MPCParams file does not hold, and one that no prover's sum
// sum_j q(x_j) H_j (q = h Z, deg h <= n - 2) has a component in.  snarkjs accepts such a key.  So the H
// combination keeps the stream's r_j for points 0..n-2 and gives point n - 1 the coefficient
//   r'_(n-1) = -w sum_(j < n-1) r_j w^j  (mod r),
// which puts the coefficient vector on the hyperplane sum_j r_j w^j = 0, where the combination does not see
// that direction.  The sum is a device reduction over the coefficient chunks (k_rlc_power_sum, each chunk with
// its offset w^start); the one full-width coefficient is kept out of the 128-bit plan and taken by two host
// scalar multiplications.  A wrong H section still passes with probability <= 2^-128 unless it differs from
// the right one by a multiple of (w^j)_j.  The L check is unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "host_ec.hpp"

namespace zkp {

// device ms (HIP events) and host ms of the stages of the linear combinations, summed over chunks
struct RlcTimings {
  double upload_ms = 0;  // host wall of the chunk uploads (they overlap the previous chunk's compute)
  double check_ms = 0;   // k_check_points, both point sets
  double coeffs_ms = 0;  // k_rlc_coeffs
  double plan_ms = 0;    // base conversion + MsmPlan::build
  double acc_ms[2] = {0, 0};  // accumulate + finish per base set
  double fold_ms = 0;    // host msm_fold of both sums
  double total_ms = 0;   // host wall of the whole call
  size_t chunks = 0;
  void add(const RlcTimings& o) {
    upload_ms += o.upload_ms, check_ms += o.check_ms, coeffs_ms += o.coeffs_ms, plan_ms += o.plan_ms;
    acc_ms[0] += o.acc_ms[0], acc_ms[1] += o.acc_ms[1], fold_ms += o.fold_ms, total_ms += o.total_ms;
    chunks += o.chunks;
  }
};

constexpr uint64_t RLC_NO_BAD = ~uint64_t(0);

// sum_i r_(first_index + i) * a_i and the same over b_i.  A point that is not canonical, or neither
// all-zero nor on the curve, stops the run at its chunk: first_bad_* is then the smallest such index
// of that set (RLC_NO_BAD otherwise) and the sums are not to be used.
struct RlcResult {
  host::Jac<host::Fq> sum_a = host::Jac<host::Fq>::inf(), sum_b = host::Jac<host::Fq>::inf();
  uint64_t first_bad_a = RLC_NO_BAD, first_bad_b = RLC_NO_BAD;
  RlcTimings t;
};

// ZKP_VERIFY_CHUNK: points per chunk of the linear combinations (default 2^22, as scale_section);
// a malformed value or one below 1 is a ZKP_ERR_INVALID_ARG
size_t verify_chunk_points();

// coefficient i = the 128-bit LE integer of words 4i..4i+3 of ChaChaRng(seed_from_hash(seed32));
// out: n x 16 bytes LE (generated on the device)
void rlc_coeffs(int device, const uint8_t* seed32, uint64_t first_index, size_t n, uint8_t* out);
// coefficients first_index .. first_index + n - 1 as 8-word scalars (upper four words zero) into d_out
// (device, n x 8 words), queued on st
void rlc_coeffs_resident(const uint8_t* seed32, uint64_t first_index, size_t n, uint32_t* d_out, hipStream_t st);
// window bits of a depth-1 plan over n uniform 128-bit scalars (scalar_bits = 129)
int rlc_window_bits(size_t n);
// zkey-layout points (G1 64 bytes, G2 128): *n_bad of them are not canonical (a coordinate >= p) or
// neither all-zero nor on the curve; *first_bad: the smallest such index (RLC_NO_BAD if none)
void points_check(int device, bool g2, const uint8_t* points, size_t n, uint64_t* n_bad, uint64_t* first_bad);
// the same check of n points already in HBM (as uploaded, zkey layout), queued on st: bad[0] += the bad
// points, bad[1] = min(bad[1], base + i) over them (two device words; points_bad_reset sets 0 and ~0)
void points_bad_reset(unsigned long long* bad, hipStream_t st);
void points_check_resident(bool g2, const uint32_t* d_points, size_t n, uint64_t base, unsigned long long* bad,
                           hipStream_t st);
// on_hyperplane (n = 2^p, w = Fr.w[p]): points 0..n-2 keep the stream's coefficients r_j and point n - 1 takes
// r' = -w sum_(j < n-1) r_j w^j mod r, so that sum_j r_j w^j = 0 (the H check below)
RlcResult rlc_g1(int device, const uint8_t* seed32, uint64_t first_index, const uint8_t* a, const uint8_t* b, size_t n,
                 bool on_hyperplane = false);

// timings of one zkey_verify_frominit (ms)
struct VerifyTimings {
  double host_ms = 0;     // parsing, transcript chain, pairings
  double compare_ms = 0;  // sections 3-7 against the initial key's
  RlcTimings rlc;         // L and H together
  double total_ms = 0;
};

// The verdict of `zkey verify` of `key` against `init` (the key `zkey new` writes for the same circuit
// and ptau) and its message ("OK", or the first failing check in oracle/mpc.py's words).  seed32: the
// coefficient seed (nullptr: 32 bytes from the OS CSPRNG).  Throws ZkpError on malformed input.
bool zkey_verify_frominit(int device, const uint8_t* init, size_t init_len, const uint8_t* key, size_t key_len,
                          const uint8_t* seed32, std::string& msg, VerifyTimings* timings = nullptr);

}  // namespace zkp
