// Batched Groth16 verification from a verification key (groth16_verify.hip, pairing_kernels.hpp), and the
// kernel-level pairing entry points.  DESIGN.md §8l.
//
// A batch of proofs is gated per proof on the GPU (coordinates < p, A and C on the curve, B on the twist
// and of order r), then checked by one randomised equation with the 128-bit coefficients r_i of
// rlc_coeffs(seed):
//   FE( prod_i ML(r_i A_i, B_i) * ML(-sum_j s_j IC_j, gamma) * ML(-sum_i r_i C_i, delta) * ML(-(sum_i r_i) alpha, beta) ) == 1
// with s_0 = sum r_i, s_j = sum_i r_i pub_(i,j).  The GPU computes r_i A_i, r_i C_i, the per-proof Miller
// loops and their product; the host the three fixed-Q Miller loops and the one final exponentiation.  A
// failing batch is searched by a binary tree over the per-proof values (failing nodes only).
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <mutex>

#include "../../include/zkp_amd.h"
#include "vkey.hpp"

namespace zkp {

// ms of the calling thread's last Verifier::verify (zkp_verifier_timings)
struct Groth16VerifyTimings {
  double gates_ms = 0;       // upload, coefficients, k_verify_gates
  double scalar_ms = 0;      // k_verify_scale: r_i A_i, r_i C_i
  double miller_ms = 0;      // k_miller_proj
  double product_ms = 0;     // k_f12_product and the copies back
  double host_miller_ms = 0; // s-vector, point sums, the three fixed-Q Miller loops
  double final_exp_ms = 0;   // the batch equation's final exponentiation
  double search_ms = 0;      // the tree search of a failing batch (0 when the batch passes)
  double total_ms = 0;       // host wall of the call
  double node_checks = 0;    // equations evaluated, the batch's own included
};
Groth16VerifyTimings& verify_timings();

class Verifier {
 public:
  Verifier(int device, VKey&& vk);
  ~Verifier();
  uint32_t n_public() const { return vk_.n_public; }
  // valid: n bytes.  A proof whose n_public differs from the key's (or lacks its signals) throws
  // ZKP_ERR_INVALID_ARG; a proof that merely fails gives valid[i] = 0.  seed32 null: OS CSPRNG.
  void verify(const zkp_proof* proofs, size_t n, const uint8_t* seed32, uint8_t* valid, size_t* n_valid);

 private:
  void verify_chunk(const zkp_proof* proofs, size_t n, const uint8_t* seed32, uint64_t first, uint8_t* valid);
  int dev_;
  VKey vk_;
  std::mutex mu_;  // one verify at a time
};

// proofs per device pass: ZKP_VERIFY_CHUNK (default 16384, 64..1048576; malformed: ZKP_ERR_INVALID_ARG)
int verify_chunk_size();

// n Miller loops, one per lane: g1 n x 64, g2 n x 128 bytes standard-form LE (all-zero: infinity, f = 1),
// out n x 384 bytes in zkp_pairing's coefficient order.  The values differ from the host's Miller values by
// Fq2 factors: equal only after final_exponentiation.
void miller_loop_points(int device, const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out);
// product of n Fq12 values (n x 384 bytes); n = 0 gives 1
void fq12_product(int device, const uint8_t* in, size_t n, uint8_t* out384);

}  // namespace zkp
