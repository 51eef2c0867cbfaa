// `snarkjs zkey export bellman | zkey bellman contribute | zkey import bellman`: the path by which a third party
// contributes to phase 2 without ever holding the .zkey, over an `MPCParams` file that the Rust phase2 tools also
// read.  The point work runs on the GPU (zkey_bellman.hip) on the streaming of ptau_stream.hpp and the
// group FFT of gfft_kernels.hpp; the file layout, the contribution draw and the records are host code (mpc.cpp).
// The byte-level model all three must equal is tests/helpers/bellman_model.py (restated from snarkjs 0.4.22,
// parity unpinned: no snarkjs-written MPCParams file exists here).
//
// MPCParams: every integer a big-endian u32, every point "uncompressed" (big-endian standard form, x then y, G2
// with c1 before c0, infinity as 0x40 then zeros):
//
//   alpha1 | beta1 | beta2 | gamma2 | delta1 | delta2          G1 G1 G2 G2 G1 G2: 576 bytes
//   u32 nPublic + 1        | IC                                section 3
//   u32 n - 1              | B_0 .. B_(n-2)                    B_i = delta^-1 tau^i (tau^n - 1) G1, from section 9
//   u32 nVars - nPublic - 1| L                                 section 8
//   u32 nVars              | A                                 section 5
//   u32 nVars              | B1                                section 6
//   u32 nVars              | B2 (G2)                           section 7
//   csHash (64)
//   u32 nContributions     | deltaAfter | g1_s | g1_sx | g2_spx | transcript(64)     384 bytes each
//
// Up to csHash this is the byte string whose Blake2b-512 `zkey new` records as csHash.
//
// The H section.  With n = 2^p the key's domain, w = Fr.w[p], w2 = Fr.w[p + 1] and x_j = w2^(2j + 1), section 9
// holds H_j = delta^-1 L^(2n)_(2j+1)(tau) G1, the Lagrange points of the 2n-domain at its odd nodes.  x^i Z(x)
// vanishes at the even nodes and is -2 x_j^i at the odd ones, so
//
//   export:  B_i  = -2 w2^i sum_j w^(ij) H_j,   i < n - 1     forward group FFT, then point i times -2 w2^i
//   import:  H'_j = n^-1 sum_i w^(-ij) (-1/2 w2^-i) B_i       B_(n-1) := infinity; scaling, then the inverse FFT
//
// H' differs from the H a direct `zkey contribute` writes by a multiple of (w^j)_j, the direction of the missing
// B_(n-1); no prover sees it (deg h <= n - 2), and zkey_verify's H check leaves that direction out.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mpc.hpp"

namespace zkp {

constexpr size_t MPCPARAMS_HEADER = 576, MPCPARAMS_CONTRIBUTION = 384;

// An MPCParams file's layout (no copies: points into the caller's buffer)
struct MpcParamsFile {
  uint32_t n_public = 0, domain_size = 0, log_domain = 0, n_vars = 0, n_contributions = 0;
  size_t n_ic = 0, n_h = 0, n_l = 0;
  const uint8_t* header = nullptr;  // alpha1 beta1 beta2 gamma2 delta1 delta2
  const uint8_t *ic = nullptr, *h = nullptr, *l = nullptr, *a = nullptr, *b1 = nullptr, *b2 = nullptr;
  const uint8_t* cs_hash = nullptr;
  const uint8_t* contributions = nullptr;
};
constexpr size_t MPCPARAMS_DELTA1_AT = 64 + 64 + 128 + 128, MPCPARAMS_DELTA2_AT = MPCPARAMS_DELTA1_AT + 64;

// Parses and validates the layout: the counts against the length, n - 1 = 2^p - 1 with p <= 27, the counts of
// L, A, B1, B2 and IC against each other, no trailing bytes.  ZKP_ERR_FORMAT "mpcparams: ..." otherwise.
MpcParamsFile mpcparams_parse(const uint8_t* buf, size_t len);

// ---- host parts (mpc.cpp)
// a key's six header points as the file holds them
void mpcparams_header(const host::Affine<host::Fq>& alpha1, const host::Affine<host::Fq>& beta1,
                      const host::Affine<host::Fq2>& beta2, const host::Affine<host::Fq2>& gamma2,
                      const host::Affine<host::Fq>& delta1, const host::Affine<host::Fq2>& delta2,
                      uint8_t out[MPCPARAMS_HEADER]);
void mpcparams_put_contribution(const MpcContribution& c, uint8_t out[MPCPARAMS_CONTRIBUTION]);
// canonical and on its curve, else ZKP_ERR_FORMAT "mpcparams: <what> is not on the curve"
host::Affine<host::Fq> mpcparams_g1(const uint8_t in[64], const std::string& what);
host::Affine<host::Fq2> mpcparams_g2(const uint8_t in[128], const std::string& what);
// the file's csHash and contributions (type 0, no parameters: the file holds neither)
MpcParams mpcparams_read_mpc(const MpcParamsFile& f);
// k * P on the host
host::Affine<host::Fq2> mpc_g2_times(const host::Affine<host::Fq2>& p, const uint8_t k32[32]);

// ms of the last of the three commands on this thread; device time (HIP events) unless marked host
struct BellmanTimings {
  double total_ms = 0;      // host wall
  double parse_ms = 0;      // host: parsing, the header and record work, the compares
  double upload_ms = 0;     // host wall of the chunk uploads
  double decode_ms = 0;     // k_decode_points
  double check_ms = 0;      // k_check_points
  double scale_ms = 0;      // k_scale_powers by the contribution's k^-1 (bellman contribute)
  double transform_ms = 0;  // the group FFT (export) or inverse FFT (import) of the H section
  double coset_ms = 0;      // k_scale_powers by -2 w2^i (export) or -1/2 w2^-i (import)
  double encode_ms = 0;     // k_encode_points
  double download_ms = 0;   // host wall of the waits for a chunk and the copies into the file
  size_t chunks = 0;
};
BellmanTimings& zkey_bellman_timings();

std::vector<uint8_t> zkey_export_bellman(int device, const uint8_t* zkey, size_t len);
// One contribution drawn from rng as zkey contribute draws it; hash64 (if not null): the contribution hash
std::vector<uint8_t> zkey_bellman_contribute(int device, const uint8_t* challenge, size_t len, ChaChaRng& rng,
                                             uint8_t* hash64);
// The key that follows old_zkey by the contribution of `response` (a type-0 record; name == nullptr: none
// recorded).  The contribution's same-ratio checks are zkey_verify's, not run here.
std::vector<uint8_t> zkey_import_bellman(int device, const uint8_t* old_zkey, size_t len, const uint8_t* response,
                                         size_t response_len, const char* name);

}  // namespace zkp
