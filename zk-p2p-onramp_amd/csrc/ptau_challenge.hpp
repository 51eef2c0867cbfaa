// `snarkjs powersoftau export challenge | challenge contribute | import response` (reference
// circuit/scripts/generate_keys_phase1.sh:12-14): the path by which a third party contributes without ever
// holding the ptau file.  The point work runs on the GPU (ptau_challenge.hip, ptau_decompress_kernels.hpp;
// DESIGN §8i) on the streaming of ptau_stream.hpp; the key, the record and the hashes are host code (mpc.cpp).
// The byte-level model all three must equal is tests/helpers/ptau_challenge_model.py (restated from snarkjs
// 0.4.22, parity unpinned).
//
//   challenge file  384 N + 128 bytes: the last response hash (64), then tauG1 (2N - 1), tauG2 (N), alphaTauG1
//                   (N), betaTauG1 (N), betaG2 (1) uncompressed.  Its Blake2b-512 is the challenge.
//   response file   192 N + 864 bytes: the challenge hash (64), the five sections after the contribution
//                   compressed, the contributor's key uncompressed (768).  Its Blake2b-512 is the response hash.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ptau_contribute.hpp"

namespace zkp {

// ms of the last of the three calls on this thread; device time (HIP events) unless marked host
struct PtauChallengeTimings : PtauContributeTimings {
  double decode_ms = 0;                       // k_decode_points
  double decomp_g1_ms = 0, decomp_g2_ms = 0;  // k_decompress_points
};
PtauChallengeTimings& ptau_challenge_timings();

// The challenge file of a ptau.  A truncated file is refused (ZKP_ERR_INVALID_ARG); a file whose sections do
// not hash to the challenge its section 7 implies is ZKP_ERR_FORMAT.
std::vector<uint8_t> ptau_export_challenge(int device, const uint8_t* ptau, size_t len);

// One contribution to a challenge file, drawn from rng: the response file.
std::vector<uint8_t> ptau_challenge_contribute(int device, const uint8_t* challenge, size_t len, ChaChaRng& rng);

// The ptau that follows `ptau` by the contribution of `response` (a type-0 record; name == nullptr: none
// recorded).  The contribution's same-ratio checks are ptau_verify's, not run here.
std::vector<uint8_t> ptau_import_response(int device, const uint8_t* ptau, size_t len, const uint8_t* response,
                                          size_t response_len, const char* name);

constexpr uint64_t POINTS_NO_BAD = ~uint64_t(0);
// n compressed points (G1 32 bytes, G2 64) -> the zkey layout; *n_bad of them are refused (written as zeros),
// *first_bad the smallest such index (POINTS_NO_BAD if none)
void points_decompress(int device, bool g2, const uint8_t* compressed, size_t n, uint8_t* out_lem, uint64_t* n_bad,
                       uint64_t* first_bad);
// n uncompressed points (G1 64 bytes, G2 128) -> the zkey layout, with the same two counts; a point off its
// curve is not refused here (points_check asks that of the result)
void points_from_uncompressed(int device, bool g2, const uint8_t* bytes, size_t n, uint8_t* out_lem, uint64_t* n_bad,
                              uint64_t* first_bad);
// n elements of Fq (32 bytes LE, standard form) or Fq2 (c0 then c1), each coordinate below p (else
// ZKP_ERR_INVALID_ARG) -> a root of each (or zeros) and whether it has one
void field_sqrt(int device, bool fq2, const uint8_t* in, size_t n, uint8_t* out, uint8_t* is_square);

}  // namespace zkp
