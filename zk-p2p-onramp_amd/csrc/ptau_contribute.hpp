// `snarkjs powersoftau new | contribute | beacon` (reference circuit/scripts/generate_keys_phase1.sh:6,8,10,18).
// The point arithmetic of a contribution runs on the GPU (ptau_contribute.hip, ptau_scale_kernels.hpp;
// DESIGN §8h); the key draw, the record of section 7 and the hashes are host code (mpc.cpp).  The byte-level
// model both must equal is tests/helpers/ptau_model.py (restated from snarkjs 0.4.22, parity unpinned).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "host_ec.hpp"
#include "mpc.hpp"

namespace zkp {

// ms of one ptau_contribute; device time (HIP events) unless marked host
struct PtauContributeTimings {
  double total_ms = 0;            // host wall
  double parse_check_ms = 0;      // host parse + k_check_points
  double challenge_ms = 0;        // host: the challenge answered (first_challenge, or the last record's)
  double key_ms = 0;              // host: the key draw and its G2 points
  double upload_ms = 0;           // host wall of the chunk uploads
  double g1_ms = 0, g2_ms = 0;    // k_scale_powers
  double encode_ms = 0;           // k_encode_points
  double download_ms = 0;         // host wall of the waits for a chunk and the copies into the file
  double partial_hash_ms = 0;     // host, its own thread: Blake2b over the compressed sections
  double next_challenge_ms = 0;   // host, its own thread: Blake2b over the uncompressed sections
  size_t chunks = 0;
};
PtauContributeTimings& ptau_contribute_timings();  // of the last call on this thread

// ZKP_PTAU_CHUNK: points per chunk (default 2^22); a malformed value or one below 1 is a ZKP_ERR_INVALID_ARG
size_t ptau_chunk_points();

// `powersoftau new bn128 <power>`: sections 1-7, every point a generator, no contribution.  Host only.
std::vector<uint8_t> ptau_new(uint32_t power, uint32_t ceremony_power);

// out_i = (first * ratio^i) * P_i over n zkey-layout points (canonical and on the curve, else
// ZKP_ERR_INVALID_ARG); first32 / ratio32: 32-byte LE, reduced mod r here
void points_scale_powers(int device, bool g2, const uint8_t* points, size_t n, const uint8_t* first32,
                         const uint8_t* ratio32, uint8_t* out);

// One contribution drawn from rng (type 0) or the beacon's rng (type 1, with its parameters): the new file.
// name == nullptr: no name is recorded.
std::vector<uint8_t> ptau_contribute(int device, const uint8_t* ptau, size_t len, ChaChaRng& rng, uint32_t type,
                                     const char* name, const uint8_t* beacon, size_t beacon_len,
                                     uint32_t num_iterations_exp);

// ---- host parts (mpc.cpp)

// What draw_key takes from the rng; none of it depends on the challenge.
struct PtauDraw {
  host::U256 prv[3];  // tau, alpha, beta: standard form, nonzero
  host::Affine<host::Fq> g1_s[3], g1_sx[3];
};
PtauDraw ptau_draw(ChaChaRng& rng);

// Section 7 checked as zkp_ptau_verify reads it (ZKP_ERR_FORMAT naming section 7).  -> true and the last
// record's nextChallenge, or false when the file has no contribution (the challenge is then
// ptau_first_challenge(ceremonyPower): 384 * 2^ceremonyPower bytes of hashing).
bool ptau_last_challenge(const uint8_t* sec7, size_t len, uint8_t out[64]);
void ptau_first_challenge(uint32_t ceremony_power, uint8_t out[64]);

constexpr size_t PTAU_RECORD_NEXT_AT = 448 + 768 + 216;  // offset of nextChallenge in a record

// The record of the contribution: points_lem = tauG1, tauG2, alphaG1, betaG1, betaG2 as the new sections hold
// them; partial = the hash after challenge || the new sections compressed.  nextChallenge is left zero (at
// PTAU_RECORD_NEXT_AT); response_hash = partial continued over the key's nine points uncompressed.
std::vector<uint8_t> ptau_record(const PtauDraw& d, const uint8_t challenge[64], const uint8_t points_lem[448],
                                 const Blake2b& partial, uint32_t type, const char* name, const uint8_t* beacon,
                                 size_t beacon_len, uint32_t num_iterations_exp, uint8_t response_hash[64]);

// The same record from the key's nine points themselves, in the zkey layout and uncompressed (768 bytes each,
// the record's order: g1_s, g1_sx per secret, then the three g2_spx): what `import response` has, which never
// sees the secrets.  ptau_record is this over ptau_key_forms.
std::vector<uint8_t> ptau_record_of_key(const uint8_t key_lem[768], const uint8_t key_u[768], const uint8_t points_lem[448],
                                        const Blake2b& partial, uint32_t type, const char* name, const uint8_t* beacon,
                                        size_t beacon_len, uint32_t num_iterations_exp, uint8_t response_hash[64]);
// The key of a draw against a challenge (its three G2 points are made here) in both forms
void ptau_key_forms(const PtauDraw& d, const uint8_t challenge[64], uint8_t key_lem[768], uint8_t key_u[768]);
// A key as a response file holds it -> the zkey layout.  Every point canonical (coordinates below p; infinity
// as 0x40 then zeros) and on its curve, else ZKP_ERR_FORMAT "response: key point <k> ..." (k: 0-5 G1, 6-8 G2)
void ptau_key_from_uncompressed(const uint8_t key_u[768], uint8_t key_lem[768]);
// ptau_last_challenge and the last record's response hash with it (false: no contribution, nothing written)
bool ptau_last_hashes(const uint8_t* sec7, size_t len, uint8_t challenge[64], uint8_t response[64]);

}  // namespace zkp
