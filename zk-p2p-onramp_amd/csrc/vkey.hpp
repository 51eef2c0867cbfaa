// A Groth16 verification key on the host: snarkjs' verification_key.json read by a small strict parser
// of its own, the same key taken from sections 2 and 3 of a .zkey, and the JSON written back
// (`zkey export verificationkey`).  Host code only: tests/test_vkey_parse_sanitized.py links it into a
// stand-alone program under AddressSanitizer.
//
// JSON layout: JSON.stringify(vKey, null, 1) with snarkjs' keys in snarkjs' order (protocol, curve,
// nPublic, vk_alpha_1, vk_beta_2, vk_gamma_2, vk_delta_2, vk_alphabeta_12, IC), points as projective
// decimal strings with the "1" / ["1","0"] tails -- restated from memory, format-unpinned.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "host_pairing.hpp"

namespace zkp {

struct VKey {
  host::Affine<host::Fq> alpha1;
  host::Affine<host::Fq2> beta2, gamma2, delta2;
  std::vector<host::Affine<host::Fq>> ic;  // n_public + 1 points
  uint32_t n_public = 0;
};

// Every failure is a ZkpError: malformed JSON, a missing / repeated / mistyped field, a coordinate >= p,
// a point off its curve or (G2) outside the subgroup, IC length != nPublic + 1, a vk_alphabeta_12 that
// is not e(alpha, beta): ZKP_ERR_FORMAT with a message naming the field; protocol != "groth16":
// ZKP_ERR_PROTOCOL; curve != "bn128": ZKP_ERR_CURVE.
VKey parse_vkey_json(const char* json, size_t len);
// sections 2 and 3 of a key, under the same point checks
VKey vkey_from_zkey(const uint8_t* zkey, size_t len);
// the point checks both loaders run (field names as in the JSON)
void check_vkey(const VKey& vk);
std::string vkey_json(const VKey& vk);

}  // namespace zkp
