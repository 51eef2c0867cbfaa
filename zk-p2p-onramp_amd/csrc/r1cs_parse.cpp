// circom .r1cs v1 -> one CSR (r1cs_parse.hpp).  Host-only C++, no HIP: one pass over the constraints
// section, every length checked against the bytes left before it is used.
#include "r1cs_parse.hpp"

#include <cstring>

namespace zkp {

namespace {

const uint8_t R_LE[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                          0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};

uint32_t rd32(const uint8_t* p) {
  uint32_t v;
  std::memcpy(&v, p, 4);
  return v;
}
uint64_t rd64(const uint8_t* p) {
  uint64_t v;
  std::memcpy(&v, p, 8);
  return v;
}

struct Sec {
  const uint8_t* ptr = nullptr;
  uint64_t len = 0;
};

// a 32-byte LE coefficient below 2^256 (< 6 r) as 8 words below r
void reduced_words(const uint8_t* p, uint32_t* out) {
  uint64_t v[4], m[4];
  std::memcpy(v, p, 32);
  std::memcpy(m, R_LE, 32);
  for (;;) {
    bool ge = true;  // v >= r
    for (int i = 3; i >= 0; --i)
      if (v[i] != m[i]) {
        ge = v[i] > m[i];
        break;
      }
    if (!ge) break;
    uint64_t borrow = 0;
    for (int i = 0; i < 4; ++i) {
      const uint64_t d = v[i] - m[i] - borrow;
      borrow = (v[i] < m[i] || (v[i] == m[i] && borrow)) ? 1 : 0;
      v[i] = d;
    }
  }
  std::memcpy(out, v, 32);
}

zkp_status fail(std::string& err, zkp_status s, const std::string& m) {
  err = m;
  return s;
}

}  // namespace

zkp_status parse_r1cs(const uint8_t* buf, size_t len, R1csCsr& out, std::string& err) {
  out = R1csCsr{};
  if (!buf || len < 12 || std::memcmp(buf, "r1cs", 4) != 0) return fail(err, ZKP_ERR_FORMAT, "r1cs: Invalid File format");
  if (rd32(buf + 4) > 1) return fail(err, ZKP_ERR_FORMAT, "r1cs: Version not supported");
  const uint32_t nsec = rd32(buf + 8);
  Sec s1, s2;
  size_t pos = 12;
  for (uint32_t i = 0; i < nsec; ++i) {
    if (len - pos < 12) return fail(err, ZKP_ERR_FORMAT, "r1cs: truncated section header");
    const uint32_t id = rd32(buf + pos);
    const uint64_t sl = rd64(buf + pos + 4);
    pos += 12;
    if (sl > len - pos) return fail(err, ZKP_ERR_FORMAT, "r1cs: truncated section " + std::to_string(id));
    if (id == 1 && !s1.ptr) s1 = Sec{buf + pos, sl};
    if (id == 2 && !s2.ptr) s2 = Sec{buf + pos, sl};
    pos += (size_t)sl;
  }
  if (!s1.ptr || !s2.ptr) return fail(err, ZKP_ERR_FORMAT, "r1cs: missing header or constraints section");
  if (s1.len < 4) return fail(err, ZKP_ERR_FORMAT, "r1cs: truncated header section");
  if (rd32(s1.ptr) != 32) return fail(err, ZKP_ERR_CURVE, "r1cs: curve not supported (need bn128): n8 is not 32");
  if (s1.len != 4 + 32 + 16 + 8 + 4) return fail(err, ZKP_ERR_FORMAT, "r1cs: header section has an invalid size");
  if (std::memcmp(s1.ptr + 4, R_LE, 32) != 0)
    return fail(err, ZKP_ERR_CURVE, "r1cs: curve not supported (need bn128): the prime is not r");
  const uint8_t* h = s1.ptr + 36;
  out.n_wires = rd32(h);
  out.n_pub_out = rd32(h + 4);
  out.n_pub_in = rd32(h + 8);
  out.n_prv_in = rd32(h + 12);
  out.n_labels = rd64(h + 16);
  out.n_constraints = rd32(h + 24);
  if (out.n_wires == 0) return fail(err, ZKP_ERR_FORMAT, "r1cs: no wires");
  if ((uint64_t)out.n_pub_out + out.n_pub_in + 1 > out.n_wires)
    return fail(err, ZKP_ERR_FORMAT, "r1cs: more public signals than wires");
  // a constraint is at least its three term counts, a term 36 bytes: both bound what is allocated
  if ((uint64_t)out.n_constraints > s2.len / 12)
    return fail(err, ZKP_ERR_FORMAT, "r1cs: truncated constraints section");
  if (s2.len / 36 > 0xffffffffull) return fail(err, ZKP_ERR_FORMAT, "r1cs: more than 2^32 - 1 terms");
  out.rowptr.resize((size_t)out.n_constraints * 3 + 1);
  out.col.reserve((size_t)(s2.len / 36));
  out.val.reserve((size_t)(s2.len / 36) * 8);
  const uint8_t* p = s2.ptr;
  uint64_t left = s2.len;
  uint64_t terms = 0;
  out.rowptr[0] = 0;
  for (size_t row = 0; row < (size_t)out.n_constraints * 3; ++row) {
    if (left < 4) return fail(err, ZKP_ERR_FORMAT, "r1cs: truncated constraint " + std::to_string(row / 3));
    const uint32_t n = rd32(p);
    p += 4, left -= 4;
    if ((uint64_t)n > left / 36) return fail(err, ZKP_ERR_FORMAT, "r1cs: truncated constraint " + std::to_string(row / 3));
    terms += n;
    if (terms > 0xffffffffull) return fail(err, ZKP_ERR_FORMAT, "r1cs: more than 2^32 - 1 terms");
    for (uint32_t k = 0; k < n; ++k, p += 36) {
      const uint32_t wire = rd32(p);
      if (wire >= out.n_wires)
        return fail(err, ZKP_ERR_FORMAT, "r1cs: constraint " + std::to_string(row / 3) + " names wire " +
                                             std::to_string(wire) + " of " + std::to_string(out.n_wires));
      out.col.push_back(wire);
      const size_t at = out.val.size();
      out.val.resize(at + 8);
      reduced_words(p + 4, &out.val[at]);
    }
    left -= (uint64_t)n * 36;
    out.rowptr[row + 1] = (uint32_t)terms;
  }
  if (left) return fail(err, ZKP_ERR_FORMAT, "r1cs: constraints section has an invalid size");
  return ZKP_OK;
}

}  // namespace zkp
