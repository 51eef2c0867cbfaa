// Verification key: strict JSON reader, zkey sections 2 / 3, JSON writer (vkey.hpp).
#include "vkey.hpp"

#include <utility>

#include "prover.hpp"

namespace zkp {

namespace {

using host::Affine;
using host::Fq;
using host::Fq2;
using host::U256;

[[noreturn]] void bad(const std::string& m) { throw ZkpError(ZKP_ERR_FORMAT, "vkey: " + m); }

// ---------------------------------------------------------------- a small strict JSON reader
// RFC 8259 values restricted to what a verification key holds: objects, arrays, strings without escapes,
// non-negative integers.  Nesting is bounded, nothing may follow the top value, a repeated key is an error.
struct Val {
  enum Kind { STR, NUM, ARR, OBJ } kind = STR;
  std::string str;
  uint64_t num = 0;
  std::vector<Val> arr;
  std::vector<std::pair<std::string, Val>> obj;
  const Val* find(const std::string& k) const {
    for (const auto& e : obj)
      if (e.first == k) return &e.second;
    return nullptr;
  }
};

class Reader {
 public:
  Reader(const char* p, size_t n) : p_(p), n_(n) {}
  Val top() {
    Val v = value(0);
    ws();
    if (at_ != n_) bad("bytes after the JSON value");
    return v;
  }

 private:
  static constexpr int MAX_DEPTH = 6;  // the key's deepest value, vk_alphabeta_12, sits at depth 4
  void ws() {
    while (at_ < n_ && (p_[at_] == ' ' || p_[at_] == '\n' || p_[at_] == '\r' || p_[at_] == '\t')) ++at_;
  }
  char peek() {
    if (at_ >= n_) bad("truncated JSON");
    return p_[at_];
  }
  void expect(char c) {
    if (peek() != c) bad(std::string("expected '") + c + "' at byte " + std::to_string(at_));
    ++at_;
  }
  std::string string() {
    expect('"');
    const size_t s = at_;
    for (;;) {
      const unsigned char c = (unsigned char)peek();
      if (c == '"') break;
      if (c == '\\' || c < 0x20 || c >= 0x7f) bad("string with an escape or a non-ASCII byte at " + std::to_string(at_));
      ++at_;
      if (at_ - s > 256) bad("string longer than 256 bytes");
    }
    std::string r(p_ + s, at_ - s);
    ++at_;
    return r;
  }
  Val value(int depth) {
    if (depth > MAX_DEPTH) bad("nested too deeply");
    ws();
    Val v;
    const char c = peek();
    if (c == '"') {
      v.kind = Val::STR;
      v.str = string();
    } else if (c >= '0' && c <= '9') {
      v.kind = Val::NUM;
      const size_t s = at_;
      while (at_ < n_ && p_[at_] >= '0' && p_[at_] <= '9') {
        if (at_ - s >= 9) bad("number too large");
        v.num = v.num * 10 + (uint64_t)(p_[at_] - '0');
        ++at_;
      }
      if (at_ - s > 1 && p_[s] == '0') bad("number with a leading zero");
    } else if (c == '[') {
      v.kind = Val::ARR;
      ++at_;
      ws();
      if (peek() == ']') {
        ++at_;
        return v;
      }
      for (;;) {
        v.arr.push_back(value(depth + 1));
        if (v.arr.size() > (1u << 20)) bad("array too long");
        ws();
        if (peek() == ',') {
          ++at_;
          continue;
        }
        expect(']');
        break;
      }
    } else if (c == '{') {
      v.kind = Val::OBJ;
      ++at_;
      ws();
      if (peek() == '}') {
        ++at_;
        return v;
      }
      for (;;) {
        ws();
        std::string k = string();
        if (v.find(k)) bad("repeated key " + k);
        ws();
        expect(':');
        Val e = value(depth + 1);
        v.obj.emplace_back(std::move(k), std::move(e));
        if (v.obj.size() > 64) bad("object with too many keys");
        ws();
        if (peek() == ',') {
          ++at_;
          continue;
        }
        expect('}');
        break;
      }
    } else {
      bad("unexpected byte at " + std::to_string(at_));
    }
    return v;
  }
  const char* p_;
  size_t n_, at_ = 0;
};

// ---------------------------------------------------------------- fields
// canonical decimal (no sign, no leading zero but "0" itself) below 2^256
U256 dec_u256(const Val& v, const std::string& field) {
  if (v.kind != Val::STR) bad(field + ": coordinate is not a string");
  const std::string& s = v.str;
  if (s.empty() || s.size() > 78 || (s.size() > 1 && s[0] == '0')) bad(field + ": not a canonical decimal");
  U256 r{{0, 0, 0, 0}};
  for (char c : s) {
    if (c < '0' || c > '9') bad(field + ": not a canonical decimal");
    host::u128 carry = (host::u128)(c - '0');
    for (int i = 0; i < 4; ++i) {
      const host::u128 t = (host::u128)r.w[i] * 10 + carry;
      r.w[i] = (uint64_t)t;
      carry = t >> 64;
    }
    if (carry) bad(field + ": coordinate >= p");
  }
  return r;
}
Fq coord(const Val& v, const std::string& field) {
  const U256 x = dec_u256(v, field);
  if (host::u256_geq(x, host::FQ_DESC.mod)) bad(field + ": coordinate >= p");
  return Fq::from_std(x);
}
bool is_dec(const Val& v, const char* want) { return v.kind == Val::STR && v.str == want; }

// [x, y, "1"], or the point at infinity ["0", "1", "0"]
Affine<Fq> g1_field(const Val& v, const std::string& field) {
  if (v.kind != Val::ARR || v.arr.size() != 3) bad(field + ": not a projective G1 point of three coordinates");
  const Fq x = coord(v.arr[0], field), y = coord(v.arr[1], field);
  if (is_dec(v.arr[2], "0") && x.is_zero()) return Affine<Fq>{Fq::zero(), Fq::zero(), true};
  if (!is_dec(v.arr[2], "1")) bad(field + ": third coordinate is not \"1\"");
  return Affine<Fq>{x, y, false};
}
Fq2 fq2_field(const Val& v, const std::string& field) {
  if (v.kind != Val::ARR || v.arr.size() != 2) bad(field + ": not a pair of coordinates");
  return Fq2{coord(v.arr[0], field), coord(v.arr[1], field)};
}
Affine<Fq2> g2_field(const Val& v, const std::string& field) {
  if (v.kind != Val::ARR || v.arr.size() != 3) bad(field + ": not a projective G2 point of three coordinates");
  const Fq2 x = fq2_field(v.arr[0], field), y = fq2_field(v.arr[1], field);
  const Val& z = v.arr[2];
  if (z.kind != Val::ARR || z.arr.size() != 2) bad(field + ": third coordinate is not a pair");
  if (is_dec(z.arr[0], "0") && is_dec(z.arr[1], "0") && x.is_zero()) return Affine<Fq2>{Fq2::zero(), Fq2::zero(), true};
  if (!is_dec(z.arr[0], "1") || !is_dec(z.arr[1], "0")) bad(field + ": third coordinate is not [\"1\", \"0\"]");
  return Affine<Fq2>{x, y, false};
}
const Val& need(const Val& top, const char* key) {
  const Val* v = top.find(key);
  if (!v) bad(std::string("missing field ") + key);
  return *v;
}

const Fq2* f12_coeffs(const host::Fq12& f, int i) {
  const Fq2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  return c[i];
}

std::string dec(const Fq& a) { return host::u256_to_dec(a.to_std()); }

}  // namespace

void check_vkey(const VKey& vk) {
  if (vk.ic.size() != (size_t)vk.n_public + 1) bad("IC: length is not nPublic + 1");
  if (!host::g1_on_curve(vk.alpha1)) bad("vk_alpha_1: point is not on the curve");
  const Affine<Fq2>* g2s[3] = {&vk.beta2, &vk.gamma2, &vk.delta2};
  const char* names[3] = {"vk_beta_2", "vk_gamma_2", "vk_delta_2"};
  for (int i = 0; i < 3; ++i) {
    if (!host::g2_on_curve(*g2s[i])) bad(std::string(names[i]) + ": point is not on the curve");
    if (!host::g2_in_subgroup(*g2s[i])) bad(std::string(names[i]) + ": point is not in the subgroup of order r");
  }
  for (size_t i = 0; i < vk.ic.size(); ++i)
    if (!host::g1_on_curve(vk.ic[i])) bad("IC[" + std::to_string(i) + "]: point is not on the curve");
}

VKey parse_vkey_json(const char* json, size_t len) {
  if (!json) bad("null input");
  const Val top = Reader(json, len).top();
  if (top.kind != Val::OBJ) bad("top value is not an object");
  const Val& proto = need(top, "protocol");
  if (proto.kind != Val::STR) bad("protocol: not a string");
  if (proto.str != "groth16") throw ZkpError(ZKP_ERR_PROTOCOL, "vkey: protocol is not groth16");
  const Val& curve = need(top, "curve");
  if (curve.kind != Val::STR) bad("curve: not a string");
  if (curve.str != "bn128") throw ZkpError(ZKP_ERR_CURVE, "vkey: curve is not bn128");
  const Val& np = need(top, "nPublic");
  if (np.kind != Val::NUM) bad("nPublic: not a number");
  VKey vk;
  vk.n_public = (uint32_t)np.num;
  vk.alpha1 = g1_field(need(top, "vk_alpha_1"), "vk_alpha_1");
  vk.beta2 = g2_field(need(top, "vk_beta_2"), "vk_beta_2");
  vk.gamma2 = g2_field(need(top, "vk_gamma_2"), "vk_gamma_2");
  vk.delta2 = g2_field(need(top, "vk_delta_2"), "vk_delta_2");
  const Val& ic = need(top, "IC");
  if (ic.kind != Val::ARR) bad("IC: not an array");
  if (ic.arr.size() != (size_t)vk.n_public + 1) bad("IC: length is not nPublic + 1");
  for (size_t i = 0; i < ic.arr.size(); ++i) vk.ic.push_back(g1_field(ic.arr[i], "IC[" + std::to_string(i) + "]"));
  check_vkey(vk);
  if (const Val* ab = top.find("vk_alphabeta_12")) {
    const std::string f = "vk_alphabeta_12";
    if (ab->kind != Val::ARR || ab->arr.size() != 2) bad(f + ": not 2 x 3 x 2 coordinates");
    const host::Fq12 want = host::pairing(vk.alpha1, vk.beta2);
    for (int i = 0; i < 2; ++i) {
      const Val& h = ab->arr[i];
      if (h.kind != Val::ARR || h.arr.size() != 3) bad(f + ": not 2 x 3 x 2 coordinates");
      for (int j = 0; j < 3; ++j)
        if (!(fq2_field(h.arr[j], f) == *f12_coeffs(want, 3 * i + j))) bad(f + ": is not e(vk_alpha_1, vk_beta_2)");
    }
  }
  return vk;
}

VKey vkey_from_zkey(const uint8_t* zkey, size_t len) {
  const ZkeyParsed z = parse_zkey(zkey, len, false);
  const ZkeyHeader& h = z.hdr;
  VKey vk;
  vk.n_public = h.n_public;
  vk.alpha1 = h.alpha1, vk.beta2 = h.beta2, vk.gamma2 = h.gamma2, vk.delta2 = h.delta2;
  vk.ic = h.ic;
  if (vk.ic.size() != (size_t)vk.n_public + 1) throw ZkpError(ZKP_ERR_FORMAT, "zkey: no IC section");
  check_vkey(vk);
  return vk;
}

std::string vkey_json(const VKey& vk) {
  auto g1 = [](const Affine<Fq>& p, const std::string& in) {
    if (p.inf) return "[\n" + in + " \"0\",\n" + in + " \"1\",\n" + in + " \"0\"\n" + in + "]";
    return "[\n" + in + " \"" + dec(p.x) + "\",\n" + in + " \"" + dec(p.y) + "\",\n" + in + " \"1\"\n" + in + "]";
  };
  auto pair = [](const std::string& a, const std::string& b, const std::string& in) {
    return "[\n" + in + " \"" + a + "\",\n" + in + " \"" + b + "\"\n" + in + "]";
  };
  auto g2 = [&](const Affine<Fq2>& p) {
    const std::string in = "  ";
    if (p.inf)
      return "[\n" + in + pair("0", "0", in) + ",\n" + in + pair("1", "0", in) + ",\n" + in + pair("0", "0", in) + "\n ]";
    return "[\n" + in + pair(dec(p.x.c0), dec(p.x.c1), in) + ",\n" + in + pair(dec(p.y.c0), dec(p.y.c1), in) + ",\n" + in +
           pair("1", "0", in) + "\n ]";
  };
  std::string s = "{\n \"protocol\": \"groth16\",\n \"curve\": \"bn128\",\n \"nPublic\": " + std::to_string(vk.n_public) + ",\n";
  s += " \"vk_alpha_1\": " + g1(vk.alpha1, " ") + ",\n";
  s += " \"vk_beta_2\": " + g2(vk.beta2) + ",\n";
  s += " \"vk_gamma_2\": " + g2(vk.gamma2) + ",\n";
  s += " \"vk_delta_2\": " + g2(vk.delta2) + ",\n";
  const host::Fq12 ab = host::pairing(vk.alpha1, vk.beta2);
  s += " \"vk_alphabeta_12\": [\n";
  for (int i = 0; i < 2; ++i) {
    s += "  [\n";
    for (int j = 0; j < 3; ++j) {
      const Fq2& c = *f12_coeffs(ab, 3 * i + j);
      s += "   " + pair(dec(c.c0), dec(c.c1), "   ") + (j < 2 ? ",\n" : "\n");
    }
    s += i == 0 ? "  ],\n" : "  ]\n";
  }
  s += " ],\n \"IC\": [\n";
  for (size_t i = 0; i < vk.ic.size(); ++i) s += "  " + g1(vk.ic[i], "  ") + (i + 1 < vk.ic.size() ? ",\n" : "\n");
  s += " ]\n}";
  return s;
}

}  // namespace zkp
