// Per-lane bodies of `powersoftau challenge contribute` / `import response` (ptau_challenge.hip): __host__
// __device__ so that tools/hosttest/ptau_decompress_emu.cpp can replay them on the CPU.
//
//   decode      an "uncompressed" point (big-endian standard form, x then y; G2: c1 before c0; 0x40 then zeros
//               for infinity) -> the zkey layout
//   decompress  a compressed point (big-endian x, 0x80 in the first byte when y is the greater root, 0x40 then
//               zeros for infinity) -> the zkey layout and the uncompressed form: y = sqrt(x^3 + b)
//
// Square roots (p = 3 mod 4; E = (p - 3) / 4, 252 bits of which 109 are set: 251 squarings and 108
// products by plain square-and-multiply, the exponent a compile-time constant and so wave-uniform):
//   Fq   r = a^E a = a^((p + 1) / 4), a root iff r^2 = a.                              361 field products
//   Fq2  the norm method.  n = a0^2 + a1^2, s = n^E n (a root of n iff a is a square), d = (a0 + s) / 2,
//        t = d^E, e = t d, f = a1 t / 2.  d (a0 - s) / 2 = -a1^2 / 4 and -1 is a non-residue, so for a1 != 0
//        exactly one of d and (a0 - s) / 2 is a residue:
//          d a residue      e^2 = d,  1 / e = t       the root is  e + f u
//          d a non-residue  e^2 = -d, 1 / e = -t      the root is  f - e u   (f^2 = (a0 - s) / 2)
//        Both roots come from the ONE exponentiation t; which one is a select, and so is the only zero the
//        method would divide by: d = 0 (a1 = 0 and a0 a non-residue, s = -a0) takes d = a0 instead, whose
//        second case gives the purely imaginary root.  The result is checked by squaring, which is also the
//        verdict for a non-square a (s is then no root of n and the candidate is garbage).  728 field
//        products (2 E-powers, 5 products, 3 squarings and the Fq2 square of the check), against 1672-1894
//        for the algorithm of mpc.cpp's fq2_sqrt (two Fq2 exponentiations: 503 Fq2 squarings of 2 products
//        and 222 Fq2 products of 3-4).
//
// Field entry points and their inputs (all bounds proven by tools/hosttest/bounds.cpp): unpack gives exact
// limbs of a value < 2^254 (the flag bits are stripped) or < 2^256 (decode), both inside to_mont's < 8m;
// every other operand of mul / sqr / add / sub / canon / from_mont here is a normalised value < 2m (an
// output of mul, sqr, add, sub or of load_fe on a canonical constant); the one Fq2 product (x^2 x) passes
// through canon4 before add, as k_check_points composes it.
#pragma once
#include "ptau_scale_kernels.hpp"

namespace zkp {
namespace pdec {

// A launch's constants, passed by value.  Fq entries: device Montgomery form, canonical, 8 LE words.
struct alignas(16) Consts {
  uint32_t half[8];     // 1 / 2
  uint32_t b[16];       // the curve's b: c0, c1 (G1: 3, 0; G2: 3 / (9 + u))
  uint32_t to_zkey[8];  // 2^256 mod q as raw words (pscale::fill_to_zkey)
};

inline Fq fq_small(uint32_t v) {
  const uint32_t w[8] = {v, 0, 0, 0, 0, 0, 0, 0};
  return to_mont(unpack<FqCfg>(w));
}
inline void fill_consts(Consts& k, bool g2) {
  pack(canon(inv(fq_small(2))), k.half);
  uint32_t b0[8], b1[8];
  if (!g2) {
    pack(canon(fq_small(3)), b0);
    pack(fe_zero<FqCfg>(), b1);
  } else {  // 3 / (9 + u) = 3 (9 - u) / 82
    const Fq i82 = inv(fq_small(82));
    pack(canon(mul(fq_small(27), i82)), b0);
    pack(canon(neg(mul(fq_small(3), i82))), b1);
  }
  for (int i = 0; i < 8; ++i) k.b[i] = b0[i], k.b[8 + i] = b1[i];
  pscale::fill_to_zkey(k.to_zkey);
}

// ---------------------------------------------------------------- square roots

// a^((p - 3) / 4); 0 -> 0.  a: normalised, < 2m
ZDEV Fq pow_p34(const Fq& a) {
  Fq r = a;
  bool started = false;
  for (int wi = 7; wi >= 0; --wi) {
    const uint32_t lo = FqCfg::MOD_W[wi] - (wi == 0 ? 3u : 0u);  // the low word ends in 0x47: no borrow
    const uint32_t e = (lo >> 2) | (wi < 7 ? FqCfg::MOD_W[(wi + 1) & 7] << 30 : 0u);
    for (int b = 31; b >= 0; --b) {
      const bool bit = (e >> b) & 1u;
      if (!started) {  // the top set bit: r = a
        started = bit;
        continue;
      }
      r = sqr(r);
      if (bit) r = mul(r, a);
    }
  }
  return r;
}

ZDEV Fq select_fq(bool c, const Fq& a, const Fq& b) {
  Fq r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}

// root: a^((p + 1) / 4); -> whether it is a root of a (else a is a non-residue).  a: < 2m
ZDEV bool fsqrt(const Fq& a, const Fq& /*half*/, Fq& root) {
  root = mul(pow_p34(a), a);
  return eq(sqr(root), a);
}

// the norm method (above).  a: components < 2m
ZDEV bool fsqrt(const Fq2& a, const Fq& half, Fq2& root) {
  const Fq n = add(sqr(a.c0), sqr(a.c1));
  const Fq s = mul(pow_p34(n), n);
  Fq d = mul(add(a.c0, s), half);
  d = select_fq(is_zero(d), a.c0, d);
  const Fq t = pow_p34(d);
  const Fq e = mul(t, d), f = mul(mul(a.c1, t), half);
  const bool residue = eq(sqr(e), d);
  root.c0 = select_fq(residue, e, f);
  root.c1 = select_fq(residue, f, neg(e));
  const Fq2 chk = sqr(root);
  return eq(chk.c0, a.c0) && eq(chk.c1, a.c1);
}

// ---------------------------------------------------------------- byte forms

ZDEV bool geq_mod(const Fq& a) {  // a (exact limbs of a value < 2^256) >= p
#pragma unroll
  for (int l = NL - 1; l >= 0; --l)
    if (a.v[l] != FqCfg::MOD[l]) return a.v[l] > FqCfg::MOD[l];
  return true;
}

// 32 big-endian bytes at p as exact limbs; keep: the bits of the first byte that belong to the value
ZDEV Fq load_be(const uint32_t* p, uint32_t keep) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  const uint32_t be[8] = {a.x & (0xffffff00u | keep), a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) w[7 - k] = pscale::bswap32(be[k]);
  return unpack<FqCfg>(w);
}
// words [1, words) of a record and the bytes after the first of word 0 are all zero
ZDEV bool tail_zero(const uint32_t* p, int words) {
  uint32_t o = p[0] & 0xffffff00u;
  for (int k = 1; k < words; ++k) o |= p[k];
  return o == 0;
}

ZDEV void load_coord(const uint32_t* p, uint32_t keep, Fq& x, bool& bad) {
  x = load_be(p, keep);
  bad = geq_mod(x);
  x = to_mont(x);
}
ZDEV void load_coord(const uint32_t* p, uint32_t keep, Fq2& x, bool& bad) {  // c1 first
  const Fq c1 = load_be(p, keep), c0 = load_be(p + 8, 0xffu);
  bad = geq_mod(c1) || geq_mod(c0);
  x = Fq2{to_mont(c0), to_mont(c1)};
}

ZDEV Fq below2m(const Fq& a) { return a; }
ZDEV Fq2 below2m(const Fq2& a) { return canon4(a); }
ZDEV void load_b(const Consts& k, Fq& b) { b = load_fe<FqCfg>(k.b); }
ZDEV void load_b(const Consts& k, Fq2& b) { b = Fq2{load_fe<FqCfg>(k.b), load_fe<FqCfg>(k.b + 8)}; }

// pscale::encode's "greater root" predicate on a Montgomery-form y < 2m
ZDEV bool greater(const Fq& y) {
  uint32_t w[8];
  pack(from_mont(y), w);
  return pscale::above_half(w);
}
ZDEV bool greater(const Fq2& y) {
  uint32_t w0[8], w1[8];
  pack(from_mont(y.c0), w0), pack(from_mont(y.c1), w1);
  return pscale::is_zero8(w1) ? pscale::above_half(w0) : pscale::above_half(w1);
}
ZDEV Fq negated(const Fq& y) { return neg(y); }
ZDEV Fq2 negated(const Fq2& y) { return Fq2{neg(y.c0), neg(y.c1)}; }
ZDEV Fq select_f(bool c, const Fq& a, const Fq& b) { return select_fq(c, a, b); }
ZDEV Fq2 select_f(bool c, const Fq2& a, const Fq2& b) {
  return Fq2{select_fq(c, a.c0, b.c0), select_fq(c, a.c1, b.c1)};
}

// a bad point: zeros in every stream that is asked for
template <class F>
ZDEV void store_bad(uint32_t* lem, uint32_t* u, size_t idx) {
  constexpr int W = 2 * FWords<F>::W;
  if (lem) pscale::store_zero(lem + idx * W, W, 0);
  if (u) pscale::store_zero(u + idx * W, W, 0);
}

// Point idx of `in` (uncompressed, 2 W words each) into lem (zkey layout).  -> bad: a coordinate >= p, or a
// first byte with 0x40 set that is not 0x40 followed by zeros.  Whether the point is on its curve is
// k_check_points' question, asked of the zkey layout written here.
template <class F>
ZDEV bool decode_lane(const uint32_t* in, const uint32_t (&to_zkey)[8], uint32_t* lem, size_t idx) {
  constexpr int W = FWords<F>::W;
  const uint32_t* p = in + idx * 2 * W;
  const uint32_t first = p[0] & 0xffu;
  const bool inf = (first & pscale::FLAG_INF) != 0;
  bool bad_x, bad_y;
  Aff<F> a;
  load_coord(p, 0xffu, a.x, bad_x);
  load_coord(p + W, 0xffu, a.y, bad_y);
  const bool bad = inf ? !(first == pscale::FLAG_INF && tail_zero(p, 2 * W)) : (bad_x || bad_y);
  if (bad)
    store_bad<F>(lem, nullptr, idx);
  else
    pscale::encode(a, inf, to_zkey, lem, nullptr, nullptr, idx);
  return bad;
}

// Point idx of `in` (compressed, W words each) into lem (zkey layout) and u (uncompressed), either may be
// null.  -> bad: 0x40 set and anything else but zeros beside it (0x80 included), x >= p, or x^3 + b a
// non-residue.  The exponentiations run for every lane; what a lane is (infinity, bad, which root) is
// selected at the end.
template <class F>
ZDEV bool decompress_lane(const uint32_t* in, const Consts& k, uint32_t* lem, uint32_t* u, size_t idx) {
  constexpr int W = FWords<F>::W;
  const uint32_t* p = in + idx * W;
  const uint32_t first = p[0] & 0xffu;
  const bool inf = (first & pscale::FLAG_INF) != 0, want_greater = (first & pscale::FLAG_GREATER) != 0;
  bool bad_x;
  Aff<F> a;
  load_coord(p, 0x3fu, a.x, bad_x);
  F b, y;
  load_b(k, b);
  const Fq half = load_fe<FqCfg>(k.half);
  const F rhs = add(below2m(mul(sqr(a.x), a.x)), b);
  const bool square = fsqrt(rhs, half, y);
  a.y = select_f(greater(y) != want_greater, negated(y), y);
  const bool bad = inf ? !(first == pscale::FLAG_INF && tail_zero(p, W)) : (bad_x || !square);
  if (bad)
    store_bad<F>(lem, u, idx);
  else
    pscale::encode(a, inf, k.to_zkey, lem, u, nullptr, idx);
  return bad;
}

// element idx of `in` (32 bytes LE standard form per Fq; Fq2: c0 then c1, canonical) -> a root in the same
// form or zeros, and whether there is one
template <class F>
ZDEV void sqrt_lane(const uint32_t* in, const Consts& k, uint32_t* out, uint8_t* is_square, size_t idx) {
  constexpr int W = FWords<F>::W;
  F a, r;
  if constexpr (W == 8) {
    a = to_mont(load_fe<FqCfg>(in + idx * W));
  } else {
    a = F{to_mont(load_fe<FqCfg>(in + idx * W)), to_mont(load_fe<FqCfg>(in + idx * W + 8))};
  }
  const bool ok = fsqrt(a, load_fe<FqCfg>(k.half), r);
  uint32_t* o = out + idx * W;
  if (!ok) {
    pscale::store_zero(o, W, 0);
  } else if constexpr (W == 8) {
    store_fe(o, from_mont(r));
  } else {
    store_fe(o, from_mont(r.c0)), store_fe(o + 8, from_mont(r.c1));
  }
  is_square[idx] = ok ? 1 : 0;
}

}  // namespace pdec
}  // namespace zkp
