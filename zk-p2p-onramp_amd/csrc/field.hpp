// BN254 prime-field arithmetic for gfx950 (CDNA4) — device side.
//
// Representation (DESIGN.md "Field arithmetic"):
//   * compute form: 9 limbs x 29 bits in uint32_t, Montgomery radix R' = 2^261,
//     values kept REDUNDANT in [0, 2m) — never a final subtraction inside mul.
//   * storage form (HBM): 8 x 32-bit little-endian words, value < 2^256.
//
// Why 29-bit limbs: gfx950 issues v_mad_u64_u32 (32x32+64 -> 64) at close to the
// full VALU rate (tools/ubench: measured), while every carry out of a 32-bit limb
// costs extra adds/movs.  With 29-bit limbs a product-scanning (FIPS) Montgomery
// multiply accumulates each column of up to 18 partial products in ONE 64-bit
// register pair without overflow (18 * 2^58 < 2^63), so each partial product is
// exactly one v_mad_u64_u32 and carries are resolved once per column (shift).
// Measured 171 G mul/s (vs 98 G mul/s for compiler CIOS on 8x32-bit limbs).
//
// Restates the arithmetic of ffjavascript/wasmcurves (f1m/frm Montgomery
// multiply) in a different radix: results are converted back to
// the snarkjs byte conventions at the boundary, so they are bit-identical.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "consts.hpp"

namespace zkp {

constexpr int NL = 9;
constexpr int LB = 29;
constexpr uint32_t LMASK = (1u << LB) - 1;

// (a host tool that instantiates these templates on heavier types may define ZDEV without the forced inlining)
#ifndef ZDEV
#define ZDEV __host__ __device__ __forceinline__
#endif

// The limb and column-accumulator types of a field config, and what each primitive below reports about
// its result.  Every real config computes on uint32_t limbs with a uint64_t column accumulator and
// reports nothing: note() is empty and the op name it is given (ZFN: the name of the calling function,
// "lsub8" for the borrow_sub inside lsub8) is dropped with it.  The bounds prover
// (tools/hosttest/bounds.cpp) specialises FeTypes and Fe for configs whose limbs are integer intervals
// and runs these same templates on them; its note() applies the value-level transfer function of the
// primitive and checks its operand contract.  The few casts that depend on the limb type are spelled
// as the functions wide / lo32 / sgn / unsg / select, which the prover overloads for its types.
struct n_sop {};
struct n_sqr {};
struct n_shoup {};
struct n_normalize {};
struct n_cond_sub {};
struct n_qreduce {};
struct n_add_raw {};
struct n_borrow_sub {};
struct n_shl1 {};
template <class C>
struct FeTypes {
  using limb = uint32_t;
  using slimb = int32_t;
  using acc = uint64_t;
  template <class... A>
  static ZDEV void note(const A&...) {}
};
#define ZFN const char* fn = __builtin_FUNCTION()

template <class C>
struct Fe {
  typename FeTypes<C>::limb v[NL];
};

using Fq = Fe<FqCfg>;
using Fr = Fe<FrCfg>;

ZDEV uint64_t wide(uint32_t x) { return x; }             // limb -> accumulator
ZDEV uint32_t lo32(uint64_t a) { return (uint32_t)a; }   // accumulator -> limb: truncates unless a < 2^32
ZDEV int32_t sgn(uint32_t x) { return (int32_t)x; }      // limb read as a signed word
ZDEV uint32_t unsg(int32_t x) { return (uint32_t)x; }
template <class T>
ZDEV T select(bool c, T a, T b) { return c ? a : b; }

// acc += x * y.  CH (C::CHAIN, device code): every product column stays ONE dependent chain seeded
// by the previous column's carry.  Left to itself the compiler re-associates each column into a sum
// from 0 plus a 64-bit join of the carry (v_lshl_add_u64 per column).  After each product the
// accumulator passes through an EMPTY asm statement that claims to modify it, so the column cannot be
// re-associated while the compiler still sees, schedules and hazard-checks real v_mad_u64_u32
// instructions (it interleaves independent products' chains to cover the wait states between
// dependent 64-bit mads).  tools/ubench/mul_chain.hip, profiles/mul_chain_r03.txt.  mac_k takes a
// constant.  Host code is always plain C.
template <bool CH, class A, class T>
ZDEV void mac(A& acc, T x, T y) {
  acc += wide(x) * y;
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (CH) asm("" : "+v"(acc));
#endif
}
template <bool CH, class A, class T>
ZDEV void mac_k(A& acc, T x, uint32_t k) {
  acc += wide(x) * k;
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (CH) asm("" : "+v"(acc));
#endif
}

template <class C>
ZDEV Fe<C> fe_zero() {
  Fe<C> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = 0;
  return r;
}

template <class C>
ZDEV Fe<C> fe_const(const uint32_t (&k)[NL]) {
  Fe<C> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = k[i];
  return r;
}

template <class C>
ZDEV Fe<C> fe_one() { return fe_const<C>(C::ONE); }

// ---------------------------------------------------------------- product cores
// Every field product is one of three product-scanning column loops, each written once for L
// independent LANES in lockstep.  With chained columns (CH) the lanes' chains interleave, so a
// dependent mad of one chain follows an independent mad of the other instead of a wait state; L = 1
// is the plain form.  The statement order inside a column is what the scheduler sees and is the
// tuning knob: the products of all lanes for one (j, k), then the constant (m MOD / q NM) terms lane
// by lane.  All loops unroll fully; the operand arrays of pointers cost nothing.
#define ZLANES _Pragma("unroll") for (int l = 0; l < L; ++l)

// Montgomery sum of products (FIPS / product scanning): r[l] = sum_k a[l][k] b[l][k] / 2^261 mod m
// with ONE reduction per lane ("lazy reduction": the N products' and the m MOD partial products of a
// column accumulate together).  Column i takes a_j b_(i-j) for every j in range; m_i, the quotient
// digit that clears the column, is fixed once the column's last product (j = i) is in.
//   N = 1: both operands' limbs 0..7 < 2^30 (value < 8m; up to ~11m as long as a b < 169 m^2), or ONE
//          operand with limbs < 2.5 * 2^30 (the largest raw form, sub_raw8) against a normalised one
//          (column sums < 9 * 2.5 * 2^59 + 9 * 2^58 + 2^35 = 0.84 * 2^64).
//   N = 2: all operands normalised but at most ONE, with limbs < 2^31 (the G1 Y3's d = rsub(0, PPP):
//          columns < 9 * 2^60 + 18 * 2^58 + 2^35 = 0.84 * 2^64; two raw operands could reach 2^64).
//   N = 4: all operands normalised (columns hold <= 36 + 9 partial products < 2^58, < 2^63.5).
//   Every N: the sum < m 2^261 (~169 m^2).
// Output: normalised limbs, value < 2m (sum / 2^261 + m).
// These contracts, and every bound quoted in this file, are proven for all inputs by
// tools/hosttest/bounds.cpp, which runs these templates on interval limbs.
template <class C, bool CH, int L, int N>
ZDEV void mont_sop(const Fe<C>* const (&a)[L][N], const Fe<C>* const (&b)[L][N], Fe<C>* const (&r)[L], ZFN) {
  typename FeTypes<C>::limb m[L][NL];
  typename FeTypes<C>::acc acc[L];
  ZLANES acc[l] = 0;
#pragma unroll
  for (int i = 0; i < 2 * NL - 1; ++i) {
#pragma unroll
    for (int j = (i < NL ? 0 : i - NL + 1); j <= (i < NL ? i : NL - 1); ++j) {
#pragma unroll
      for (int k = 0; k < N; ++k) ZLANES mac<CH>(acc[l], a[l][k]->v[j], b[l][k]->v[i - j]);
      if (j == i) ZLANES m[l][i] = (lo32(acc[l]) * C::INV) & LMASK;
      ZLANES mac_k<CH>(acc[l], m[l][j], C::MOD[i - j]);
    }
    if (i >= NL) ZLANES r[l]->v[i - NL] = lo32(acc[l]) & LMASK;
    ZLANES acc[l] >>= LB;
  }
  ZLANES r[l]->v[NL - 1] = lo32(acc[l]);
  ZLANES FeTypes<C>::note(n_sop{}, fn, a[l], b[l], *r[l]);
}

// Montgomery squares r[l] = a[l]^2 / 2^261 mod m: cross products computed once against a doubled
// operand.  Operand and output as mont_sop with N = 1 (a < 11m).
template <class C, bool CH, int L>
ZDEV void mont_sqr(const Fe<C>* const (&a)[L], Fe<C>* const (&r)[L], ZFN) {
  typename FeTypes<C>::limb m[L][NL], d[L][NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) ZLANES d[l][i] = a[l]->v[i] << 1;
  typename FeTypes<C>::acc acc[L];
  ZLANES acc[l] = 0;
#pragma unroll
  for (int i = 0; i < 2 * NL - 1; ++i) {
    const int lo = i < NL ? 0 : i - NL + 1, hi = i < NL ? i : NL - 1;
#pragma unroll
    for (int j = lo; j < (i + 1) / 2; ++j) ZLANES mac<CH>(acc[l], d[l][j], a[l]->v[i - j]);
    if ((i & 1) == 0) ZLANES mac<CH>(acc[l], a[l]->v[i / 2], a[l]->v[i / 2]);
#pragma unroll
    for (int j = lo; j <= hi; ++j) {
      if (j == i) ZLANES m[l][i] = (lo32(acc[l]) * C::INV) & LMASK;
      ZLANES mac_k<CH>(acc[l], m[l][j], C::MOD[i - j]);
    }
    if (i >= NL) ZLANES r[l]->v[i - NL] = lo32(acc[l]) & LMASK;
    ZLANES acc[l] >>= LB;
  }
  ZLANES r[l]->v[NL - 1] = lo32(acc[l]);
  ZLANES FeTypes<C>::note(n_sqr{}, fn, *a[l], *r[l]);
}

// Products by CONSTANTS with precomputed quotients (Shoup): r[l] = a[l] w[l] mod m for w < m given
// as plain limbs and wq = floor(w 2^261 / m) (both normalised, 9 limbs).  q = floor(a wq / 2^261)
// from the product columns 7..17 only (the dropped columns 0..6 sum to < 2^237, so q is the exact
// floor or one less), then a w - q m = (a w + q (2^261 - m)) mod 2^261 from the low columns 0..8.
// Since a w / m - a wq / 2^261 < a / 2^261 <= 1, the result is in [0, 3m).  a: limbs < 2.5 * 2^30 (a raw
// sum or borrow-form difference is fine: sub_raw8's is the largest), value < 2^261.  A Montgomery-form a stays in Montgomery
// form (w is plain).  143 v_mad_u64_u32 and no per-column quotient digits, against 162 mads plus
// 9 v_mul_lo_u32 for mul(); NTT roots, twiddles and the coset key are all constants.
template <class C, int L>
ZDEV void mont_shoup(const Fe<C>* const (&a)[L], const Fe<C>* const (&w)[L], const Fe<C>* const (&wq)[L],
                     Fe<C>* const (&r)[L], ZFN) {
  typename FeTypes<C>::limb q[L][NL];
  typename FeTypes<C>::acc acc[L];
  ZLANES acc[l] = 0;
#pragma unroll
  for (int c = 7; c < 2 * NL - 1; ++c) {
#pragma unroll
    for (int i = (c < NL ? 0 : c - NL + 1); i <= (c < NL ? c : NL - 1); ++i)
      ZLANES mac<C::CHAIN>(acc[l], a[l]->v[i], wq[l]->v[c - i]);
    if (c >= NL) ZLANES q[l][c - NL] = lo32(acc[l]) & LMASK;
    ZLANES acc[l] >>= LB;
  }
  ZLANES q[l][NL - 1] = lo32(acc[l]);  // columns 9..16 give q's limbs 0..7, the carry out its top limb (q < 2^261)
  ZLANES acc[l] = 0;
#pragma unroll
  for (int c = 0; c < NL; ++c) {
#pragma unroll
    for (int i = 0; i <= c; ++i) {
      ZLANES mac<C::CHAIN>(acc[l], a[l]->v[i], w[l]->v[c - i]);
      ZLANES mac_k<C::CHAIN>(acc[l], q[l][i], C::NM[c - i]);
    }
    ZLANES r[l]->v[c] = lo32(acc[l]) & LMASK;
    ZLANES acc[l] >>= LB;
  }
  ZLANES FeTypes<C>::note(n_shoup{}, fn, *a[l], *w[l], *wq[l], *r[l]);
}
#undef ZLANES

// Montgomery product a*b/2^261 mod m.
// Inputs: limbs 0..7 < 2^30, value < 8m.  Output: normalised limbs, value < 2m.
template <class C>
ZDEV Fe<C> mul(const Fe<C>& a, const Fe<C>& b) {
  Fe<C> r;
  mont_sop<C, C::CHAIN, 1, 1>({{&a}}, {{&b}}, {&r});
  return r;
}

// (a*b + c*d)/2^261 mod m with ONE reduction.  All four operands normalised (limbs < 2^29; column
// sums <= 27 * 2^58 < 2^63) and a*b + c*d < m*2^261 (~169 m^2) for an output < 2m.  Used for
// Y3 = R (Q - X3) - Y1 PPP as R*(Q - X3) + Y1*(2m - PPP): one reduction and no
// subtraction instead of two multiplies and a subtraction (~230 instructions saved).
template <class C>
ZDEV Fe<C> mul2(const Fe<C>& a, const Fe<C>& b, const Fe<C>& c, const Fe<C>& d) {
  Fe<C> r;
  mont_sop<C, C::CHAIN, 1, 2>({{&a, &c}}, {{&b, &d}}, {&r});
  return r;
}

template <class C>
ZDEV Fe<C> sqr(const Fe<C>& a) {
  Fe<C> r;
  mont_sqr<C, C::CHAIN, 1>({&a}, {&r});
  return r;
}

// a w for a constant w with its Shoup quotient wq (mont_shoup): output in [0, 3m)
template <class C>
ZDEV Fe<C> mul_shoup(const Fe<C>& a, const Fe<C>& w, const Fe<C>& wq) {
  Fe<C> r;
  mont_shoup<C, 1>({&a}, {&w}, {&wq}, {&r});
  return r;
}

// Two independent products r = a b, s = c d / squares r = a^2, s = c^2 / Shoup products r = a w,
// s = c v in lockstep.  Same arithmetic as mul() / sqr() / mul_shoup() on each pair.
template <class C>
ZDEV void mul_pair(const Fe<C>& a, const Fe<C>& b, const Fe<C>& c, const Fe<C>& d, Fe<C>& r, Fe<C>& s) {
  mont_sop<C, C::CHAIN, 2, 1>({{&a}, {&c}}, {{&b}, {&d}}, {&r, &s});
}
template <class C>
ZDEV void sqr_pair(const Fe<C>& a, const Fe<C>& c, Fe<C>& r, Fe<C>& s) {
  mont_sqr<C, C::CHAIN, 2>({&a, &c}, {&r, &s});
}
template <class C>
ZDEV void mul_shoup_pair(const Fe<C>& a, const Fe<C>& w, const Fe<C>& wq, const Fe<C>& c, const Fe<C>& v,
                         const Fe<C>& vq, Fe<C>& r, Fe<C>& s) {
  mont_shoup<C, 2>({&a, &c}, {&w, &v}, {&wq, &vq}, {&r, &s});
}

// Shoup quotient of a constant from its canonical Montgomery form wm = w 2^261 mod m (< m):
// w 2^261 = wq m + wm, so wq = floor(w 2^261 / m) = -wm m^-1 mod 2^261 (a low-half product).
template <class C>
ZDEV Fe<C> shoup_quot(const Fe<C>& wm) {
  uint32_t p[NL];
  uint64_t acc = 0;
#pragma unroll
  for (int c = 0; c < NL; ++c) {
#pragma unroll
    for (int i = 0; i <= c; ++i) acc += (uint64_t)wm.v[i] * C::MINV261[c - i];
    p[c] = (uint32_t)acc & LMASK;
    acc >>= LB;
  }
  Fe<C> r;  // 2^261 - p  (mod 2^261)
  uint32_t carry = 1;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const uint32_t t = (LMASK - p[i]) + carry;
    r.v[i] = t & LMASK;
    carry = t >> LB;
  }
  return r;
}

// ---------------------------------------------------------------- sums and differences
// A sum or difference is ONE limb pass (add_raw / borrow_sub) followed by one of three tails:
//   raw         nothing: limbs stay unnormalised
//   normalized  the carry pass alone: no conditional subtraction
//   reduce2 / reduce8   down to < 2m from < 4m / < 8m
// The functions below only name a (table, tail) pair; their comments carry the value bounds.

// carry-propagate limbs 0..7 into 29-bit digits (limb values must be >= 0 and < 2^31)
template <class C>
ZDEV void normalize(Fe<C>& a, ZFN) {
#pragma unroll
  for (int i = 0; i < NL - 1; ++i) {
    a.v[i + 1] += a.v[i] >> LB;
    a.v[i] &= LMASK;
  }
  FeTypes<C>::note(n_normalize{}, fn, a);
}
template <class C>
ZDEV Fe<C> normalized(Fe<C> s, ZFN) {
  normalize(s, fn);
  return s;
}

// a - M if a >= M else a   (a normalised, < 2^261; M normalised limbs)
template <class C>
ZDEV Fe<C> cond_sub(const Fe<C>& a, const uint32_t (&M)[NL], ZFN) {
  Fe<C> d;
  typename FeTypes<C>::slimb carry = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const auto t = sgn(a.v[i]) - (int32_t)M[i] + carry;
    d.v[i] = unsg(t) & LMASK;
    carry = t >> LB;
  }
  // no borrow out of the top limb: a >= M, and the masked top limb of d is its whole value
  const auto ge = carry >= 0;
  Fe<C> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = select(ge, d.v[i], a.v[i]);
  FeTypes<C>::note(n_cond_sub{}, fn, a, M, r);
  return r;
}

// Quotient-estimate reduction: s (limbs 0..7 in [0, 2^32 - 2^10), unnormalised; value
// v in [0, 2^261)) -> v - q m, normalised, value < 1.2m, in ONE carry pass.  q comes from the
// top limb alone, q = floor(s8 * floor(2^264/m) / 2^32) <= v/m (all limbs >= 0), and
// v/m - q < 1 + 2^-3 + (low limbs) / m, so 0 <= v - q m < 1.2m.  v - q m = (v + q (2^261 - m))
// mod 2^261: per limb one v_mad_u64_u32 (q * NM[i] + s[i] + carry < 2^39), a mask and a shift,
// instead of a carry pass plus one or two borrow-chain conditional subtractions with selects
// (34 vs 65-105 instructions).  A top limb that went "negative" (uint32 wrap of a wide-borrow
// form whose true top, after the lower carries, is >= 0) has a value below the low limbs' own weight,
// < 2^32 * 2^203 = 2^235 < m: q = 0, and the carry pass brings the top limb back because v >= 0.
template <class C>
ZDEV Fe<C> qreduce(const Fe<C>& s, ZFN) {
  using limb = typename FeTypes<C>::limb;
  const auto top = sgn(s.v[NL - 1]);
  const limb q = top > 0 ? limb(lo32((wide(unsg(top)) * C::QK) >> 32)) : limb(0u);
  Fe<C> r;
  limb carry = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const auto acc = wide(q) * C::NM[i] + wide(s.v[i] + carry);
    r.v[i] = lo32(acc) & LMASK;
    carry = lo32(acc >> LB);
  }
  FeTypes<C>::note(n_qreduce{}, fn, s, r);
  return r;
}

// s (limbs < 2^31, value < 4m) -> < 2m: qreduce for Fr (C::QRED: the NTT, 3 waves/SIMD, 5 % faster
// per transform), carry pass + one conditional subtraction for Fq, whose XYZZ kernels are
// register-bound (qreduce's 64-bit temporaries: 124 -> 135 VGPRs in k_accumulate, 4 -> 3 waves).
template <class C>
ZDEV Fe<C> reduce2(Fe<C> s, ZFN) {
  if constexpr (C::QRED) {
    return qreduce(s, fn);
  } else {
    normalize(s, fn);
    return cond_sub(s, C::MOD2, fn);
  }
}

// x < 8m (normalised) -> < 2m
template <class C>
ZDEV Fe<C> canon8(const Fe<C>& a, ZFN) { return cond_sub(cond_sub(a, C::MOD4, fn), C::MOD2, fn); }

// s (limbs 0..7 >= 0 and < 2^32 - 2^10, Fq: < 2^31; value in [0, 8m)) -> < 2m (Fr: qreduce, < 1.2m)
template <class C>
ZDEV Fe<C> reduce8(Fe<C> s, ZFN) {
  if constexpr (C::QRED) {
    return qreduce(s, fn);
  } else {
    normalize(s, fn);
    return canon8(s, fn);
  }
}

// a + b limb by limb, raw: no carry pass, no reduction
template <class C>
ZDEV Fe<C> add_raw(const Fe<C>& a, const Fe<C>& b, ZFN) {
  Fe<C> s;
#pragma unroll
  for (int i = 0; i < NL; ++i) s.v[i] = a.v[i] + b.v[i];
  FeTypes<C>::note(n_add_raw{}, fn, a, b, s);
  return s;
}

// a + K - b (- 2c) limb by limb, raw, for a borrow form K of a multiple of m (consts.hpp): K's low
// limbs are raised by what the subtrahends can reach (MODk_BORROW: 2^29, one normalised b;
// MOD8_B30: 2^30, a raw sum b; MOD6_WIDE: 2^31, b and 2c normalised) so that no limb 0..7 goes
// below zero.  The caller names the tail.  K comes as ZTAB(name), a function i -> C::name[i], and
// not as a reference to the table: device code folds a table into literals only where it is indexed
// directly; a table bound to a reference stays in memory and its limbs arrive by scalar loads.
#define ZTAB(K) [](int i) { return C::K[i]; }
template <class C, class T>
ZDEV Fe<C> borrow_sub(const Fe<C>& a, T K, const Fe<C>& b, const Fe<C>* c = nullptr, ZFN) {
  Fe<C> s;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    s.v[i] = a.v[i] + K(i) - b.v[i];
    if (c) s.v[i] -= c->v[i] << 1;
  }
  FeTypes<C>::note(n_borrow_sub{}, fn, a, K, b, c, s);
  return s;
}

// a + b, inputs < 2m (normalised) -> output < 2m
template <class C>
ZDEV Fe<C> add(const Fe<C>& a, const Fe<C>& b) { return reduce2(add_raw(a, b)); }

// a - b, inputs < 2m -> output < 2m   (computes a + 2m - b)
template <class C>
ZDEV Fe<C> sub(const Fe<C>& a, const Fe<C>& b) { return reduce2(borrow_sub(a, ZTAB(MOD2_BORROW), b)); }

// a - b for a normalised a < 4m and b <= 4m (computes a + 4m - b): output < 2m (Fr: qreduce < 1.2m).
// The NTT with Shoup root products (outputs < 3m) subtracts with it.
template <class C>
ZDEV Fe<C> sub4(const Fe<C>& a, const Fe<C>& b) { return reduce8(borrow_sub(a, ZTAB(MOD4_BORROW), b)); }

// ---- lazy subtractions: results that only ever feed a multiplication skip the final
// conditional subtraction (and, for one mul operand, even the carry normalisation):
// mul() accepts values < 8m, and one operand with limbs < 2^31 when the other is
// normalised (column sums stay < 9*2^60 + 9*2^58 + 2^35 < 2^64).  ~46 resp. ~70 VALU
// instructions saved per use (an XYZZ mixed add has ~3000).

// a - b + 2m, normalised, value < 4m: an operand of mul() / sqr() only
template <class C>
ZDEV Fe<C> lsub(const Fe<C>& a, const Fe<C>& b) { return normalized(borrow_sub(a, ZTAB(MOD2_BORROW), b)); }

// a - b + 4m for a, b < 2m, NOT normalised (every limb in [0, 2^31), value < 6m; b < 3m as in the NTT:
// limbs < 1.5 * 2^30, value < 7m for a < 3m): ONE operand of mul() / mul2() whose other operands are
// normalised, or of mul_shoup() / qreduce(); never sqr(), add(), sub(), is_zero(), storage
template <class C>
ZDEV Fe<C> rsub(const Fe<C>& a, const Fe<C>& b) { return borrow_sub(a, ZTAB(MOD4_BORROW), b); }

// a - b - 2c for a, b, c < 2m (normalised), result < 2m: one limb pass against 6m in the
// wide borrow form (low limbs + 2^31, so three subtrahends never borrow), one carry
// normalisation (value in (0, 8m)), then conditional subtractions of 4m and 2m.  The
// X3 = R^2 - PPP - 2Q of every XYZZ add in one go (~150 instead of ~250 instructions).
template <class C>
ZDEV Fe<C> sub_2x(const Fe<C>& a, const Fe<C>& b, const Fe<C>& c) {
  return reduce8(borrow_sub(a, ZTAB(MOD6_WIDE), b, &c));
}

// ---- lazily reduced accumulator x (G1 XYZZ additions): X3 = R^2 - PPP - 2Q stays in (0, 8m)
// without its two conditional subtractions (~90 instructions per addition).  Every consumer takes
// an x < 8m: mul()/sqr() operands (the output stays < 2m up to operands of ~11m: a*b/2^261 + m
// < 2m for a*b < 169 m^2), lsub8() for the differences, canon8() before storage.

// a - b - 2c + 6m for a, b, c < 2m (normalised): normalised, value in (0, 8m)
template <class C>
ZDEV Fe<C> sub_2x8(const Fe<C>& a, const Fe<C>& b, const Fe<C>& c) {
  return normalized(borrow_sub(a, ZTAB(MOD6_WIDE), b, &c));
}

// a - b + 8m for a < 2m, b < 8m (normalised): normalised, value < 10m -- a mul / sqr operand
template <class C>
ZDEV Fe<C> lsub8(const Fe<C>& a, const Fe<C>& b) { return normalized(borrow_sub(a, ZTAB(MOD8_BORROW), b)); }

// a - b + 4m (b < 4m) and a - b + 6m (b < 6m), normalised: mul / sqr operands
template <class C>
ZDEV Fe<C> lsub4(const Fe<C>& a, const Fe<C>& b) { return normalized(borrow_sub(a, ZTAB(MOD4_BORROW), b)); }
template <class C>
ZDEV Fe<C> lsub6(const Fe<C>& a, const Fe<C>& b) { return normalized(borrow_sub(a, ZTAB(MOD6_BORROW), b)); }

// 2a, limbs shifted (raw: limbs < 2^30 for a normalised a): ONE operand of mul()
template <class C>
ZDEV Fe<C> shl1_raw(const Fe<C>& a, ZFN) {
  Fe<C> s;
#pragma unroll
  for (int i = 0; i < NL; ++i) s.v[i] = a.v[i] << 1;
  FeTypes<C>::note(n_shl1{}, fn, a, s);
  return s;
}

// ---- lazy radix-4 sums (NTT): a first-stage sum x + y of two normalised values < 2m is kept
// raw (add_raw: limbs < 2^30, value < 4m, no carry pass and no conditional subtraction); the second
// stage consumes two such sums:

// a + b for raw sums a, b < 4m: normalised and reduced from < 8m to < 2m
template <class C>
ZDEV Fe<C> add_raw_reduce(const Fe<C>& a, const Fe<C>& b) { return reduce8(add_raw(a, b)); }

// a - b + 6m for raw sums a, b < 4m (wide borrow form: every limb stays >= 0), normalised,
// value < 10m: an operand of mul() against a normalised value < 2m only (product < 20 m^2)
template <class C>
ZDEV Fe<C> sub_raw6(const Fe<C>& a, const Fe<C>& b) { return normalized(borrow_sub(a, ZTAB(MOD6_WIDE), b)); }

// a - b + 8m for raw sums a, b < 6m of two normalised values each (limbs < 2^30), WITHOUT a carry
// pass: the 8m borrow form whose low limbs are raised by 2^30 (consts MOD8_B30) keeps every limb
// >= 0 and < 2^30 + 2^30 + 2^29 = 2.5 * 2^30, value < 14m.  An operand of mul_shoup (column sums
// <= 9 (2.5 + 0.5) 2^59 < 2^63.8), of mul() against a normalised value, or of qreduce (limbs
// < 2^32 - 2^10) -- never a second raw operand (the NTT's radix-4 unit, round 5: 24 instructions
// fewer than sub_raw6 per use).  The top limb: b's is at most 2 x (3m - 1)'s (0x12259d6), and 8m's
// raised form keeps 0x1832270 there, so it stays >= 0 for every a (round 6, ADVICE r5: the 6m form's
// 0x12259d4 wrapped below zero for a ~ 0 against b ~ 6m; tools/hosttest r4lazy covers that quad)
template <class C>
ZDEV Fe<C> sub_raw8(const Fe<C>& a, const Fe<C>& b) { return borrow_sub(a, ZTAB(MOD8_B30), b); }

template <class C>
ZDEV Fe<C> dbl(const Fe<C>& a) { return add(a, a); }

template <class C>
ZDEV Fe<C> neg(const Fe<C>& a) { return sub(fe_zero<C>(), a); }

// canonical representative in [0, m) of a value < 2m
template <class C>
ZDEV Fe<C> canon(const Fe<C>& a) { return cond_sub(a, C::MOD); }

template <class C>
ZDEV bool is_zero_raw(const Fe<C>& a) {
  typename FeTypes<C>::limb o = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) o |= a.v[i];
  return o == 0;
}

// value (< 2m) congruent to 0 mod m
template <class C>
ZDEV bool is_zero(const Fe<C>& a) {
  typename FeTypes<C>::limb o = 0, q = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    o |= a.v[i];
    q |= a.v[i] ^ C::MOD[i];
  }
  return o == 0 || q == 0;
}

template <class C>
ZDEV bool eq(const Fe<C>& a, const Fe<C>& b) { return is_zero(sub(a, b)); }

// ---------------------------------------------------------------- storage conversions

// 8 x 32-bit words (value < 2^256) -> 9 x 29-bit limbs
template <class C>
ZDEV Fe<C> unpack(const uint32_t (&w)[8]) {
  Fe<C> r;
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const int bit = LB * k, j = bit >> 5, s = bit & 31;
    uint32_t lo = w[j] >> s;
    uint32_t hi = (j + 1 < 8 && s != 0) ? (w[j + 1] << (32 - s)) : 0u;
    r.v[k] = (k == NL - 1) ? (lo | hi) : ((lo | hi) & LMASK);
  }
  return r;
}

// 9 x 29-bit normalised limbs (value < 2^256) -> 8 x 32-bit words
template <class C>
ZDEV void pack(const Fe<C>& a, uint32_t (&w)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int bit = 32 * j, k = bit / LB, s = bit - LB * k;  // word starts s bits into limb k
    uint32_t x = a.v[k] >> s;
    if (k + 1 < NL) x |= a.v[k + 1] << (LB - s);
    if (k + 2 < NL && 2 * LB - s < 32) x |= a.v[k + 2] << (2 * LB - s);
    w[j] = x;
  }
}

template <class C>
ZDEV Fe<C> load_fe(const uint32_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return unpack<C>(w);
}

template <class C>
ZDEV void store_fe(uint32_t* p, const Fe<C>& x) {
  uint32_t w[8];
  pack(x, w);
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// standard integer (< 2^256) -> Montgomery(R') compute form
template <class C>
ZDEV Fe<C> to_mont(const Fe<C>& a) { return mul(a, fe_const<C>(C::R2)); }

// Montgomery(R') -> canonical standard integer (< m)
template <class C>
ZDEV Fe<C> from_mont(const Fe<C>& a) {
  Fe<C> one = fe_zero<C>();
  one.v[0] = 1;
  return canon(mul(a, one));
}

// a^(m-2) = a^-1 (Fermat), Montgomery form in and out; 0 -> 0.  Square-and-multiply
// over the fixed exponent: ~254 S + ~130 M.  Load-time only (base-table precompute).
template <class C>
ZDEV Fe<C> inv(const Fe<C>& a) {
  Fe<C> r = fe_one<C>();
  for (int wi = 7; wi >= 0; --wi) {
    const uint32_t e = C::MOD_W[wi] - (wi == 0 ? 2u : 0u);
    for (int b = 31; b >= 0; --b) {
      r = sqr(r);
      if ((e >> b) & 1u) r = mul(r, a);
    }
  }
  return r;
}

// ---------------------------------------------------------------- Fq2 = Fq[u]/(u^2+1)

// Written for any config of the base field (the kernels use Fq2 = Fq2T<FqCfg> only).
template <class C>
struct Fq2T {
  Fe<C> c0, c1;
};
using Fq2 = Fq2T<FqCfg>;

// 4m - a, normalised, for a normalised a <= 4m (Fq2 components are < 4m: rsub's); result <= 4m
template <class C>
ZDEV Fe<C> neg4(const Fe<C>& a) {
  return normalized(borrow_sub(fe_zero<C>(), ZTAB(MOD4_BORROW), a));
}

// (a0 + a1 u)(b0 + b1 u) = (a0 b0 - a1 b1) + (a0 b1 + a1 b0) u as two lazily reduced sums
// of products (2 x 162 + 2 x 81 mads, like Karatsuba's 3 x 162, but no Karatsuba adds and
// subtractions: ~650 instead of ~1100 instructions).  Components normalised, < 4m.
// The two components' sums of products are the two lanes of one mont_sop with chained columns: the
// 2-wave G2 kernels gain with paired chains (profiles/g2_chain_r03.txt).
template <class C>
ZDEV Fq2T<C> mul(const Fq2T<C>& a, const Fq2T<C>& b) {
  Fq2T<C> r;
  const Fe<C> nb1 = neg4(b.c1);
  mont_sop<C, true, 2, 2>({{&a.c0, &a.c1}, {&a.c0, &a.c1}}, {{&b.c0, &nb1}, {&b.c1, &b.c0}}, {&r.c0, &r.c1});
  return r;
}

// a*b + c*d in Fq2 with two lazily reduced four-product sums
template <class C>
ZDEV Fq2T<C> mul2(const Fq2T<C>& a, const Fq2T<C>& b, const Fq2T<C>& c, const Fq2T<C>& d) {
  Fq2T<C> r;
  const Fe<C> nb1 = neg4(b.c1), nd1 = neg4(d.c1);
  mont_sop<C, true, 2, 4>({{&a.c0, &a.c1, &c.c0, &c.c1}, {&a.c0, &a.c1, &c.c0, &c.c1}},
                          {{&b.c0, &nb1, &d.c0, &nd1}, {&b.c1, &b.c0, &d.c1, &d.c0}}, {&r.c0, &r.c1});
  return r;
}

template <class C>
ZDEV Fq2T<C> sqr(const Fq2T<C>& a) {
  // (a0 + a1 u)^2 = (a0+a1)(a0-a1) + 2 a0 a1 u
  Fq2T<C> r;
  r.c0 = mul(add(a.c0, a.c1), sub(a.c0, a.c1));
  Fe<C> t = mul(a.c0, a.c1);
  r.c1 = add(t, t);
  return r;
}

// ---- lazily reduced G2 accumulator forms (curve.hpp acc_*): every component normalised, value
// bounds as noted; the products stay < 2m as long as each Fq sum of products of a Fq2 mul/mul2
// (neg4 on the second operand's c1, which must be <= 4m) stays below ~169 m^2.
// a - b + 2m per component for a, b < 2m: < 4m, no conditional subtraction
template <class C>
ZDEV Fq2T<C> lsub2_lazy(const Fq2T<C>& a, const Fq2T<C>& b) { return Fq2T<C>{lsub(a.c0, b.c0), lsub(a.c1, b.c1)}; }
// a - b + 4m per component for a < 2m, b < 4m: < 6m
template <class C>
ZDEV Fq2T<C> lsub4_lazy(const Fq2T<C>& a, const Fq2T<C>& b) { return Fq2T<C>{lsub4(a.c0, b.c0), lsub4(a.c1, b.c1)}; }
// a^2 for components < 6m: (a0 + a1)(a0 - a1 + 6m) [raw sum x normalised, < 144 m^2] and
// (2 a0) a1 [raw x normalised, < 72 m^2] -- no additions reduced, no doubling of the product
template <class C>
ZDEV Fq2T<C> sqr_lazy(const Fq2T<C>& a) {
  const Fe<C> s = add_raw(a.c0, a.c1), d = lsub6(a.c0, a.c1), t = shl1_raw(a.c0);
  Fq2T<C> r;
  mont_sop<C, true, 2, 1>({{&s}, {&t}}, {{&d}, {&a.c1}}, {&r.c0, &r.c1});
  return r;
}
// R^2 - PPP - 2Q per component (each < 2m) -> < 4m: one conditional subtraction instead of two.
// (Not qreduce: its single 27-deep dependent chain per component measured 6 % slower in the
// G2 accumulation, which runs at two waves per SIMD and cannot hide the latency.)
template <class C>
ZDEV Fq2T<C> sub_2x4(const Fq2T<C>& a, const Fq2T<C>& b, const Fq2T<C>& c) {
  return Fq2T<C>{cond_sub(sub_2x8(a.c0, b.c0, c.c0), C::MOD4), cond_sub(sub_2x8(a.c1, b.c1, c.c1), C::MOD4)};
}
// components < 4m -> < 2m
template <class C>
ZDEV Fq2T<C> canon4(const Fq2T<C>& a) { return Fq2T<C>{cond_sub(a.c0, C::MOD2), cond_sub(a.c1, C::MOD2)}; }

template <class C>
ZDEV Fq2T<C> add(const Fq2T<C>& a, const Fq2T<C>& b) { return Fq2T<C>{add(a.c0, b.c0), add(a.c1, b.c1)}; }
// The generic (non-accumulator) lazy names on Fq2, as the doubling formulas of curve.hpp use them.
// An Fq2 mul() / mul2() is a sum of several products per component, so EVERY operand must be
// normalised (no raw operand as in the one-product Fq mul), and neg4 wants the second operand's c1
// <= 4m: rsub is therefore the normalised lsub per component (< 4m).  sqr() reduces its operand's
// components with add() / sub(), which take values < 2m: lsub is the fully reduced sub.
template <class C>
ZDEV Fq2T<C> sub_2x(const Fq2T<C>& a, const Fq2T<C>& b, const Fq2T<C>& c) {
  return Fq2T<C>{sub_2x(a.c0, b.c0, c.c0), sub_2x(a.c1, b.c1, c.c1)};
}
template <class C>
ZDEV Fq2T<C> lsub(const Fq2T<C>& a, const Fq2T<C>& b) { return Fq2T<C>{sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
template <class C>
ZDEV Fq2T<C> rsub(const Fq2T<C>& a, const Fq2T<C>& b) { return Fq2T<C>{lsub(a.c0, b.c0), lsub(a.c1, b.c1)}; }
template <class C>
ZDEV Fq2T<C> sub(const Fq2T<C>& a, const Fq2T<C>& b) { return Fq2T<C>{sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
template <class C>
ZDEV Fq2T<C> dbl(const Fq2T<C>& a) { return add(a, a); }
template <class C>
ZDEV bool is_zero(const Fq2T<C>& a) { return is_zero(a.c0) && is_zero(a.c1); }
template <class C>
ZDEV bool is_zero_raw(const Fq2T<C>& a) { return is_zero_raw(a.c0) && is_zero_raw(a.c1); }
// (c0 + c1 u)^-1 = (c0 - c1 u) / (c0^2 + c1^2)
template <class C>
ZDEV Fq2T<C> inv(const Fq2T<C>& a) {
  const Fe<C> t = inv(add(sqr(a.c0), sqr(a.c1)));
  return Fq2T<C>{mul(a.c0, t), mul(sub(fe_zero<C>(), a.c1), t)};
}

}  // namespace zkp
