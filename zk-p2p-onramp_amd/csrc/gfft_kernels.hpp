// Per-thread bodies of the group FFT (ptau_prepare.hip), both directions: __host__ __device__ so that
// tools/hosttest/gfft_emu.cpp can replay the launches on the CPU.
//
//   inverse:  out_c = n^-1 * sum_j w^(-c j) * P_j,   n = 2^p, w = Fr.w[p]   (natural order in and out)
//   forward:  out_c =        sum_j w^(+c j) * P_j    (the same schedule with the twiddles w_(2m)^+k and no
//             n^-1 stage; `zkey export bellman`, zkey_bellman.hip, takes section 9 through it)
//
// Radix-2 decimation in time over XYZZ points: the loads read the input in bit-reversed order, stage
// s < p (half-length m = 2^s) pairs positions lo = (i >> s << s + 1) | k and lo + m, k = i mod m, with
// the twiddle t = w_(2m)^-k, and replaces (a, b) by (a + t b, a - t b).  The factor n^-1 rides on the
// last stage (s = p - 1), which computes (n^-1 a) +- (n^-1 t) b: n / 2 more scalar multiplications
// per level, where a pass of its own over the result would take n.
//
// The twiddles are not stored per position.  A table of 58 entries of 8 words (standard form) serves
// every level: entry i < 28 is w_28^-(2^i), so w_(2m)^-(2^j) = entry[j + 27 - s] whatever the level,
// and a thread multiplies the entries of k's set bits (at most 27 Fr products beside the ~380 group
// operations of its butterfly); entry 28 + p is 2^-p; entry 57 is 2^256 mod q, the factor from the
// device's Montgomery form to the zkey's; entries 58 + i, i < 28, are w_28^+(2^i), the forward direction's.
#pragma once
#include "curve.hpp"

namespace zkp {
namespace gfft {

constexpr int TW_ROOT = 28;                    // the table's root of unity: Fr.w[28]
constexpr int TW_NINV = TW_ROOT;               // entry TW_NINV + p = 2^-p, p <= 28
constexpr int TW_TO_ZKEY = TW_ROOT + 29;       // 2^256 mod q
constexpr int TW_FWD = TW_TO_ZKEY + 1;          // entry TW_FWD + i = w_28^(2^i), i < 28
constexpr int TW_ENTRIES = TW_FWD + TW_ROOT;
constexpr int MAX_LOG_N = TW_ROOT;

// Points of one level that one workgroup transforms in LDS (64 KB of XYZZ points: 512 G1, 256 G2),
// one butterfly per thread and stage
template <class F>
struct Geom {
  static constexpr int W = FWords<F>::W;
  static constexpr int LG = W == 8 ? 9 : 8;
  static constexpr int TILE = 1 << LG;
  static constexpr int TPB = TILE / 2;
  static constexpr int LDS_WORDS = TILE * 4 * W;
};

// ---------------------------------------------------------------- index and twiddle schedule

ZDEV size_t brev(size_t i, int p) {  // the low p bits of i reversed
  size_t r = 0;
  for (int b = 0; b < p; ++b) {
    r = (r << 1) | (i & 1);
    i >>= 1;
  }
  return r;
}

// butterfly i of stage s: positions lo and lo + 2^s, twiddle exponent k
ZDEV void pair_of(int s, size_t i, size_t& lo, size_t& k) {
  const size_t m = (size_t)1 << s;
  k = i & (m - 1);
  lo = ((i >> s) << (s + 1)) | k;
}

ZDEV Fr tw_entry(const uint32_t* tw, int e) { return to_mont(load_fe<FrCfg>(tw + (size_t)e * 8)); }

ZDEV void fr_words(const Fr& a_mont, uint32_t (&w)[8]) { pack(from_mont(a_mont), w); }

// The scalars of butterfly k of stage s of level p, standard form: b takes tb, and a takes ta where
// scale_a (the last stage: ta = 2^-p, tb = 2^-p w_(2m)^-k); elsewhere tb = w_(2m)^-k.  fwd: tb = w_(2m)^+k
// in every stage, and no stage scales a.
ZDEV void twiddles(const uint32_t* tw, int p, int s, size_t k, uint32_t (&ta)[8], uint32_t (&tb)[8], bool& scale_a,
                   bool fwd = false) {
  Fr t = fe_one<FrCfg>();
  const int root = fwd ? TW_FWD : 0;
  for (int j = 0; j < s; ++j)
    if ((k >> j) & 1) t = mul(t, tw_entry(tw, root + j + TW_ROOT - 1 - s));
  scale_a = !fwd && s == p - 1;
  if (scale_a) {
    const Fr ninv = tw_entry(tw, TW_NINV + p);
    t = mul(t, ninv);
    fr_words(ninv, ta);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) ta[i] = i == 0 ? 1u : 0u;
  }
  fr_words(t, tb);
}

// The table (TW_ENTRIES x 8 words), computed on the host with the device's field code.
inline void fill_table(uint32_t* tw) {
  auto put = [&](int e, const Fr& a_mont) {
    uint32_t w[8];
    fr_words(a_mont, w);
    for (int i = 0; i < 8; ++i) tw[(size_t)e * 8 + i] = w[i];
  };
  uint32_t rw[8];
  for (int i = 0; i < 8; ++i) rw[i] = FR_ROOTS_W[TW_ROOT][i];
  Fr f = to_mont(unpack<FrCfg>(rw)), g = inv(f);
  for (int i = 0; i < TW_ROOT; ++i) {
    put(i, g);
    put(TW_FWD + i, f);
    g = mul(g, g);
    f = mul(f, f);
  }
  const uint32_t two[8] = {2, 0, 0, 0, 0, 0, 0, 0};
  const Fr half = inv(to_mont(unpack<FrCfg>(two)));
  Fr h = fe_one<FrCfg>();
  for (int p = 0; p <= 28; ++p) {
    put(TW_NINV + p, h);
    h = mul(h, half);
  }
  const uint32_t top[8] = {0, 0, 0, 0, 0, 0, 0, 0x80000000u};  // 2^255
  const Fq a = to_mont(unpack<FqCfg>(top));
  uint32_t w[8];
  pack(from_mont(add(a, a)), w);
  for (int i = 0; i < 8; ++i) tw[(size_t)TW_TO_ZKEY * 8 + i] = w[i];
}

// ---------------------------------------------------------------- scalar multiplication, butterfly

ZDEV bool scalar_is_one(const uint32_t (&t)[8]) {
  uint32_t o = t[0] ^ 1u;
#pragma unroll
  for (int i = 1; i < 8; ++i) o |= t[i];
  return o == 0;
}
ZDEV bool scalar_is_minus_one(const uint32_t (&t)[8]) {  // r - 1
  uint32_t o = t[0] ^ (FrCfg::MOD_W[0] - 1u);
#pragma unroll
  for (int i = 1; i < 8; ++i) o |= t[i] ^ FrCfg::MOD_W[i];
  return o == 0;
}

// -y of an XYZZ coordinate in any of the accumulator's lazy forms (< 8m per component): below 2m
template <class C>
ZDEV Fe<C> neg_lazy(const Fe<C>& a) { return sub(fe_zero<C>(), canon8(a)); }
template <class C>
ZDEV Fq2T<C> neg_lazy(const Fq2T<C>& a) { return Fq2T<C>{neg_lazy(a.c0), neg_lazy(a.c1)}; }

template <class F>
ZDEV Xyzz<F> negated(Xyzz<F> p) {  // infinity (ZZ = 0) stays infinity
  p.y = neg_lazy(p.y);
  return p;
}

// t * b for a standard-form scalar t < r held in registers: 1 and -1 without a loop, else left to right
// from t's top set digit (the words shift left, so no word is indexed by a run-time value).
// WB = 1: double-and-add, one bit per step.  WB = 2: the digits 1..3 from a table {b, 2b, 3b} in
// registers, two doublings and at most one addition per step.
// The twiddles differ from lane to lane, so the additions are LANE-DIVERGENT: a wave spends an addition
// in every step in which any of its lanes has a nonzero digit -- with 64 lanes, nearly every step.  That
// is what the window buys: per two bits a wave pays two doublings and one addition instead of two and two.
template <int WB, class F>
ZDEV Xyzz<F> scale(const Xyzz<F>& b, const uint32_t (&t)[8]) {
  static_assert(WB == 1 || WB == 2, "window of 1 or 2 bits");
  if (xyzz_is_inf(b) || scalar_is_one(t)) return b;
  if (scalar_is_minus_one(t)) return negated(b);
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = t[i];
  auto shl = [&] {
#pragma unroll
    for (int i = 7; i > 0; --i) w[i] = (w[i] << WB) | (w[i - 1] >> (32 - WB));
    w[0] <<= WB;
  };
  int left = 256 / WB;
  while (left > 0 && !(w[7] >> (32 - WB))) {
    shl();
    --left;
  }
  Xyzz<F> acc = xyzz_inf<F>();
  if constexpr (WB == 1) {
    for (; left > 0; --left) {
      acc = xyzz_dbl(acc);
      if (w[7] >> 31) xyzz_add(acc, b);
      shl();
    }
  } else {
    const Xyzz<F> b2 = xyzz_dbl(b);
    Xyzz<F> b3 = b2;
    xyzz_add(b3, b);
    for (; left > 0; --left) {
      acc = xyzz_dbl(xyzz_dbl(acc));
      const uint32_t d = w[7] >> 30;
      if (d) xyzz_add(acc, d == 1 ? b : d == 2 ? b2 : b3);
      shl();
    }
  }
  return acc;
}

// (a, b) <- (ta a + tb b, ta a - tb b); ta = 1 unless scale_a.  The additions are the complete
// xyzz_add: either side at infinity, ta a = tb b (a doubling) and ta a = -tb b (infinity) all occur
// (stage 0 of a constant vector meets the last two in every butterfly).
template <int WB, class F>
ZDEV void butterfly(Xyzz<F>& a, Xyzz<F>& b, const uint32_t (&ta)[8], const uint32_t (&tb)[8], bool scale_a) {
  const Xyzz<F> v = scale<WB>(b, tb);
  const Xyzz<F> u = scale_a ? scale<WB>(a, ta) : a;
  a = u;
  xyzz_add(a, v);
  b = u;
  xyzz_add(b, negated(v));
}

// ---------------------------------------------------------------- per-thread bodies of the launches

// point idx of a zkey-layout array (affine, Montgomery 2^256; all-zero = infinity) as a device XYZZ
template <class F>
ZDEV Xyzz<F> load_point(const uint32_t* in, size_t idx) {
  Aff<F> a = load_aff<F>(in, idx);
  if (aff_is_inf(a)) return xyzz_inf<F>();
  const Fq conv = fe_const<FqCfg>(Conv::FQ_ZKEY_TO_DEV);
  Xyzz<F> r;
  if constexpr (FWords<F>::W == 8) {
    r.x = mul(a.x, conv);
    r.y = mul(a.y, conv);
  } else {
    r.x = F{mul(a.x.c0, conv), mul(a.x.c1, conv)};
    r.y = F{mul(a.y.c0, conv), mul(a.y.c1, conv)};
  }
  r.zz = f_one<F>();
  r.zzz = f_one<F>();
  return r;
}

// butterfly i of stage s of level p on the XYZZ points at buf: a workgroup's tile in LDS (i counts
// inside the tile; the twiddle depends on i mod 2^s only, so it is the same in every tile) or the
// level's vector in HBM.  fwd: the forward transform's stage (twiddles)
template <class F, int WB>
ZDEV void stage(uint32_t* buf, const uint32_t* tw, int p, int s, size_t i, bool fwd = false) {
  size_t lo, k;
  pair_of(s, i, lo, k);
  const size_t hi = lo + ((size_t)1 << s);
  uint32_t ta[8], tb[8];
  bool scale_a;
  twiddles(tw, p, s, k, ta, tb, scale_a, fwd);
  Xyzz<F> a = load_xyzz<F>(buf, lo), b = load_xyzz<F>(buf, hi);
  butterfly<WB>(a, b, ta, tb, scale_a);
  store_xyzz(buf, lo, a);
  store_xyzz(buf, hi, b);
}

// result point -> affine, zkey layout, at out[idx]
template <class F>
ZDEV void finish(const Xyzz<F>& p, const uint32_t* tw, uint32_t* out, size_t idx) {
  constexpr int W = FWords<F>::W;
  Aff<F> a = xyzz_to_aff(p);  // infinity -> (0, 0)
  if (!xyzz_is_inf(p)) {
    const Fq conv = load_fe<FqCfg>(tw + (size_t)TW_TO_ZKEY * 8);
    if constexpr (W == 8) {
      a.x = canon(mul(a.x, conv));
      a.y = canon(mul(a.y, conv));
    } else {
      a.x = F{canon(mul(a.x.c0, conv)), canon(mul(a.x.c1, conv))};
      a.y = F{canon(mul(a.y.c0, conv)), canon(mul(a.y.c1, conv))};
    }
  }
  store_aff(out, idx, a);
}

}  // namespace gfft
}  // namespace zkp
