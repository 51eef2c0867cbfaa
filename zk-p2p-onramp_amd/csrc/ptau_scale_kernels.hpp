// Per-lane bodies of `powersoftau contribute` / `beacon` (ptau_contribute.hip): __host__ __device__ so that
// tools/hosttest/ptau_scale_emu.cpp can replay them on the CPU.
//
//   out_j = (base * ratio^j) * P_j,   j = the point's index inside the launch (j < 2^POW_BITS)
//
// base = first * ratio^(chunk start) and the table ratio^(2^b), b < POW_BITS, come from the host
// (fill_powers, with the device's field code); a lane multiplies the entries of j's set bits, at most
// POW_BITS - 1 Fr products beside the ~380 group operations of its ladder (gfft::scale).  The scalars differ
// from lane to lane, so the ladder's additions are lane-divergent; gfft_kernels.hpp says what the 2-bit
// window buys there.  The result goes to affine with one inversion per point and leaves as up to three byte
// streams (encode): the zkey layout of the file, the "uncompressed" form of the next-challenge hash and the
// compressed form of the partial hash.
#pragma once
#include "gfft_kernels.hpp"

namespace zkp {
namespace pscale {

constexpr int POW_BITS = 28;  // a launch covers at most 2^28 points

// A launch's constants, passed by value as a kernel argument.  Fr entries: Montgomery form, canonical.
struct alignas(16) Powers {
  uint32_t base[8];
  uint32_t pw[POW_BITS][8];  // ratio^(2^b)
  uint32_t to_zkey[8];       // 2^256 mod q as raw words: device Montgomery form -> the zkey's
};

inline void put_fr(uint32_t (&o)[8], const Fr& a_mont) { pack(canon(a_mont), o); }

inline void fill_to_zkey(uint32_t (&o)[8]) {
  const uint32_t top[8] = {0, 0, 0, 0, 0, 0, 0, 0x80000000u};  // 2^255
  const Fq a = to_mont(unpack<FqCfg>(top));
  pack(from_mont(add(a, a)), o);
}

// first, ratio: standard form, below r.  start: the index in its section of the launch's point 0.
inline void fill_powers(Powers& p, const uint32_t (&first)[8], const uint32_t (&ratio)[8], uint64_t start) {
  Fr r = to_mont(unpack<FrCfg>(ratio)), b = to_mont(unpack<FrCfg>(first));
  for (int i = 0; i < 64; ++i) {
    if (i < POW_BITS) put_fr(p.pw[i], r);
    if ((start >> i) & 1) b = mul(b, r);
    r = mul(r, r);
  }
  put_fr(p.base, b);
  fill_to_zkey(p.to_zkey);
}

// base * ratio^j in standard form
ZDEV void lane_scalar(const Powers& p, size_t j, uint32_t (&s)[8]) {
  Fr t = load_fe<FrCfg>(p.base);
#pragma unroll
  for (int b = 0; b < POW_BITS; ++b)
    if ((j >> b) & 1) t = mul(t, load_fe<FrCfg>(p.pw[b]));
  gfft::fr_words(t, s);
}

// point j of the launch times its scalar.  Infinity stays infinity, a zero scalar gives infinity, 1 and
// r - 1 take gfft::scale's short cuts, everything else its ladder on the complete XYZZ formulas.
template <class F, int WB>
ZDEV Xyzz<F> scale_lane(const uint32_t* in, const Powers& p, size_t j) {
  uint32_t s[8];
  lane_scalar(p, j, s);
  return gfft::scale<WB>(gfft::load_point<F>(in, j), s);
}

// ---------------------------------------------------------------- the three encodings

ZDEV uint32_t bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

ZDEV void store8(uint32_t* o, const uint32_t (&w)[8]) {
  uint4* q = reinterpret_cast<uint4*>(o);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// 32 bytes big-endian of the value in w (LE words); flag goes into the first byte (its top bits are free:
// the value is below p < 2^254)
ZDEV void store8_be(uint32_t* o, const uint32_t (&w)[8], uint32_t flag) {
  uint32_t b[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) b[k] = bswap32(w[7 - k]);
  b[0] |= flag;
  store8(o, b);
}
ZDEV void store_zero(uint32_t* o, int words, uint32_t first_byte) {
  uint4* q = reinterpret_cast<uint4*>(o);
  for (int k = 0; k < words / 4; ++k) q[k] = make_uint4(k == 0 ? first_byte : 0u, 0u, 0u, 0u);
}

// a standard-form coordinate above (p - 1) / 2: "the greater root" of ffjavascript's compressed points
ZDEV bool above_half(const uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 7; i >= 0; --i) {
    const uint32_t h = (FqCfg::MOD_W[i] >> 1) | (i < 7 ? FqCfg::MOD_W[(i + 1) & 7] << 31 : 0u);
    if (w[i] != h) return w[i] > h;
  }
  return false;
}
ZDEV bool is_zero8(const uint32_t (&w)[8]) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= w[i];
  return o == 0;
}

struct Coord {
  uint32_t zk[8], st[8];  // Montgomery 2^256 and standard form, both canonical, LE words
};
ZDEV Coord coord(const Fq& a, const Fq& conv) {
  Coord c;
  pack(canon(mul(a, conv)), c.zk);
  pack(from_mont(a), c.st);
  return c;
}

constexpr uint32_t FLAG_INF = 0x40u, FLAG_GREATER = 0x80u;

// The affine point a (device Montgomery form; inf: the point at infinity) as point idx of each stream that
// is asked for (a null stream is skipped):
//   lem  zkey layout, 2 W words: Montgomery 2^256 little-endian, all-zero for infinity
//   u    uncompressed, 2 W words: big-endian standard form, x then y (G2: c1 before c0); 0x40 then zeros
//   c    compressed, W words: big-endian x, 0x80 in the first byte when y is the greater root (G2: of c1,
//        or of c0 when c1 is zero); 0x40 then zeros
ZDEV void encode(const Aff<Fq>& a, bool inf, const uint32_t (&to_zkey)[8], uint32_t* lem, uint32_t* u, uint32_t* c,
                 size_t idx) {
  if (lem) lem += idx * 16;
  if (u) u += idx * 16;
  if (c) c += idx * 8;
  if (inf) {
    if (lem) store_zero(lem, 16, 0);
    if (u) store_zero(u, 16, FLAG_INF);
    if (c) store_zero(c, 8, FLAG_INF);
    return;
  }
  const Fq conv = load_fe<FqCfg>(to_zkey);
  const Coord x = coord(a.x, conv), y = coord(a.y, conv);
  if (lem) store8(lem, x.zk), store8(lem + 8, y.zk);
  if (u) store8_be(u, x.st, 0), store8_be(u + 8, y.st, 0);
  if (c) store8_be(c, x.st, above_half(y.st) ? FLAG_GREATER : 0u);
}

ZDEV void encode(const Aff<Fq2>& a, bool inf, const uint32_t (&to_zkey)[8], uint32_t* lem, uint32_t* u, uint32_t* c,
                 size_t idx) {
  if (lem) lem += idx * 32;
  if (u) u += idx * 32;
  if (c) c += idx * 16;
  if (inf) {
    if (lem) store_zero(lem, 32, 0);
    if (u) store_zero(u, 32, FLAG_INF);
    if (c) store_zero(c, 16, FLAG_INF);
    return;
  }
  const Fq conv = load_fe<FqCfg>(to_zkey);
  const Coord x0 = coord(a.x.c0, conv), x1 = coord(a.x.c1, conv), y0 = coord(a.y.c0, conv), y1 = coord(a.y.c1, conv);
  if (lem) store8(lem, x0.zk), store8(lem + 8, x1.zk), store8(lem + 16, y0.zk), store8(lem + 24, y1.zk);
  if (u) store8_be(u, x1.st, 0), store8_be(u + 8, x0.st, 0), store8_be(u + 16, y1.st, 0), store8_be(u + 24, y0.st, 0);
  if (c) {
    const bool greater = is_zero8(y1.st) ? above_half(y0.st) : above_half(y1.st);
    store8_be(c, x1.st, greater ? FLAG_GREATER : 0u);
    store8_be(c + 8, x0.st, 0);
  }
}

// the ladder's result
template <class F>
ZDEV void encode_xyzz(const Xyzz<F>& p, const uint32_t (&to_zkey)[8], uint32_t* lem, uint32_t* u, uint32_t* c, size_t idx) {
  encode(xyzz_to_aff(p), xyzz_is_inf(p), to_zkey, lem, u, c, idx);
}

// point idx of a zkey-layout array (canonical, as the file holds it)
template <class F>
ZDEV void encode_lem(const uint32_t* in, const uint32_t (&to_zkey)[8], uint32_t* lem, uint32_t* u, uint32_t* c, size_t idx) {
  const Xyzz<F> p = gfft::load_point<F>(in, idx);
  Aff<F> a;
  a.x = p.x;
  a.y = p.y;
  encode(a, xyzz_is_inf(p), to_zkey, lem, u, c, idx);
}

}  // namespace pscale
}  // namespace zkp
