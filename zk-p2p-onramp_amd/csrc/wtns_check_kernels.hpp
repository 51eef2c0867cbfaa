// Per-lane bodies of `wtns check` (wtns_check.hip): __host__ __device__ so that
// tools/hosttest/wtns_check_emu.cpp can replay a launch lane by lane on the CPU.
//
// The matrix: one CSR over 3 n rows, row 3c + m = matrix m (A, B, C) of constraint c; val holds
// coef * 2^522 (8 words per term, below 2m), the witness standard-form values below r (8 words per
// signal).  mul(val, w) = coef w 2^261, the Montgomery form of the term, so ev(row) is the Montgomery
// form of the row's sum and mul(ev(A), ev(B)) that of the product: constraint c holds iff
// mul(ev(A), ev(B)) == ev(C) modulo r.  Every value here is a lazily reduced representative (below 2m;
// Fr's add gives below 1.2m), so the comparison is the field's eq (is_zero of the difference), never limb
// by limb.  Only the field's own operations inside their documented bounds: add(<2m, <2m), mul(<2m, <r),
// eq(<2m, <2m); no raw sums, nothing new for tools/hosttest/bounds.cpp.
//
// Two paths, chosen per constraint on the host by its total term count (wtns_check.hip LONG_TERMS):
//   short  one lane per constraint: the three rows one after the other (lane_dot with stride 1)
//   long   one wavefront per constraint: lane l takes terms l, l + 64, ... of each row (however long
//          the row: the stride loop runs until the row ends), the 64 partial sums meet in a butterfly
//          of 6 exchanges (pair_sum; on the device the nine limbs travel by cross-lane shuffles), and
//          every lane ends with the row's sum; lane 0 does the product and the comparison.
// A failing constraint sets its bit in a bitmap (an atomic OR on the device: commutative, so the
// bitmap does not depend on the order of the lanes); collect_word turns the bitmap into the count and the
// lowest failing indices in ascending order.
#pragma once
#include "field.hpp"

namespace zkp {
namespace wcheck {

constexpr int WAVE = 64;
constexpr int MAX_LISTED = 16;  // zkp_check_result::bad

// what the device hands back (one struct, reset per check)
struct Outcome {
  uint32_t n_bad;              // failing constraints
  uint32_t n_listed;           // min(MAX_LISTED, n_bad)
  uint32_t bad[MAX_LISTED];    // the lowest failing indices, ascending
  uint32_t first_unreduced;    // lowest signal with a value >= r (0xffffffff: none)
  uint32_t w0_not_one;         // signal 0 is not 1
};
constexpr uint32_t NONE = 0xffffffffu;

// terms first, first + stride, ... (below end) of a row against the witness.  Every col[e] is below
// the witness's length: the parser checked it, and nothing else indexes w.
ZDEV Fr lane_dot(const uint32_t* __restrict__ col, const uint32_t* __restrict__ val, const uint32_t* __restrict__ w,
                 uint32_t first, uint32_t end, uint32_t stride) {
  Fr acc = fe_zero<FrCfg>();
  // first + stride may pass 2^32 in a matrix of close to 2^32 terms: count in 64 bits
  for (uint64_t e = first; e < end; e += stride)
    acc = add(acc, mul(load_fe<FrCfg>(val + (size_t)e * 8), load_fe<FrCfg>(w + (size_t)col[e] * 8)));
  return acc;
}

// one step of the butterfly: a lane's partial sum and its partner's
ZDEV Fr pair_sum(const Fr& mine, const Fr& other) { return add(mine, other); }

// the final test: ev(A) ev(B) == ev(C) modulo r
ZDEV bool satisfied(const Fr& a, const Fr& b, const Fr& c) { return eq(mul(a, b), c); }

// the short path's whole lane: constraint c fails
ZDEV bool short_lane_fails(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col,
                           const uint32_t* __restrict__ val, const uint32_t* __restrict__ w, uint32_t c) {
  const uint32_t* rp = rowptr + (size_t)c * 3;
  const Fr a = lane_dot(col, val, w, rp[0], rp[1], 1);
  const Fr b = lane_dot(col, val, w, rp[1], rp[2], 1);
  const Fr cc = lane_dot(col, val, w, rp[2], rp[3], 1);
  return !satisfied(a, b, cc);
}

// the long path's lane before the butterfly: its partial sum of row m of constraint c
ZDEV Fr long_lane_partial(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col,
                          const uint32_t* __restrict__ val, const uint32_t* __restrict__ w, uint32_t c, int m,
                          uint32_t lane) {
  const uint32_t* rp = rowptr + (size_t)c * 3 + m;
  // rp[0] + lane <= 2^32 - 1 + 63 does not fit 32 bits either
  const uint64_t first = (uint64_t)rp[0] + lane;
  return first < rp[1] ? lane_dot(col, val, w, (uint32_t)first, rp[1], WAVE) : fe_zero<FrCfg>();
}

// a witness value (8 LE words, standard form) is not below r
ZDEV bool not_reduced(const uint32_t* __restrict__ v) {
#pragma unroll
  for (int i = 7; i >= 0; --i)
    if (v[i] != FrCfg::MOD_W[i]) return v[i] > FrCfg::MOD_W[i];
  return true;
}
ZDEV bool is_one(const uint32_t* __restrict__ v) {
  uint32_t o = v[0] ^ 1u;
#pragma unroll
  for (int i = 1; i < 8; ++i) o |= v[i];
  return o == 0;
}

// word `index` of the fail bitmap (constraints 32 index .. 32 index + 31), `before` failing constraints
// below it: its set bits into the list at their ranks, while the list has room
ZDEV void collect_word(uint32_t word, uint32_t index, uint32_t before, uint32_t* bad) {
  for (uint32_t k = before; word && k < (uint32_t)MAX_LISTED; ++k) {
    uint32_t bit = 0;
    while (!((word >> bit) & 1u)) ++bit;
    bad[k] = index * 32u + bit;
    word &= word - 1u;
  }
}
ZDEV uint32_t popcount32(uint32_t x) {
  x = x - ((x >> 1) & 0x55555555u);
  x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
  return (((x + (x >> 4)) & 0x0f0f0f0fu) * 0x01010101u) >> 24;
}

}  // namespace wcheck
}  // namespace zkp
