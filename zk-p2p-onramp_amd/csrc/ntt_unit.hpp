// The arithmetic of the NTT's butterfly units (ntt.hip dft_stages), apart from their LDS addressing.
//
// Each unit is ONE text, a macro body over the names of its inputs, with three hooks:
//   RMP(a, ja, c, jc, r, s)   r = a w^ja, s = c w^jc: a lockstep pair of Shoup products by stage roots
//   RM1(a, j)                 a w^j alone
//   PUT(k, y)                 output k of the unit
// ntt.hip expands the bodies inside its kernels, with its LDS root table and its addresses behind the
// hooks.  The functions below expand the same bodies for callers that bring their own roots: the host
// tests (tools/hosttest: field_host.cpp op r4lazy, and bounds.cpp, which proves the value bounds
// quoted here for every input).  Why macros and not calls of these functions from the
// kernels: the call form compiles to the same instructions in another order, with 2 more VGPRs, and
// that takes k_ntt<2, 0> from 3 waves per SIMD to 2 (170 VGPRs against 168).
//
// Every tile value between rounds is normalised (limbs < 2^29) and < 3m: Shoup outputs are < 3m,
// qreduce outputs < 1.2m.
#pragma once
#include "field.hpp"

namespace zkp {

// x - y for stage values (Shoup products: < 3m)
template <class F>
ZDEV F stage_sub(const F& x, const F& y) { return sub4(x, y); }

// One radix-4 unit on x0..x3 (F values; also in scope: uint32_t i, Hh; int t; bool raw): stage t
// (span H = 2 Hh) on (x0, x2) with w_(2H)^i and on (x1, x3) with w_(2H)^(i + H/2), then stage t+1
// (span H/2) on the sums and on the differences, both with w_H^i.  Roots as exponents of w_(2^b)
// (stage t: i << t).
// The first-stage sums stay raw (< 6m, limbs < 2^30); their difference takes the 2^30-raised 8m borrow
// form without a carry pass (sub_raw8: limbs < 2.5 * 2^30, < 14m), a mul_shoup operand.  The unit's
// independent root products run in lockstep pairs (d02 / d13, then y1 / y3 by the same root); inside
// a round every lane multiplies (w^0 = 1 for i = 0: no divergent j == 0 path).  The last pair of a
// DFT (Hh == 1, a round-uniform branch; odd b too, dft_stages) has i = 0 for every lane: stage t's
// first difference takes w^0 = 1 and is only reduced (qreduce: < 1.2m, ~43 instructions instead of
// half a lockstep Shoup pair).  RAW: the unit is the last one of a DFT whose outputs only feed a
// Montgomery product (the DIF pass's inter-pass twiddle, the coset key between the fused kernel's two
// DFTs): its four outputs stay unreduced (limbs < 2^31; values < 12m, < 14m, < 6m, < 7m), each a
// mul() operand against the normalised table value < 2m (at most 28 m^2, far below the 169 m^2 that
// keeps a product < 2m, field.hpp mont_sop): 4 reductions fewer.  Otherwise the last pair's outputs
// are stored with one reduction each.
#define ZKP_NTT_R4(F, RMP, RM1, PUT)                                         \
  const uint32_t j = i << (t + 1);                                           \
  F d02, d13;                                                                \
  if (Hh > 1) {                                                              \
    RMP(rsub(x0, x2), i << t, rsub(x1, x3), (i + Hh) << t, d02, d13);        \
  } else {                                                                   \
    d02 = qreduce(rsub(x0, x2));                                             \
    d13 = RM1(rsub(x1, x3), 1u << t);                                        \
  }                                                                          \
  const F s02 = add_raw(x0, x2), s13 = add_raw(x1, x3);                      \
  if (Hh > 1) {                                                              \
    PUT(0, add_raw_reduce(s02, s13));                                        \
    F y1, y3;                                                                \
    RMP(sub_raw8(s02, s13), j, rsub(d02, d13), j, y1, y3);                   \
    PUT(1, y1);                                                              \
    PUT(3, y3);                                                              \
    PUT(2, add(d02, d13));                                                   \
  } else if (raw) {                                                          \
    PUT(0, add_raw(s02, s13));                                               \
    PUT(1, sub_raw8(s02, s13));                                              \
    PUT(2, add_raw(d02, d13));                                               \
    PUT(3, rsub(d02, d13));                                                  \
  } else {                                                                   \
    PUT(0, add_raw_reduce(s02, s13));                                        \
    PUT(1, qreduce(sub_raw8(s02, s13)));                                     \
    PUT(2, add(d02, d13));                                                   \
    PUT(3, stage_sub(d02, d13));                                             \
  }

// An odd b's lone radix-2 stage, which goes first (span 2^(b-1), roots w_(2^b)^r): x0 + x1 and
// (x0 - x1) w^ra; outputs < 1.2m (qreduce) and < 3m (Shoup), normalised.  PAIR: with a second
// butterfly (y0, y1, rc) in lockstep, outputs 0..3; ONE: alone, outputs 0 and 1.
#define ZKP_NTT_R2_FIRST_PAIR(F, RMP, PUT)                   \
  F u, v;                                                    \
  RMP(rsub(x0, x1), ra, rsub(y0, y1), rc, u, v);             \
  PUT(0, add(x0, x1));                                       \
  PUT(1, u);                                                 \
  PUT(2, add(y0, y1));                                       \
  PUT(3, v);
#define ZKP_NTT_R2_FIRST_ONE(RM1, PUT) \
  PUT(1, RM1(rsub(x0, x1), ra));       \
  PUT(0, add(x0, x1));

// b == 1: the one radix-2 stage on (x, y) (span 1: the root is w_2^0 = 1).  raw: < 6m and < 7m,
// into a Montgomery product
#define ZKP_NTT_R2_LAST(PUT)     \
  if (raw) {                     \
    PUT(0, add_raw(x, y));       \
    PUT(1, rsub(x, y));          \
  } else {                       \
    PUT(0, add(x, y));           \
    PUT(1, stage_sub(x, y));     \
  }

// The same units as functions: rm.pair(a, ja, c, jc, r, s) and rm.one(a, j) are the root products,
// put(k, y) takes output k.
template <class F, class RM, class Put>
ZDEV void r4_arith(const F& x0, const F& x1, const F& x2, const F& x3, uint32_t i, uint32_t Hh, int t, bool raw,
                   const RM& rm, const Put& put) {
  ZKP_NTT_R4(F, rm.pair, rm.one, put)
}
template <class F, class RM, class Put>
ZDEV void r2_first_pair(const F& x0, const F& x1, uint32_t ra, const F& y0, const F& y1, uint32_t rc, const RM& rm,
                        const Put& put) {
  ZKP_NTT_R2_FIRST_PAIR(F, rm.pair, put)
}
template <class F, class RM, class Put>
ZDEV void r2_first(const F& x0, const F& x1, uint32_t ra, const RM& rm, const Put& put) {
  ZKP_NTT_R2_FIRST_ONE(rm.one, put)
}
template <class F, class Put>
ZDEV void r2_last(const F& x, const F& y, bool raw, const Put& put) {
  ZKP_NTT_R2_LAST(put)
}

}  // namespace zkp
