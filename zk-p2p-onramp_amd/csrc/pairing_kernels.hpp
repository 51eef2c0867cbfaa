// Device BN254 pairing arithmetic (groth16_verify.hip): the Fq6 / Fq12 tower over Fq2T and the per-lane
// body of the optimal-ate Miller loop.  __host__ __device__ so that tools/hosttest/pairing_emu.cpp runs
// the same text on the CPU against host_pairing.cpp.
//
// Tower as the host's: Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v), xi = 9 + u.
//
// Field forms.  The tower is built only from the Fq / Fq2 `mul`, `mul2`, `sqr`, `add`, `sub`, `dbl`
// of field.hpp on normalised operands below 2m, which all return normalised values below 2m: the
// bounds tools/hosttest/bounds.cpp proves for these ops cover every value here, and no
// lazily reduced form is introduced.
//
// Miller values are NOT the host's.  T stays in homogeneous projective coordinates and P may be
// projective too, so no step inverts: every line is the host's line (host_pairing.cpp
// miller_loop_multi) times a nonzero factor of Fq2.  The final exponentiation sends Fq2 to 1, so
// final_exponentiation(device value) == final_exponentiation(host value), and only there: compare
// nowhere before it.
//
// Where f lives.  f is 12 x 9 limbs = 108 words per lane.  The Miller kernel keeps it in LDS, limb
// major (word w of lane l at w * 64 + l: consecutive lanes hit consecutive banks, every access is
// conflict free), 27 KB per wave; T, P, Q and the line stay in registers.  LaneMem names such a
// strided home; the host emulation uses stride 1.
#pragma once
#include "curve.hpp"

namespace zkp {
namespace pairing {

constexpr int F12_WORDS = 12 * NL;  // 108

// Between the Fq6-sized steps of an Fq12 operation and between the steps of the Miller loop's body: the
// instruction scheduler may not move code across.  Left alone it interleaves the independent Fq2 products
// of neighbouring steps to hide latency, which keeps several Fq6 temporaries alive at once and spills.
#if defined(__HIP_DEVICE_COMPILE__)
#define ZKP_STEP_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define ZKP_STEP_FENCE()
#endif
// bits 63..0 of 6u + 2 = 2^64 + ATE_LO (u = 4965661367192848881); bit 64 is the start T = Q
constexpr uint64_t ATE_LO = 0x9d797039be763ba8ull;

struct F6 {
  Fq2 c0, c1, c2;
};
struct F12 {
  F6 c0, c1;  // c0 + c1 w
};

// ---------------------------------------------------------------- Fq2 helpers
ZDEV Fq2 f2_zero() { return f_zero<Fq2>(); }
ZDEV Fq2 f2_one() { return f_one<Fq2>(); }
ZDEV Fq2 f2_neg(const Fq2& a) { return sub(f2_zero(), a); }
ZDEV Fq2 f2_conj(const Fq2& a) { return Fq2{a.c0, neg(a.c1)}; }
ZDEV Fq2 f2_muls(const Fq2& a, const Fq& k) { return Fq2{mul(a.c0, k), mul(a.c1, k)}; }
ZDEV Fq nine(const Fq& x) {
  const Fq x8 = dbl(dbl(dbl(x)));
  return add(x8, x);
}
// (a0 + a1 u)(9 + u) = (9 a0 - a1) + (a0 + 9 a1) u
ZDEV Fq2 f2_mul_xi(const Fq2& a) { return Fq2{sub(nine(a.c0), a.c1), add(a.c0, nine(a.c1))}; }

// ---------------------------------------------------------------- Fq6
ZDEV F6 f6_add(const F6& a, const F6& b) { return F6{add(a.c0, b.c0), add(a.c1, b.c1), add(a.c2, b.c2)}; }
ZDEV F6 f6_sub(const F6& a, const F6& b) { return F6{sub(a.c0, b.c0), sub(a.c1, b.c1), sub(a.c2, b.c2)}; }
ZDEV F6 f6_mul_v(const F6& a) { return F6{f2_mul_xi(a.c2), a.c0, a.c1}; }  // (a0 + a1 v + a2 v^2) v
// Karatsuba over Fq2: 6 products
ZDEV F6 f6_mul(const F6& a, const F6& b) {
  const Fq2 t0 = mul(a.c0, b.c0), t1 = mul(a.c1, b.c1), t2 = mul(a.c2, b.c2);
  F6 r;
  r.c0 = add(t0, f2_mul_xi(sub(sub(mul(add(a.c1, a.c2), add(b.c1, b.c2)), t1), t2)));
  r.c1 = add(sub(sub(mul(add(a.c0, a.c1), add(b.c0, b.c1)), t0), t1), f2_mul_xi(t2));
  r.c2 = add(sub(sub(mul(add(a.c0, a.c2), add(b.c0, b.c2)), t0), t2), t1);
  return r;
}
ZDEV F6 f6_mul_f2(const F6& a, const Fq2& k) { return F6{mul(a.c0, k), mul(a.c1, k), mul(a.c2, k)}; }
// (a0 + a1 v + a2 v^2)(b0 + b1 v): the two-term coefficients as one sum of products each (Fq2 mul2)
ZDEV F6 f6_mul_01(const F6& a, const Fq2& b0, const Fq2& b1) {
  F6 r;
  r.c0 = add(mul(a.c0, b0), f2_mul_xi(mul(a.c2, b1)));
  r.c1 = mul2(a.c0, b1, a.c1, b0);
  r.c2 = mul2(a.c1, b1, a.c2, b0);
  return r;
}

// ---------------------------------------------------------------- Fq12 in registers
ZDEV F12 f12_one() {
  F12 r;
  r.c0 = F6{f2_one(), f2_zero(), f2_zero()};
  r.c1 = F6{f2_zero(), f2_zero(), f2_zero()};
  return r;
}
ZDEV F12 f12_mul(const F12& a, const F12& b) {
  const F6 t0 = f6_mul(a.c0, b.c0);
  ZKP_STEP_FENCE();
  const F6 t1 = f6_mul(a.c1, b.c1);
  ZKP_STEP_FENCE();
  F12 r;
  r.c1 = f6_sub(f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1)), t0), t1);
  ZKP_STEP_FENCE();
  r.c0 = f6_add(t0, f6_mul_v(t1));
  return r;
}
// ---------------------------------------------------------------- f's strided home
struct LaneMem {
  uint32_t* p;
  int stride;
};
ZDEV Fq lm_get_fe(const LaneMem& m, int k) {
  Fq r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = m.p[(size_t)(k * NL + i) * m.stride];
  return r;
}
ZDEV void lm_set_fe(const LaneMem& m, int k, const Fq& a) {
#pragma unroll
  for (int i = 0; i < NL; ++i) m.p[(size_t)(k * NL + i) * m.stride] = a.v[i];
}
ZDEV Fq2 lm_get(const LaneMem& m, int k) { return Fq2{lm_get_fe(m, 2 * k), lm_get_fe(m, 2 * k + 1)}; }
ZDEV void lm_set(const LaneMem& m, int k, const Fq2& a) {
  lm_set_fe(m, 2 * k, a.c0);
  lm_set_fe(m, 2 * k + 1, a.c1);
}
ZDEV F12 lm_load(const LaneMem& m) {
  F12 r;
  r.c0 = F6{lm_get(m, 0), lm_get(m, 1), lm_get(m, 2)};
  r.c1 = F6{lm_get(m, 3), lm_get(m, 4), lm_get(m, 5)};
  return r;
}
ZDEV void lm_store(const LaneMem& m, const F12& a) {
  lm_set(m, 0, a.c0.c0), lm_set(m, 1, a.c0.c1), lm_set(m, 2, a.c0.c2);
  lm_set(m, 3, a.c1.c0), lm_set(m, 4, a.c1.c1), lm_set(m, 5, a.c1.c2);
}

// Fq12 <-> 96 words in zkp_pairing's order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1), standard form
ZDEV Fq2 f2_load_std(const uint32_t* in) { return Fq2{to_mont(load_fe<FqCfg>(in)), to_mont(load_fe<FqCfg>(in + 8))}; }
ZDEV void f2_store_std(uint32_t* out, const Fq2& a) {
  store_fe(out, from_mont(a.c0));
  store_fe(out + 8, from_mont(a.c1));
}
ZDEV F12 f12_load_std(const uint32_t* in) {
  F12 r;
  r.c0 = F6{f2_load_std(in), f2_load_std(in + 16), f2_load_std(in + 32)};
  r.c1 = F6{f2_load_std(in + 48), f2_load_std(in + 64), f2_load_std(in + 80)};
  return r;
}
ZDEV void f12_store_std(uint32_t* out, const F12& a) {
  f2_store_std(out, a.c0.c0), f2_store_std(out + 16, a.c0.c1), f2_store_std(out + 32, a.c0.c2);
  f2_store_std(out + 48, a.c1.c0), f2_store_std(out + 64, a.c1.c1), f2_store_std(out + 80, a.c1.c2);
}

// ---------------------------------------------------------------- Miller loop
// The G2 Frobenius pi(x, y) = (conj(x) gx, conj(y) gy): gx = xi^((p-1)/3), gy = xi^((p-1)/2), standard
// form words (c0, c1), computed by the host (host::g2_frobenius_consts) and passed by value.
struct alignas(16) FrobConsts {
  uint32_t gx[16], gy[16];
};

struct ProjG1 {  // homogeneous: x = X/Z, y = Y/Z; never at infinity inside the loop
  Fq x, y, z;
};
struct ProjG2 {
  Fq2 x, y, z;
};

// T <- 2T and the tangent at T evaluated at P, times 2 Y Z^2 Pz (EFD dbl-2007-bl, a = 0):
// lambda = w / s with w = 3 X^2, s = 2 Y Z
ZDEV void dbl_step(ProjG2& t, const ProjG1& p, Fq2& l0, Fq2& l1, Fq2& l3) {
  const Fq2 xx = sqr(t.x);
  const Fq2 w = add(dbl(xx), xx);
  const Fq2 s = dbl(mul(t.y, t.z));
  const Fq2 r = mul(t.y, s);
  l0 = f2_muls(mul(s, t.z), p.y);
  l1 = f2_neg(f2_muls(mul(w, t.z), p.x));
  l3 = f2_muls(sub(mul(w, t.x), r), p.z);
  const Fq2 ss = sqr(s);
  const Fq2 rr = sqr(r);
  const Fq2 b = dbl(mul(t.x, r));
  const Fq2 h = sub(sqr(w), dbl(b));
  t.x = mul(h, s);
  t.y = sub(mul(w, sub(b, h)), dbl(rr));
  t.z = mul(s, ss);
}

// T <- T + Q (Q affine, Q != +-T) and the chord through them at P, times (xq Z - X) Pz
// (EFD madd-1998-cmo): lambda = u / v
ZDEV void add_step(ProjG2& t, const Aff<Fq2>& q, const ProjG1& p, Fq2& l0, Fq2& l1, Fq2& l3) {
  const Fq2 u = sub(mul(q.y, t.z), t.y);
  const Fq2 v = sub(mul(q.x, t.z), t.x);
  l0 = f2_muls(v, p.y);
  l1 = f2_neg(f2_muls(u, p.x));
  l3 = f2_muls(sub(mul(u, q.x), mul(v, q.y)), p.z);
  const Fq2 uu = sqr(u), vv = sqr(v);
  const Fq2 vvv = mul(v, vv);
  const Fq2 r = mul(vv, t.x);
  const Fq2 a = sub(sub(mul(uu, t.z), vvv), dbl(r));
  t.x = mul(v, a);
  t.y = sub(mul(u, sub(r, a)), mul(vvv, t.y));
  t.z = mul(vvv, t.z);
}

ZDEV Aff<Fq2> g2_frobenius(const Aff<Fq2>& q, const Fq2& gx, const Fq2& gy) {
  return Aff<Fq2>{mul(f2_conj(q.x), gx), mul(f2_conj(q.y), gy)};
}

// The in-place forms on f's home.  Each reads f again where a second step needs it instead of holding
// all of it across the first (ZKP_REREAD keeps the compiler from merging the two reads): at most one Fq6
// of f, the step's result and one product's temporaries are live beside T and Q.
#define ZKP_REREAD() asm volatile("" ::: "memory")
ZDEV F6 lm_load6(const LaneMem& m, int h) { return F6{lm_get(m, 3 * h), lm_get(m, 3 * h + 1), lm_get(m, 3 * h + 2)}; }
ZDEV void lm_store6(const LaneMem& m, int h, const F6& a) {
  lm_set(m, 3 * h, a.c0), lm_set(m, 3 * h + 1, a.c1), lm_set(m, 3 * h + 2, a.c2);
}
// complex squaring: c1 = 2 a0 a1, c0 = (a0 + a1)(a0 + v a1) - a0 a1 - v a0 a1: 2 Fq6 products
ZDEV void f12_sqr_mem(const LaneMem& fm) {
  const F6 t = f6_mul(lm_load6(fm, 0), lm_load6(fm, 1));
  ZKP_STEP_FENCE();
  ZKP_REREAD();
  F6 s;
  {
    const F6 a0 = lm_load6(fm, 0), a1 = lm_load6(fm, 1);
    s = f6_mul(f6_add(a0, a1), f6_add(a0, f6_mul_v(a1)));
  }
  ZKP_STEP_FENCE();
  lm_store6(fm, 0, f6_sub(f6_sub(s, t), f6_mul_v(t)));
  lm_store6(fm, 1, f6_add(t, t));
}
// f * l for the sparse l = (l0, 0, 0) + (l1, l3, 0) w (the shape of the host's f12_mul_line, with l0 in
// Fq2 because the line carries its projective factor): 15 Fq2 products
ZDEV void f12_mul_line_mem(const LaneMem& fm, const Fq2& l0, const Fq2& l1, const Fq2& l3) {
  const F6 t0 = f6_mul_f2(lm_load6(fm, 0), l0);
  ZKP_STEP_FENCE();
  const F6 t1 = f6_mul_01(lm_load6(fm, 1), l1, l3);
  ZKP_STEP_FENCE();
  ZKP_REREAD();
  const F6 c1 = f6_sub(f6_sub(f6_mul_01(f6_add(lm_load6(fm, 0), lm_load6(fm, 1)), add(l0, l1), l3), t0), t1);
  ZKP_STEP_FENCE();
  lm_store6(fm, 1, c1);
  lm_store6(fm, 0, f6_add(t0, f6_mul_v(t1)));
}

// f <- the Miller value of (P, Q) over 6u + 2 with the lines through pi(Q) and -pi^2(Q), f in `fm`.
// P, Q finite, Montgomery form, coordinates below 2m; Q of order r (an add step never meets T = +-Q).
// One loop body serves every step: kind 0 squares f and doubles T, kinds 1..3 add Q, pi(Q), -pi^2(Q);
// the step order depends on the constant alone, so the branches are wave-uniform.
ZDEV void miller_loop(const ProjG1& p, const Aff<Fq2>& q0, const FrobConsts& fc, const LaneMem& fm) {
  lm_store(fm, f12_one());
  ProjG2 t{q0.x, q0.y, f2_one()};
  Aff<Fq2> qa = q0;  // the addend of the next add step
  int bit = 63, kind = 0;
  for (;;) {
    Fq2 l0, l1, l3;
    if (kind == 0) {
      f12_sqr_mem(fm);
      ZKP_STEP_FENCE();
      dbl_step(t, p, l0, l1, l3);
    } else {
      add_step(t, qa, p, l0, l1, l3);
    }
    ZKP_STEP_FENCE();
    f12_mul_line_mem(fm, l0, l1, l3);
    ZKP_STEP_FENCE();
    if (kind == 0 && ((ATE_LO >> bit) & 1)) {
      kind = 1;
    } else if (kind <= 1) {
      kind = --bit >= 0 ? 0 : 2;
    } else if (kind == 2) {
      kind = 3;
    } else {
      break;
    }
    if (kind >= 2) {  // Q -> pi(Q) -> -pi^2(Q)
      Fq2 gx, gy;
      load_f(fc.gx, gx), load_f(fc.gy, gy);
      qa = g2_frobenius(qa, Fq2{to_mont(gx.c0), to_mont(gx.c1)}, Fq2{to_mont(gy.c0), to_mont(gy.c1)});
      if (kind == 3) qa.y = f2_neg(qa.y);
    }
  }
}

// Pair i of standard-form arrays (g1: 16 words, g2: 32 words, all-zero = infinity) -> out (96 words,
// standard form); a pair with a point at infinity gives 1.
ZDEV void miller_pair_std(const uint32_t* g1, const uint32_t* g2, size_t i, const FrobConsts& fc, const LaneMem& fm,
                          uint32_t* out) {
  const Aff<Fq> pa = load_aff<Fq>(g1, i);
  const Aff<Fq2> qa = load_aff<Fq2>(g2, i);
  if (aff_is_inf(pa) || aff_is_inf(qa)) {
    f12_store_std(out + i * 96, f12_one());
    return;
  }
  const ProjG1 p{to_mont(pa.x), to_mont(pa.y), fe_one<FqCfg>()};
  const Aff<Fq2> q{Fq2{to_mont(qa.x.c0), to_mont(qa.x.c1)}, Fq2{to_mont(qa.y.c0), to_mont(qa.y.c1)}};
  miller_loop(p, q, fc, fm);
  f12_store_std(out + i * 96, lm_load(fm));
}

}  // namespace pairing
}  // namespace zkp
