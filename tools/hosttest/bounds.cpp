// Bounds prover for the lazily reduced field arithmetic (CPU only).
//
// Runs the project's own op sequences -- field.hpp's primitives, curve.hpp's XYZZ additions and
// doublings for G1 and G2, ntt_unit.hpp's butterfly units -- on interval elements (bounds.hpp) instead
// of uint32_t limbs, from each chain's documented input invariant, through every combination of the
// data-dependent branches, and checks for EVERY input at once that no limb expression leaves
// [0, 2^32), no column accumulator reaches 2^64, only the intended truncations truncate, a borrow
// form's top limb is negative only where the value proves it comes back, and each chain's outputs land
// back inside the invariant it started from.  Then it runs the same chains on real limbs (random,
// extreme and corner inputs) and checks every limb and value against the interval proven for that step.
//
//   hipcc --offload-host-only -O1 -std=c++17 tools/hosttest/bounds.cpp -o bounds && ./bounds
//
// Output: CONST / STEP / BOUND / SOUND lines and a final PROVEN line, exit status 0; or one FAIL line
// naming the chain, the op and the limb or column, exit status 1.  tests/test_host_bounds.py reads it.
#include "bounds.hpp"

#include <algorithm>
#include <functional>

using namespace zkp;

// ------------------------------------------------------------------ inputs
static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
  return g_seed;
}
static int g_mode = 0;  // concrete inputs: 0 random, 1 the value extremes, 2 the interval corners

template <class B>
static Big km(long long num, long long den = 1) {  // floor(num m / den)
  Big x = modulus<B>() * Big(num);
  if (den == 1) return x;
  // small divisor: long division over 64-bit words
  Big q;
  unsigned __int128 r = 0;
  for (int i = Big::W - 1; i >= 0; --i) {
    r = (r << 64) | x.w[i];
    q.w[i] = (uint64_t)(r / (uint64_t)den);
    r %= (uint64_t)den;
  }
  return q;
}

// an element with limbs 0..7 in [0, limbmax] and value in [0, vhi]
template <class B>
static Fe<Abs<B>> element(Abs<B>*, long long limbmax, const Big& vhi) {
  Fe<Abs<B>> e;
  for (int i = 0; i < NL - 1; ++i) e.v[i] = ALimb(0, limbmax);
  const Big t = vhi.sar(LB * (NL - 1));
  e.v[NL - 1] = ALimb(0, std::min<long long>(t.fits64() ? t.i64() : (1ll << 32) - 1, (1ll << 32) - 1));
  refine(e, Big(0), vhi, "input");
  return e;
}
template <class B>
static Fe<Rec<B>> element(Rec<B>*, long long limbmax, const Big& vhi) {
  const Big m = modulus<B>(), T = Big::pow2(LB * (NL - 1));
  Big v;
  const uint64_t pick = rnd();
  bool raw_spread = limbmax > LMASK;
  if (g_mode == 0) {  // uniform below vhi + 1: (vhi + 1) r / 2^64
    v = ((vhi + Big(1)) * Big((long long)(rnd() >> 1))).sar(63);
  } else if (g_mode == 1) {  // check_field.py's extremes, those that fit
    const Big c[] = {Big(0), Big(1), m - Big(1), m, m + Big(1), m + m - Big(1), T - Big(1), T, m + m - T, vhi, vhi - Big(1),
                     vhi - m, m + m, m * Big(4) - Big(1), m * Big(3) - Big(1)};
    v = c[pick % (sizeof c / sizeof c[0])];
    if (v.neg() || vhi < v) v = vhi;
  } else {  // corners: every low limb at its maximum or at zero, the top limb at either end
    Fe<Rec<B>> e;
    const bool low_max = pick & 1, top_max = pick & 2;
    Big low;
    for (int i = NL - 2; i >= 0; --i) {
      e.v[i] = low_max ? (uint32_t)limbmax : 0u;
      low = low.shl(LB) + Big((long long)e.v[i]);
    }
    const Big room = (vhi - low).sar(LB * (NL - 1));
    if (!room.neg()) {
      e.v[NL - 1] = top_max ? (uint32_t)std::min<long long>(room.i64(), 0xffffffffll) : 0u;
      return e;
    }
    v = vhi;  // the low limbs alone overshoot vhi: take the largest value instead
  }
  Fe<Rec<B>> e;
  for (int i = 0; i < NL - 1; ++i) e.v[i] = (uint32_t)(v.sar(LB * i).w[0] & LMASK);
  e.v[NL - 1] = (uint32_t)v.sar(LB * (NL - 1)).w[0];
  if (raw_spread)  // un-normalise: move carries back down while the limb stays <= limbmax
    for (int i = NL - 2; i >= 0; --i) {
      const uint64_t roomk = ((uint64_t)limbmax - e.v[i]) >> LB;
      const uint64_t k = std::min<uint64_t>(roomk, e.v[i + 1]);
      const uint64_t take = k ? rnd() % (k + 1) : 0;
      e.v[i] += (uint32_t)(take << LB);
      e.v[i + 1] -= (uint32_t)take;
    }
  return e;
}

// field-generic makers: F = Fe<C> or Fq2T<C>
template <class F>
struct Mk;
template <class C>
struct Mk<Fe<C>> {
  using Cfg = C;
  static Fe<C> el(long long limbmax, long long num, long long den = 1) {
    return element((C*)nullptr, limbmax, km<C>(num, den) - Big(1));
  }
  template <class Fn>
  static void each(const Fe<C>& x, Fn f) { f(x, ""); }
};
template <class C>
struct Mk<Fq2T<C>> {
  using Cfg = C;
  static Fq2T<C> el(long long limbmax, long long num, long long den = 1) {
    return Fq2T<C>{Mk<Fe<C>>::el(limbmax, num, den), Mk<Fe<C>>::el(limbmax, num, den)};
  }
  template <class Fn>
  static void each(const Fq2T<C>& x, Fn f) { f(x.c0, ".c0"), f(x.c1, ".c1"); }
};

// ------------------------------------------------------------------ documented bounds
struct BoundLine {
  std::string chain, name;
  Big vhi;
  long long num, den, lowmax, topmax;
};
static std::map<std::string, BoundLine> g_bounds;
static std::vector<std::string> g_bound_order;

// x is an output or a documented intermediate: value < num m / den, limbs 0..7 <= limbmax, top >= 0
template <class B>
static void expect1(const Fe<Abs<B>>& x, const std::string& name, long long limbmax, long long num, long long den) {
  Big lo, hi;
  get_val(x, lo, hi);
  long long lm = 0;
  for (int i = 0; i < NL; ++i) {
    if (x.v[i].lo < 0) fail(name, "documented bound: " + x.v[i].who() + " may wrap below zero, " + x.v[i].str());
    if (i < NL - 1) lm = std::max(lm, x.v[i].hi);
  }
  if (lo.neg()) fail(name, "documented bound: value may be negative");
  if (!(hi * Big(den) < modulus<B>() * Big(num)))
    fail(name, "documented bound < " + i2s(num) + "m/" + i2s(den) + " not proven: value up to " + hi.hex());
  if (lm > limbmax) fail(name, "documented bound: a limb reaches " + i2s(lm) + " > " + i2s(limbmax));
  const std::string key = g.chain + "|" + name;
  auto it = g_bounds.find(key);
  if (it == g_bounds.end()) {
    g_bound_order.push_back(key);
    g_bounds[key] = BoundLine{g.chain, name, hi, num, den, lm, x.v[NL - 1].hi};
  } else {
    it->second.vhi = bmax(it->second.vhi, hi);
    it->second.lowmax = std::max(it->second.lowmax, lm);
    it->second.topmax = std::max(it->second.topmax, x.v[NL - 1].hi);
  }
}
template <class B>
static void expect1(const Fe<Rec<B>>&, const std::string&, long long, long long, long long) {}
template <class F>
static void expect(const F& x, const std::string& name, long long limbmax, long long num, long long den = 1) {
  Mk<F>::each(x, [&](const auto& c, const char* suf) { expect1(c, name + suf, limbmax, num, den); });
}

// ------------------------------------------------------------------ running chains
struct Chain {
  std::string name;
  std::function<void()> abs, rec;
};
static std::vector<Chain> g_chains;
static long g_paths = 0;

static void prove(const Chain& c) {
  g.chain = c.name;
  g.path.clear();
  long n = 0;
  do {
    g.begin_run();
    c.abs();
    if (!g.pending.empty()) fail("(end of chain)", g.pending);
    if (!g.negpend.empty()) fail("(end of chain)", g.negpend);
    if (++n > 2000000) fail("(paths)", "more than 2000000 branch combinations");
  } while (g.next_path());
  g_paths += n;
  printf("CHAIN %s paths=%ld\n", c.name.c_str(), n);
}
static void sample(const Chain& c, int n_random, int n_extreme, int n_corner) {
  g.chain = c.name;
  const long e0 = g.escapes, c0 = g.checked;
  const int n[3] = {n_random, n_extreme, n_corner};
  for (g_mode = 0; g_mode < 3; ++g_mode)
    for (int k = 0; k < n[g_mode]; ++k) {
      g.begin_run();
      c.rec();
    }
  printf("SOUND %s checked=%ld escapes=%ld\n", c.name.c_str(), g.checked - c0, g.escapes - e0);
}

// ------------------------------------------------------------------ G1 / G2 accumulation
// accumulator invariant: x < 8m (G1) / components < 4m (G2), y, zz, zzz < 2m; all normalised
template <class F>
struct XBound {
  static constexpr int K = 8;
};
template <class C>
struct XBound<Fq2T<C>> {
  static constexpr int K = 4;
};
template <class F>
static Xyzz<F> mk_acc() {
  return Xyzz<F>{Mk<F>::el(LMASK, XBound<F>::K), Mk<F>::el(LMASK, 2), Mk<F>::el(LMASK, 2), Mk<F>::el(LMASK, 2)};
}
template <class F>
static Aff<F> mk_aff(int k = 1) {  // as loaded: < m
  return Aff<F>{Mk<F>::el(LMASK, k), Mk<F>::el(LMASK, k)};
}
template <class F>
static void closes(const Xyzz<F>& a) {  // the outputs land back inside the invariant
  expect(a.x, "x", LMASK, XBound<F>::K);
  expect(a.y, "y", LMASK, 2);
  expect(a.zz, "zz", LMASK, 2);
  expect(a.zzz, "zzz", LMASK, 2);
}
template <class F>
static void ch_from_aff_pair(bool np, bool nq) {
  closes(xyzz_from_aff_pair(mk_aff<F>(), np, mk_aff<F>(), nq));
}
template <class F>
static void ch_add_aff(bool neg) {
  Xyzz<F> acc = mk_acc<F>();
  xyzz_add_aff(acc, mk_aff<F>(), neg);
  closes(acc);
}
template <class F>
static void ch_add() {
  Xyzz<F> acc = mk_acc<F>();
  xyzz_add(acc, mk_acc<F>());
  closes(acc);
}
template <class F>
static void ch_dbl_aff() {  // callers pass coordinates < 2m (a negated y, a canonicalised accumulator x)
  closes(xyzz_dbl_aff(mk_aff<F>(2)));
}
template <class F>
static void ch_dbl() {
  closes(xyzz_dbl(mk_acc<F>()));
}
template <class F>
static void ch_xcanon() {  // store_xyzz
  expect(acc_xcanon(Mk<F>::el(LMASK, XBound<F>::K)), "x stored", LMASK, 2);
}
// the named lazy forms on their own, at their documented operand limits
template <class F>
static void ch_forms_g1() {
  const F a = Mk<F>::el(LMASK, 2), b = Mk<F>::el(LMASK, 2), c = Mk<F>::el(LMASK, 2), x8 = Mk<F>::el(LMASK, 8);
  expect(sub_2x8(a, b, c), "sub_2x8", LMASK, 8);
  expect(lsub8(a, x8), "lsub8", LMASK, 10);
  expect(lsub(a, b), "lsub", LMASK, 4);
  expect(rsub(a, b), "rsub", (1ll << 31) - 1, 6);
  expect(sub_2x(a, b, c), "sub_2x", LMASK, 2);
  expect(canon8(x8), "canon8", LMASK, 2);
  expect(sqr(lsub8(a, x8)), "sqr(lsub8)", LMASK, 2);
  expect(mul(x8, lsub8(a, x8)), "mul(x8, lsub8)", LMASK, 2);
  expect(mul2(Mk<F>::el(LMASK, 4), lsub8(a, x8), b, rsub(fe_zero<typename Mk<F>::Cfg>(), c)), "mul2(r, t, y, d)", LMASK, 2);
}
template <class C>
static void ch_forms_g2() {
  using F = Fq2T<C>;
  const F a = Mk<F>::el(LMASK, 2), b = Mk<F>::el(LMASK, 2), c = Mk<F>::el(LMASK, 2), x4 = Mk<F>::el(LMASK, 4);
  expect(sub_2x4(a, b, c), "sub_2x4", LMASK, 4);
  expect(lsub4_lazy(a, x4), "lsub4_lazy", LMASK, 6);
  expect(lsub2_lazy(a, b), "lsub2_lazy", LMASK, 4);
  expect(sqr_lazy(Mk<F>::el(LMASK, 6)), "sqr_lazy", LMASK, 2);
  expect(neg4(Mk<Fe<C>>::el(LMASK, 4)), "neg4 (<= 4m)", LMASK, 5);
  // Y3 = t r + d y with t < 6m, r < 4m, d < 4m, y < 2m (the mul2 ordering of acc_y3)
  expect(acc_y3(Mk<F>::el(LMASK, 4), Mk<F>::el(LMASK, 6), Mk<F>::el(LMASK, 2), Mk<F>::el(LMASK, 4)), "acc_y3", LMASK, 2);
  expect(mul(Mk<F>::el(LMASK, 4), Mk<F>::el(LMASK, 4)), "mul", LMASK, 2);
  expect(canon4(x4), "canon4", LMASK, 2);
}

// ------------------------------------------------------------------ NTT units
template <class F>
struct Roots {  // two stage roots with their Shoup quotients
  F w, wq, v, vq;
  void pair(const F& a, uint32_t, const F& c, uint32_t, F& r, F& s) const { mul_shoup_pair(a, w, wq, c, v, vq, r, s); }
  F one(const F& a, uint32_t) const { return mul_shoup(a, w, wq); }
};
template <class B>
static void mk_root(Abs<B>* t, Fe<Abs<B>>& w, Fe<Abs<B>>& wq) {
  w = element(t, LMASK, modulus<B>() - Big(1));
  wq = element(t, LMASK, Big::pow2(LB * NL) - Big(1));
}
template <class B>
static void mk_root(Rec<B>* t, Fe<Rec<B>>& w, Fe<Rec<B>>& wq) {  // wq = floor(w 2^261 / m), by the plain config
  const Fe<Rec<B>> x = element(t, LMASK, modulus<B>() - Big(1));
  Fe<B> p;
  for (int i = 0; i < NL; ++i) p.v[i] = x.v[i];
  const Fe<B> q = shoup_quot(canon(to_mont(p)));
  for (int i = 0; i < NL; ++i) w.v[i] = x.v[i], wq.v[i] = q.v[i];
}
template <class C>
static Roots<Fe<C>> mk_roots() {
  Roots<Fe<C>> r;
  mk_root((C*)nullptr, r.w, r.wq);
  mk_root((C*)nullptr, r.v, r.vq);
  return r;
}
// a raw last-round output goes into mul() against a normalised table value < 2m, or into mul_shoup
template <class F>
static void raw_consumers(const F& y, const std::string& name, const Roots<F>& R) {
  expect(mul(y, Mk<F>::el(LMASK, 2)), name + " x table", LMASK, 2);
  expect(mul_shoup(y, R.w, R.wq), name + " x root", LMASK, 3);
}
template <class C>
static void ch_r4(uint32_t Hh, bool raw) {
  using F = Fe<C>;
  const Roots<F> R = mk_roots<C>();
  F y[4];
  const F x0 = Mk<F>::el(LMASK, 3), x1 = Mk<F>::el(LMASK, 3), x2 = Mk<F>::el(LMASK, 3), x3 = Mk<F>::el(LMASK, 3);
  r4_arith(x0, x1, x2, x3, 0u, Hh, 0, raw, R, [&](int k, const F& v) { y[k] = v; });
  if (Hh == 1 && raw) {
    const long long L31 = (1ll << 31) - 1;
    expect(y[0], "p0 raw", L31, 12);
    expect(y[1], "p1 raw (sub_raw8)", 5 * (1ll << 29) - 1, 14);
    expect(y[2], "p2 raw", L31, 6);
    expect(y[3], "p3 raw", L31, 7);
    for (int k = 0; k < 4; ++k) raw_consumers(y[k], "p" + i2s(k), R);
  } else {
    for (int k = 0; k < 4; ++k) expect(y[k], "p" + i2s(k), LMASK, 3);  // back inside the tile invariant
  }
}
template <class C>
static void ch_r2_first(bool pair) {
  using F = Fe<C>;
  const Roots<F> R = mk_roots<C>();
  F y[4];
  const F x0 = Mk<F>::el(LMASK, 3), x1 = Mk<F>::el(LMASK, 3), y0 = Mk<F>::el(LMASK, 3), y1 = Mk<F>::el(LMASK, 3);
  auto put = [&](int k, const F& v) { y[k] = v; };
  if (pair) r2_first_pair(x0, x1, 0u, y0, y1, 0u, R, put);
  else r2_first(x0, x1, 0u, R, put);
  for (int k = 0; k < (pair ? 4 : 2); ++k) expect(y[k], "p" + i2s(k), LMASK, 3);
}
template <class C>
static void ch_r2_last(bool raw) {
  using F = Fe<C>;
  const Roots<F> R = mk_roots<C>();
  F y[2];
  r2_last(Mk<F>::el(LMASK, 3), Mk<F>::el(LMASK, 3), raw, [&](int k, const F& v) { y[k] = v; });
  if (raw) {
    expect(y[0], "p0 raw", (1ll << 31) - 1, 6);
    expect(y[1], "p1 raw", (1ll << 31) - 1, 7);
    for (int k = 0; k < 2; ++k) raw_consumers(y[k], "p" + i2s(k), R);
  } else {
    for (int k = 0; k < 2; ++k) expect(y[k], "p" + i2s(k), LMASK, 3);
  }
}
// the Fr sums and differences as commented: qreduce outputs < 1.2m = 6m/5
template <class C>
static void ch_fr_forms() {
  using F = Fe<C>;
  const F a = Mk<F>::el(LMASK, 2), b = Mk<F>::el(LMASK, 2), a3 = Mk<F>::el(LMASK, 3), b3 = Mk<F>::el(LMASK, 3);
  expect(add(a, b), "add", LMASK, 6, 5);
  expect(sub(a, b), "sub", LMASK, 6, 5);
  expect(sub4(a3, Mk<F>::el(LMASK, 4)), "sub4", LMASK, 6, 5);
  expect(add(a3, b3), "add (tile values < 3m)", LMASK, 6, 5);
  const F s02 = add_raw(a3, b3), s13 = add_raw(Mk<F>::el(LMASK, 3), Mk<F>::el(LMASK, 3));
  expect(add_raw_reduce(s02, s13), "add_raw_reduce", LMASK, 6, 5);
  expect(sub_raw8(s02, s13), "sub_raw8", 5 * (1ll << 29) - 1, 14);
  expect(qreduce(sub_raw8(s02, s13)), "qreduce(sub_raw8)", LMASK, 6, 5);
  expect(sub_2x(a, b, Mk<F>::el(LMASK, 2)), "sub_2x", LMASK, 6, 5);
}

// ------------------------------------------------------------------ primitives at their operand limits
template <class C>
static void ch_prims() {
  using F = Fe<C>;
  const long long L30 = (1ll << 30) - 1, L31 = 5 * (1ll << 29) - 1;  // "raw": limbs < 2.5 * 2^30, the largest form (sub_raw8)
  expect(mul(Mk<F>::el(L30, 8), Mk<F>::el(L30, 8)), "mont_sop N=1, both limbs < 2^30, < 8m", LMASK, 2);
  expect(mul(Mk<F>::el(L31, 14), Mk<F>::el(LMASK, 2)), "mont_sop N=1, raw limbs < 2.5 * 2^30 x normalised", LMASK, 2);
  expect(mul(Mk<F>::el(LMASK, 11), Mk<F>::el(LMASK, 11)), "mont_sop N=1, 11m x 11m", LMASK, 2);
  expect(mul2(Mk<F>::el(LMASK, 9), Mk<F>::el(LMASK, 9), Mk<F>::el(LMASK, 9), Mk<F>::el(LMASK, 9)), "mont_sop N=2, 162 m^2", LMASK, 2);
  {
    const F a0 = Mk<F>::el(LMASK, 6), a1 = Mk<F>::el(LMASK, 6), a2 = Mk<F>::el(LMASK, 6), a3 = Mk<F>::el(LMASK, 6);
    const F b0 = Mk<F>::el(LMASK, 6), b1 = Mk<F>::el(LMASK, 6), b2 = Mk<F>::el(LMASK, 6), b3 = Mk<F>::el(LMASK, 6);
    F r;
    mont_sop<C, true, 1, 4>({{&a0, &a1, &a2, &a3}}, {{&b0, &b1, &b2, &b3}}, {&r}, "sop4");
    expect(r, "mont_sop N=4, 144 m^2", LMASK, 2);
  }
  expect(sqr(Mk<F>::el(LMASK, 11)), "mont_sqr, 11m", LMASK, 2);
  const Roots<F> R = mk_roots<C>();
  expect(mul_shoup(element((C*)nullptr, L31, Big::pow2(LB * NL) - Big(1)), R.w, R.wq), "mont_shoup, raw limbs < 2.5 * 2^30, < 2^261", LMASK, 3);
  expect(qreduce(element((C*)nullptr, (1ll << 32) - (1ll << 10) - 1, Big::pow2(LB * NL) - Big(1))), "qreduce, limbs < 2^32 - 2^10", LMASK, 6, 5);
}

// ------------------------------------------------------------------ start-up: the constants the transfer functions assume
template <class B>
static void check_consts(const char* name) {
  const Big m = modulus<B>(), R = Big::pow2(LB * NL);
  auto need = [&](bool ok, const char* what) {
    if (!ok) {
      g.chain = std::string("consts ") + name;
      fail(what, "table does not hold what the proofs assume");
    }
  };
  need(tab_val<B>(B::NM) + m == R, "NM = 2^261 - m");
  need(Big((long long)B::QK) * m <= Big::pow2(264) && Big::pow2(264) < Big((long long)B::QK + 1) * m, "QK = floor(2^264 / m)");
  need((((uint64_t)B::MOD[0] * B::INV + 1) & LMASK) == 0, "INV = -1/m mod 2^29");
  // (the MODk and borrow-form tables are not assumed: cond_sub and borrow_sub take their values from the limbs)
  for (int i = 0; i < NL; ++i) need(B::MOD[i] <= LMASK && B::NM[i] <= LMASK, "normalised tables");
  printf("CONST %s m=%s\n", name, m.hex().c_str());
}

template <class B>
static std::string as_m(const Big& v) {
  char buf[64];
  snprintf(buf, sizeof buf, "%.6Lf", v.ld() / modulus<B>().ld());
  return buf;
}

template <class B>
static void add_g1(const std::string& G) {
  for (int s = 0; s < 4; ++s)
    g_chains.push_back(Chain{G + " xyzz_from_aff_pair np=" + i2s(s & 1) + " nq=" + i2s(s >> 1),
                             [s] { ch_from_aff_pair<Fe<Abs<B>>>(s & 1, s >> 1); }, [s] { ch_from_aff_pair<Fe<Rec<B>>>(s & 1, s >> 1); }});
  for (int s = 0; s < 2; ++s)
    g_chains.push_back(Chain{G + " xyzz_add_aff neg=" + i2s(s), [s] { ch_add_aff<Fe<Abs<B>>>(s); }, [s] { ch_add_aff<Fe<Rec<B>>>(s); }});
  g_chains.push_back(Chain{G + " xyzz_add", [] { ch_add<Fe<Abs<B>>>(); }, [] { ch_add<Fe<Rec<B>>>(); }});
  g_chains.push_back(Chain{G + " xyzz_dbl_aff", [] { ch_dbl_aff<Fe<Abs<B>>>(); }, [] { ch_dbl_aff<Fe<Rec<B>>>(); }});
  g_chains.push_back(Chain{G + " xyzz_dbl", [] { ch_dbl<Fe<Abs<B>>>(); }, [] { ch_dbl<Fe<Rec<B>>>(); }});
  g_chains.push_back(Chain{G + " store_xyzz", [] { ch_xcanon<Fe<Abs<B>>>(); }, [] { ch_xcanon<Fe<Rec<B>>>(); }});
  g_chains.push_back(Chain{G + " forms", [] { ch_forms_g1<Fe<Abs<B>>>(); }, [] { ch_forms_g1<Fe<Rec<B>>>(); }});
  g_chains.push_back(Chain{G + " primitives", [] { ch_prims<Abs<B>>(); }, [] { ch_prims<Rec<B>>(); }});
}
template <class B>
static void add_g2(const std::string& G) {
  g_chains.push_back(Chain{G + " forms", [] { ch_forms_g2<Abs<B>>(); }, [] { ch_forms_g2<Rec<B>>(); }});
  for (int s = 0; s < 2; ++s)
    g_chains.push_back(Chain{G + " xyzz_add_aff neg=" + i2s(s), [s] { ch_add_aff<Fq2T<Abs<B>>>(s); }, [s] { ch_add_aff<Fq2T<Rec<B>>>(s); }});
  g_chains.push_back(Chain{G + " xyzz_add", [] { ch_add<Fq2T<Abs<B>>>(); }, [] { ch_add<Fq2T<Rec<B>>>(); }});
  g_chains.push_back(Chain{G + " xyzz_dbl_aff", [] { ch_dbl_aff<Fq2T<Abs<B>>>(); }, [] { ch_dbl_aff<Fq2T<Rec<B>>>(); }});
  g_chains.push_back(Chain{G + " xyzz_dbl", [] { ch_dbl<Fq2T<Abs<B>>>(); }, [] { ch_dbl<Fq2T<Rec<B>>>(); }});
  g_chains.push_back(Chain{G + " store_xyzz", [] { ch_xcanon<Fq2T<Abs<B>>>(); }, [] { ch_xcanon<Fq2T<Rec<B>>>(); }});
  for (int s = 0; s < 4; ++s)
    g_chains.push_back(Chain{G + " xyzz_from_aff_pair np=" + i2s(s & 1) + " nq=" + i2s(s >> 1),
                             [s] { ch_from_aff_pair<Fq2T<Abs<B>>>(s & 1, s >> 1); },
                             [s] { ch_from_aff_pair<Fq2T<Rec<B>>>(s & 1, s >> 1); }});
}
template <class B>
static void add_ntt(const std::string& G) {
  g_chains.push_back(Chain{G + " r4 unit (Hh > 1)", [] { ch_r4<Abs<B>>(2, false); }, [] { ch_r4<Rec<B>>(2, false); }});
  g_chains.push_back(Chain{G + " r4 last pair raw", [] { ch_r4<Abs<B>>(1, true); }, [] { ch_r4<Rec<B>>(1, true); }});
  g_chains.push_back(Chain{G + " r4 last pair stored", [] { ch_r4<Abs<B>>(1, false); }, [] { ch_r4<Rec<B>>(1, false); }});
  g_chains.push_back(Chain{G + " r2 first stage pair", [] { ch_r2_first<Abs<B>>(true); }, [] { ch_r2_first<Rec<B>>(true); }});
  g_chains.push_back(Chain{G + " r2 first stage one", [] { ch_r2_first<Abs<B>>(false); }, [] { ch_r2_first<Rec<B>>(false); }});
  g_chains.push_back(Chain{G + " r2 only stage raw", [] { ch_r2_last<Abs<B>>(true); }, [] { ch_r2_last<Rec<B>>(true); }});
  g_chains.push_back(Chain{G + " r2 only stage stored", [] { ch_r2_last<Abs<B>>(false); }, [] { ch_r2_last<Rec<B>>(false); }});
  g_chains.push_back(Chain{G + " forms", [] { ch_fr_forms<Abs<B>>(); }, [] { ch_fr_forms<Rec<B>>(); }});
  g_chains.push_back(Chain{G + " primitives", [] { ch_prims<Abs<B>>(); }, [] { ch_prims<Rec<B>>(); }});
}

int main(int argc, char** argv) {
  // --quiet: no STEP lines.  --list: the chain names.  --chains a,b,...: only the chains whose name
  // contains one of the comma-separated strings (the chains are independent, so a caller may spread
  // them over processes; the G2 pair chains visit ~41000 branch combinations each).
  bool quiet = false, list = false;
  std::vector<std::string> only;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--quiet") quiet = true;
    else if (a == "--list") list = true;
    else if (a == "--chains" && i + 1 < argc) {
      std::string v = argv[++i];
      size_t p0 = 0, p1;
      while ((p1 = v.find(',', p0)) != std::string::npos) only.push_back(v.substr(p0, p1 - p0)), p0 = p1 + 1;
      only.push_back(v.substr(p0));
    }
  }
  check_consts<FqCfg>("Fq");
  check_consts<FrCfg>("Fr");
  add_ntt<FrCfg>("NTT[Fr]");
  add_g1<FqAccCfg>("G1[FqAcc]");
  add_g1<FqCfg>("G1[Fq]");
  add_g2<FqCfg>("G2[Fq2]");

  if (!only.empty()) {
    std::vector<Chain> keep;
    for (const Chain& c : g_chains)
      for (const std::string& o : only)
        if (c.name.find(o) != std::string::npos) {
          keep.push_back(c);
          break;
        }
    g_chains = keep;
  }
  if (list) {
    for (const Chain& c : g_chains) printf("%s\n", c.name.c_str());
    return 0;
  }
  for (const Chain& c : g_chains) prove(c);
  const Big mq = modulus<FqCfg>();
  if (!quiet)
    for (const std::string& lab : g_order) {
      const Rec1& r = g_rec[lab];
      long long lm = 0;
      for (int i = 0; i < NL - 1; ++i) lm = std::max(lm, r.hi[i]);
      printf("STEP %s | value <= %s m (%s) | low limbs <= %lld (%.3f x 2^29), top in [%lld, %lld] | column %.4Lf x 2^64", lab.c_str(),
             as_m<FqCfg>(r.vhi).c_str(), r.vhi.hex().c_str(), lm, (double)lm / (1 << 29), r.lo[NL - 1], r.hi[NL - 1], r.col);
      if (r.shoup_k >= 0) printf(" | q >= floor - %d", r.shoup_k);
      printf("\n");
    }
  for (const std::string& key : g_bound_order) {
    const BoundLine& b = g_bounds[key];
    printf("BOUND %s | %s | proven <= %s m | %s | documented < %lld/%lld m | low limbs <= %lld | top <= %lld\n", b.chain.c_str(), b.name.c_str(),
           as_m<FqCfg>(b.vhi).c_str(), b.vhi.hex().c_str(), b.num, b.den, b.lowmax, b.topmax);
  }
  (void)mq;
  for (const Chain& c : g_chains) sample(c, 300, 120, 40);
  printf("%s chains=%zu paths=%ld steps=%zu concrete_checks=%ld escapes=%ld\n", g.escapes ? "UNSOUND" : "PROVEN", g_chains.size(), g_paths,
         g_order.size(), g.checked, g.escapes);
  return g.escapes ? 2 : 0;
}
