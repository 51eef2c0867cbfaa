// The abstract domain of the bounds prover (bounds.cpp): field elements whose nine limbs are integer
// intervals and which carry an exact integer interval for the value they represent, plus the types
// that stand in for uint32_t / int32_t / uint64_t inside field.hpp's templates.
//
// Abs<B> is the interval twin of a field config B (same tables, same QRED / CHAIN).  FeTypes<Abs<B>>
// names the interval types, so mont_sop, qreduce, borrow_sub, ... run unchanged on them and every limb
// expression and column accumulator is range-checked as it is evaluated; FeTypes<Abs<B>>::note() is
// called by each primitive on its result and applies the primitive's VALUE-level transfer function,
// checks its operand contract, and lets limbs and value constrain each other (refine()).
// Rec<B> is the concrete twin: real uint32_t limbs, with a note() that checks every limb and value the
// real arithmetic produces against the interval proven for the same step (the soundness cross-check).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

// the interval types make every primitive a large function: let the compiler decide what to inline
#define ZDEV __host__ __device__ inline
#include "../../zk-p2p-onramp_amd/csrc/curve.hpp"
#include "../../zk-p2p-onramp_amd/csrc/ntt_unit.hpp"

namespace zkp {

// ------------------------------------------------------------------ signed fixed-width integers
// 768-bit two's complement: value bounds reach 2^270, their products 2^540.
struct Big {
  static constexpr int W = 12;
  uint64_t w[W];
  Big(long long x = 0) {
    w[0] = (uint64_t)x;
    for (int i = 1; i < W; ++i) w[i] = x < 0 ? ~0ull : 0;
  }
  bool neg() const { return w[W - 1] >> 63; }
  Big operator+(const Big& b) const {
    Big r;
    unsigned __int128 c = 0;
    for (int i = 0; i < W; ++i) {
      c += (unsigned __int128)w[i] + b.w[i];
      r.w[i] = (uint64_t)c;
      c >>= 64;
    }
    return r;
  }
  Big operator-() const {
    Big r;
    for (int i = 0; i < W; ++i) r.w[i] = ~w[i];
    return r + Big(1);
  }
  Big operator-(const Big& b) const { return *this + (-b); }
  Big operator*(const Big& b) const {  // exact while |a| |b| < 2^767
    const bool n = neg() != b.neg();
    const Big x = neg() ? -*this : *this, y = b.neg() ? -b : b;
    Big r;
    for (int i = 0; i < W; ++i) {
      unsigned __int128 c = 0;
      for (int j = 0; i + j < W; ++j) {
        c += (unsigned __int128)x.w[i] * y.w[j] + r.w[i + j];
        r.w[i + j] = (uint64_t)c;
        c >>= 64;
      }
    }
    return n ? -r : r;
  }
  Big shl(int k) const {
    Big r;
    const int q = k / 64, s = k % 64;
    for (int i = W - 1; i >= q; --i) {
      r.w[i] = w[i - q] << s;
      if (s && i - q - 1 >= 0) r.w[i] |= w[i - q - 1] >> (64 - s);
    }
    return r;
  }
  Big sar(int k) const {  // floor(x / 2^k)
    Big r;
    const int q = k / 64, s = k % 64;
    const uint64_t f = neg() ? ~0ull : 0;
    for (int i = 0; i < W; ++i) {
      const uint64_t lo = i + q < W ? w[i + q] : f, hi = i + q + 1 < W ? w[i + q + 1] : f;
      r.w[i] = s ? (lo >> s) | (hi << (64 - s)) : lo;
    }
    return r;
  }
  Big cdiv2k(int k) const { return -((-*this).sar(k)); }  // ceil(x / 2^k)
  int cmp(const Big& b) const {
    if (neg() != b.neg()) return neg() ? -1 : 1;
    for (int i = W - 1; i >= 0; --i)
      if (w[i] != b.w[i]) return w[i] < b.w[i] ? -1 : 1;
    return 0;
  }
  bool operator<(const Big& b) const { return cmp(b) < 0; }
  bool operator<=(const Big& b) const { return cmp(b) <= 0; }
  bool operator==(const Big& b) const { return cmp(b) == 0; }
  static Big pow2(int k) { return Big(1).shl(k); }
  long long i64() const { return (long long)w[0]; }  // the caller knows it fits
  bool fits64() const {
    const uint64_t f = neg() ? ~0ull : 0;
    for (int i = 1; i < W; ++i)
      if (w[i] != f) return false;
    return (w[0] >> 63) == (f & 1);
  }
  std::string hex() const {
    const Big a = neg() ? -*this : *this;
    std::string s;
    bool on = false;
    char buf[20];
    for (int i = W - 1; i >= 0; --i) {
      if (!on && a.w[i] == 0 && i > 0) continue;
      snprintf(buf, sizeof buf, on ? "%016llx" : "%llx", (unsigned long long)a.w[i]);
      s += buf;
      on = true;
    }
    return (neg() ? "-0x" : "0x") + s;
  }
  long double ld() const {
    const Big a = neg() ? -*this : *this;
    long double r = 0;
    for (int i = W - 1; i >= 0; --i) r = r * 18446744073709551616.0L + (long double)a.w[i];
    return neg() ? -r : r;
  }
};
static inline Big bmin(const Big& a, const Big& b) { return a < b ? a : b; }
static inline Big bmax(const Big& a, const Big& b) { return a < b ? b : a; }

// ------------------------------------------------------------------ failures, paths, labels
struct Ctx {
  std::string chain;                       // the chain being evaluated
  std::string pending;                     // first failure seen inside a primitive: reported by its note()
  std::string negpend;                     // a possibly wrapped top limb was read as an operand
  std::vector<int> path;                   // data-dependent branch outcomes of this run
  size_t pos = 0;
  std::map<std::string, int> count;        // notes so far per (op, primitive), this run
  unsigned __int128 colmax = 0;            // worst column accumulator since the last note
  int shoup_k = 0;                         // mont_shoup: q >= floor - shoup_k (last note)
  long escapes = 0, checked = 0;           // concrete cross-check
  int next_bit() {
    if (pos == path.size()) path.push_back(0);
    return path[pos++];
  }
  bool next_path() {
    while (!path.empty() && path.back() == 1) path.pop_back();
    if (path.empty()) return false;
    path.back() = 1;
    return true;
  }
  void begin_run() {
    pos = 0;
    count.clear();
    pending.clear();
    negpend.clear();
    colmax = 0;
  }
};
inline Ctx g;

[[noreturn]] static inline void fail(const std::string& op, const std::string& what) {
  printf("FAIL chain=%s op=%s: %s\n", g.chain.c_str(), op.c_str(), what.c_str());
  fflush(stdout);
  exit(1);
}
static inline void defer_fail(const std::string& what) {
  if (g.pending.empty()) g.pending = what;
}
static inline std::string i2s(long long x) { return std::to_string(x); }

// ------------------------------------------------------------------ interval stand-ins for the scalar types
struct ABool {  // a comparison whose outcome the intervals may leave open: then every outcome is visited
  bool t, f;
  operator bool() const { return t && f ? g.next_bit() != 0 : t; }
};

struct ATrunc;
struct ALimb {  // uint32_t limb.  lo < 0: a borrow form's top limb that may have wrapped below zero
  long long lo = 0, hi = 0;
  const char* org = nullptr;  // the borrow form it came from, and its limb index
  int idx = -1;
  ALimb() {}
  ALimb(long long k) : lo(k), hi(k) {}
  ALimb(long long l, long long h) : lo(l), hi(h) {}
  inline ALimb(const ATrunc& t);
  std::string str() const { return "[" + i2s(lo) + ", " + i2s(hi) + "]"; }
  std::string who() const {
    return org ? std::string(idx == NL - 1 ? "top limb" : "limb " + i2s(idx)) + " of a " + org + " result" : std::string("a limb");
  }
  void need_nonneg(const char* use) const {
    if (lo < 0) defer_fail(who() + " may wrap below zero, " + str() + ", and is " + use);
  }
  ALimb chk() const {
    if (hi >= (1ll << 32)) defer_fail("a limb expression reaches 2^32: " + str());
    return *this;
  }
};
static inline ALimb operator+(const ALimb& a, const ALimb& b) {
  ALimb r(a.lo + b.lo, a.hi + b.hi);
  r.org = a.org, r.idx = a.idx;
  return r.chk();
}
static inline ALimb operator+(const ALimb& a, long long k) { return a + ALimb(k); }
static inline ALimb operator-(const ALimb& a, const ALimb& b) { return ALimb(a.lo - b.hi, a.hi - b.lo); }
static inline ALimb& operator+=(ALimb& a, const ALimb& b) { return a = a + b; }
static inline ALimb& operator-=(ALimb& a, const ALimb& b) { return a = a - b; }
static inline ALimb operator<<(const ALimb& a, int k) {
  a.need_nonneg("shifted");
  if (k < 0 || k > 31) defer_fail("shift count out of range");
  if ((a.hi << k) >= (1ll << 32)) defer_fail("<< " + i2s(k) + " loses a bit: " + a.str());
  return ALimb(a.lo << k, a.hi << k);
}
static inline ALimb operator>>(const ALimb& a, int k) {
  a.need_nonneg("shifted");
  if (k < 0 || k > 31) defer_fail("shift count out of range");
  return ALimb(a.lo >> k, a.hi >> k);
}
// x mod 2^n over an interval (two's complement: also right for negative x)
static inline ALimb mask_iv(__int128 lo, __int128 hi, uint32_t mask) {
  const __int128 M = (__int128)mask + 1;
  if ((M & mask) != 0) return ALimb(0, mask);  // not 2^n - 1
  auto fl = [&](__int128 x) { return x >= 0 ? x / M : -((-x + M - 1) / M); };
  if (fl(lo) != fl(hi)) return ALimb(0, mask);
  return ALimb((long long)(lo - fl(lo) * M), (long long)(hi - fl(hi) * M));
}
static inline ALimb operator&(const ALimb& a, uint32_t mask) {
  a.need_nonneg("masked");
  return mask_iv(a.lo, a.hi, mask);
}
static inline ALimb& operator&=(ALimb& a, uint32_t mask) { return a = a & mask; }
static inline ALimb bitop(const ALimb& a, const ALimb& b, bool exact_or) {
  a.need_nonneg("a bit operand");
  b.need_nonneg("a bit operand");
  if (a.lo == a.hi && b.lo == b.hi) return ALimb(exact_or ? (a.lo | b.lo) : (a.lo ^ b.lo));
  long long m = 1;
  while (m <= a.hi || m <= b.hi) m <<= 1;
  return ALimb(0, m - 1);
}
static inline ALimb operator|(const ALimb& a, const ALimb& b) { return bitop(a, b, true); }
static inline ALimb operator^(const ALimb& a, const ALimb& b) { return bitop(a, b, false); }
static inline ALimb& operator|=(ALimb& a, const ALimb& b) { return a = a | b; }
static inline ABool operator==(const ALimb& a, long long k) {
  return ABool{a.lo <= k && k <= a.hi, !(a.lo == k && a.hi == k)};
}

struct ASLimb {  // int32_t
  long long lo = 0, hi = 0;
  ASLimb() {}
  ASLimb(long long k) : lo(k), hi(k) {}
  ASLimb(long long l, long long h) : lo(l), hi(h) {
    if (lo < -(1ll << 31) || hi >= (1ll << 31)) defer_fail("a signed limb expression leaves int32_t");
  }
};
static inline ASLimb operator-(const ASLimb& a, int32_t k) { return ASLimb(a.lo - k, a.hi - k); }
static inline ASLimb operator+(const ASLimb& a, const ASLimb& b) { return ASLimb(a.lo + b.lo, a.hi + b.hi); }
static inline ASLimb operator>>(const ASLimb& a, int k) { return ASLimb(a.lo >> k, a.hi >> k); }  // arithmetic
static inline ABool operator>=(const ASLimb& a, int k) { return ABool{a.hi >= k, a.lo < k}; }
static inline ABool operator>(const ASLimb& a, int k) { return ABool{a.hi > k, a.lo <= k}; }
// a limb read as int32_t: a wrapped (negative) interval reads as itself
static inline ASLimb sgn(const ALimb& a) { return ASLimb(a.lo, a.hi); }

struct ATrunc {  // (uint32_t)x of a wider x: fine when masked or multiplied and masked, else x must fit
  __int128 lo, hi;
  bool any;  // nothing known (a wrapped product)
};
static inline ATrunc unsg(const ASLimb& a) { return ATrunc{a.lo, a.hi, false}; }
static inline ALimb operator&(const ATrunc& t, uint32_t mask) { return t.any ? ALimb(0, mask) : mask_iv(t.lo, t.hi, mask); }
static inline ATrunc operator*(const ATrunc&, uint32_t) { return ATrunc{0, 0, true}; }
inline ALimb::ALimb(const ATrunc& t) {
  if (t.any || t.lo < 0 || t.hi >= ((__int128)1 << 32)) {
    defer_fail("a 64-bit value is truncated to 32 bits without a mask");
    lo = 0, hi = 0xffffffffll;
  } else {
    lo = (long long)t.lo, hi = (long long)t.hi;
  }
}

struct AAcc {  // uint64_t column accumulator
  unsigned __int128 lo = 0, hi = 0;
  int col = 0;  // columns shifted out so far
  AAcc() {}
  AAcc(long long k) : lo(k), hi(k) {}
  AAcc(unsigned __int128 l, unsigned __int128 h, int c = 0) : lo(l), hi(h), col(c) {
    if (hi > g.colmax) g.colmax = hi;
    if (hi >> 64) defer_fail("a 64-bit column accumulator reaches 2^64 (column step " + i2s(col) + ")");
  }
};
static inline AAcc wide(const ALimb& a) {
  if (a.lo < 0) {  // read as the wrapped word: only qreduce's top limb may, and its note() must justify it
    if (g.negpend.empty()) g.negpend = a.who() + " may wrap below zero, " + a.str();
    return AAcc(0, (unsigned __int128)(a.hi < 0 ? 0xffffffffll : std::max(a.hi, 0xffffffffll)));
  }
  return AAcc((unsigned __int128)a.lo, (unsigned __int128)a.hi);
}
static inline AAcc wide(const ATrunc& t) {
  if (t.any || t.lo < 0 || t.hi >= ((__int128)1 << 32)) return AAcc(0, 0xffffffffull);
  return AAcc((unsigned __int128)t.lo, (unsigned __int128)t.hi);
}
static inline AAcc operator*(const AAcc& a, const ALimb& b) {
  b.need_nonneg("multiplied");
  const unsigned __int128 bl = b.lo < 0 ? 0 : b.lo, bh = b.hi < 0 ? 0 : b.hi;
  return AAcc(a.lo * bl, a.hi * bh, a.col);
}
static inline AAcc operator*(const AAcc& a, uint32_t k) { return AAcc(a.lo * k, a.hi * k, a.col); }
static inline AAcc operator+(const AAcc& a, const AAcc& b) { return AAcc(a.lo + b.lo, a.hi + b.hi, a.col); }
static inline AAcc& operator+=(AAcc& a, const AAcc& b) { return a = AAcc(a.lo + b.lo, a.hi + b.hi, a.col); }
static inline AAcc operator>>(const AAcc& a, int k) { return AAcc(a.lo >> k, a.hi >> k, a.col + 1); }
static inline AAcc& operator>>=(AAcc& a, int k) { return a = a >> k; }
static inline ATrunc lo32(const AAcc& a) { return ATrunc{(__int128)a.lo, (__int128)a.hi, false}; }

// cond_sub's select: both arms joined unless the comparison is decided
static inline ALimb select(const ABool& c, const ALimb& a, const ALimb& b) {
  if (!c.f) return a;
  if (!c.t) return b;
  return ALimb(std::min(a.lo, b.lo), std::max(a.hi, b.hi));
}

// ------------------------------------------------------------------ the abstract element
template <class B>
struct Abs : B {};
template <class B>
struct Rec : B {};

template <class B>
struct Fe<Abs<B>> {
  ALimb v[NL];
  bool hv = false;  // vlo / vhi set by a note(); otherwise the value is what the limbs say
  Big vlo, vhi;
};

template <class T>
struct CfgName;
template <>
struct CfgName<FqCfg> {
  static const char* s() { return "Fq"; }
};
template <>
struct CfgName<FqAccCfg> {
  static const char* s() { return "FqAcc"; }
};
template <>
struct CfgName<FrCfg> {
  static const char* s() { return "Fr"; }
};

template <class B>
static Big tab_val(const uint32_t (&k)[NL]) {
  Big r;
  for (int i = NL - 1; i >= 0; --i) r = r.shl(LB) + Big((long long)k[i]);
  return r;
}
template <class B>
static Big modulus() { return tab_val<B>(B::MOD); }

template <class E>
static void limb_sum(const E& e, int n, Big& lo, Big& hi) {  // sum of limbs 0..n-1 by weight
  lo = Big(0), hi = Big(0);
  for (int i = n - 1; i >= 0; --i) {
    lo = lo.shl(LB) + Big(e.v[i].lo);
    hi = hi.shl(LB) + Big(e.v[i].hi);
  }
}
// The value interval of an element: what a note() proved, cut with what the limbs allow.
template <class B>
static void get_val(const Fe<Abs<B>>& e, Big& lo, Big& hi) {
  limb_sum(e, NL, lo, hi);
  if (e.hv) lo = bmax(lo, e.vlo), hi = bmin(hi, e.vhi);
}
// Limbs and value constrain each other: value = low + top 2^232 exactly (raw or normalised), so the
// top limb lies in [ceil((vlo - low_hi) / 2^232), floor((vhi - low_lo) / 2^232)], and the value
// inside the limbs' own range.  An empty cut means a transfer function contradicts the limb code.
template <class B>
static void refine(Fe<Abs<B>>& e, const Big& vlo, const Big& vhi, const std::string& op) {
  Big llo, lhi, slo, shi;
  limb_sum(e, NL - 1, llo, lhi);
  limb_sum(e, NL, slo, shi);
  e.hv = true;
  e.vlo = bmax(vlo, slo);
  e.vhi = bmin(vhi, shi);
  if (e.vhi < e.vlo) fail(op, "value interval and limb intervals contradict each other");
  const Big tl = (e.vlo - lhi).cdiv2k(LB * (NL - 1)), th = (e.vhi - llo).sar(LB * (NL - 1));
  ALimb& t = e.v[NL - 1];
  if (tl.fits64() && t.lo < tl.i64()) t.lo = tl.i64();
  if (th.fits64() && th.i64() < t.hi) t.hi = th.i64();
  if (t.hi < t.lo) fail(op, "value interval and top limb contradict each other");
}

// ------------------------------------------------------------------ what is recorded per step
struct Rec1 {
  Big vlo, vhi;
  long long lo[NL], hi[NL];
  long double col = 0;  // worst column accumulator / 2^64
  int shoup_k = -1;
  int order = 0;
};
inline std::map<std::string, Rec1> g_rec;
inline std::vector<std::string> g_order;

static inline std::string step_label(const char* fn, const char* prim) {
  std::string k = std::string(fn) + "." + prim;
  if (k == std::string(fn) + "." + fn) k = fn;
  const int n = g.count[k]++;
  return g.chain + " " + k + "#" + i2s(n);
}
// what went wrong inside the primitive is reported under its op name; a possibly wrapped top limb that
// was read as an operand comes first (what follows from reading it is noise), except in qreduce,
// whose note() decides whether the value justifies it
static inline void begin_note(const char* fn, bool wrapped_top_ok = false) {
  if (!wrapped_top_ok && !g.negpend.empty()) fail(fn, "operand: " + g.negpend);
  if (!g.pending.empty()) fail(fn, g.pending);
}

template <class B>
static void record(const std::string& lab, const Fe<Abs<B>>& e) {
  Big lo, hi;
  get_val(e, lo, hi);
  auto it = g_rec.find(lab);
  if (it == g_rec.end()) {
    Rec1 r;
    r.vlo = lo, r.vhi = hi;
    for (int i = 0; i < NL; ++i) r.lo[i] = e.v[i].lo, r.hi[i] = e.v[i].hi;
    r.order = (int)g_order.size();
    g_order.push_back(lab);
    it = g_rec.emplace(lab, r).first;
  } else {
    Rec1& r = it->second;
    r.vlo = bmin(r.vlo, lo), r.vhi = bmax(r.vhi, hi);
    for (int i = 0; i < NL; ++i) r.lo[i] = std::min(r.lo[i], e.v[i].lo), r.hi[i] = std::max(r.hi[i], e.v[i].hi);
  }
  const long double c = (long double)g.colmax / 18446744073709551616.0L;
  if (c > it->second.col) it->second.col = c;
  if (g.shoup_k > it->second.shoup_k) it->second.shoup_k = g.shoup_k;
  g.colmax = 0;
  g.shoup_k = -1;
}

template <class B>
static void need_known_nonneg(const Fe<Abs<B>>& a, const char* fn, const char* what, Big& lo, Big& hi) {
  get_val(a, lo, hi);
  if (lo.neg()) fail(fn, std::string(what) + " may be negative");
  for (int i = 0; i < NL; ++i)
    if (a.v[i].lo < 0) fail(fn, std::string(what) + ": " + a.v[i].who() + " may wrap below zero, " + a.v[i].str());
}
template <class B>
static long long max_low_limb(const Fe<Abs<B>>& a) {
  long long m = 0;
  for (int i = 0; i < NL - 1; ++i) m = std::max(m, a.v[i].hi);
  return m;
}

// ------------------------------------------------------------------ the transfer functions
template <class B>
struct FeTypes<Abs<B>> {
  using C = Abs<B>;
  using E = Fe<C>;
  using limb = ALimb;
  using slimb = ASLimb;
  using acc = AAcc;
  static constexpr int TOPW = LB * (NL - 1);

  static void no_negpend(const char* fn) {
    if (!g.negpend.empty()) fail(fn, "operand: " + g.negpend);
  }

  // Montgomery sum of products.  The column loop computes (sum a_k b_k + M m) / 2^261 exactly, M the
  // number whose digits are the quotient digits m_i < 2^29, so 0 <= M < 2^261 (C::INV is checked to be
  // -1/m mod 2^29 at start-up, which is what makes the division exact); all operands >= 0.
  // Contract (field.hpp): N = 1: both operands' limbs 0..7 < 2^30, or one < 2.5 * 2^30 against a normalised
  // one; N = 2: every operand normalised but at most ONE, with limbs < 2^31; N = 4: every operand normalised.
  template <int N>
  static void note(n_sop, const char* fn, const E* const (&a)[N], const E* const (&b)[N], E& r) {
    begin_note(fn);
    no_negpend(fn);
    Big slo, shi;
    int raw_ops = 0;
    for (int k = 0; k < N; ++k) {
      Big al, ah, bl, bh;
      need_known_nonneg(*a[k], fn, "operand", al, ah);
      need_known_nonneg(*b[k], fn, "operand", bl, bh);
      slo = slo + al * bl, shi = shi + ah * bh;
      const long long ma = max_low_limb(*a[k]), mb = max_low_limb(*b[k]);
      raw_ops += (ma > LMASK) + (mb > LMASK);
      if (N > 1 && (raw_ops > (N == 2 ? 1 : 0) || std::max(ma, mb) >= (1ll << 31)))
        fail(fn, "a sum of " + i2s(N) + " products has " + i2s(raw_ops) + " operands that are not normalised (limb up to " +
                     i2s(std::max(ma, mb)) + ")");
      if (N == 1 && !((ma < (1ll << 30) && mb < (1ll << 30)) || (std::max(ma, mb) < 5 * (1ll << 29) && std::min(ma, mb) <= LMASK)))
        fail(fn, "operand limbs outside the product's contract (" + i2s(ma) + ", " + i2s(mb) + ")");
    }
    const Big m = modulus<B>();
    refine(r, slo.sar(LB * NL), (shi + (Big::pow2(LB * NL) - Big(1)) * m).sar(LB * NL), fn);
    record(step_label(fn, "sop"), r);
  }
  static void note(n_sqr, const char* fn, const E& a, E& r) {
    begin_note(fn);
    no_negpend(fn);
    Big al, ah;
    need_known_nonneg(a, fn, "operand", al, ah);
    if (max_low_limb(a) >= (1ll << 30)) fail(fn, "operand limbs outside the square's contract");
    const Big m = modulus<B>();
    refine(r, (al * al).sar(LB * NL), (ah * ah + (Big::pow2(LB * NL) - Big(1)) * m).sar(LB * NL), fn);
    record(step_label(fn, "sqr"), r);
  }
  // Shoup product by a constant w < m with wq = floor(w 2^261 / m) (both taken as the root tables'
  // invariant).  With A the operand's value, qt = floor(A wq / 2^261) has A w - qt m in
  // [0, m (1 + A / 2^261)): from w 2^261 / m - 1 < wq <= w 2^261 / m.  The code's q is the floor of
  // (A wq - D) / 2^261, D the dropped columns 0..6, so qt - k <= q <= qt for k = ceil(D_max / 2^261)
  // (D_max from the limb maxima; k = 1 is the comment's "exact floor or one less"), and the result
  // A w - q m lies in [0, m (1 + k + A / 2^261)).  It must stay below 2^261, which the low 9 columns hold.
  static void note(n_shoup, const char* fn, const E& a, const E& w, const E& wq, E& r) {
    begin_note(fn);
    no_negpend(fn);
    Big al, ah, wl, wh, ql, qh;
    need_known_nonneg(a, fn, "operand", al, ah);
    need_known_nonneg(w, fn, "root", wl, wh);
    need_known_nonneg(wq, fn, "root quotient", ql, qh);
    const Big m = modulus<B>(), R = Big::pow2(LB * NL);
    if (!(wh < m) || !(qh < R)) fail(fn, "root operands outside the table invariant");
    Big D;
    for (int c = 6; c >= 0; --c) {
      Big col;
      for (int i = 0; i <= c; ++i) col = col + Big(a.v[i].hi) * Big(wq.v[c - i].hi);
      D = D.shl(LB) + col;
    }
    const Big k = D.cdiv2k(LB * NL);
    g.shoup_k = (int)k.i64();
    const Big hi = (((Big(1) + k) * R + ah) * m).sar(LB * NL);
    if (!(hi < R)) fail(fn, "result may reach 2^261");
    refine(r, Big(0), hi, fn);
    record(step_label(fn, "shoup"), r);
  }
  // The carry pass keeps the value; afterwards limbs 0..7 are < 2^29, so the top limb is
  // floor(value / 2^232): it is >= 0 exactly when the value is, whatever the raw top limb looked like.
  static void note(n_normalize, const char* fn, E& a) {
    begin_note(fn);
    Big lo, hi;
    get_val(a, lo, hi);
    if (lo.neg()) fail(fn, "the value may be negative (" + lo.hex() + "): the top limb wraps below zero");
    ALimb& t = a.v[NL - 1];
    refine(a, lo, hi, fn);
    if (t.lo < 0) fail(fn, "top limb may stay below zero");
    if (t.hi >= (1ll << 32)) fail(fn, "top limb reaches 2^32");
    record(step_label(fn, "normalize"), a);
  }
  // a normalised and >= 0, M normalised: the borrow chain's last carry is >= 0 exactly when a >= M, so
  // the result is a - M on [max(vlo, M), vhi] and a on [vlo, min(vhi, M - 1)].  The masked top limb of
  // a - M is its whole value as long as a - M < 2^261.
  static void note(n_cond_sub, const char* fn, const E& a, const uint32_t (&M)[NL], E& r) {
    begin_note(fn);
    Big lo, hi;
    need_known_nonneg(a, fn, "operand", lo, hi);
    if (max_low_limb(a) > LMASK) fail(fn, "operand of a conditional subtraction is not normalised");
    const Big Mv = tab_val<B>(M);
    if (!(hi - Mv < Big::pow2(LB * NL))) fail(fn, "difference may reach 2^261");
    Big rl, rh;
    if (hi < Mv) rl = lo, rh = hi;
    else if (Mv <= lo) rl = lo - Mv, rh = hi - Mv;
    else rl = Big(0), rh = bmax(hi - Mv, Mv - Big(1));
    r.v[NL - 1] = ALimb(0, std::max(r.v[NL - 1].hi, a.v[NL - 1].hi));
    refine(r, rl, rh, fn);
    record(step_label(fn, "cond_sub"), r);
  }
  // s: limbs 0..7 >= 0 (checked where they are read) with s_i + carry < 2^32, value v in [0, 2^261).
  // top = s_8 read as int32_t.  top > 0: q = floor(top QK / 2^32) with QK = floor(2^264 / m) (checked at
  // start-up), so q m <= top 2^232 <= v (low limbs >= 0): the result v - q m is >= 0; and
  // q > top (2^264 / m - 1) / 2^32 - 1 gives q m > top 2^232 - top m / 2^32 - m, so the result is
  // < low + m + top m / 2^32 for low = the raw limbs 0..7 by weight.  top <= 0: q = 0 and the carry
  // pass returns v itself (v >= 0 is what makes the wrapped top limb come back above zero), and
  // v <= low.  Both arms: result <= min(vhi, low_hi + m + top_hi m / 2^32), computed mod 2^261 = itself.
  static void note(n_qreduce, const char* fn, const E& s, E& r) {
    begin_note(fn, true);
    if (!s.hv && s.v[NL - 1].lo < 0) fail(fn, "reducing an element of unknown value");
    Big lo, hi;
    get_val(s, lo, hi);
    if (lo.neg()) fail(fn, "the value may be negative (" + lo.hex() + "): " + (g.negpend.empty() ? "top limb wraps" : g.negpend));
    g.negpend.clear();  // justified: the value is >= 0
    for (int i = 0; i < NL - 1; ++i)
      if (s.v[i].lo < 0) fail(fn, s.v[i].who() + " may wrap below zero");
    if (!(hi < Big::pow2(LB * NL))) fail(fn, "the value may reach 2^261");
    Big llo, lhi;
    limb_sum(s, NL - 1, llo, lhi);
    const Big m = modulus<B>();
    const long long th = std::max(s.v[NL - 1].hi, 0ll);
    const Big rh = bmin(hi, lhi + m + (Big(th) * m).sar(32));
    refine(r, Big(0), rh, fn);
    record(step_label(fn, "qreduce"), r);
  }
  static void note(n_add_raw, const char* fn, const E& a, const E& b, E& s) {
    begin_note(fn);
    Big al, ah, bl, bh;
    get_val(a, al, ah);
    get_val(b, bl, bh);
    refine(s, al + bl, ah + bh, fn);
    record(step_label(fn, "add_raw"), s);
  }
  // s = a + K - b - 2c limb by limb and therefore by value.  Limbs 0..7 must stay >= 0; the top limb
  // may look negative here (its consumer decides: normalize and qreduce accept it when the value is >= 0).
  template <class T>
  static void note(n_borrow_sub, const char* fn, const E& a, T K, const E& b, const E* c, E& s) {
    begin_note(fn);
    Big al, ah, bl, bh, cl, ch, Kv;
    get_val(a, al, ah);
    get_val(b, bl, bh);
    if (c) get_val(*c, cl, ch);
    for (int i = NL - 1; i >= 0; --i) Kv = Kv.shl(LB) + Big((long long)K(i));
    for (int i = 0; i < NL; ++i) s.v[i].org = fn, s.v[i].idx = i;
    for (int i = 0; i < NL - 1; ++i)
      if (s.v[i].lo < 0) fail(fn, "limb " + i2s(i) + " may go below zero: " + s.v[i].str());
    refine(s, al + Kv - bh - ch - ch, ah + Kv - bl - cl - cl, fn);
    for (int i = 0; i < NL; ++i) s.v[i].org = fn, s.v[i].idx = i;
    record(step_label(fn, "borrow_sub"), s);
  }
  static void note(n_shl1, const char* fn, const E& a, E& s) {
    begin_note(fn);
    Big al, ah;
    get_val(a, al, ah);
    refine(s, al + al, ah + ah, fn);
    record(step_label(fn, "shl1"), s);
  }
};

// ------------------------------------------------------------------ the concrete twin
template <class B>
struct FeTypes<Rec<B>> {
  using limb = uint32_t;
  using slimb = int32_t;
  using acc = uint64_t;
  using E = Fe<Rec<B>>;
  static void check(const std::string& lab, const E& e) {
    auto it = g_rec.find(lab);
    ++g.checked;
    if (it == g_rec.end()) {
      ++g.escapes;
      printf("ESCAPE %s: step not visited by the abstract run\n", lab.c_str());
      return;
    }
    const Rec1& r = it->second;
    Big v;
    for (int i = NL - 1; i >= 0; --i) {
      // a top limb the proof allows below zero is compared as the signed word
      const long long x = (i == NL - 1 && r.lo[i] < 0) ? (long long)(int32_t)e.v[i] : (long long)e.v[i];
      v = v.shl(LB) + Big(x);
      if (x < r.lo[i] || x > r.hi[i]) {
        ++g.escapes;
        printf("ESCAPE %s: limb %d = %lld outside [%lld, %lld]\n", lab.c_str(), i, x, r.lo[i], r.hi[i]);
      }
    }
    if (v < r.vlo || r.vhi < v) {
      ++g.escapes;
      printf("ESCAPE %s: value %s outside [%s, %s]\n", lab.c_str(), v.hex().c_str(), r.vlo.hex().c_str(), r.vhi.hex().c_str());
    }
  }
  template <int N>
  static void note(n_sop, const char* fn, const E* const (&)[N], const E* const (&)[N], E& r) { check(step_label(fn, "sop"), r); }
  static void note(n_sqr, const char* fn, const E&, E& r) { check(step_label(fn, "sqr"), r); }
  static void note(n_shoup, const char* fn, const E&, const E&, const E&, E& r) { check(step_label(fn, "shoup"), r); }
  static void note(n_normalize, const char* fn, E& a) { check(step_label(fn, "normalize"), a); }
  static void note(n_cond_sub, const char* fn, const E&, const uint32_t (&)[NL], E& r) { check(step_label(fn, "cond_sub"), r); }
  static void note(n_qreduce, const char* fn, const E&, E& r) { check(step_label(fn, "qreduce"), r); }
  static void note(n_add_raw, const char* fn, const E&, const E&, E& s) { check(step_label(fn, "add_raw"), s); }
  template <class T>
  static void note(n_borrow_sub, const char* fn, const E&, T, const E&, const E*, E& s) { check(step_label(fn, "borrow_sub"), s); }
  static void note(n_shl1, const char* fn, const E&, E& s) { check(step_label(fn, "shl1"), s); }
};

}  // namespace zkp
