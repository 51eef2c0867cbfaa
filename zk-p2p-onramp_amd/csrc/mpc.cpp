// Phase-2 MPC record of a zkey (see mpc.hpp; restatement checked against oracle/mpc.py).
#include "mpc.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <fstream>
#include <thread>

#include "beacon.hpp"
#include "host_pairing.hpp"
#include "prover.hpp"
#include "ptau_contribute.hpp"
#include "ptau_verify.hpp"
#include "spans.hpp"
#include "zkey_bellman.hpp"
#include "zkey_verify.hpp"

namespace zkp {

using host::Affine;
using host::Jac;
using host::U256;
using HFq = host::Fq;
using HFq2 = host::Fq2;
using HFr = host::Fr;

// ---------------------------------------------------------------- Blake2b-512 (RFC 7693)
namespace {
constexpr uint64_t B2_IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                               0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                               0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
constexpr uint8_t B2_SIGMA[12][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
inline uint64_t rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
inline uint32_t rotl32(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
}  // namespace

Blake2b::Blake2b() {
  for (int i = 0; i < 8; ++i) h_[i] = B2_IV[i];
  h_[0] ^= 0x01010000ull ^ 64ull;  // no key, 64-byte digest
}

void Blake2b::compress(bool last) {
  uint64_t m[16], v[16];
  for (int i = 0; i < 16; ++i) {
    uint64_t x = 0;
    for (int b = 7; b >= 0; --b) x = (x << 8) | buf_[8 * i + b];
    m[i] = x;
  }
  for (int i = 0; i < 8; ++i) v[i] = h_[i], v[i + 8] = B2_IV[i];
  v[12] ^= t_[0];
  v[13] ^= t_[1];
  if (last) v[14] = ~v[14];
  auto g = [&](int a, int b, int c, int d, uint64_t x, uint64_t y) {
    v[a] = v[a] + v[b] + x;
    v[d] = rotr64(v[d] ^ v[a], 32);
    v[c] = v[c] + v[d];
    v[b] = rotr64(v[b] ^ v[c], 24);
    v[a] = v[a] + v[b] + y;
    v[d] = rotr64(v[d] ^ v[a], 16);
    v[c] = v[c] + v[d];
    v[b] = rotr64(v[b] ^ v[c], 63);
  };
  for (int r = 0; r < 12; ++r) {
    const uint8_t* s = B2_SIGMA[r];
    g(0, 4, 8, 12, m[s[0]], m[s[1]]);
    g(1, 5, 9, 13, m[s[2]], m[s[3]]);
    g(2, 6, 10, 14, m[s[4]], m[s[5]]);
    g(3, 7, 11, 15, m[s[6]], m[s[7]]);
    g(0, 5, 10, 15, m[s[8]], m[s[9]]);
    g(1, 6, 11, 12, m[s[10]], m[s[11]]);
    g(2, 7, 8, 13, m[s[12]], m[s[13]]);
    g(3, 4, 9, 14, m[s[14]], m[s[15]]);
  }
  for (int i = 0; i < 8; ++i) h_[i] ^= v[i] ^ v[i + 8];
}

void Blake2b::update(const void* data, size_t len) {
  const uint8_t* p = static_cast<const uint8_t*>(data);
  while (len > 0) {
    if (n_ == 128) {  // the buffered block is not the last one: compress it
      t_[0] += 128;
      if (t_[0] < 128) ++t_[1];
      compress(false);
      n_ = 0;
    }
    const size_t k = std::min(len, (size_t)128 - n_);
    std::memcpy(buf_ + n_, p, k);
    n_ += k, p += k, len -= k;
  }
}

void Blake2b::final(uint8_t out[64]) {
  t_[0] += n_;
  if (t_[0] < n_) ++t_[1];
  std::memset(buf_ + n_, 0, 128 - n_);
  compress(true);
  for (int i = 0; i < 8; ++i)
    for (int b = 0; b < 8; ++b) out[8 * i + b] = (uint8_t)(h_[i] >> (8 * b));
}

// ---------------------------------------------------------------- ChaCha word stream
ChaChaRng::ChaChaRng(const uint32_t seed[8]) {
  const uint32_t c[4] = {0x61707865, 0x3320646E, 0x79622D32, 0x6B206574};
  for (int i = 0; i < 4; ++i) st[i] = c[i];
  for (int i = 0; i < 8; ++i) st[4 + i] = seed[i];
  for (int i = 12; i < 16; ++i) st[i] = 0;
}

uint32_t ChaChaRng::next_u32() {
  if (idx == 16) {
    auto qr = [](uint32_t* x, int a, int b, int c, int d) {
      x[a] += x[b], x[d] = rotl32(x[d] ^ x[a], 16);
      x[c] += x[d], x[b] = rotl32(x[b] ^ x[c], 12);
      x[a] += x[b], x[d] = rotl32(x[d] ^ x[a], 8);
      x[c] += x[d], x[b] = rotl32(x[b] ^ x[c], 7);
    };
    std::memcpy(buf, st, sizeof st);
    for (int r = 0; r < 10; ++r) {
      qr(buf, 0, 4, 8, 12), qr(buf, 1, 5, 9, 13), qr(buf, 2, 6, 10, 14), qr(buf, 3, 7, 11, 15);
      qr(buf, 0, 5, 10, 15), qr(buf, 1, 6, 11, 12), qr(buf, 2, 7, 8, 13), qr(buf, 3, 4, 9, 14);
    }
    for (int i = 0; i < 16; ++i) buf[i] += st[i];
    idx = 0;
    for (int w = 12; w < 16; ++w)
      if (++st[w] != 0) break;
  }
  return buf[idx++];
}

uint64_t ChaChaRng::next_u64() {
  const uint64_t hi = next_u32();
  return hi << 32 | next_u32();
}

void seed_from_hash(const uint8_t* h, uint32_t seed[8]) {
  for (int i = 0; i < 8; ++i)
    seed[i] = (uint32_t)h[4 * i] << 24 | (uint32_t)h[4 * i + 1] << 16 | (uint32_t)h[4 * i + 2] << 8 | h[4 * i + 3];
}

namespace {

// ---------------------------------------------------------------- field / curve draws
U256 draw254(ChaChaRng& rng, const U256& mod) {  // ffjavascript F.fromRng: 4 x u64, 254 bits, < mod
  U256 v;
  do {
    for (int i = 0; i < 4; ++i) v.w[i] = rng.next_u64();
    v.w[3] &= (uint64_t(1) << 62) - 1;
  } while (host::u256_geq(v, mod));
  return v;
}
HFq fq_from_rng(ChaChaRng& rng) { return HFq::raw(draw254(rng, host::FQ_DESC.mod)); }  // Montgomery reading
HFr fr_from_rng(ChaChaRng& rng) { return HFr::raw(draw254(rng, host::FR_DESC.mod)); }

U256 half_p() {  // (p - 1) / 2
  U256 h = host::FQ_DESC.mod;
  for (int i = 0; i < 4; ++i) h.w[i] = (h.w[i] >> 1) | (i < 3 ? h.w[i + 1] << 63 : 0);
  return h;
}
bool fq_negative(const HFq& y) {
  const U256 v = y.to_std(), h = half_p();
  return !host::u256_geq(h, v);  // v > (p - 1) / 2
}
bool fq2_negative(const HFq2& y) { return y.c1.is_zero() ? fq_negative(y.c0) : fq_negative(y.c1); }

U256 exp_of(uint64_t add, int shift_right) {  // (p + add) >> shift_right (add may be "negative" via wrap)
  U256 e = host::FQ_DESC.mod, a{{add, 0, 0, 0}};
  host::u256_add(e, a);
  for (int s = 0; s < shift_right; ++s)
    for (int i = 0; i < 4; ++i) e.w[i] = (e.w[i] >> 1) | (i < 3 ? e.w[i + 1] << 63 : 0);
  return e;
}

bool fq_sqrt(const HFq& a, HFq& out) {  // p = 3 mod 4
  const HFq s = a.pow(exp_of(1, 2));  // (p + 1) / 4
  if (!(s.sqr() == a)) return false;
  out = s;
  return true;
}

HFq2 f2_pow(HFq2 b, const U256& e) {
  HFq2 r = HFq2::one();
  for (int i = 0; i < 256; ++i) {
    if ((e.w[i >> 6] >> (i & 63)) & 1) r = r * b;
    b = b.sqr();
  }
  return r;
}

bool fq2_sqrt(const HFq2& a, HFq2& out) {  // "Square root computation over even extension fields", p = 3 mod 4
  if (a.is_zero()) {
    out = a;
    return true;
  }
  U256 e34 = host::FQ_DESC.mod;  // (p - 3) / 4
  {
    U256 three{{3, 0, 0, 0}};
    host::u256_sub(e34, three);
    for (int s = 0; s < 2; ++s)
      for (int i = 0; i < 4; ++i) e34.w[i] = (e34.w[i] >> 1) | (i < 3 ? e34.w[i + 1] << 63 : 0);
  }
  const HFq2 a1 = f2_pow(a, e34);
  const HFq2 alpha = a1.sqr() * a;
  const HFq2 a0 = f2_pow(alpha, host::FQ_DESC.mod) * alpha;
  const HFq2 minus_one{HFq::one().neg(), HFq::zero()};
  if (a0 == minus_one) return false;
  const HFq2 x0 = a1 * a;
  HFq2 x;
  if (alpha == minus_one) {
    x = HFq2{HFq::zero(), HFq::one()} * x0;
  } else {
    U256 e12 = host::FQ_DESC.mod;  // (p - 1) / 2
    U256 one{{1, 0, 0, 0}};
    host::u256_sub(e12, one);
    for (int i = 0; i < 4; ++i) e12.w[i] = (e12.w[i] >> 1) | (i < 3 ? e12.w[i + 1] << 63 : 0);
    x = f2_pow(HFq2::one() + alpha, e12) * x0;
  }
  if (!(x.sqr() == a)) return false;
  out = x;
  return true;
}

HFq fq_small(uint64_t v) { return HFq::from_std(U256{{v, 0, 0, 0}}); }

Affine<HFq> g1_from_rng(ChaChaRng& rng) {
  HFq x, y;
  bool greatest;
  for (;;) {
    x = fq_from_rng(rng);
    greatest = rng.next_bool();
    if (fq_sqrt(x.sqr() * x + fq_small(3), y)) break;
  }
  if (greatest != fq_negative(y)) y = y.neg();
  return Affine<HFq>{x, y, false};
}

Affine<HFq2> g2_from_rng(ChaChaRng& rng) {
  static const HFq2 b2 = HFq2{fq_small(3), HFq::zero()} * HFq2{fq_small(9), fq_small(1)}.inv();
  HFq2 x, y;
  bool greatest;
  for (;;) {
    x.c0 = fq_from_rng(rng);
    x.c1 = fq_from_rng(rng);
    greatest = rng.next_bool();
    if (fq2_sqrt(x.sqr() * x + b2, y)) break;
  }
  if (greatest != fq2_negative(y)) y = y.neg();
  // times the twist's cofactor 2p - r (not reduced mod r: the point is not yet in G2)
  U256 cof = host::FQ_DESC.mod;
  host::u256_add(cof, host::FQ_DESC.mod);
  host::u256_sub(cof, host::FR_DESC.mod);
  return host::jac_to_aff(host::jac_mul(host::jac_from_aff(Affine<HFq2>{x, y, false}), cof));
}

Affine<HFq2> hash_to_g2(const uint8_t transcript[64]) {
  uint32_t seed[8];
  seed_from_hash(transcript, seed);
  ChaChaRng rng(seed);
  return g2_from_rng(rng);
}

// ---------------------------------------------------------------- encodings
void put_be(const HFq& x, uint8_t* o) {  // standard form, 32 bytes big-endian
  const U256 v = x.to_std();
  for (int i = 0; i < 32; ++i) o[31 - i] = (uint8_t)(v.w[i >> 3] >> (8 * (i & 7)));
}
void g1_u(const Affine<HFq>& p, uint8_t o[64]) {
  std::memset(o, 0, 64);
  if (p.inf) {
    o[0] = 0x40;
    return;
  }
  put_be(p.x, o);
  put_be(p.y, o + 32);
}
void g2_u(const Affine<HFq2>& p, uint8_t o[128]) {
  std::memset(o, 0, 128);
  if (p.inf) {
    o[0] = 0x40;
    return;
  }
  put_be(p.x.c1, o);
  put_be(p.x.c0, o + 32);
  put_be(p.y.c1, o + 64);
  put_be(p.y.c0, o + 96);
}
// LEM (zkey layout: Montgomery, little-endian; all-zero = infinity)
HFq fq_lem(const uint8_t* p) {
  const U256 v = host::u256_from_le(p);
  if (host::u256_geq(v, host::FQ_DESC.mod)) throw ZkpError(ZKP_ERR_FORMAT, "zkey: coordinate out of range");
  return HFq::raw(v);
}
bool zero_bytes(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (p[i]) return false;
  return true;
}
Affine<HFq> g1_lem(const uint8_t* p) {
  if (zero_bytes(p, 64)) return Affine<HFq>{HFq::zero(), HFq::zero(), true};
  return Affine<HFq>{fq_lem(p), fq_lem(p + 32), false};
}
Affine<HFq2> g2_lem(const uint8_t* p) {
  if (zero_bytes(p, 128)) return Affine<HFq2>{HFq2::zero(), HFq2::zero(), true};
  return Affine<HFq2>{HFq2{fq_lem(p), fq_lem(p + 32)}, HFq2{fq_lem(p + 64), fq_lem(p + 96)}, false};
}
void put_lem(std::vector<uint8_t>& o, const HFq& x) {
  uint8_t b[32];
  host::u256_to_le(x.v, b);
  o.insert(o.end(), b, b + 32);
}
void put_g1_lem(std::vector<uint8_t>& o, const Affine<HFq>& p) {
  if (p.inf) {
    o.insert(o.end(), 64, 0);
    return;
  }
  put_lem(o, p.x), put_lem(o, p.y);
}
void put_g2_lem(std::vector<uint8_t>& o, const Affine<HFq2>& p) {
  if (p.inf) {
    o.insert(o.end(), 128, 0);
    return;
  }
  put_lem(o, p.x.c0), put_lem(o, p.x.c1), put_lem(o, p.y.c0), put_lem(o, p.y.c1);
}
void put32(std::vector<uint8_t>& o, uint32_t v) {
  for (int i = 0; i < 4; ++i) o.push_back((uint8_t)(v >> (8 * i)));
}
uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
void u32be(Blake2b& h, uint32_t v) {
  const uint8_t b[4] = {(uint8_t)(v >> 24), (uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v};
  h.update(b, 4);
}

void hash_g1(Blake2b& h, const Affine<HFq>& p) {
  uint8_t b[64];
  g1_u(p, b);
  h.update(b, 64);
}
void hash_g2(Blake2b& h, const Affine<HFq2>& p) {
  uint8_t b[128];
  g2_u(p, b);
  h.update(b, 128);
}
void hash_pubkey(Blake2b& h, const MpcContribution& c) {
  hash_g1(h, c.delta_after);
  hash_g1(h, c.g1_s);
  hash_g1(h, c.g1_sx);
  hash_g2(h, c.g2_spx);
  h.update(c.transcript, 64);
}

Affine<HFq> g1_times(const Affine<HFq>& p, const U256& k) {
  return host::jac_to_aff(host::jac_mul(host::jac_from_aff(p), k));
}
Affine<HFq2> g2_times(const Affine<HFq2>& p, const U256& k) {
  return host::jac_to_aff(host::jac_mul(host::jac_from_aff(p), k));
}

// the "uncompressed" encoding of `count` zkey-layout points into the hash: converted by a few
// threads per block (a Venmo key holds ~34 M points), hashed in order
template <int PW>  // bytes per point: 64 (G1) or 128 (G2)
void hash_points(Blake2b& h, const uint8_t* lem, size_t count) {
  constexpr size_t BLOCK = size_t(1) << 16;
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<uint8_t> u(BLOCK * PW);
  for (size_t at = 0; at < count; at += BLOCK) {
    const size_t m = std::min(BLOCK, count - at);
    auto work = [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        const uint8_t* s = lem + (at + i) * PW;
        if (PW == 64)
          g1_u(g1_lem(s), u.data() + i * PW);
        else
          g2_u(g2_lem(s), u.data() + i * PW);
      }
    };
    if (m < 4096 || nt == 1) {
      work(0, m);
    } else {
      std::vector<std::thread> th;
      for (unsigned t = 0; t < nt; ++t) th.emplace_back(work, m * t / nt, m * (t + 1) / nt);
      for (auto& t : th) t.join();
    }
    h.update(u.data(), m * PW);
  }
}

// P - Q for affine points (one inversion per call; the H hashing batches them)
void sub_batch(const uint8_t* tau_g1, size_t n, size_t lo, size_t hi, uint8_t* out_u) {
  const size_t m = hi - lo;
  std::vector<Affine<HFq>> P(m), Q(m);
  std::vector<HFq> den(m), pre(m);
  for (size_t j = 0; j < m; ++j) {
    P[j] = g1_lem(tau_g1 + (n + lo + j) * 64);
    Q[j] = g1_lem(tau_g1 + (lo + j) * 64);
    const bool plain = !P[j].inf && !Q[j].inf && !(P[j].x == Q[j].x);
    den[j] = plain ? Q[j].x - P[j].x : HFq::one();
  }
  HFq acc = HFq::one();
  for (size_t j = 0; j < m; ++j) pre[j] = acc, acc = acc * den[j];
  HFq inv = acc.inv();
  for (size_t j = m; j-- > 0;) {
    const HFq d = den[j];
    den[j] = inv * pre[j];
    inv = inv * d;
  }
  for (size_t j = 0; j < m; ++j) {
    Affine<HFq> r;
    const Affine<HFq>& p = P[j];
    const Affine<HFq> nq{Q[j].x, Q[j].y.neg(), Q[j].inf};
    if (p.inf) {
      r = nq;
    } else if (nq.inf) {
      r = p;
    } else if (p.x == nq.x) {  // P = +-Q: through the general Jacobian formulas
      r = host::jac_to_aff(host::jac_add(host::jac_from_aff(p), host::jac_from_aff(nq)));
    } else {
      const HFq lam = (nq.y - p.y) * den[j];
      const HFq x3 = lam.sqr() - p.x - nq.x;
      r = Affine<HFq>{x3, lam * (p.x - x3) - p.y, false};
    }
    g1_u(r, out_u + j * 64);
  }
}

}  // namespace

MpcParams read_mpc(const uint8_t* sec, size_t len) {
  MpcParams m;
  if (len < 68) throw ZkpError(ZKP_ERR_FORMAT, "zkey: section 10 (MPC params) is truncated");
  std::memcpy(m.cs_hash, sec, 64);
  const uint32_t n = rd32(sec + 64);
  size_t o = 68;
  for (uint32_t i = 0; i < n; ++i) {
    if (len - o < 384 + 8) throw ZkpError(ZKP_ERR_FORMAT, "zkey: section 10 contribution is truncated");
    MpcContribution c;
    c.delta_after = g1_lem(sec + o);
    c.g1_s = g1_lem(sec + o + 64);
    c.g1_sx = g1_lem(sec + o + 128);
    c.g2_spx = g2_lem(sec + o + 192);
    std::memcpy(c.transcript, sec + o + 320, 64);
    o += 384;
    c.type = rd32(sec + o);
    const uint32_t plen = rd32(sec + o + 4);
    o += 8;
    if (len - o < plen) throw ZkpError(ZKP_ERR_FORMAT, "zkey: section 10 parameters are truncated");
    c.params.assign(sec + o, sec + o + plen);
    o += plen;
    m.contributions.push_back(std::move(c));
  }
  if (o != len) throw ZkpError(ZKP_ERR_FORMAT, "zkey: section 10 has trailing bytes");
  return m;
}

std::vector<uint8_t> write_mpc(const MpcParams& m) {
  std::vector<uint8_t> o(m.cs_hash, m.cs_hash + 64);
  put32(o, (uint32_t)m.contributions.size());
  for (const MpcContribution& c : m.contributions) {
    put_g1_lem(o, c.delta_after);
    put_g1_lem(o, c.g1_s);
    put_g1_lem(o, c.g1_sx);
    put_g2_lem(o, c.g2_spx);
    o.insert(o.end(), c.transcript, c.transcript + 64);
    put32(o, c.type);
    put32(o, (uint32_t)c.params.size());
    o.insert(o.end(), c.params.begin(), c.params.end());
  }
  return o;
}

// The name bytes snarkjs writes: name.substring(0, 64) counts UTF-16 code units, then UTF-8.  A
// supplementary character (4 UTF-8 bytes) is two units; one cut in half leaves a lone high
// surrogate, which TextEncoder writes as U+FFFD.  Bytes that are not UTF-8 are copied as one unit.
static std::string mpc_name_utf8(const std::string& name) {
  std::string out;
  size_t units = 0, i = 0;
  while (i < name.size() && units < 64) {
    const uint8_t b = (uint8_t)name[i];
    const size_t len = b < 0x80 ? 1 : (b >> 5) == 6 ? 2 : (b >> 4) == 14 ? 3 : (b >> 3) == 30 ? 4 : 1;
    if (i + len > name.size()) {
      out.push_back(name[i++]);
      ++units;
      continue;
    }
    if (len == 4 && units == 63) {  // only the high surrogate fits
      out += "\xEF\xBF\xBD";
      break;
    }
    out.append(name, i, len);
    units += len == 4 ? 2 : 1;
    i += len;
  }
  return out;
}

std::vector<uint8_t> mpc_name_params(const std::string& name) {
  const std::string nm = mpc_name_utf8(name);
  std::vector<uint8_t> prm{1, (uint8_t)nm.size()};
  prm.insert(prm.end(), nm.begin(), nm.end());
  return prm;
}

void mpc_contribute(MpcParams& m, ChaChaRng& rng, const Affine<HFq>& delta1_before, uint32_t type,
                    const std::string& name, const uint8_t* beacon, size_t beacon_len, uint32_t num_iterations_exp,
                    uint8_t k32[32]) {
  Blake2b th;
  th.update(m.cs_hash, 64);
  for (const MpcContribution& c : m.contributions) hash_pubkey(th, c);
  const HFr kf = fr_from_rng(rng);
  if (kf.is_zero()) throw ZkpError(ZKP_ERR_INTERNAL, "contribution: zero secret drawn");
  const U256 k = kf.to_std();
  MpcContribution c;
  c.g1_s = g1_from_rng(rng);
  c.g1_sx = g1_times(c.g1_s, k);
  hash_g1(th, c.g1_s);
  hash_g1(th, c.g1_sx);
  th.final(c.transcript);
  c.g2_spx = g2_times(hash_to_g2(c.transcript), k);
  c.delta_after = g1_times(delta1_before, k);
  c.type = type;
  if (!name.empty()) c.params = mpc_name_params(name);
  if (type == 1) {
    if (beacon_len > 255 || num_iterations_exp > 255) throw ZkpError(ZKP_ERR_INVALID_ARG, "beacon: parameter too long");
    c.params.push_back(2);  // numIterationsExp: the id, then its one value byte (no length byte)
    c.params.push_back((uint8_t)num_iterations_exp);
    c.params.push_back(3);
    c.params.push_back((uint8_t)beacon_len);
    c.params.insert(c.params.end(), beacon, beacon + beacon_len);
  }
  m.contributions.push_back(std::move(c));
  host::u256_to_le(k, k32);
}

void mpc_cs_hash_new(const uint8_t* zkey, size_t len, const uint8_t* tau_g1, size_t tau_g1_points, uint8_t out[64]) {
  const ZkeyParsed z = parse_zkey(zkey, len, false);
  const ZkeyHeader& hd = z.hdr;
  const size_t n = hd.domain_size;
  const Section* s = z.bf.sec;
  if (!s[3].ptr || s[3].len != ((uint64_t)hd.n_public + 1) * 64) throw ZkpError(ZKP_ERR_FORMAT, "zkey: no IC section");
  Blake2b h;
  hash_g1(h, hd.alpha1);
  hash_g1(h, hd.beta1);
  hash_g2(h, hd.beta2);
  hash_g2(h, hd.gamma2);
  hash_g1(h, hd.delta1);
  hash_g2(h, hd.delta2);
  u32be(h, hd.n_public + 1);
  hash_points<64>(h, s[3].ptr, (size_t)hd.n_public + 1);
  // H: (tau^(n+i) - tau^i) G1 by chunks of min(n - 1, 2^14) points (the recalled snarkjs loop)
  constexpr size_t CH = size_t(1) << 14;
  u32be(h, (uint32_t)(n - 1));
  std::vector<uint8_t> hu(CH * 64);
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  for (size_t i = 0; i + 1 < n; i += CH) {
    const size_t m = std::min(n - 1, CH);
    if (n + i + m > tau_g1_points) throw ZkpError(ZKP_ERR_FORMAT, "ptau: too few tauG1 points for the circuit hash");
    if (m < 2048 || nt == 1) {
      sub_batch(tau_g1, n, i, i + m, hu.data());
    } else {
      std::vector<std::thread> th;
      for (unsigned t = 0; t < nt; ++t)
        th.emplace_back(sub_batch, tau_g1, n, i + m * t / nt, i + m * (t + 1) / nt, hu.data() + (m * t / nt) * 64);
      for (auto& t : th) t.join();
    }
    h.update(hu.data(), m * 64);
  }
  const size_t nc = (size_t)hd.n_vars - hd.n_public - 1;
  u32be(h, (uint32_t)nc);
  hash_points<64>(h, s[8].ptr, nc);
  u32be(h, hd.n_vars);
  hash_points<64>(h, s[5].ptr, hd.n_vars);
  u32be(h, hd.n_vars);
  hash_points<64>(h, s[6].ptr, hd.n_vars);
  u32be(h, hd.n_vars);
  hash_points<128>(h, s[7].ptr, hd.n_vars);
  h.final(out);
}

void binfile_replace_section(std::vector<uint8_t>& file, uint32_t id, const std::vector<uint8_t>& payload) {
  if (file.size() < 12) throw ZkpError(ZKP_ERR_FORMAT, "binfile: truncated");
  const uint32_t nsec = rd32(file.data() + 8);
  std::vector<uint8_t> out(file.begin(), file.begin() + 12);
  size_t o = 12;
  bool done = false;
  for (uint32_t i = 0; i < nsec; ++i) {
    if (file.size() - o < 12) throw ZkpError(ZKP_ERR_FORMAT, "binfile: truncated section header");
    const uint32_t sid = rd32(file.data() + o);
    uint64_t ln = 0;
    for (int b = 7; b >= 0; --b) ln = (ln << 8) | file[o + 4 + b];
    if (file.size() - o - 12 < ln) throw ZkpError(ZKP_ERR_FORMAT, "binfile: truncated section");
    const uint8_t* p = file.data() + o + 12;
    const std::vector<uint8_t>* src = nullptr;
    if (sid == id && !done) src = &payload, done = true;
    const uint64_t nl = src ? src->size() : ln;
    put32(out, sid);
    for (int b = 0; b < 8; ++b) out.push_back((uint8_t)(nl >> (8 * b)));
    if (src)
      out.insert(out.end(), src->begin(), src->end());
    else
      out.insert(out.end(), p, p + ln);
    o += 12 + ln;
  }
  if (!done) {
    put32(out, id);
    const uint64_t nl = payload.size();
    for (int b = 0; b < 8; ++b) out.push_back((uint8_t)(nl >> (8 * b)));
    out.insert(out.end(), payload.begin(), payload.end());
    out[8] = (uint8_t)(nsec + 1), out[9] = (uint8_t)((nsec + 1) >> 8), out[10] = (uint8_t)((nsec + 1) >> 16),
    out[11] = (uint8_t)((nsec + 1) >> 24);
  }
  file.swap(out);
}

// ---------------------------------------------------------------- zkey verify
// e(g1a, g2b) == e(g1b, g2a); false if any point is the point at infinity
bool same_ratio(const Affine<HFq>& g1a, const Affine<HFq>& g1b, const Affine<HFq2>& g2a, const Affine<HFq2>& g2b) {
  if (g1a.inf || g1b.inf || g2a.inf || g2b.inf) return false;
  const Affine<HFq> ps[2] = {Affine<HFq>{g1a.x, g1a.y.neg(), false}, g1b};
  const Affine<HFq2> qs[2] = {g2b, g2a};
  return host::fq12_is_one(host::final_exponentiation(host::miller_loop_multi(ps, qs, 2)));
}
Affine<HFq2> g2_generator() {  // Verifier.sol:33-36
  auto fq = [](const char* dec) {
    U256 v{{0, 0, 0, 0}};
    for (const char* c = dec; *c; ++c) {
      host::u128 carry = (host::u128)(*c - '0');
      for (int i = 0; i < 4; ++i) {
        const host::u128 t = (host::u128)v.w[i] * 10 + carry;
        v.w[i] = (host::u64)t;
        carry = t >> 64;
      }
    }
    return HFq::from_std(v);
  };
  return Affine<HFq2>{HFq2{fq("10857046999023057135944570762232829481370756359578518086990519993285655852781"),
                           fq("11559732032986387107991004021392285783925812861821192530917403151452391805634")},
                      HFq2{fq("8495653923123431417604973247489272438418190587263600148770280649306958101930"),
                           fq("4082367875863433681332203403145435568316851327593401208105741076214120093531")},
                      false};
}

namespace {

template <class F>
bool same_point(const Affine<F>& a, const Affine<F>& b) {
  return a.inf == b.inf && (a.inf || (a.x == b.x && a.y == b.y));
}
bool g2_valid(const Affine<HFq2>& p) { return host::g2_on_curve(p) && host::g2_in_subgroup(p); }

// the beacon parameters of a contribution's parameter bytes (1: name, 2: numIterationsExp, one value
// byte, 3: beacon hash), every length bounded by the bytes present
struct BeaconParams {
  bool has_exp = false, has_hash = false;
  uint32_t exp = 0;
  std::vector<uint8_t> hash;
};
BeaconParams parse_contribution_params(const std::vector<uint8_t>& prm) {
  BeaconParams b;
  size_t j = 0;
  while (j < prm.size()) {
    const uint8_t pid = prm[j];
    if (prm.size() - j < 2) throw ZkpError(ZKP_ERR_FORMAT, "zkey: section 10 parameter is truncated");
    if (pid == 2) {
      b.has_exp = true;
      b.exp = prm[j + 1];
      j += 2;
      continue;
    }
    if (pid != 1 && pid != 3) throw ZkpError(ZKP_ERR_FORMAT, "zkey: MPC parameter " + std::to_string(pid) + " not recognized");
    const size_t ln = prm[j + 1];
    if (prm.size() - j - 2 < ln) throw ZkpError(ZKP_ERR_FORMAT, "zkey: section 10 parameter is truncated");
    if (pid == 3) {
      b.has_hash = true;
      b.hash.assign(prm.begin() + j + 2, prm.begin() + j + 2 + ln);
    }
    j += 2 + ln;
  }
  return b;
}

}  // namespace

void os_random(uint8_t* out, size_t n) {
  const std::string dev = "/dev/urandom";
  std::ifstream f(dev, std::ios::binary);
  if (!f.read(reinterpret_cast<char*>(out), (std::streamsize)n)) throw ZkpError(ZKP_ERR_IO, "cannot read " + dev);
}

bool zkey_verify_frominit(int device, const uint8_t* init, size_t init_len, const uint8_t* key, size_t key_len,
                          const uint8_t* seed32, std::string& msg, VerifyTimings* timings) {
  const auto t_begin = std::chrono::steady_clock::now();
  VerifyTimings tm;
  auto verdict = [&](bool ok, const std::string& m) {
    msg = m;
    tm.total_ms = wall_ms(t_begin);
    if (timings) *timings = tm;
    return ok;
  };
  auto bad = [&](const std::string& m) { return verdict(false, m); };
  auto tag = [](size_t i) { return "INVALID(" + std::to_string(i) + "): "; };

  const ZkeyParsed zk = parse_zkey(key, key_len, false), z0 = parse_zkey(init, init_len, false);
  const Section* s = zk.bf.sec;
  const Section* s0 = z0.bf.sec;
  if (!s[10].ptr) throw ZkpError(ZKP_ERR_FORMAT, "zkey: missing section 10 (MPC parameters)");
  if (!s0[10].ptr) throw ZkpError(ZKP_ERR_FORMAT, "initial zkey: missing section 10 (MPC parameters)");
  const MpcParams mpc = read_mpc(s[10].ptr, s[10].len), mpc0 = read_mpc(s0[10].ptr, s0[10].len);
  // the parameter bytes of every contribution, as the oracle's reader takes them before any check
  std::vector<BeaconParams> params;
  for (size_t i = 0; i < mpc.contributions.size(); ++i) {
    params.push_back(parse_contribution_params(mpc.contributions[i].params));
    if (mpc.contributions[i].type != 1) continue;
    if (!params[i].has_exp || !params[i].has_hash)
      throw ZkpError(ZKP_ERR_FORMAT, "zkey: section 10 beacon contribution " + std::to_string(i) + " has no beacon parameters");
    // 2^e chained hashes: the bound `zkey beacon` itself accepts
    if (params[i].exp > 63) throw ZkpError(ZKP_ERR_FORMAT, "zkey: section 10 beacon numIterationsExp must be <= 63");
  }
  const Affine<HFq> g1gen{fq_small(1), fq_small(2), false};
  const Affine<HFq2> g2gen = g2_generator();

  // 1. the transcript chain of every contribution
  Blake2b acc;
  acc.update(mpc.cs_hash, 64);
  Affine<HFq> cur = g1gen;
  for (size_t i = 0; i < mpc.contributions.size(); ++i) {
    const MpcContribution& c = mpc.contributions[i];
    if (!host::g1_on_curve(c.delta_after) || !host::g1_on_curve(c.g1_s) || !host::g1_on_curve(c.g1_sx))
      return bad(tag(i) + "a G1 point of the contribution is not on the curve");
    if (!g2_valid(c.g2_spx)) return bad(tag(i) + "the G2 point of the contribution is not in G2");
    Blake2b th = acc;
    hash_g1(th, c.g1_s);
    hash_g1(th, c.g1_sx);
    uint8_t digest[64];
    th.final(digest);
    if (std::memcmp(digest, c.transcript, 64) != 0) return bad(tag(i) + "inconsistent transcript");
    const Affine<HFq2> g2_sp = hash_to_g2(c.transcript);
    if (!same_ratio(c.g1_s, c.g1_sx, g2_sp, c.g2_spx))
      return bad(tag(i) + "public key G1 and G2 do not have the same ratio");
    if (!same_ratio(cur, c.delta_after, g2_sp, c.g2_spx)) return bad(tag(i) + "deltaAfter does not follow the public key");
    const BeaconParams bp = parse_contribution_params(c.params);  // bounded again where its values are used
    if (c.type == 1) {
      if (!bp.has_exp || !bp.has_hash)
        throw ZkpError(ZKP_ERR_FORMAT, "zkey: beacon contribution " + std::to_string(i) + " has no beacon parameters");
      if (bp.exp > 63) throw ZkpError(ZKP_ERR_FORMAT, "zkey: beacon numIterationsExp must be <= 63");
      uint8_t h[32];
      beacon_hash(bp.hash.data(), bp.hash.size(), bp.exp, h);
      uint32_t seed[8];
      seed_from_hash(h, seed);
      ChaChaRng rng(seed);
      const HFr k = fr_from_rng(rng);
      const Affine<HFq> g1_s = g1_from_rng(rng);
      if (!same_point(g1_s, c.g1_s) || !same_point(g1_times(g1_s, k.to_std()), c.g1_sx))
        return bad(tag(i) + "does not match the beacon");
    }
    hash_pubkey(acc, c);
    cur = c.delta_after;
  }
  // 2. the header against the initial key (its points checked first: section 2 is input too)
  const ZkeyHeader& h = zk.hdr;
  const ZkeyHeader& h0 = z0.hdr;
  if (!host::g1_on_curve(h.alpha1) || !host::g1_on_curve(h.beta1) || !host::g1_on_curve(h.delta1))
    return bad("INVALID: a G1 point of the header is not on the curve");
  if (!g2_valid(h.beta2) || !g2_valid(h.gamma2) || !g2_valid(h.delta2))
    return bad("INVALID: a G2 point of the header is not in G2");
  if (!g2_valid(h0.delta2)) throw ZkpError(ZKP_ERR_FORMAT, "initial zkey: delta2 is not in G2");
  auto differs = [&](const char* f) { return bad(std::string("INVALID: ") + f + " differs from the initial key"); };
  if (h.n_vars != h0.n_vars) return differs("n_vars");
  if (h.n_public != h0.n_public) return differs("n_public");
  if (h.domain_size != h0.domain_size) return differs("domain_size");
  if (!same_point(h.alpha1, h0.alpha1)) return differs("alpha1");
  if (!same_point(h.beta1, h0.beta1)) return differs("beta1");
  if (!same_point(h.beta2, h0.beta2)) return differs("beta2");
  if (!same_point(h.gamma2, h0.gamma2)) return differs("gamma2");
  // 3., 4. delta
  if (!same_point(h.delta1, cur)) return bad("INVALID: delta1 is not the last deltaAfter");
  if (!same_ratio(g1gen, cur, g2gen, h.delta2)) return bad("INVALID: delta2");
  // 5. csHash
  if (std::memcmp(mpc.cs_hash, mpc0.cs_hash, 64) != 0) return bad("INVALID: circuit does not match (csHash)");
  tm.host_ms = wall_ms(t_begin);
  // 6. the sections no contribution touches
  const auto t_cmp = std::chrono::steady_clock::now();
  for (int id : {3, 4, 5, 6, 7})
    if (s[id].len != s0[id].len || (s[id].len && std::memcmp(s[id].ptr, s0[id].ptr, s[id].len) != 0))
      return bad("INVALID: section " + std::to_string(id) + " is not identical to the initial key's");
  tm.compare_ms = wall_ms(t_cmp);
  // 7. L, then H: new = old * delta_init / delta
  uint8_t seed[32];
  if (seed32)
    std::memcpy(seed, seed32, 32);
  else
    os_random(seed, 32);
  uint64_t first_index = 0;
  for (int id : {8, 9}) {
    const std::string name = id == 8 ? "L" : "H";
    if (s[id].len != s0[id].len) return bad("INVALID: " + name + " section size");
    const size_t count = s[id].len / 64;
    // H: the last coefficient closes sum_j r_j w^j = 0, so that an imported key's section passes (zkey_verify.hpp)
    const RlcResult r = rlc_g1(device, seed, first_index, s0[id].ptr, s[id].ptr, count, id == 9);
    first_index += count;
    tm.rlc.add(r.t);
    if (r.first_bad_b != RLC_NO_BAD)
      return bad("INVALID: " + name + " section point " + std::to_string(r.first_bad_b) + " is not on the curve");
    if (r.first_bad_a != RLC_NO_BAD)
      return bad("INVALID: initial key's " + name + " section point " + std::to_string(r.first_bad_a) +
                 " is not on the curve");
    // e(sum r_i old_i, delta2) == e(sum r_i new_i, delta2_init)
    if (!same_ratio(host::jac_to_aff(r.sum_a), host::jac_to_aff(r.sum_b), h.delta2, h0.delta2))
      return bad("INVALID: " + name + " section is not the initial one times delta^-1");
  }
  return verdict(true, "OK");
}

// ---------------------------------------------------------------- powersoftau verify: section 7
// The contribution records of a ptau and their chain (ptau_verify.hpp).  The record layout and the hashes
// are recalled from snarkjs 0.4.22 (powersoftau_utils.js, powersoftau_verify.js; restated, parity
// unpinned: no snarkjs-written ptau exists here); the restatement this must equal is
// tests/helpers/ptau_model.py.  Record: tauG1, tauG2, alphaG1, betaG1, betaG2 (LEM), the key's nine points
// (tau / alpha / beta g1_s, g1_sx, then the three g2_spx), partialHash (216), nextChallenge (64), type
// (u32), parameter length (u32) and parameters as in section 10 of a zkey.
Blake2b Blake2b::resume(const uint8_t state[216]) {
  auto rd64 = [&](size_t at) {
    uint64_t v = 0;
    for (int b = 7; b >= 0; --b) v = (v << 8) | state[at + b];
    return v;
  };
  Blake2b h;
  for (int i = 0; i < 8; ++i) h.h_[i] = rd64(8 * i);
  h.t_[0] = rd64(64), h.t_[1] = 0;
  const uint64_t f = rd64(72), fill = rd64(208);
  if (f != 0 || fill > 128) throw ZkpError(ZKP_ERR_FORMAT, "Blake2b state: final flag set or buffer fill above 128");
  std::memcpy(h.buf_, state + 80, 128);
  h.n_ = (size_t)fill;
  return h;
}

namespace {

struct PtauKey {
  Affine<HFq> g1_s, g1_sx;
  Affine<HFq2> g2_spx;
};
struct PtauContribution {
  Affine<HFq> tau_g1, alpha_g1, beta_g1;
  Affine<HFq2> tau_g2, beta_g2;
  PtauKey key[3];  // tau, alpha, beta
  uint8_t points_lem[448];  // the five points as the record holds them
  uint8_t next_challenge[64], response_hash[64];
  uint32_t type = 0;
  BeaconParams beacon;
};
const char* const KEY_NAME[3] = {"tau", "alpha", "beta"};

std::vector<PtauContribution> read_ptau_contributions(const uint8_t* sec, size_t len) {
  auto cut = [](const std::string& what) { return ZkpError(ZKP_ERR_FORMAT, "ptau: section 7 " + what); };
  if (len < 4) throw cut("has no contribution count");
  const uint32_t n = rd32(sec);
  size_t o = 4;
  std::vector<PtauContribution> out;
  for (uint32_t i = 0; i < n; ++i) {
    const std::string tag = "contribution " + std::to_string(i);
    if (len - o < 1504) throw cut(tag + " is truncated");
    PtauContribution c;
    try {
      const uint8_t* p = sec + o;
      std::memcpy(c.points_lem, p, 448);
      c.tau_g1 = g1_lem(p), c.tau_g2 = g2_lem(p + 64), c.alpha_g1 = g1_lem(p + 192), c.beta_g1 = g1_lem(p + 256);
      c.beta_g2 = g2_lem(p + 320);
      p += 448;
      for (int k = 0; k < 3; ++k) {
        c.key[k].g1_s = g1_lem(p + 128 * k), c.key[k].g1_sx = g1_lem(p + 128 * k + 64);
        c.key[k].g2_spx = g2_lem(p + 384 + 128 * k);
      }
    } catch (const ZkpError&) {
      throw cut(tag + " has a coordinate out of range");
    }
    o += 448 + 768;
    {  // responseHash: the resumed state, then the key's nine points uncompressed
      Blake2b h = [&] {
        try {
          return Blake2b::resume(sec + o);
        } catch (const ZkpError&) {
          throw cut(tag + " has a malformed partialHash");
        }
      }();
      for (int k = 0; k < 3; ++k) hash_g1(h, c.key[k].g1_s), hash_g1(h, c.key[k].g1_sx);
      for (int k = 0; k < 3; ++k) hash_g2(h, c.key[k].g2_spx);
      h.final(c.response_hash);
    }
    o += 216;
    std::memcpy(c.next_challenge, sec + o, 64);
    o += 64;
    c.type = rd32(sec + o);
    const uint32_t plen = rd32(sec + o + 4);
    o += 8;
    if (len - o < plen) throw cut(tag + ": the parameter length runs past the section's end");
    try {
      c.beacon = parse_contribution_params(std::vector<uint8_t>(sec + o, sec + o + plen));
    } catch (const ZkpError&) {
      throw cut(tag + " has malformed parameters");
    }
    o += plen;
    if (c.type > 1) throw cut(tag + " has an unknown type");
    if (c.type == 1) {
      if (!c.beacon.has_exp || !c.beacon.has_hash) throw cut(tag + " is a beacon without beacon parameters");
      if (c.beacon.exp > 63) throw cut(tag + ": beacon numIterationsExp must be <= 63");
    }
    out.push_back(std::move(c));
  }
  if (o != len) throw cut("has trailing bytes");
  return out;
}

// Blake2b over Blake2b(""), then the sections of a new ceremony of power cp, all generators, uncompressed
void first_challenge(uint32_t cp, uint8_t out[64]) {
  Blake2b h;
  {
    uint8_t empty[64];
    Blake2b().final(empty);
    h.update(empty, 64);
  }
  constexpr size_t REP = 512;
  std::vector<uint8_t> b1(REP * 64), b2(REP * 128);
  g1_u(Affine<HFq>{fq_small(1), fq_small(2), false}, b1.data());
  g2_u(g2_generator(), b2.data());
  for (size_t i = 1; i < REP; ++i) std::memcpy(&b1[i * 64], &b1[0], 64), std::memcpy(&b2[i * 128], &b2[0], 128);
  auto many = [&](const std::vector<uint8_t>& blk, size_t pb, uint64_t count) {
    for (uint64_t at = 0; at < count; at += REP) h.update(blk.data(), (size_t)std::min<uint64_t>(REP, count - at) * pb);
  };
  const uint64_t N = uint64_t(1) << cp;
  many(b1, 64, 2 * N - 1), many(b2, 128, N), many(b1, 64, N), many(b1, 64, N), many(b2, 128, 1);
  h.final(out);
}

// what a contribution is checked against: the five points and the challenge it answers
struct PtauPrev {
  Affine<HFq> tau_g1, alpha_g1, beta_g1;
  Affine<HFq2> tau_g2, beta_g2;
  const uint8_t* next_challenge;
};

Affine<HFq2> key_g2_sp(int k, const uint8_t* challenge, const Affine<HFq>& g1_s, const Affine<HFq>& g1_sx) {
  Blake2b h;
  const uint8_t tag = (uint8_t)k;
  h.update(&tag, 1);
  h.update(challenge, 64);
  hash_g1(h, g1_s), hash_g1(h, g1_sx);
  uint8_t d[64];
  h.final(d);
  return hash_to_g2(d);
}

// "" if contribution i follows prev, else the message
std::string check_ptau_contribution(size_t i, const PtauContribution& c, const PtauPrev& prev) {
  const std::string tag = "contribution " + std::to_string(i) + ": ";
  bool g1_ok = host::g1_on_curve(c.tau_g1) && host::g1_on_curve(c.alpha_g1) && host::g1_on_curve(c.beta_g1);
  bool g2_ok = g2_valid(c.tau_g2) && g2_valid(c.beta_g2);
  for (int k = 0; k < 3; ++k) {
    g1_ok = g1_ok && host::g1_on_curve(c.key[k].g1_s) && host::g1_on_curve(c.key[k].g1_sx);
    g2_ok = g2_ok && g2_valid(c.key[k].g2_spx);
  }
  if (!g1_ok) return tag + "a G1 point is not on the curve";
  if (!g2_ok) return tag + "a G2 point is not in G2";
  if (c.type == 1) {
    uint8_t bh[32];
    beacon_hash(c.beacon.hash.data(), c.beacon.hash.size(), c.beacon.exp, bh);
    uint32_t seed[8];
    seed_from_hash(bh, seed);
    ChaChaRng rng(seed);
    U256 prv[3];
    for (int k = 0; k < 3; ++k) prv[k] = fr_from_rng(rng).to_std();
    for (int k = 0; k < 3; ++k) {
      const Affine<HFq> g1_s = g1_from_rng(rng), g1_sx = g1_times(g1_s, prv[k]);
      const Affine<HFq2> g2_spx = g2_times(key_g2_sp(k, prev.next_challenge, g1_s, g1_sx), prv[k]);
      auto wrong = [&](const char* what) {
        return std::string("BEACON key (") + KEY_NAME[k] + what + ") is not generated correctly";
      };
      if (!same_point(g1_s, c.key[k].g1_s)) return wrong("G1_s");
      if (!same_point(g1_sx, c.key[k].g1_sx)) return wrong("G1_sx");
      if (!same_point(g2_spx, c.key[k].g2_spx)) return wrong("G2_spx");
    }
  }
  Affine<HFq2> g2_sp[3];
  for (int k = 0; k < 3; ++k) {
    g2_sp[k] = key_g2_sp(k, prev.next_challenge, c.key[k].g1_s, c.key[k].g1_sx);
    if (!same_ratio(c.key[k].g1_s, c.key[k].g1_sx, g2_sp[k], c.key[k].g2_spx))
      return std::string("INVALID key (") + KEY_NAME[k] + ")";
  }
  if (!same_ratio(prev.tau_g1, c.tau_g1, g2_sp[0], c.key[0].g2_spx)) return "INVALID tau*G1. contribution";
  if (!same_ratio(c.key[0].g1_s, c.key[0].g1_sx, prev.tau_g2, c.tau_g2)) return "INVALID tau*G2. contribution";
  if (!same_ratio(prev.alpha_g1, c.alpha_g1, g2_sp[1], c.key[1].g2_spx)) return "INVALID alpha*G1. contribution";
  if (!same_ratio(prev.beta_g1, c.beta_g1, g2_sp[2], c.key[2].g2_spx)) return "INVALID beta*G1. contribution";
  if (!same_ratio(c.key[2].g1_s, c.key[2].g1_sx, prev.beta_g2, c.beta_g2)) return "INVALID beta*G2. contribution";
  return "";
}

}  // namespace

bool ptau_verify(int device, const uint8_t* ptau, size_t len, const uint8_t* seed32, std::string& msg) {
  const auto t_begin = std::chrono::steady_clock::now();
  ptau_verify_timings() = PtauVerifyTimings{};
  const PtauFile f = parse_ptau(ptau, len);
  const std::vector<PtauContribution> cs = read_ptau_contributions(f.sec[7].ptr, f.sec[7].len);
  // the first challenge (384 * 2^ceremonyPower bytes of hashing: ~100 GB at 28) on a thread of its own,
  // beside everything up to the first contribution's check, which alone needs it
  uint8_t first[64];
  double first_ms = 0, contrib_ms = 0, next_ms = 0;
  std::thread first_thread;
  struct Joiner {
    std::thread& t;
    ~Joiner() {
      if (t.joinable()) t.join();
    }
  } joiner{first_thread};
  auto verdict = [&](bool ok, const std::string& m) {
    if (first_thread.joinable()) first_thread.join();
    msg = m;
    PtauVerifyTimings& t = ptau_verify_timings();
    t.contributions_ms = contrib_ms, t.first_challenge_ms = first_ms, t.next_challenge_ms = next_ms;
    t.total_ms = wall_ms(t_begin);
    return ok;
  };
  if (cs.empty()) return verdict(false, "This file has no contribution! It cannot be used in production");
  first_thread = std::thread([&] {
    const auto t0 = std::chrono::steady_clock::now();
    first_challenge(f.ceremony_power, first);
    first_ms = wall_ms(t0);
  });
  const Affine<HFq> g1gen{fq_small(1), fq_small(2), false};
  const Affine<HFq2> g2gen = g2_generator();
  auto check = [&](size_t i) {
    const auto t0 = std::chrono::steady_clock::now();
    PtauPrev prev;
    if (i == 0) {
      if (first_thread.joinable()) first_thread.join();
      prev = PtauPrev{g1gen, g1gen, g1gen, g2gen, g2gen, first};
    } else {
      const PtauContribution& p = cs[i - 1];
      prev = PtauPrev{p.tau_g1, p.alpha_g1, p.beta_g1, p.tau_g2, p.beta_g2, p.next_challenge};
    }
    const std::string m = check_ptau_contribution(i, cs[i], prev);
    contrib_ms += wall_ms(t0);
    return m;
  };
  // the last contribution, its ties to the sections, the sections, the next challenge, then the earlier
  // contributions from the last but one down, as snarkjs orders them
  const PtauContribution& last = cs.back();
  std::string m = check(cs.size() - 1);
  if (!m.empty()) return verdict(false, m);
  if (std::memcmp(f.sec[2].ptr + 64, last.points_lem, 64) != 0)
    return verdict(false, "Second element of tau*G1 section does not match the one in the contribution section");
  if (std::memcmp(f.sec[3].ptr + 128, last.points_lem + 64, 128) != 0)
    return verdict(false, "Second element of tau*G2 section does not match the one in the contribution section");
  if (std::memcmp(f.sec[4].ptr, last.points_lem + 192, 64) != 0)
    return verdict(false, "First element of alpha*tau*G1 section does not match the one in the contribution section");
  if (std::memcmp(f.sec[5].ptr, last.points_lem + 256, 64) != 0)
    return verdict(false, "First element of beta*tau*G1 section does not match the one in the contribution section");
  if (std::memcmp(f.sec[6].ptr, last.points_lem + 320, 128) != 0)
    return verdict(false, "beta*G2 does not match the one in the contribution section");
  if (!ptau_verify_sections(device, ptau, len, seed32, m)) return verdict(false, m);
  if (f.power == f.ceremony_power) {
    const auto t0 = std::chrono::steady_clock::now();
    Blake2b h;
    h.update(last.response_hash, 64);
    hash_points<64>(h, f.sec[2].ptr, f.points(2));
    hash_points<128>(h, f.sec[3].ptr, f.points(3));
    hash_points<64>(h, f.sec[4].ptr, f.points(4));
    hash_points<64>(h, f.sec[5].ptr, f.points(5));
    hash_points<128>(h, f.sec[6].ptr, 1);
    uint8_t d[64];
    h.final(d);
    next_ms = wall_ms(t0);
    if (std::memcmp(d, last.next_challenge, 64) != 0)
      return verdict(false, "Hash of the values does not match the next challenge of the last contributor in the contributions section");
  }
  for (size_t i = cs.size() - 1; i-- > 0;) {
    m = check(i);
    if (!m.empty()) return verdict(false, m);
  }
  return verdict(true, "OK");
}

// ---------------------------------------------------------------- powersoftau new / contribute / beacon
// (ptau_contribute.hpp; the host parts of tests/helpers/ptau_model.py new, draw_key and contribute)

void Blake2b::save(uint8_t state[216]) const {
  auto wr64 = [&](size_t at, uint64_t v) {
    for (int b = 0; b < 8; ++b) state[at + b] = (uint8_t)(v >> (8 * b));
  };
  for (int i = 0; i < 8; ++i) wr64(8 * i, h_[i]);
  wr64(64, t_[0]), wr64(72, 0);
  std::memset(state + 80, 0, 128);
  std::memcpy(state + 80, buf_, n_);
  wr64(208, n_);
}

std::vector<uint8_t> ptau_new(uint32_t power, uint32_t ceremony_power) {
  if (!ceremony_power) ceremony_power = power;
  if (power < 1 || power > 28) throw ZkpError(ZKP_ERR_INVALID_ARG, "ptau new: power must be within 1..28");
  if (ceremony_power < power) throw ZkpError(ZKP_ERR_INVALID_ARG, "ptau new: ceremonyPower below power");
  const size_t N = (size_t)1 << power;
  const size_t count[8] = {0, 0, 2 * N - 1, N, N, N, 1, 0};
  std::vector<uint8_t> g1, g2;
  put_g1_lem(g1, Affine<HFq>{fq_small(1), fq_small(2), false});
  put_g2_lem(g2, g2_generator());
  size_t total = 12 + 12 + 44 + 12 + 4;
  for (int id = 2; id <= 6; ++id) total += 12 + count[id] * (PtauFile::is_g2(id) ? 128 : 64);
  std::vector<uint8_t> out(total);
  uint8_t* o = out.data();
  auto w32 = [&](uint32_t x) { std::memcpy(o, &x, 4), o += 4; };
  auto w64 = [&](uint64_t x) { std::memcpy(o, &x, 8), o += 8; };
  std::memcpy(o, "ptau", 4), o += 4;
  w32(1), w32(7);
  w32(1), w64(44), w32(32);
  std::memcpy(o, host::FQ_DESC.mod.w, 32), o += 32;
  w32(power), w32(ceremony_power);
  for (int id = 2; id <= 6; ++id) {
    const std::vector<uint8_t>& g = PtauFile::is_g2(id) ? g2 : g1;
    w32((uint32_t)id), w64(count[id] * g.size());
    for (size_t i = 0; i < count[id]; ++i) std::memcpy(o, g.data(), g.size()), o += g.size();
  }
  w32(7), w64(4), w32(0);
  return out;
}

PtauDraw ptau_draw(ChaChaRng& rng) {
  PtauDraw d;
  for (int k = 0; k < 3; ++k) {
    const HFr s = fr_from_rng(rng);
    // Fr.fromRng draws again on a value >= r; it can give 0 only with probability 2^-254
    if (s.is_zero()) throw ZkpError(ZKP_ERR_INTERNAL, "ptau contribute: zero secret drawn");
    d.prv[k] = s.to_std();
  }
  for (int k = 0; k < 3; ++k) {
    d.g1_s[k] = g1_from_rng(rng);
    d.g1_sx[k] = g1_times(d.g1_s[k], d.prv[k]);
  }
  return d;
}

bool ptau_last_challenge(const uint8_t* sec7, size_t len, uint8_t out[64]) {
  const std::vector<PtauContribution> cs = read_ptau_contributions(sec7, len);
  if (cs.empty()) return false;
  std::memcpy(out, cs.back().next_challenge, 64);
  return true;
}

void ptau_first_challenge(uint32_t ceremony_power, uint8_t out[64]) { first_challenge(ceremony_power, out); }

bool ptau_last_hashes(const uint8_t* sec7, size_t len, uint8_t challenge[64], uint8_t response[64]) {
  const std::vector<PtauContribution> cs = read_ptau_contributions(sec7, len);
  if (cs.empty()) return false;
  std::memcpy(challenge, cs.back().next_challenge, 64);
  std::memcpy(response, cs.back().response_hash, 64);
  return true;
}

namespace {

// the key's nine points in the record's order (g1_s, g1_sx per secret, then the three g2_spx) in both forms
void key_forms(const Affine<HFq> (&g1)[6], const Affine<HFq2> (&g2)[3], uint8_t lem[768], uint8_t u[768]) {
  std::vector<uint8_t> l;
  for (int k = 0; k < 6; ++k) put_g1_lem(l, g1[k]), g1_u(g1[k], u + 64 * k);
  for (int k = 0; k < 3; ++k) put_g2_lem(l, g2[k]), g2_u(g2[k], u + 384 + 128 * k);
  std::memcpy(lem, l.data(), 768);
}

// 32 big-endian bytes, standard form, below p
bool fq_from_be(const uint8_t* p, HFq& out) {
  uint8_t le[32];
  for (int i = 0; i < 32; ++i) le[i] = p[31 - i];
  const U256 v = host::u256_from_le(le);
  if (host::u256_geq(v, host::FQ_DESC.mod)) return false;
  out = HFq::from_std(v);
  return true;
}
// an uncompressed point of n coordinates' worth of bytes: 0x40 then zeros, or no flag bit at all
bool inf_from_u(const uint8_t* p, size_t n, bool& inf) {
  inf = (p[0] & 0x40) != 0;
  return !inf || (p[0] == 0x40 && zero_bytes(p + 1, n - 1));
}

}  // namespace

void ptau_key_forms(const PtauDraw& d, const uint8_t challenge[64], uint8_t key_lem[768], uint8_t key_u[768]) {
  Affine<HFq> g1[6];
  Affine<HFq2> g2[3];
  for (int k = 0; k < 3; ++k) {
    g1[2 * k] = d.g1_s[k], g1[2 * k + 1] = d.g1_sx[k];
    g2[k] = g2_times(key_g2_sp(k, challenge, d.g1_s[k], d.g1_sx[k]), d.prv[k]);
  }
  key_forms(g1, g2, key_lem, key_u);
}

void ptau_key_from_uncompressed(const uint8_t key_u[768], uint8_t key_lem[768]) {
  auto bad = [](int k, const char* what) {
    return ZkpError(ZKP_ERR_FORMAT, "response: key point " + std::to_string(k) + " " + what);
  };
  Affine<HFq> g1[6];
  Affine<HFq2> g2[3];
  for (int k = 0; k < 6; ++k) {
    const uint8_t* p = key_u + 64 * k;
    Affine<HFq>& a = g1[k];
    a = Affine<HFq>{HFq::zero(), HFq::zero(), false};
    if (!inf_from_u(p, 64, a.inf)) throw bad(k, "is not canonical");
    if (a.inf) continue;
    if (!fq_from_be(p, a.x) || !fq_from_be(p + 32, a.y)) throw bad(k, "is not canonical");
    if (!host::g1_on_curve(a)) throw bad(k, "is not on the curve");
  }
  for (int k = 0; k < 3; ++k) {
    const uint8_t* p = key_u + 384 + 128 * k;
    Affine<HFq2>& a = g2[k];
    a = Affine<HFq2>{HFq2::zero(), HFq2::zero(), false};
    if (!inf_from_u(p, 128, a.inf)) throw bad(6 + k, "is not canonical");
    if (a.inf) continue;
    if (!fq_from_be(p, a.x.c1) || !fq_from_be(p + 32, a.x.c0) || !fq_from_be(p + 64, a.y.c1) || !fq_from_be(p + 96, a.y.c0))
      throw bad(6 + k, "is not canonical");
    if (!host::g2_on_curve(a)) throw bad(6 + k, "is not on the curve");
  }
  uint8_t again[768];
  key_forms(g1, g2, key_lem, again);
}

std::vector<uint8_t> ptau_record(const PtauDraw& d, const uint8_t challenge[64], const uint8_t points_lem[448],
                                 const Blake2b& partial, uint32_t type, const char* name, const uint8_t* beacon,
                                 size_t beacon_len, uint32_t num_iterations_exp, uint8_t response_hash[64]) {
  uint8_t key_lem[768], key_u[768];
  ptau_key_forms(d, challenge, key_lem, key_u);
  return ptau_record_of_key(key_lem, key_u, points_lem, partial, type, name, beacon, beacon_len, num_iterations_exp,
                            response_hash);
}

std::vector<uint8_t> ptau_record_of_key(const uint8_t key_lem[768], const uint8_t key_u[768], const uint8_t points_lem[448],
                                        const Blake2b& partial, uint32_t type, const char* name, const uint8_t* beacon,
                                        size_t beacon_len, uint32_t num_iterations_exp, uint8_t response_hash[64]) {
  std::vector<uint8_t> rec(points_lem, points_lem + 448);
  rec.insert(rec.end(), key_lem, key_lem + 768);
  uint8_t state[216];
  partial.save(state);
  rec.insert(rec.end(), state, state + 216);
  Blake2b h = partial;
  h.update(key_u, 768);
  h.final(response_hash);
  rec.insert(rec.end(), 64, 0);  // nextChallenge: the caller's, once the uncompressed sections are hashed
  std::vector<uint8_t> prm;
  if (name) {
    const std::string nm = mpc_name_utf8(name);
    prm.push_back(1);
    prm.push_back((uint8_t)nm.size());
    prm.insert(prm.end(), nm.begin(), nm.end());
  }
  if (type == 1) {
    if (beacon_len > 255 || num_iterations_exp > 255) throw ZkpError(ZKP_ERR_INVALID_ARG, "beacon: parameter too long");
    prm.push_back(2);
    prm.push_back((uint8_t)num_iterations_exp);
    prm.push_back(3);
    prm.push_back((uint8_t)beacon_len);
    prm.insert(prm.end(), beacon, beacon + beacon_len);
  }
  put32(rec, type), put32(rec, (uint32_t)prm.size());
  rec.insert(rec.end(), prm.begin(), prm.end());
  return rec;
}

// ---------------------------------------------------------------- the MPCParams file (zkey_bellman.hpp)
namespace {

uint32_t rd32be(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; }

}  // namespace

MpcParamsFile mpcparams_parse(const uint8_t* buf, size_t len) {
  MpcParamsFile f;
  size_t o = 0;
  auto need = [&](uint64_t bytes, const char* what) {
    if ((uint64_t)(len - o) < bytes) throw ZkpError(ZKP_ERR_FORMAT, std::string("mpcparams: the file ends inside ") + what);
  };
  // a counted section of `pb`-byte points: -> its first point, the count in *count
  auto section = [&](const char* what, size_t pb, size_t* count) {
    need(4, what);
    *count = rd32be(buf + o);
    o += 4;
    need((uint64_t)*count * pb, what);
    const uint8_t* p = buf + o;
    o += *count * pb;
    return p;
  };
  need(MPCPARAMS_HEADER, "the header");
  f.header = buf;
  o = MPCPARAMS_HEADER;
  size_t n_a = 0, n_b1 = 0, n_b2 = 0;
  f.ic = section("IC", 64, &f.n_ic);
  f.h = section("H", 64, &f.n_h);
  f.l = section("L", 64, &f.n_l);
  f.a = section("A", 64, &n_a);
  f.b1 = section("B1", 64, &n_b1);
  f.b2 = section("B2", 128, &n_b2);
  if (!f.n_ic) throw ZkpError(ZKP_ERR_FORMAT, "mpcparams: IC has no point");
  const uint64_t n = (uint64_t)f.n_h + 1;
  if ((n & (n - 1)) || n > (uint64_t(1) << 27))
    throw ZkpError(ZKP_ERR_FORMAT, "mpcparams: H has " + std::to_string(f.n_h) + " points, which is not 2^p - 1 with p <= 27");
  if (n_b1 != n_a || n_b2 != n_a) throw ZkpError(ZKP_ERR_FORMAT, "mpcparams: A, B1 and B2 differ in their point counts");
  if (n_a < f.n_ic || f.n_l != n_a - f.n_ic)
    throw ZkpError(ZKP_ERR_FORMAT, "mpcparams: L has " + std::to_string(f.n_l) + " points where A and IC want " +
                                       std::to_string((long long)n_a - (long long)f.n_ic));
  f.n_public = (uint32_t)(f.n_ic - 1), f.n_vars = (uint32_t)n_a, f.domain_size = (uint32_t)n;
  while ((uint64_t(1) << f.log_domain) < n) ++f.log_domain;
  need(64, "csHash");
  f.cs_hash = buf + o;
  o += 64;
  size_t nc = 0;
  f.contributions = section("the contributions", MPCPARAMS_CONTRIBUTION, &nc);
  f.n_contributions = (uint32_t)nc;
  if (o != len) throw ZkpError(ZKP_ERR_FORMAT, "mpcparams: " + std::to_string(len - o) + " trailing bytes");
  return f;
}

void mpcparams_header(const Affine<HFq>& alpha1, const Affine<HFq>& beta1, const Affine<HFq2>& beta2,
                      const Affine<HFq2>& gamma2, const Affine<HFq>& delta1, const Affine<HFq2>& delta2,
                      uint8_t out[MPCPARAMS_HEADER]) {
  g1_u(alpha1, out), g1_u(beta1, out + 64), g2_u(beta2, out + 128), g2_u(gamma2, out + 256);
  g1_u(delta1, out + MPCPARAMS_DELTA1_AT), g2_u(delta2, out + MPCPARAMS_DELTA2_AT);
}

void mpcparams_put_contribution(const MpcContribution& c, uint8_t out[MPCPARAMS_CONTRIBUTION]) {
  g1_u(c.delta_after, out), g1_u(c.g1_s, out + 64), g1_u(c.g1_sx, out + 128), g2_u(c.g2_spx, out + 192);
  std::memcpy(out + 320, c.transcript, 64);
}

Affine<HFq> mpcparams_g1(const uint8_t in[64], const std::string& what) {
  Affine<HFq> a{HFq::zero(), HFq::zero(), false};
  const bool ok = inf_from_u(in, 64, a.inf) && (a.inf || (fq_from_be(in, a.x) && fq_from_be(in + 32, a.y) && host::g1_on_curve(a)));
  if (!ok) throw ZkpError(ZKP_ERR_FORMAT, "mpcparams: " + what + " is not on the curve");
  return a;
}

Affine<HFq2> mpcparams_g2(const uint8_t in[128], const std::string& what) {
  Affine<HFq2> a{HFq2::zero(), HFq2::zero(), false};
  const bool ok = inf_from_u(in, 128, a.inf) &&
                  (a.inf || (fq_from_be(in, a.x.c1) && fq_from_be(in + 32, a.x.c0) && fq_from_be(in + 64, a.y.c1) &&
                             fq_from_be(in + 96, a.y.c0) && host::g2_on_curve(a)));
  if (!ok) throw ZkpError(ZKP_ERR_FORMAT, "mpcparams: " + what + " is not on the curve");
  return a;
}

MpcParams mpcparams_read_mpc(const MpcParamsFile& f) {
  MpcParams m;
  std::memcpy(m.cs_hash, f.cs_hash, 64);
  for (uint32_t i = 0; i < f.n_contributions; ++i) {
    const uint8_t* p = f.contributions + (size_t)i * MPCPARAMS_CONTRIBUTION;
    const std::string what = "contribution " + std::to_string(i);
    MpcContribution c;
    c.delta_after = mpcparams_g1(p, what + " deltaAfter");
    c.g1_s = mpcparams_g1(p + 64, what + " g1_s");
    c.g1_sx = mpcparams_g1(p + 128, what + " g1_sx");
    c.g2_spx = mpcparams_g2(p + 192, what + " g2_spx");
    std::memcpy(c.transcript, p + 320, 64);
    m.contributions.push_back(std::move(c));
  }
  return m;
}

Affine<HFq2> mpc_g2_times(const Affine<HFq2>& p, const uint8_t k32[32]) { return g2_times(p, host::u256_from_le(k32)); }

}  // namespace zkp
