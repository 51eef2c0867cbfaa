// CPU run of the device pairing bodies (csrc/pairing_kernels.hpp: the Fq6 / Fq12 tower and the per-lane
// Miller loop of groth16_verify.hip) beside the host pairing (host_pairing.cpp), without a GPU.
// usage: pairing_emu tower <seed>
//          Fq12 mul, sqr and sparse line mul on operands drawn from {0, 1, p - 1, random} per coefficient,
//          on 0 and 1 themselves and on unitary elements (final exponentiations of random values).
//          -> one line `tower <checks> <mismatches>`
//        pairing_emu miller <file of pairs: G1 64 bytes + G2 128 bytes, standard-form LE, all-zero = infinity>
//          -> one line per pair: 1 if final_exponentiation(device-body Miller value) == host::pairing
// Device Miller values carry Fq2 factors the host's do not: they are compared after the final
// exponentiation only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// the field's templates without the forced inlining (field.hpp allows a host tool that): the tower inlined
// into one function per product is minutes of compile time under the sanitizers
#define ZDEV __host__ __device__ inline
#include "../../zk-p2p-onramp_amd/csrc/host_pairing.hpp"
#include "../../zk-p2p-onramp_amd/csrc/pairing_kernels.hpp"
using namespace zkp;

static void host_to_words(const host::Fq12& f, uint32_t* w) {
  const host::Fq2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  for (int i = 0; i < 6; ++i) {
    host::u256_to_le(c[i]->c0.to_std(), reinterpret_cast<uint8_t*>(w + 16 * i));
    host::u256_to_le(c[i]->c1.to_std(), reinterpret_cast<uint8_t*>(w + 16 * i + 8));
  }
}
static host::Fq12 host_from_words(const uint32_t* w) {
  host::Fq2 c[6];
  for (int i = 0; i < 6; ++i) {
    c[i].c0 = host::Fq::from_std(host::u256_from_le(reinterpret_cast<const uint8_t*>(w + 16 * i)));
    c[i].c1 = host::Fq::from_std(host::u256_from_le(reinterpret_cast<const uint8_t*>(w + 16 * i + 8)));
  }
  return host::Fq12{host::Fq6{c[0], c[1], c[2]}, host::Fq6{c[3], c[4], c[5]}};
}
static bool same(const pairing::F12& d, const host::Fq12& h) {
  uint32_t a[96], b[96];
  pairing::f12_store_std(a, d);
  host_to_words(h, b);
  return !memcmp(a, b, sizeof a);
}

static uint64_t g_rng;
static uint64_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return g_rng ^ (g_rng >> 29);
}
static host::Fq rand_fq(int kind) {  // 0: zero, 1: one, 2: p - 1, else random
  if (kind == 0) return host::Fq::zero();
  if (kind == 1) return host::Fq::one();
  if (kind == 2) return host::Fq::one().neg();
  host::U256 v{{rnd(), rnd(), rnd(), rnd() >> 3}};  // < 2^253 < p
  return host::Fq::from_std(v);
}
static host::Fq12 rand_f12(int extremes) {  // extremes: 1 in `extremes` coefficients is random, the rest 0 / 1 / p - 1
  host::Fq c[12];
  for (auto& x : c) x = rand_fq(extremes ? (int)(rnd() % (3 + extremes)) : 3);
  return host::Fq12{host::Fq6{{c[0], c[1]}, {c[2], c[3]}, {c[4], c[5]}}, host::Fq6{{c[6], c[7]}, {c[8], c[9]}, {c[10], c[11]}}};
}
static pairing::F12 to_dev(const host::Fq12& h) {
  uint32_t w[96];
  host_to_words(h, w);
  return pairing::f12_load_std(w);
}

// the in-place forms, on a home of stride 1
static pairing::F12 sqr_mem(const pairing::F12& a) {
  uint32_t mem[pairing::F12_WORDS];
  const pairing::LaneMem m{mem, 1};
  pairing::lm_store(m, a);
  pairing::f12_sqr_mem(m);
  return pairing::lm_load(m);
}
static pairing::F12 mul_line_mem(const pairing::F12& a, const Fq2& l0, const Fq2& l1, const Fq2& l3) {
  uint32_t mem[pairing::F12_WORDS];
  const pairing::LaneMem m{mem, 1};
  pairing::lm_store(m, a);
  pairing::f12_mul_line_mem(m, l0, l1, l3);
  return pairing::lm_load(m);
}

static int run_tower(uint64_t seed) {
  g_rng = seed;
  std::vector<host::Fq12> pool;
  host::Fq12 zero = host::fq12_one();
  zero.c0.c0 = host::Fq2::zero();
  pool.push_back(zero);
  pool.push_back(host::fq12_one());
  for (int i = 0; i < 6; ++i) pool.push_back(rand_f12(0));
  for (int i = 0; i < 8; ++i) pool.push_back(rand_f12(1 + i % 3));
  host::Fq12 all_pm1 = host::fq12_one();
  {
    const host::Fq m1 = host::Fq::one().neg();
    const host::Fq2 c{m1, m1};
    all_pm1 = host::Fq12{host::Fq6{c, c, c}, host::Fq6{c, c, c}};
  }
  pool.push_back(all_pm1);
  for (int i = 0; i < 3; ++i) pool.push_back(host::final_exponentiation(rand_f12(0)));  // unitary
  int checks = 0, bad = 0;
  auto check = [&](bool ok, const char* what, size_t i, size_t j) {
    ++checks;
    if (!ok) {
      ++bad;
      printf("mismatch %s %zu %zu\n", what, i, j);
    }
  };
  for (size_t i = 0; i < pool.size(); ++i) {
    const pairing::F12 a = to_dev(pool[i]);
    check(same(a, pool[i]), "roundtrip", i, i);
    check(same(sqr_mem(a), host::fq12_mul(pool[i], pool[i])), "sqr", i, i);
    for (size_t j = 0; j < pool.size(); ++j) {
      const pairing::F12 b = to_dev(pool[j]);
      check(same(pairing::f12_mul(a, b), host::fq12_mul(pool[i], pool[j])), "mul", i, j);
      // the line's three coefficients from b's
      host::Fq12 line = host::fq12_one();
      line.c0 = host::Fq6{pool[j].c0.c0, host::Fq2::zero(), host::Fq2::zero()};
      line.c1 = host::Fq6{pool[j].c1.c0, pool[j].c1.c1, host::Fq2::zero()};
      check(same(mul_line_mem(a, b.c0.c0, b.c1.c0, b.c1.c1), host::fq12_mul(pool[i], line)), "mul_line", i, j);
    }
  }
  // the strided home: a round trip at stride 3 leaves the neighbours alone
  {
    std::vector<uint32_t> mem(pairing::F12_WORDS * 3, 0xdeadbeefu);
    const pairing::LaneMem m{mem.data() + 1, 3};
    pairing::lm_store(m, to_dev(pool[3]));
    check(same(pairing::lm_load(m), pool[3]), "lanemem", 3, 3);
    bool clean = true;
    for (size_t k = 0; k < mem.size(); ++k)
      if (k % 3 != 1) clean &= mem[k] == 0xdeadbeefu;
    check(clean, "lanemem-neighbours", 3, 3);
  }
  printf("tower %d %d\n", checks, bad);
  return bad ? 1 : 0;
}

static int run_miller(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  std::vector<uint32_t> g1, g2;
  uint32_t rec[48];
  while (fread(rec, 4, 48, f) == 48) {
    g1.insert(g1.end(), rec, rec + 16);
    g2.insert(g2.end(), rec + 16, rec + 48);
  }
  fclose(f);
  const size_t n = g1.size() / 16;
  pairing::FrobConsts fc;
  {
    host::Fq2 gx, gy;
    host::g2_frobenius_consts(gx, gy);
    host::u256_to_le(gx.c0.to_std(), reinterpret_cast<uint8_t*>(fc.gx));
    host::u256_to_le(gx.c1.to_std(), reinterpret_cast<uint8_t*>(fc.gx + 8));
    host::u256_to_le(gy.c0.to_std(), reinterpret_cast<uint8_t*>(fc.gy));
    host::u256_to_le(gy.c1.to_std(), reinterpret_cast<uint8_t*>(fc.gy + 8));
  }
  std::vector<uint32_t> out(n * 96), mem(pairing::F12_WORDS);
  int bad = 0;
  for (size_t i = 0; i < n; ++i) {
    pairing::miller_pair_std(g1.data(), g2.data(), i, fc, pairing::LaneMem{mem.data(), 1}, out.data());
    const uint8_t* p = reinterpret_cast<const uint8_t*>(g1.data() + i * 16);
    const uint8_t* q = reinterpret_cast<const uint8_t*>(g2.data() + i * 32);
    bool pinf = true, qinf = true;
    for (int k = 0; k < 64; ++k) pinf &= p[k] == 0;
    for (int k = 0; k < 128; ++k) qinf &= q[k] == 0;
    auto fq = [](const uint8_t* b) { return host::Fq::from_std(host::u256_from_le(b)); };
    const host::Affine<host::Fq> hp{fq(p), fq(p + 32), pinf};
    const host::Affine<host::Fq2> hq{host::Fq2{fq(q), fq(q + 32)}, host::Fq2{fq(q + 64), fq(q + 96)}, qinf};
    const host::Fq12 want = host::pairing(hp, hq);
    const host::Fq12 got = host::final_exponentiation(host_from_words(out.data() + i * 96));
    uint32_t a[96], b[96];
    host_to_words(want, a);
    host_to_words(got, b);
    const bool ok = !memcmp(a, b, sizeof a);
    bad += !ok;
    printf("%d\n", ok ? 1 : 0);
  }
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "tower")) return run_tower(strtoull(argv[2], nullptr, 10));
  if (argc == 3 && !strcmp(argv[1], "miller")) return run_miller(argv[2]);
  fprintf(stderr, "usage: pairing_emu tower <seed> | miller <file>\n");
  return 2;
}
