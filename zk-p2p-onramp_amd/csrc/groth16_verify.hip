// Batched Groth16 verification and the kernel-level pairing entry points (groth16_verify.hpp).
//
// Kernels (one wave per workgroup where f lives in LDS):
//   k_miller         zkp_miller_loop: pairs of standard-form affine points -> Miller values
//   k_f12_product    256 Fq12 values per workgroup -> one (4 per lane in registers, then a tree in LDS)
//   k_verify_gates   one flag per proof: the point checks
//   k_verify_scale   r_i A_i (homogeneous projective, device form) and r_i C_i (affine, standard form)
//   k_miller_proj    Miller loop of (r_i A_i, B_i) for the proofs that passed the gates
#include "groth16_verify.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>
#include <vector>

#include "device_pipeline.hpp"
#include "gfft_kernels.hpp"
#include "hip_raii.hpp"
#include "mpc.hpp"
#include "pairing_kernels.hpp"
#include "zkey_verify.hpp"

namespace zkp {

namespace {

using pairing::F12;
using pairing::F12_WORDS;
using pairing::FrobConsts;
using pairing::LaneMem;

constexpr int WAVE = 64;
constexpr int PROD_PER_LANE = 4;
constexpr int PROD_SHARE = WAVE * PROD_PER_LANE;  // values per workgroup of k_f12_product

unsigned wave_grid(size_t n) { return (unsigned)((n + WAVE - 1) / WAVE); }

double wall_ms(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---------------------------------------------------------------- kernels
__global__ __launch_bounds__(WAVE) void k_miller(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2,
                                                 size_t n, FrobConsts fc, uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[F12_WORDS * WAVE];
  const size_t i = (size_t)blockIdx.x * WAVE + threadIdx.x;
  if (i >= n) return;
  pairing::miller_pair_std(g1, g2, i, fc, LaneMem{lds + threadIdx.x, WAVE}, out);
}

__global__ __launch_bounds__(WAVE) void k_f12_product(const uint32_t* __restrict__ in, size_t n,
                                                      uint32_t* __restrict__ part) {
  __shared__ uint32_t lds[F12_WORDS * WAVE];
  const int lane = threadIdx.x;
  F12 acc = pairing::f12_one();
  for (int k = 0; k < PROD_PER_LANE; ++k) {
    const size_t i = (size_t)blockIdx.x * PROD_SHARE + (size_t)k * WAVE + lane;
    if (i < n) acc = pairing::f12_mul(acc, pairing::f12_load_std(in + i * 96));
  }
  pairing::lm_store(LaneMem{lds + lane, WAVE}, acc);
  for (int half = WAVE / 2; half > 0; half >>= 1) {
    __syncthreads();
    if (lane < half) acc = pairing::f12_mul(acc, pairing::lm_load(LaneMem{lds + lane + half, WAVE}));
    __syncthreads();
    if (lane < half) pairing::lm_store(LaneMem{lds + lane, WAVE}, acc);
  }
  if (lane == 0) pairing::f12_store_std(part + (size_t)blockIdx.x * 96, acc);
}

// curve constants, standard form: b of G1 is 3; b2 = 3 / (9 + u)
struct alignas(16) GateConsts {
  uint32_t b2[16];
};

ZDEV bool geq_mod(const Fq& a) {  // a (exact limbs of a 256-bit value) >= p
#pragma unroll
  for (int l = NL - 1; l >= 0; --l)
    if (a.v[l] != FqCfg::MOD[l]) return a.v[l] > FqCfg::MOD[l];
  return true;
}
ZDEV Fq2 to_mont2(const Fq2& a) { return Fq2{to_mont(a.c0), to_mont(a.c1)}; }

// all-zero (infinity), or canonical coordinates with y^2 = x^3 + 3
ZDEV bool g1_gate(const Aff<Fq>& s) {
  if (aff_is_inf(s)) return true;
  if (geq_mod(s.x) || geq_mod(s.y)) return false;
  const Fq x = to_mont(s.x), y = to_mont(s.y);
  Fq three = fe_zero<FqCfg>();
  three.v[0] = 3;
  return eq(sqr(y), add(mul(sqr(x), x), to_mont(three)));
}

// all-zero, or canonical coordinates on the twist with [r]B = infinity (g2_subgroup_kernels.hpp's ladder)
ZDEV bool g2_gate(const Aff<Fq2>& s, const GateConsts& gc) {
  if (aff_is_inf(s)) return true;
  if (geq_mod(s.x.c0) || geq_mod(s.x.c1) || geq_mod(s.y.c0) || geq_mod(s.y.c1)) return false;
  const Fq2 x = to_mont2(s.x), y = to_mont2(s.y);
  Fq2 b2;
  load_f(gc.b2, b2);
  const Fq2 d = sub(sqr(y), add(mul(sqr(x), x), to_mont2(b2)));
  if (!is_zero(d)) return false;
  uint32_t r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = FrCfg::MOD_W[k];
  const Xyzz<Fq2> p{x, y, f_one<Fq2>(), f_one<Fq2>()};
  return xyzz_is_inf(gfft::scale<2>(p, r));
}

// a, c: n x 16 words, b: n x 32 words (standard form); ok[i] = 1 if proof i passes every point check
__global__ __launch_bounds__(WAVE) void k_verify_gates(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                       const uint32_t* __restrict__ c, size_t n, GateConsts gc,
                                                       uint32_t* __restrict__ ok) {
  const size_t i = (size_t)blockIdx.x * WAVE + threadIdx.x;
  if (i >= n) return;
  bool good = g1_gate(load_aff<Fq>(a, i)) && g1_gate(load_aff<Fq>(c, i));
  if (good) good = g2_gate(load_aff<Fq2>(b, i), gc);
  ok[i] = good ? 1u : 0u;
}

ZDEV Xyzz<Fq> g1_xyzz(const Aff<Fq>& s) {
  if (aff_is_inf(s)) return xyzz_inf<Fq>();
  return Xyzz<Fq>{to_mont(s.x), to_mont(s.y), fe_one<FqCfg>(), fe_one<FqCfg>()};
}

// pa[i]: r_i A_i as (X ZZZ, Y ZZ, ZZ ZZZ), device form, 24 words (all-zero: infinity or a gated-out proof);
// rc[i]: r_i C_i affine, standard form, 16 words (all-zero: infinity or gated out)
__global__ __launch_bounds__(WAVE) void k_verify_scale(const uint32_t* __restrict__ a, const uint32_t* __restrict__ c,
                                                       const uint32_t* __restrict__ coeffs,
                                                       const uint32_t* __restrict__ ok, size_t n,
                                                       uint32_t* __restrict__ pa, uint32_t* __restrict__ rc) {
  const size_t i = (size_t)blockIdx.x * WAVE + threadIdx.x;
  if (i >= n) return;
  Fq px = fe_zero<FqCfg>(), py = px, pz = px;
  Aff<Fq> rca{px, px};
  if (ok[i]) {
    uint32_t r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = coeffs[i * 8 + k];
    const Xyzz<Fq> ra = gfft::scale<2>(g1_xyzz(load_aff<Fq>(a, i)), r);
    if (!xyzz_is_inf(ra)) {
      px = mul(acc_xcanon(ra.x), ra.zzz);
      py = mul(ra.y, ra.zz);
      pz = mul(ra.zz, ra.zzz);
    }
    const Xyzz<Fq> rcx = gfft::scale<2>(g1_xyzz(load_aff<Fq>(c, i)), r);
    if (!xyzz_is_inf(rcx)) {
      const Aff<Fq> t = xyzz_to_aff(rcx);
      rca = Aff<Fq>{from_mont(t.x), from_mont(t.y)};
    }
  }
  store_fe(pa + i * 24, canon(px));
  store_fe(pa + i * 24 + 8, canon(py));
  store_fe(pa + i * 24 + 16, canon(pz));
  store_aff(rc, i, rca);
}

__global__ __launch_bounds__(WAVE) void k_miller_proj(const uint32_t* __restrict__ pa, const uint32_t* __restrict__ b,
                                                      const uint32_t* __restrict__ ok, size_t n, FrobConsts fc,
                                                      uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[F12_WORDS * WAVE];
  const size_t i = (size_t)blockIdx.x * WAVE + threadIdx.x;
  if (i >= n) return;
  const pairing::ProjG1 p{load_fe<FqCfg>(pa + i * 24), load_fe<FqCfg>(pa + i * 24 + 8), load_fe<FqCfg>(pa + i * 24 + 16)};
  const Aff<Fq2> qs = load_aff<Fq2>(b, i);
  if (!ok[i] || is_zero_raw(p.z) || aff_is_inf(qs)) {
    pairing::f12_store_std(out + i * 96, pairing::f12_one());
    return;
  }
  const LaneMem fm{lds + threadIdx.x, WAVE};
  pairing::miller_loop(p, Aff<Fq2>{to_mont2(qs.x), to_mont2(qs.y)}, fc, fm);
  pairing::f12_store_std(out + i * 96, pairing::lm_load(fm));
}

// ---------------------------------------------------------------- host helpers
void put_fq2(const host::Fq2& a, uint32_t* w) {
  host::u256_to_le(a.c0.to_std(), reinterpret_cast<uint8_t*>(w));
  host::u256_to_le(a.c1.to_std(), reinterpret_cast<uint8_t*>(w + 8));
}
FrobConsts frob_consts() {
  FrobConsts fc;
  host::Fq2 gx, gy;
  host::g2_frobenius_consts(gx, gy);
  put_fq2(gx, fc.gx);
  put_fq2(gy, fc.gy);
  return fc;
}
GateConsts gate_consts() {
  GateConsts gc;
  const host::Fq2 xi{host::Fq::from_std(host::U256{{9, 0, 0, 0}}), host::Fq::one()};
  const host::Fq2 b2 = host::Fq2{host::Fq::from_std(host::U256{{3, 0, 0, 0}}), host::Fq::zero()} * xi.inv();
  put_fq2(b2, gc.b2);
  return gc;
}

host::Fq12 f12_from_bytes(const uint8_t* b) {
  host::Fq2 c[6];
  for (int i = 0; i < 6; ++i) {
    c[i].c0 = host::Fq::from_std(host::u256_from_le(b + 64 * i));
    c[i].c1 = host::Fq::from_std(host::u256_from_le(b + 64 * i + 32));
  }
  return host::Fq12{host::Fq6{c[0], c[1], c[2]}, host::Fq6{c[3], c[4], c[5]}};
}
void f12_to_bytes(const host::Fq12& f, uint8_t* out) {
  const host::Fq2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  for (int i = 0; i < 6; ++i) {
    host::u256_to_le(c[i]->c0.to_std(), out + 64 * i);
    host::u256_to_le(c[i]->c1.to_std(), out + 64 * i + 32);
  }
}

// the product of the n values at d_in (device, n x 96 words), finished on the host
host::Fq12 product_resident(const uint32_t* d_in, size_t n, hipStream_t st) {
  host::Fq12 r = host::fq12_one();
  if (n == 0) return r;
  const size_t blocks = (n + PROD_SHARE - 1) / PROD_SHARE;
  DevBuf<> dpart(blocks * 96);
  hipLaunchKernelGGL(k_f12_product, dim3((unsigned)blocks), dim3(WAVE), 0, st, d_in, n, dpart.get());
  HIPX(hipGetLastError());
  std::vector<uint32_t> part(blocks * 96);
  HIPX(hipMemcpyAsync(part.data(), dpart, part.size() * 4, hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  for (size_t b = 0; b < blocks; ++b) r = host::fq12_mul(r, f12_from_bytes(reinterpret_cast<const uint8_t*>(&part[b * 96])));
  return r;
}

template <class Fn>
void parallel_for(size_t n, Fn&& fn) {
  const size_t nt = std::min<size_t>(n, std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency())));
  if (nt <= 1) {
    for (size_t i = 0; i < n; ++i) fn(i);
    return;
  }
  std::vector<std::thread> th;
  std::atomic<size_t> next{0};
  for (size_t t = 0; t < nt; ++t)
    th.emplace_back([&] {
      for (size_t i; (i = next.fetch_add(1)) < n;) fn(i);
    });
  for (auto& t : th) t.join();
}

}  // namespace

Groth16VerifyTimings& verify_timings() {
  thread_local Groth16VerifyTimings t;
  return t;
}

int verify_chunk_size() { return env_int_range("ZKP_VERIFY_CHUNK", 16384, 64, 1 << 20); }

void miller_loop_points(int device, const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out) {
  if (n == 0) return;
  HIPX(hipSetDevice(device));
  Stream st(hipStreamNonBlocking);
  const FrobConsts fc = frob_consts();
  const size_t chunk = (size_t)verify_chunk_size();
  DevBuf<> d1(std::min(n, chunk) * 16), d2(std::min(n, chunk) * 32), dout(std::min(n, chunk) * 96);
  for (size_t at = 0; at < n; at += chunk) {
    const size_t m = std::min(chunk, n - at);
    HIPX(hipMemcpyAsync(d1, g1 + at * 64, m * 64, hipMemcpyHostToDevice, st));
    HIPX(hipMemcpyAsync(d2, g2 + at * 128, m * 128, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_miller, dim3(wave_grid(m)), dim3(WAVE), 0, st, d1.get(), d2.get(), m, fc, dout.get());
    HIPX(hipGetLastError());
    HIPX(hipMemcpyAsync(out + at * 384, dout, m * 384, hipMemcpyDeviceToHost, st));
    HIPX(hipStreamSynchronize(st));
  }
}

void fq12_product(int device, const uint8_t* in, size_t n, uint8_t* out384) {
  host::Fq12 r = host::fq12_one();
  if (n) {
    HIPX(hipSetDevice(device));
    Stream st(hipStreamNonBlocking);
    const size_t chunk = (size_t)verify_chunk_size();
    DevBuf<> din(std::min(n, chunk) * 96);
    for (size_t at = 0; at < n; at += chunk) {
      const size_t m = std::min(chunk, n - at);
      HIPX(hipMemcpyAsync(din, in + at * 384, m * 384, hipMemcpyHostToDevice, st));
      r = host::fq12_mul(r, product_resident(din, m, st));
    }
  }
  f12_to_bytes(r, out384);
}

// ---------------------------------------------------------------- the verifier
Verifier::Verifier(int device, VKey&& vk) : dev_(device), vk_(std::move(vk)) {
  int count = 0;
  HIPX(hipGetDeviceCount(&count));
  if (device < 0 || device >= count) throw ZkpError(ZKP_ERR_INVALID_ARG, "verifier: no such device");
}
Verifier::~Verifier() = default;

void Verifier::verify(const zkp_proof* proofs, size_t n, const uint8_t* seed32, uint8_t* valid, size_t* n_valid) {
  std::lock_guard<std::mutex> lock(mu_);
  const auto t0 = std::chrono::steady_clock::now();
  Groth16VerifyTimings& t = verify_timings();
  t = Groth16VerifyTimings{};
  for (size_t i = 0; i < n; ++i)
    if (proofs[i].n_public != vk_.n_public || proofs[i].public_capacity < vk_.n_public ||
        (vk_.n_public && !proofs[i].public_signals))
      throw ZkpError(ZKP_ERR_INVALID_ARG, "verify: proof " + std::to_string(i) + ": public signals do not match the key's nPublic");
  uint8_t seed[32];
  if (seed32)
    std::memcpy(seed, seed32, 32);
  else
    os_random(seed, 32);
  const size_t chunk = (size_t)verify_chunk_size();
  for (size_t at = 0; at < n; at += chunk) verify_chunk(proofs + at, std::min(chunk, n - at), seed, at, valid + at);
  size_t good = 0;
  for (size_t i = 0; i < n; ++i) good += valid[i] ? 1 : 0;
  if (n_valid) *n_valid = good;
  t.total_ms = wall_ms(t0);
}

void Verifier::verify_chunk(const zkp_proof* proofs, size_t n, const uint8_t* seed, uint64_t first, uint8_t* valid) {
  Groth16VerifyTimings& t = verify_timings();
  const uint32_t np = vk_.n_public;
  auto t0 = std::chrono::steady_clock::now();
  // host gate: every public signal below r
  std::vector<uint8_t> pub_ok(n, 1);
  for (size_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < np; ++j)
      if (host::u256_geq(host::u256_from_le(proofs[i].public_signals + 32 * (size_t)j), host::FR_DESC.mod)) pub_ok[i] = 0;
  std::vector<uint8_t> ha(n * 64), hb(n * 128), hc(n * 64);
  for (size_t i = 0; i < n; ++i) {
    std::memcpy(&ha[i * 64], proofs[i].pi_a, 64);
    std::memcpy(&hb[i * 128], proofs[i].pi_b, 128);
    std::memcpy(&hc[i * 64], proofs[i].pi_c, 64);
  }
  HIPX(hipSetDevice(dev_));
  Stream st(hipStreamNonBlocking);
  DevBuf<> da(n * 16), db(n * 32), dc(n * 16), dcoef(n * 8), dok(n), dpa(n * 24), drc(n * 16), df(n * 96);
  HIPX(hipMemcpyAsync(da, ha.data(), n * 64, hipMemcpyHostToDevice, st));
  HIPX(hipMemcpyAsync(db, hb.data(), n * 128, hipMemcpyHostToDevice, st));
  HIPX(hipMemcpyAsync(dc, hc.data(), n * 64, hipMemcpyHostToDevice, st));
  rlc_coeffs_resident(seed, first, n, dcoef, st);
  hipLaunchKernelGGL(k_verify_gates, dim3(wave_grid(n)), dim3(WAVE), 0, st, da.get(), db.get(), dc.get(), n, gate_consts(),
                     dok.get());
  HIPX(hipGetLastError());
  std::vector<uint32_t> ok(n);
  HIPX(hipMemcpyAsync(ok.data(), dok, n * 4, hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  for (size_t i = 0; i < n; ++i) ok[i] = (ok[i] && pub_ok[i]) ? 1u : 0u;
  HIPX(hipMemcpyAsync(dok, ok.data(), n * 4, hipMemcpyHostToDevice, st));  // the host gate joins the device's
  t.gates_ms += wall_ms(t0);

  t0 = std::chrono::steady_clock::now();
  hipLaunchKernelGGL(k_verify_scale, dim3(wave_grid(n)), dim3(WAVE), 0, st, da.get(), dc.get(), dcoef.get(), dok.get(), n,
                     dpa.get(), drc.get());
  HIPX(hipGetLastError());
  HIPX(hipStreamSynchronize(st));
  t.scalar_ms += wall_ms(t0);

  t0 = std::chrono::steady_clock::now();
  hipLaunchKernelGGL(k_miller_proj, dim3(wave_grid(n)), dim3(WAVE), 0, st, dpa.get(), db.get(), dok.get(), n, frob_consts(),
                     df.get());
  HIPX(hipGetLastError());
  HIPX(hipStreamSynchronize(st));
  t.miller_ms += wall_ms(t0);

  t0 = std::chrono::steady_clock::now();
  const host::Fq12 fprod = product_resident(df, n, st);
  std::vector<uint32_t> coef(n * 8), rc(n * 16);
  HIPX(hipMemcpyAsync(coef.data(), dcoef, n * 32, hipMemcpyDeviceToHost, st));
  HIPX(hipMemcpyAsync(rc.data(), drc, n * 64, hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  t.product_ms += wall_ms(t0);

  // per-proof host values of the survivors
  using HFr = host::Fr;
  using HJac = host::Jac<host::Fq>;
  std::vector<HFr> r(n);
  std::vector<host::Affine<host::Fq>> rcp(n);
  for (size_t i = 0; i < n; ++i) {
    valid[i] = ok[i] ? 1 : 0;
    r[i] = HFr::from_std(host::u256_from_le(reinterpret_cast<const uint8_t*>(&coef[i * 8])));
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&rc[i * 16]);
    bool inf = true;
    for (int k = 0; k < 64; ++k) inf &= p[k] == 0;
    rcp[i] = host::Affine<host::Fq>{host::Fq::from_std(host::u256_from_le(p)), host::Fq::from_std(host::u256_from_le(p + 32)), inf};
  }
  auto pub = [&](size_t i, uint32_t j) { return HFr::from_std(host::u256_from_le(proofs[i].public_signals + 32 * (size_t)j)); };
  // the equation of the proofs [lo, hi) that passed the gates, given the product of their Miller values
  auto node_ok = [&](size_t lo, size_t hi, const host::Fq12& f, double* ml_ms, double* fe_ms) {
    auto a0 = std::chrono::steady_clock::now();
    std::vector<HFr> s(np + 1, HFr::zero());
    HJac csum = HJac::inf();
    for (size_t i = lo; i < hi; ++i) {
      if (!ok[i]) continue;
      s[0] = s[0] + r[i];
      for (uint32_t j = 0; j < np; ++j) s[j + 1] = s[j + 1] + r[i] * pub(i, j);
      csum = host::jac_add(csum, host::jac_from_aff(rcp[i]));
    }
    HJac x = HJac::inf();
    for (uint32_t j = 0; j <= np; ++j) x = host::jac_add(x, host::jac_mul(host::jac_from_aff(vk_.ic[j]), s[j].to_std()));
    const HJac al = host::jac_mul(host::jac_from_aff(vk_.alpha1), s[0].to_std());
    host::Affine<host::Fq> ps[3] = {host::jac_to_aff(x), host::jac_to_aff(csum), host::jac_to_aff(al)};
    for (auto& p : ps)
      if (!p.inf) p.y = p.y.neg();
    const host::Affine<host::Fq2> qs[3] = {vk_.gamma2, vk_.delta2, vk_.beta2};
    const host::Fq12 m = host::fq12_mul(f, host::miller_loop_multi(ps, qs, 3));
    if (ml_ms) *ml_ms += wall_ms(a0);
    a0 = std::chrono::steady_clock::now();
    const bool one = host::fq12_is_one(host::final_exponentiation(m));
    if (fe_ms) *fe_ms += wall_ms(a0);
    return one;
  };
  t.node_checks += 1;
  if (node_ok(0, n, fprod, &t.host_miller_ms, &t.final_exp_ms)) return;

  // the batch fails: the per-proof Miller values come to the host and a binary tree over the proofs is
  // searched level by level.  A failing node's left half is checked; if it passes, the right half fails
  // without a check (the node's value is the product of its halves), else the right half is checked too.
  // A failing node of one proof is an invalid proof.
  t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> fb(n * 384);
  HIPX(hipMemcpyAsync(fb.data(), df, n * 384, hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  std::vector<host::Fq12> f(n);
  parallel_for(n, [&](size_t i) { f[i] = f12_from_bytes(&fb[i * 384]); });
  auto range_ok = [&](size_t lo, size_t hi) {
    host::Fq12 p = host::fq12_one();
    for (size_t i = lo; i < hi; ++i)
      if (ok[i]) p = host::fq12_mul(p, f[i]);
    return node_ok(lo, hi, p, nullptr, nullptr);
  };
  struct Range {
    size_t lo, hi;
  };
  std::vector<Range> failing{{0, n}};
  std::atomic<uint64_t> checks{0};
  while (!failing.empty()) {
    std::vector<Range> next(failing.size() * 2, Range{0, 0});
    parallel_for(failing.size(), [&](size_t k) {
      const Range g = failing[k];
      if (g.hi - g.lo == 1) {
        valid[g.lo] = 0;
        return;
      }
      const size_t mid = g.lo + (g.hi - g.lo) / 2;
      ++checks;
      bool right_fails = true;
      if (!range_ok(g.lo, mid)) {
        next[2 * k] = Range{g.lo, mid};
        ++checks;
        right_fails = !range_ok(mid, g.hi);
      }
      if (right_fails) next[2 * k + 1] = Range{mid, g.hi};
    });
    failing.clear();
    for (const Range& g : next)
      if (g.hi > g.lo) failing.push_back(g);
  }
  t.node_checks += (double)checks.load();
  t.search_ms += wall_ms(t0);
}

}  // namespace zkp
