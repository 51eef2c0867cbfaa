// Device side of `zkey verify` (zkey_verify.hpp): the verifier's coefficients, the validation of the
// L / H points and the paired random linear combination of two point sets under one MSM plan.
//
// Per chunk of points: both slices are uploaded (the next chunk's upload on a second stream overlaps
// this chunk's accumulation: two buffer pairs), k_check_points validates them as they arrived,
// k_rlc_coeffs writes the chunk's coefficients, one MsmPlan is built from them and the MsmEngine runs
// once per base set against that plan.  The bases are used once: depth T = 1, no tables.  The
// coefficients are below 2^128, so the plan covers 129 bits (MsmParams::scalar_bits): ceil(129 / c)
// bucket groups instead of ceil(255 / c).  Chunk sums are folded (msm_fold) and added on the host.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "curve.hpp"
#include "device_pipeline.hpp"
#include "mpc.hpp"
#include "points_through.hpp"
#include "ptau_scale_kernels.hpp"
#include "qap.hpp"
#include "spans.hpp"
#include "zkey_verify.hpp"

namespace zkp {

namespace {

constexpr int TPB = 256;
unsigned grid(size_t n) { return (unsigned)((n + TPB - 1) / TPB); }

struct Seed8 {
  uint32_t w[8];
};

// One thread per 16-word ChaCha20 block (ffjavascript's ChaCha: the block counter in state words
// 12..15, carried; blocks below 2^64 leave 14 and 15 zero): the block's four 128-bit coefficients
// that fall into [first_index, first_index + n) as 8-word scalars, upper four words zero.
__global__ __launch_bounds__(TPB) void k_rlc_coeffs(Seed8 seed, uint64_t first_index, uint64_t n,
                                                    uint32_t* __restrict__ out) {
  const uint64_t blk = (first_index >> 2) + (uint64_t)blockIdx.x * TPB + threadIdx.x;
  if (blk > ((first_index + n - 1) >> 2)) return;
  uint32_t s[16], x[16];
  s[0] = 0x61707865u, s[1] = 0x3320646Eu, s[2] = 0x79622D32u, s[3] = 0x6B206574u;
#pragma unroll
  for (int i = 0; i < 8; ++i) s[4 + i] = seed.w[i];
  s[12] = (uint32_t)blk, s[13] = (uint32_t)(blk >> 32), s[14] = 0u, s[15] = 0u;
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = s[i];
  auto rotl = [](uint32_t v, int k) { return (v << k) | (v >> (32 - k)); };
  auto qr = [&](uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
    a += b, d = rotl(d ^ a, 16);
    c += d, b = rotl(b ^ c, 12);
    a += b, d = rotl(d ^ a, 8);
    c += d, b = rotl(b ^ c, 7);
  };
  for (int r = 0; r < 10; ++r) {
    qr(x[0], x[4], x[8], x[12]), qr(x[1], x[5], x[9], x[13]), qr(x[2], x[6], x[10], x[14]), qr(x[3], x[7], x[11], x[15]);
    qr(x[0], x[5], x[10], x[15]), qr(x[1], x[6], x[11], x[12]), qr(x[2], x[7], x[8], x[13]), qr(x[3], x[4], x[9], x[14]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] += s[i];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint64_t idx = blk * 4 + j;
    if (idx < first_index || idx - first_index >= n) continue;
    uint4* o = reinterpret_cast<uint4*>(out + (idx - first_index) * 8);
    o[0] = make_uint4(x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]);
    o[1] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// sum_(i < n) r_i * base * ratio^i over the chunk's coefficients (8-word standard form, as k_rlc_coeffs writes
// them): every thread one term, the block's sum by a tree in LDS into part[blockIdx.x] (8 words, standard
// form); the host adds the blocks.  pw: pscale::fill_powers(1, w, chunk start), so base = w^start.
__global__ __launch_bounds__(TPB) void k_rlc_power_sum(const uint32_t* __restrict__ coeffs, size_t n, pscale::Powers pw,
                                                       uint32_t* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint32_t sh[TPB * 8];
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  Fr term = fe_zero<FrCfg>();
  if (i < n) {
    Fr t = load_fe<FrCfg>(pw.base);
#pragma unroll
    for (int b = 0; b < pscale::POW_BITS; ++b)
      if ((i >> b) & 1) t = mul(t, load_fe<FrCfg>(pw.pw[b]));
    term = mul(t, to_mont(load_fe<FrCfg>(coeffs + i * 8)));
  }
  store_fe(sh + threadIdx.x * 8, canon(term));
  __syncthreads();
  for (int half = TPB / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) {
      const Fr a = load_fe<FrCfg>(sh + threadIdx.x * 8), b = load_fe<FrCfg>(sh + (threadIdx.x + half) * 8);
      store_fe(sh + threadIdx.x * 8, canon(add(a, b)));
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    uint32_t w[8];
    gfft::fr_words(load_fe<FrCfg>(sh), w);
    pscale::store8(part + (size_t)blockIdx.x * 8, w);
  }
}

// the curve constant b (G1: 3, G2: 3 / (9 + u)) as the zkey stores field elements
struct alignas(16) CurveB {
  uint32_t w[16];
};

ZDEV bool geq_mod(const Fq& a) {  // a (exact limbs of a 256-bit value) >= p
#pragma unroll
  for (int l = NL - 1; l >= 0; --l)
    if (a.v[l] != FqCfg::MOD[l]) return a.v[l] > FqCfg::MOD[l];
  return true;
}
ZDEV bool canonical(const Fq& a) { return !geq_mod(a); }
ZDEV bool canonical(const Fq2& a) { return !geq_mod(a.c0) && !geq_mod(a.c1); }
ZDEV Fq to_dev(const Fq& a, const Fq& k) { return mul(a, k); }
ZDEV Fq2 to_dev(const Fq2& a, const Fq& k) { return Fq2{mul(a.c0, k), mul(a.c1, k)}; }
ZDEV Fq below2m(const Fq& a) { return a; }          // an Fq product is < 2m
ZDEV Fq2 below2m(const Fq2& a) { return canon4(a); }  // an Fq2 product's components are < 4m

// Point i of `pts` (zkey layout: Montgomery 2^256 LE, as uploaded, before any conversion) is good if
// it is all-zero (infinity), or every coordinate is canonical (< p: x + p fits in 256 bits and names
// the same residue) and y^2 = x^3 + b.  The mixed additions never use b, so a sum over points of
// another curve would prove nothing.  out[0] += bad points, out[1] = min(out[1], base + i) over them.
template <class F>
__global__ __launch_bounds__(TPB) void k_check_points(const uint32_t* __restrict__ pts, size_t n, uint64_t base,
                                                      CurveB b, unsigned long long* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const Aff<F> a = load_aff<F>(pts, i);
  if (aff_is_inf(a)) return;
  bool ok = canonical(a.x) && canonical(a.y);
  if (ok) {
    const Fq k = fe_const<FqCfg>(Conv::FQ_ZKEY_TO_DEV);
    F bb;
    load_f(b.w, bb);
    const F x = to_dev(a.x, k), y = to_dev(a.y, k), bd = to_dev(bb, k);
    const F rhs = add(below2m(mul(sqr(x), x)), bd);
    ok = is_zero(sub(sqr(y), rhs));
  }
  if (!ok) {
    atomicAdd(&out[0], 1ull);
    atomicMin(&out[1], (unsigned long long)(base + i));
  }
}

CurveB curve_b(bool g2) {
  CurveB b{};
  auto put = [&](const HFq& v, int at) {
    for (int i = 0; i < 4; ++i) b.w[at + 2 * i] = (uint32_t)v.v.w[i], b.w[at + 2 * i + 1] = (uint32_t)(v.v.w[i] >> 32);
  };
  auto small = [](uint64_t v) { return HFq::from_std(U256{{v, 0, 0, 0}}); };
  if (!g2) {
    put(small(3), 0);
  } else {
    const HFq2 b2 = HFq2{small(3), HFq::zero()} * HFq2{small(9), small(1)}.inv();
    put(b2.c0, 0), put(b2.c1, 8);
  }
  return b;
}

void launch_check(bool g2, const uint32_t* pts, size_t n, uint64_t base, const CurveB& b, unsigned long long* out,
                  hipStream_t st) {
  if (!n) return;
  if (g2)
    hipLaunchKernelGGL(k_check_points<Fq2>, dim3(grid(n)), dim3(TPB), 0, st, pts, n, base, b, out);
  else
    hipLaunchKernelGGL(k_check_points<Fq>, dim3(grid(n)), dim3(TPB), 0, st, pts, n, base, b, out);
  HIPX(hipGetLastError());
}

// out[0] = 0 (count), out[1] = all ones (no bad index yet), for `sets` point sets
void reset_bad(unsigned long long* out, int sets, hipStream_t st) {
  HIPX(hipMemsetAsync(out, 0, (size_t)sets * 16, st));
  for (int s = 0; s < sets; ++s) HIPX(hipMemsetAsync(out + 2 * s + 1, 0xFF, 8, st));
}

Seed8 seed_words(const uint8_t* seed32) {
  Seed8 s;
  seed_from_hash(seed32, s.w);
  return s;
}

void check_index_range(uint64_t first_index, size_t n) {
  if (first_index > (uint64_t(1) << 62) || (uint64_t)n > (uint64_t(1) << 62))
    throw ZkpError(ZKP_ERR_INVALID_ARG, "rlc: coefficient index out of range");
}

}  // namespace

// window bits for n uniform 128-bit scalars at depth 1: lg n - 3 as the kernel-level MSMs take, moved
// off the widths whose top window (128 - (W - 1) c bits) collapses into a few buckets of one group
// (dense_window_bits states the cost for 254-bit scalars)
int rlc_window_bits(size_t n) {
  int lg = 0;
  while ((size_t(1) << lg) < n) ++lg;
  const int c = std::min(20, std::max(8, lg - 3));
  auto top = [](int cc) { return 128 - ((129 + cc - 1) / cc - 1) * cc; };
  if (n < (size_t(1) << 17) || top(c) >= 12) return c;
  for (int d = 1; d <= 6; ++d) {
    if (c + d <= 20 && top(c + d) >= 12) return c + d;
    if (c - d >= 8 && top(c - d) >= 12) return c - d;
  }
  return c;
}

size_t verify_chunk_points() {
  constexpr size_t DEFAULT = size_t(1) << 22, MAX = size_t(1) << 24;
  const char* e = std::getenv("ZKP_VERIFY_CHUNK");
  if (!e) return DEFAULT;
  char* stop = nullptr;
  const long long v = std::strtoll(e, &stop, 10);
  if (!*e || *stop || v < 1 || (unsigned long long)v > MAX)
    throw ZkpError(ZKP_ERR_INVALID_ARG, "ZKP_VERIFY_CHUNK: points per chunk must be an integer within 1.." +
                                            std::to_string(MAX) + " (got '" + e + "')");
  return (size_t)v;
}

void rlc_coeffs(int device, const uint8_t* seed32, uint64_t first_index, size_t n, uint8_t* out) {
  check_index_range(first_index, n);
  if (!n) return;
  HIPX(hipSetDevice(device));
  Stream st(hipStreamNonBlocking);
  const size_t CH = std::min(n, size_t(1) << 22);
  DevBuf<> d(CH * 8);
  std::vector<uint32_t> h(CH * 8);
  const Seed8 seed = seed_words(seed32);
  for (size_t at = 0; at < n; at += CH) {
    const size_t m = std::min(CH, n - at);
    const uint64_t first = first_index + at, blocks = ((first + m - 1) >> 2) - (first >> 2) + 1;
    hipLaunchKernelGGL(k_rlc_coeffs, dim3(grid(blocks)), dim3(TPB), 0, st, seed, first, (uint64_t)m, d.get());
    HIPX(hipGetLastError());
    HIPX(hipMemcpyAsync(h.data(), d, m * 32, hipMemcpyDeviceToHost, st));
    HIPX(hipStreamSynchronize(st));
    for (size_t i = 0; i < m; ++i) std::memcpy(out + (at + i) * 16, h.data() + i * 8, 16);
  }
}

void rlc_coeffs_resident(const uint8_t* seed32, uint64_t first_index, size_t n, uint32_t* d_out, hipStream_t st) {
  check_index_range(first_index, n);
  if (!n) return;
  const uint64_t blocks = ((first_index + n - 1) >> 2) - (first_index >> 2) + 1;
  hipLaunchKernelGGL(k_rlc_coeffs, dim3(grid(blocks)), dim3(TPB), 0, st, seed_words(seed32), first_index, (uint64_t)n, d_out);
  HIPX(hipGetLastError());
}

void points_check(int device, bool g2, const uint8_t* points, size_t n, uint64_t* n_bad, uint64_t* first_bad) {
  *n_bad = 0, *first_bad = RLC_NO_BAD;
  if (!n) return;
  HIPX(hipSetDevice(device));
  const CurveB b = curve_b(g2);
  points_through(verify_chunk_points(), g2 ? 128 : 64, 0, points, n, nullptr, n_bad, first_bad,
                 [&](const uint32_t* d, size_t m, uint64_t base, uint32_t*, unsigned long long* bad, hipStream_t st) {
                   launch_check(g2, d, m, base, b, bad, st);
                 });
}

void points_bad_reset(unsigned long long* bad, hipStream_t st) { reset_bad(bad, 1, st); }

void points_check_resident(bool g2, const uint32_t* d_points, size_t n, uint64_t base, unsigned long long* bad,
                           hipStream_t st) {
  launch_check(g2, d_points, n, base, curve_b(g2), bad, st);
}

RlcResult rlc_g1(int device, const uint8_t* seed32, uint64_t first_index, const uint8_t* a, const uint8_t* b,
                 size_t n, bool on_hyperplane) {
  const auto t_begin = std::chrono::steady_clock::now();
  check_index_range(first_index, n);
  RlcResult res;
  if (!n) return res;
  int log_n = 0;
  while ((size_t(1) << log_n) < n) ++log_n;
  if (on_hyperplane && ((size_t(1) << log_n) != n || log_n > 28))
    throw ZkpError(ZKP_ERR_INVALID_ARG, "rlc: the hyperplane rule wants 2^p points, p <= 28");
  // w = Fr.w[log_n] and the running sum_(j < n - 1) r_j w^j (on_hyperplane)
  uint32_t w_words[8];
  for (int i = 0; i < 8; ++i) w_words[i] = FR_ROOTS_W[log_n][i];
  const uint32_t one_words[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  host::Fr power_sum = host::Fr::zero();
  const size_t CH = std::min(n, verify_chunk_points()), nchunks = (n + CH - 1) / CH, tail = n % CH;
  HIPX(hipSetDevice(device));
  Stream st(hipStreamNonBlocking), sup(hipStreamNonBlocking);  // first: destroyed after what runs on them
  MsmParams prm = make_params(CH, rlc_window_bits(CH), 1, 129);
  const MsmOptions opt = msm_options();
  apply_task_options(prm, opt.task_h, opt);
  // two buffer pairs of CH points; a ragged last chunk has a pair of its own size (a base set's size
  // is the plan's n)
  std::unique_ptr<MsmBases> base[2][2], tailb[2];
  for (size_t k = 0; k < std::min<size_t>(n / CH, 2); ++k)
    for (int s = 0; s < 2; ++s) base[k][s] = std::make_unique<MsmBases>(Curve::G1, CH, prm.c, 1);
  if (tail)
    for (int s = 0; s < 2; ++s) tailb[s] = std::make_unique<MsmBases>(Curve::G1, tail, prm.c, 1);
  MsmPlan plan(CH, prm, st);
  plan.set_dense(true);
  MsmEngine eng(Curve::G1, prm, CH, st);
  const size_t ww = eng.window_words();
  DevBuf<> ds(CH * 8), dwin(2 * ww);
  const size_t max_blocks = grid(CH);
  DevBuf<> dpart(on_hyperplane ? max_blocks * 8 : 1);
  PinnedBuf<uint32_t> hpart(on_hyperplane ? max_blocks * 8 : 1);
  DevBuf<unsigned long long> dbad(4);
  PinnedBuf<uint32_t> hwin(2 * ww);
  PinnedBuf<unsigned long long> hbad(4);
  Event uploaded[2] = {Event(false), Event(false)}, done(false);
  Event ev[6] = {Event(true), Event(true), Event(true), Event(true), Event(true), Event(true)};
  const CurveB cb = curve_b(false);
  const Seed8 seed = seed_words(seed32);
  const uint8_t* src[2] = {a, b};

  auto chunk_len = [&](size_t k) { return std::min(CH, n - k * CH); };
  auto bases_of = [&](size_t k, int s) -> MsmBases& { return chunk_len(k) == CH ? *base[k & 1][s] : *tailb[s]; };
  auto upload = [&](size_t k) {
    const auto t0 = std::chrono::steady_clock::now();
    const size_t m = chunk_len(k);
    for (int s = 0; s < 2; ++s)
      HIPX(hipMemcpyAsync(bases_of(k, s).row0(), src[s] + k * CH * 64, m * 64, hipMemcpyHostToDevice, sup));
    HIPX(hipEventRecord(uploaded[k & 1], sup));
    res.t.upload_ms += wall_ms(t0);
  };

  upload(0);
  for (size_t k = 0; k < nchunks; ++k) {
    const size_t m = chunk_len(k), at = k * CH;
    MsmBases& ba = bases_of(k, 0);
    MsmBases& bb = bases_of(k, 1);
    HIPX(hipStreamWaitEvent(st, uploaded[k & 1], 0));
    reset_bad(dbad, 2, st);
    HIPX(hipEventRecord(ev[0], st));
    launch_check(false, ba.row0(), m, at, cb, dbad, st);
    launch_check(false, bb.row0(), m, at, cb, dbad + 2, st);
    HIPX(hipEventRecord(ev[1], st));
    const uint64_t first = first_index + at, blocks = ((first + m - 1) >> 2) - (first >> 2) + 1;
    hipLaunchKernelGGL(k_rlc_coeffs, dim3(grid(blocks)), dim3(TPB), 0, st, seed, first, (uint64_t)m, ds.get());
    HIPX(hipGetLastError());
    // the last point's coefficient is not the stream's: it is left out of the sum and of the plan, and taken
    // by the host after the loop
    const bool has_last = on_hyperplane && k + 1 == nchunks;
    const size_t m_sum = has_last ? m - 1 : m;
    if (on_hyperplane && m_sum) {
      pscale::Powers pw;
      pscale::fill_powers(pw, one_words, w_words, at);
      hipLaunchKernelGGL(k_rlc_power_sum, dim3(grid(m_sum)), dim3(TPB), 0, st, ds.get(), m_sum, pw, dpart.get());
      HIPX(hipGetLastError());
      HIPX(hipMemcpyAsync(hpart, dpart, (size_t)grid(m_sum) * 32, hipMemcpyDeviceToHost, st));
    }
    if (has_last) HIPX(hipMemsetAsync(ds.get() + (m - 1) * 8, 0, 32, st));
    HIPX(hipEventRecord(ev[2], st));
    launch_convert_fq_zkey(ba.row0(), m * 2, st);
    launch_convert_fq_zkey(bb.row0(), m * 2, st);
    plan.build(ds, m);
    HIPX(hipEventRecord(ev[3], st));
    eng.run(plan, ba, dwin);
    HIPX(hipEventRecord(ev[4], st));
    eng.run(plan, bb, dwin + ww);
    HIPX(hipEventRecord(ev[5], st));
    HIPX(hipMemcpyAsync(hwin, dwin, 2 * ww * 4, hipMemcpyDeviceToHost, st));
    HIPX(hipMemcpyAsync(hbad, dbad, 32, hipMemcpyDeviceToHost, st));
    HIPX(hipEventRecord(done, st));
    // the next chunk goes into the other buffer pair (its last reader, chunk k - 1, is complete)
    // while this chunk computes
    if (k + 1 < nchunks) upload(k + 1);
    HIPX(hipEventSynchronize(done));
    float ms[5];
    for (int i = 0; i < 5; ++i) HIPX(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    res.t.check_ms += ms[0], res.t.coeffs_ms += ms[1], res.t.plan_ms += ms[2];
    res.t.acc_ms[0] += ms[3], res.t.acc_ms[1] += ms[4];
    ++res.t.chunks;
    if (hbad[0] || hbad[2]) {
      if (hbad[0]) res.first_bad_a = hbad[1];
      if (hbad[2]) res.first_bad_b = hbad[3];
      HIPX(hipStreamSynchronize(sup));  // an upload in flight reads the caller's buffers
      break;
    }
    const auto t0 = std::chrono::steady_clock::now();
    res.sum_a = host::jac_add(res.sum_a, msm_fold<HFq>(hwin, prm));
    res.sum_b = host::jac_add(res.sum_b, msm_fold<HFq>(hwin + ww, prm));
    if (on_hyperplane)
      for (size_t blk = 0; blk < (m_sum ? grid(m_sum) : 0); ++blk) {
        host::U256 v;
        for (int i = 0; i < 4; ++i) v.w[i] = (uint64_t)hpart[blk * 8 + 2 * i] | (uint64_t)hpart[blk * 8 + 2 * i + 1] << 32;
        power_sum = power_sum + host::Fr::from_std(v);
      }
    res.t.fold_ms += wall_ms(t0);
  }
  if (on_hyperplane && res.first_bad_a == RLC_NO_BAD && res.first_bad_b == RLC_NO_BAD) {
    // r'_(n-1) = -w sum_(j < n-1) r_j w^j: a full-width coefficient, two host scalar multiplications (both
    // points were checked with their chunk)
    const auto t0 = std::chrono::steady_clock::now();
    host::U256 wv;
    for (int i = 0; i < 4; ++i) wv.w[i] = (uint64_t)w_words[2 * i] | (uint64_t)w_words[2 * i + 1] << 32;
    const host::U256 r_last = (host::Fr::from_std(wv) * power_sum).neg().to_std();
    auto point = [&](const uint8_t* p) {
      bool inf = true;
      for (int i = 0; i < 64; ++i) inf &= p[i] == 0;
      if (inf) return host::Jac<HFq>::inf();
      return host::Jac<HFq>{HFq::raw(host::u256_from_le(p)), HFq::raw(host::u256_from_le(p + 32)), HFq::one()};
    };
    res.sum_a = host::jac_add(res.sum_a, host::jac_mul(point(a + (n - 1) * 64), r_last));
    res.sum_b = host::jac_add(res.sum_b, host::jac_mul(point(b + (n - 1) * 64), r_last));
    res.t.fold_ms += wall_ms(t0);
  }
  res.t.total_ms = wall_ms(t_begin);
  return res;
}

}  // namespace zkp
