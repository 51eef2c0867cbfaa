// Setup acceleration, phase 1 end: `snarkjs powersoftau prepare phase2 <pot_beacon.ptau>
// <pot_final.ptau>` (reference circuit/scripts/generate_keys_phase1.sh:20; the step
// circuit/scripts/generate_keys_phase2_groth16.sh:6-7 asks about) on the GPU: the Lagrange forms of the
// powers of tau, which `zkey new` (zkey_new.hip) reads as sections 12-15.
//
// For every level p = 0..power the first 2^p points of tauG1 (2), tauG2 (3), alphaTauG1 (4) and
// betaTauG1 (5) go through the group inverse FFT of gfft_kernels.hpp; the results are appended to
// lTauG1 (12), lTauG2 (13), lAlphaTauG1 (14), lBetaTauG1 (15), level p at point offset 2^p - 1.
// Output file: sections 1-7 copied byte for byte in that order (the header's ceremonyPower and the
// contributions included), then 12, 13, 14, 15.  Sections 12-15 of the input are ignored and rebuilt;
// any other section id of the input is not copied.  Layout: oracle/binfile.py write_ptau (restated,
// parity unpinned offline).
//
// Launches.  The three G1 vectors of a level share n, schedule and twiddles: every launch covers all
// three (grid y).  All levels of at most Geom::TILE points (512 G1, 256 G2: 64 KB of XYZZ in LDS) are
// ONE launch, a workgroup per (level, vector): load, all stages, affine, store.  A larger level is
// one launch of the first Geom::LG stages tile by tile in LDS, one launch per remaining stage in
// place over the XYZZ vector in HBM, and one launch to affine (one inversion per point: ~380 field
// products beside the ~5000 of each of the point's p / 2 scalar multiplications, so the Montgomery
// trick would save below 1 % of a level).  The LDS tiles are read with a 128- or 256-byte stride per
// thread (bank conflicts); a butterfly's loads and stores are 4 x 32 to 8 x 32 bytes beside those
// ~5000 products and do not show.
//
// Levels run from the top down: the download of level p (second stream, into its place in the output
// file) overlaps the computation of level p - 1, so only the smallest levels' copy is exposed.  The
// input sections are uploaded on the second stream while the point check of the previous one runs.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "gfft_kernels.hpp"
#include "hip_check.hpp"
#include "hip_raii.hpp"
#include "host_ec.hpp"
#include "prover.hpp"
#include "spans.hpp"
#include "zkey_verify.hpp"

namespace zkp {

namespace {

using gfft::Geom;

// window bits of gfft::scale: 2 measured 17 % (G1) and 18 % (G2) faster than 1 at power 20
// (profiles/ptau_prepare.json), G1 at one wave per SIMD instead of two
constexpr int DEFAULT_WINDOW_G1 = 2, DEFAULT_WINDOW_G2 = 2;

struct Vecs {
  const uint32_t* in[3];  // zkey-layout input points of each vector (its first 2^p are read)
  uint32_t* out[3];       // each vector's Lagrange section: level p at point 2^p - 1
};

// level < 0: the small levels, blockIdx.x = the level p <= LG, the whole transform and the affine
// results.  Otherwise tile blockIdx.x of level `level` > LG: stages 0..LG-1, XYZZ to work.
// blockIdx.y = the vector; work holds the vectors back to back.
template <class F, int WB>
__global__ __launch_bounds__(Geom<F>::TPB) void k_gfft_local(Vecs v, uint32_t* __restrict__ work,
                                                             const uint32_t* __restrict__ tw, int level,
                                                             bool fwd) {
  using G = Geom<F>;
  __shared__ __attribute__((aligned(16))) uint32_t lds[G::LDS_WORDS];
  const int vec = blockIdx.y;
  const bool small = level < 0;
  const int p = small ? (int)blockIdx.x : level;
  const size_t tile = small ? 0 : blockIdx.x;
  const int l = p < G::LG ? p : G::LG;
  const size_t cnt = (size_t)1 << l, n = (size_t)1 << p;
  for (size_t q = threadIdx.x; q < cnt; q += G::TPB)
    store_xyzz(lds, q, gfft::load_point<F>(v.in[vec], gfft::brev(tile * cnt + q, p)));
  __syncthreads();
  for (int s = 0; s < l; ++s) {
    if (threadIdx.x < cnt / 2) gfft::stage<F, WB>(lds, tw, p, s, threadIdx.x, fwd);
    __syncthreads();
  }
  for (size_t q = threadIdx.x; q < cnt; q += G::TPB) {
    const Xyzz<F> r = load_xyzz<F>(lds, q);
    if (small)
      gfft::finish<F>(r, tw, v.out[vec], (n - 1) + q);
    else
      store_xyzz(work, (size_t)vec * n + tile * cnt + q, r);
  }
}

// stage s >= LG of level p, in place: one butterfly per thread
template <class F, int WB>
__global__ __launch_bounds__(Geom<F>::TPB) void k_gfft_stage(uint32_t* __restrict__ work, const uint32_t* __restrict__ tw,
                                                             int p, int s, bool fwd) {
  const size_t n = (size_t)1 << p, i = (size_t)blockIdx.x * Geom<F>::TPB + threadIdx.x;
  if (i >= n / 2) return;
  gfft::stage<F, WB>(work + (size_t)blockIdx.y * n * 4 * Geom<F>::W, tw, p, s, i, fwd);
}

// the level's XYZZ results -> affine, zkey layout, at the level's place in each section
template <class F>
__global__ __launch_bounds__(Geom<F>::TPB) void k_gfft_affine(const uint32_t* __restrict__ work, Vecs v,
                                                              const uint32_t* __restrict__ tw, int p) {
  const size_t n = (size_t)1 << p, i = (size_t)blockIdx.x * Geom<F>::TPB + threadIdx.x;
  if (i >= n) return;
  gfft::finish<F>(load_xyzz<F>(work, (size_t)blockIdx.y * n + i), tw, v.out[blockIdx.y], (n - 1) + i);
}

thread_local PrepareTimings g_timings;

// words of XYZZ work space for nvec vectors of levels up to `power` (none if every level is small)
template <class F>
size_t work_words(int power, int nvec) {
  return power > Geom<F>::LG ? ((size_t)nvec << power) * 4 * Geom<F>::W : 0;
}

// Queues the transforms of levels power..0 of nvec vectors on st.  After the launches of a level (or of
// the small levels together) level_done(p_lo, p_hi) is called: the results of levels p_lo..p_hi are
// queued behind everything recorded on st so far.
template <class F, int WB, class Done>
void run_levels(const Vecs& v, int nvec, int power, uint32_t* work, const uint32_t* tw, hipStream_t st, Spans& sp,
                double* fft_ms, PrepareTimings& t, Done level_done) {
  using G = Geom<F>;
  for (int p = power; p > G::LG; --p) {
    const size_t n = (size_t)1 << p;
    sp.begin(st);
    hipLaunchKernelGGL((k_gfft_local<F, WB>), dim3((unsigned)(n >> G::LG), nvec), dim3(G::TPB), 0, st, v, work, tw, p, false);
    for (int s = G::LG; s < p; ++s)
      hipLaunchKernelGGL((k_gfft_stage<F, WB>), dim3((unsigned)(n / 2 / G::TPB), nvec), dim3(G::TPB), 0, st, work, tw, p, s, false);
    sp.end(st, fft_ms);
    sp.begin(st);
    hipLaunchKernelGGL(k_gfft_affine<F>, dim3((unsigned)(n / G::TPB), nvec), dim3(G::TPB), 0, st, work, v, tw, p);
    sp.end(st, &t.affine_ms);
    HIPX(hipGetLastError());
    t.launches += 2 + (p - G::LG);
    level_done(p, p);
  }
  const int top = std::min(power, G::LG);
  sp.begin(st);  // the small levels' affine conversion is inside their one launch
  hipLaunchKernelGGL((k_gfft_local<F, WB>), dim3(top + 1, nvec), dim3(G::TPB), 0, st, v, work, tw, -1, false);
  sp.end(st, fft_ms);
  HIPX(hipGetLastError());
  t.launches += 1;
  level_done(0, top);
}

// window bits of the scalar multiplications (gfft::scale): ZKP_GFFT_WINDOW=1|2 overrides the default
int window_bits(bool g2) {
  const char* e = std::getenv("ZKP_GFFT_WINDOW");
  if (e && *e) {
    if ((e[0] != '1' && e[0] != '2') || e[1])
      throw ZkpError(ZKP_ERR_INVALID_ARG, std::string("ZKP_GFFT_WINDOW: 1 or 2 (got '") + e + "')");
    return e[0] - '0';
  }
  return g2 ? DEFAULT_WINDOW_G2 : DEFAULT_WINDOW_G1;
}

DevBuf<> upload_table(hipStream_t st) {
  std::vector<uint32_t> h((size_t)gfft::TW_ENTRIES * 8);
  gfft::fill_table(h.data());
  DevBuf<> d(h.size());
  HIPX(hipMemcpyAsync(d, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));
  HIPX(hipStreamSynchronize(st));  // h goes away
  return d;
}

// refuses before any launch what does not fit in free HBM
void require_free(size_t bytes) {
  size_t free_b = 0, total_b = 0;
  HIPX(hipMemGetInfo(&free_b, &total_b));
  if (bytes > free_b)
    throw ZkpError(ZKP_ERR_OUT_OF_MEMORY, "group FFT: the working set of " + std::to_string(bytes >> 20) +
                                              " MiB does not fit in " + std::to_string(free_b >> 20) + " MiB of free HBM");
}

}  // namespace

PrepareTimings ptau_prepare_timings() { return g_timings; }

namespace {

// one transform of n = 2^log_n points, either direction; kernel_ms (if asked for): the launches' device time
void group_transform(int device, bool g2, const uint8_t* points, int log_n, uint8_t* out, bool fwd, double* kernel_ms) {
  if (log_n < 0 || log_n > gfft::MAX_LOG_N)
    throw ZkpError(ZKP_ERR_INVALID_ARG, std::string(fwd ? "group FFT" : "group iFFT") + ": log_n must be within 0..28");
  HIPX(hipSetDevice(device));
  const size_t n = (size_t)1 << log_n, pb = g2 ? 128 : 64;
  const size_t ww = g2 ? work_words<Fq2>(log_n, 1) : work_words<Fq>(log_n, 1);
  // the output section holds levels 0..log_n; only level log_n is returned
  const size_t out_pts = 2 * n - 1;
  require_free(n * pb + out_pts * pb + ww * 4 + (size_t(64) << 20));
  Stream st(hipStreamNonBlocking);
  const DevBuf<> tw = upload_table(st);
  DevBuf<> din(n * pb / 4), dout(out_pts * pb / 4), work(std::max<size_t>(ww, 1));
  HIPX(hipMemcpyAsync(din, points, n * pb, hipMemcpyHostToDevice, st));
  Vecs v{{din, nullptr, nullptr}, {dout, nullptr, nullptr}};
  // one level: the vector's top level alone (the levels below it read prefixes of the same input and are
  // not asked for), through the same kernels as ptau_prepare_phase2
  auto one = [&](auto f, auto wb) {
    using F = decltype(f);
    using G = Geom<F>;
    constexpr int WB = decltype(wb)::value;
    if (log_n > G::LG) {
      hipLaunchKernelGGL((k_gfft_local<F, WB>), dim3((unsigned)(n >> G::LG), 1), dim3(G::TPB), 0, st, v, work.get(), tw.get(), log_n, fwd);
      for (int s = G::LG; s < log_n; ++s)
        hipLaunchKernelGGL((k_gfft_stage<F, WB>), dim3((unsigned)(n / 2 / G::TPB), 1), dim3(G::TPB), 0, st, work.get(), tw.get(), log_n, s, fwd);
      hipLaunchKernelGGL(k_gfft_affine<F>, dim3((unsigned)(n / G::TPB), 1), dim3(G::TPB), 0, st, work.get(), v, tw.get(), log_n);
    } else {
      // the small launch computes levels 0..log_n of the vector's prefixes; level log_n is the answer
      hipLaunchKernelGGL((k_gfft_local<F, WB>), dim3(log_n + 1, 1), dim3(G::TPB), 0, st, v, work.get(), tw.get(), -1, fwd);
    }
    HIPX(hipGetLastError());
  };
  using W1 = std::integral_constant<int, 1>;
  using W2 = std::integral_constant<int, 2>;
  Event e0(true), e1(true);
  HIPX(hipEventRecord(e0, st));
  if (g2)
    window_bits(true) == 2 ? one(Fq2{}, W2{}) : one(Fq2{}, W1{});
  else
    window_bits(false) == 2 ? one(Fq{}, W2{}) : one(Fq{}, W1{});
  HIPX(hipEventRecord(e1, st));
  HIPX(hipMemcpyAsync(out, dout.get() + (n - 1) * pb / 4, n * pb, hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  if (kernel_ms) {
    float ms = 0;
    HIPX(hipEventElapsedTime(&ms, e0, e1));
    *kernel_ms = ms;
  }
}

}  // namespace

void group_ifft(int device, bool g2, const uint8_t* points, int log_n, uint8_t* out, double* kernel_ms) {
  group_transform(device, g2, points, log_n, out, false, kernel_ms);
}

void group_fft(int device, bool g2, const uint8_t* points, int log_n, uint8_t* out, double* kernel_ms) {
  group_transform(device, g2, points, log_n, out, true, kernel_ms);
}

std::vector<uint8_t> ptau_prepare_phase2(int device, const uint8_t* ptau, size_t len) {
  const auto t_begin = std::chrono::steady_clock::now();
  PrepareTimings t;
  // ---- parse
  BinFile bf = parse_binfile(ptau, len, "ptau", 1);
  for (int id = 1; id <= 7; ++id)
    if (!bf.sec[id].ptr) throw ZkpError(ZKP_ERR_FORMAT, "ptau: missing section " + std::to_string(id));
  if (bf.sec[1].len < 4 + 32 + 4) throw ZkpError(ZKP_ERR_FORMAT, "ptau: bad header");
  uint32_t n8, power;
  std::memcpy(&n8, bf.sec[1].ptr, 4);
  if (n8 != 32 || bf.sec[1].len < 4 + 32 + 4 + 4) throw ZkpError(ZKP_ERR_FORMAT, "ptau: bad header");
  if (std::memcmp(bf.sec[1].ptr + 4, host::FQ_DESC.mod.w, 32) != 0) throw ZkpError(ZKP_ERR_CURVE, "ptau: curve is not bn128");
  std::memcpy(&power, bf.sec[1].ptr + 36, 4);
  if (power > (uint32_t)gfft::MAX_LOG_N) throw ZkpError(ZKP_ERR_FORMAT, "ptau: power above 28");
  const size_t N = (size_t)1 << power, nlag = 2 * N - 1;
  const size_t want[8] = {0, 0, nlag * 64, N * 128, N * 64, N * 64, 128, 0};
  for (int id = 2; id <= 6; ++id)
    if (bf.sec[id].len != want[id])
      throw ZkpError(ZKP_ERR_FORMAT, "ptau: section " + std::to_string(id) + " has " + std::to_string(bf.sec[id].len) +
                                         " bytes, its power wants " + std::to_string(want[id]));
  // ---- the output file: sections 1-7 copied, 12-15 filled by the downloads
  const int out_ids[4] = {12, 13, 14, 15};
  size_t total = 12;
  for (int id = 1; id <= 7; ++id) total += 12 + bf.sec[id].len;
  for (int id : out_ids) total += 12 + nlag * (id == 13 ? 128 : 64);
  std::vector<uint8_t> out(total);
  uint8_t* lag[16] = {};
  {
    uint8_t* o = out.data();
    auto put32 = [&](uint32_t x) { std::memcpy(o, &x, 4), o += 4; };
    auto put64 = [&](uint64_t x) { std::memcpy(o, &x, 8), o += 8; };
    std::memcpy(o, "ptau", 4), o += 4;
    put32(1), put32(11);
    for (int id = 1; id <= 7; ++id) {
      put32((uint32_t)id), put64(bf.sec[id].len);
      std::memcpy(o, bf.sec[id].ptr, bf.sec[id].len), o += bf.sec[id].len;
    }
    for (int id : out_ids) {
      const size_t b = nlag * (id == 13 ? 128 : 64);
      put32((uint32_t)id), put64(b);
      lag[id] = o, o += b;
    }
  }
  t.parse_check_ms = wall_ms(t_begin);
  // ---- device: inputs, Lagrange sections, XYZZ work space (shared by the G1 and the G2 pass)
  HIPX(hipSetDevice(device));
  const size_t ww = std::max(work_words<Fq>((int)power, 3), work_words<Fq2>((int)power, 1));
  size_t need = ww * 4 + (size_t(64) << 20);
  for (int id = 2; id <= 5; ++id) need += bf.sec[id].len;
  for (int id : out_ids) need += nlag * (id == 13 ? 128 : 64);
  require_free(need);
  Stream st(hipStreamNonBlocking), sx(hipStreamNonBlocking);  // compute; transfers
  const DevBuf<> tw = upload_table(st);
  DevBuf<> din[6], dlag[16], work(std::max<size_t>(ww, 1));
  for (int id = 2; id <= 5; ++id) din[id] = DevBuf<>(bf.sec[id].len / 4);
  for (int id : out_ids) dlag[id] = DevBuf<>(nlag * (id == 13 ? 128 : 64) / 4);
  DevBuf<unsigned long long> dbad(8);
  Spans sp;
  // ---- upload (sx) and point check (st): section id + 1 uploads while section id is checked
  {
    Event up[6] = {Event(), Event(), Event(false), Event(false), Event(false), Event(false)};
    auto upload = [&](int id) {
      const auto t0 = std::chrono::steady_clock::now();
      HIPX(hipMemcpyAsync(din[id], bf.sec[id].ptr, bf.sec[id].len, hipMemcpyHostToDevice, sx));
      HIPX(hipEventRecord(up[id], sx));
      t.upload_ms += wall_ms(t0);
    };
    upload(2);
    for (int id = 2; id <= 5; ++id) {
      HIPX(hipStreamWaitEvent(st, up[id], 0));
      unsigned long long* bad = dbad.get() + 2 * (id - 2);
      points_bad_reset(bad, st);
      sp.begin(st);
      points_check_resident(id == 3, din[id], bf.sec[id].len / (id == 3 ? 128 : 64), 0, bad, st);
      sp.end(st, &t.parse_check_ms);
      if (id < 5) upload(id + 1);
    }
    unsigned long long hbad[8];
    HIPX(hipMemcpyAsync(hbad, dbad, sizeof hbad, hipMemcpyDeviceToHost, st));
    HIPX(hipStreamSynchronize(st));
    HIPX(hipStreamSynchronize(sx));  // no upload still reads the caller's buffer
    for (int id = 2; id <= 5; ++id)
      if (hbad[2 * (id - 2)])
        throw ZkpError(ZKP_ERR_FORMAT, "ptau: section " + std::to_string(id) + " point " +
                                           std::to_string(hbad[2 * (id - 2) + 1]) + " is not on the curve");
  }
  // ---- levels.  A level's download is issued after the next launches are queued, so the host waits in
  // the copy while the device computes.
  struct Copy {
    Event done;
    int id;
    size_t first, count;  // points of the section
  };
  std::vector<Copy> pending;
  auto flush = [&] {
    const auto t0 = std::chrono::steady_clock::now();
    for (Copy& c : pending) {
      const size_t pb = c.id == 13 ? 128 : 64;
      HIPX(hipStreamWaitEvent(sx, c.done, 0));
      HIPX(hipMemcpyAsync(lag[c.id] + c.first * pb, dlag[c.id].get() + c.first * pb / 4, c.count * pb, hipMemcpyDeviceToHost, sx));
    }
    HIPX(hipStreamSynchronize(sx));
    pending.clear();
    t.download_ms += wall_ms(t0);
  };
  auto pass = [&](std::vector<int> ids) {
    return [&, ids](int p_lo, int p_hi) {
      std::vector<Copy> mine;
      for (int id : ids) {
        mine.push_back(Copy{Event(false), id, ((size_t)1 << p_lo) - 1, ((size_t)2 << p_hi) - ((size_t)1 << p_lo)});
        HIPX(hipEventRecord(mine.back().done, st));
      }
      flush();  // the levels queued before this one
      for (Copy& c : mine) pending.push_back(std::move(c));
    };
  };
  const Vecs v1{{din[2], din[4], din[5]}, {dlag[12], dlag[14], dlag[15]}};
  const Vecs v2{{din[3], nullptr, nullptr}, {dlag[13], nullptr, nullptr}};
  if (window_bits(false) == 2)
    run_levels<Fq, 2>(v1, 3, (int)power, work, tw, st, sp, &t.g1_ms, t, pass({12, 14, 15}));
  else
    run_levels<Fq, 1>(v1, 3, (int)power, work, tw, st, sp, &t.g1_ms, t, pass({12, 14, 15}));
  if (window_bits(true) == 2)
    run_levels<Fq2, 2>(v2, 1, (int)power, work, tw, st, sp, &t.g2_ms, t, pass({13}));
  else
    run_levels<Fq2, 1>(v2, 1, (int)power, work, tw, st, sp, &t.g2_ms, t, pass({13}));
  flush();
  HIPX(hipStreamSynchronize(st));
  sp.collect();
  t.total_ms = wall_ms(t_begin);
  g_timings = t;
  return out;
}

}  // namespace zkp
