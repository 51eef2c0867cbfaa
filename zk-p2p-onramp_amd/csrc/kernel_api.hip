// Kernel-level entry points behind the C ABI (zkp_msm_g1/g2, zkp_ntt_fr) and the device-resident
// kernel benchmarks (declared in prover.hpp).
#include <algorithm>
#include <cstring>

#include "device_pipeline.hpp"
#include "qap.hpp"

namespace zkp {

// ms on stream st (HIP events) of `iters` calls of fn, which enqueues there
template <class Fn>
static float time_on(hipStream_t st, int iters, Fn&& fn) {
  Event e0(true), e1(true);
  HIPX(hipEventRecord(e0, st));
  for (int i = 0; i < iters; ++i) fn();
  HIPX(hipEventRecord(e1, st));
  HIPX(hipEventSynchronize(e1));
  float ms = 0;
  HIPX(hipEventElapsedTime(&ms, e0, e1));
  return ms;
}

// One device-resident MSM set-up for the kernel-level entry points: base table from
// zkey-layout points (row 0 uploaded + converted, rows 1..T-1 derived), a plan and an engine.
struct MsmRig {
  Stream st;  // first: destroyed after the plan, the engine and the buffers
  MsmParams prm;
  std::unique_ptr<MsmBases> bases;
  std::unique_ptr<MsmPlan> plan;
  std::unique_ptr<MsmEngine> eng;
  DevBuf<> ds, dw;
  size_t n;
  Curve curve;
  const uint32_t* present = nullptr;  // the table's list of finite bases (null: all are, or ZKP_MSM sparse=0)
  size_t n_present = 0;
  float table_ms = 0;  // base-table build: row 0 upload + conversion + the derived rows (HIP events)
  MsmRig(int device, Curve cv, const uint8_t* points, const uint8_t* scalars, size_t n_, int c, int depth)
      : n(n_), curve(cv) {
    HIPX(hipSetDevice(device));
    st = Stream(hipStreamNonBlocking);
    // automatic window bits and plan: the prover's H-MSM choice (dense plan, c = lg n - 3 clamped to
    // [8, 20] and moved off a collapsed top window); measured on configs[1] (G1 2^20, uniform
    // scalars, 273c6e8:tools/gpu/experiments/r2_msm_c.sh): 1.84 ms against 2.06 ms for a compacted plan at
    // c = lg n - 4.  ZKP_MSM plan=compact selects the witness plan's variant (tests).
    const MsmOptions opt = msm_options();
    const int c_auto = opt.h ? opt.h : h_window_bits(n);
    prm = make_params(std::max<size_t>(n, 1), c ? c : c_auto, depth);
    apply_task_options(prm, opt.task_h, opt);  // the H plan's task size too (choose_msm_params)
    bases = std::make_unique<MsmBases>(curve, n, prm.c, prm.depth);
    table_ms = time_on(st, 1, [&] { fill_bases(*bases, points, n, 0, st); });
    if (opt.sparse) present = bases->present_index();
    n_present = present ? bases->present_count() : n;
    plan = std::make_unique<MsmPlan>(std::max<size_t>(n, 1), prm, st, n_present);
    plan->set_dense(opt.dense != 0);
    eng = std::make_unique<MsmEngine>(curve, prm, std::max<size_t>(n, 1), st);
    ds = DevBuf<>(std::max<size_t>(n * 8, 8));
    dw = DevBuf<>(eng->window_words());
    if (n) HIPX(hipMemcpyAsync(ds, scalars, n * 32, hipMemcpyHostToDevice, st));
  }
  void run() {
    plan->build(ds, n, present, n_present);
    eng->run(*plan, *bases, dw);
  }
  // fold the group sums and write the affine result (standard-form LE)
  void result(uint8_t* out, int* is_inf) {
    std::vector<uint32_t> hw(eng->window_words());
    HIPX(hipMemcpyAsync(hw.data(), dw, hw.size() * 4, hipMemcpyDeviceToHost, st));
    HIPX(hipStreamSynchronize(st));
    const bool finite = curve == Curve::G1 ? jac_to_bytes_g1(msm_fold<HFq>(hw.data(), prm), out)
                                           : jac_to_bytes_g2(msm_fold<HFq2>(hw.data(), prm), out);
    *is_inf = finite ? 0 : 1;
  }
};

void msm_points(int device, Curve curve, const uint8_t* points, const uint8_t* scalars, size_t n, uint8_t* out,
                int* is_inf, int c, int depth) {
  MsmRig rig(device, curve, points, scalars, n, c, depth);
  rig.run();
  rig.result(out, is_inf);
}

MsmBench bench_msm(int device, Curve curve, const uint8_t* points, const uint8_t* scalars, size_t n, int warmup,
                   int iters, uint8_t* out, int* is_inf) {
  if (n == 0 || iters <= 0) throw ZkpError(ZKP_ERR_INVALID_ARG, "bench_msm: n and iters must be > 0");
  MsmRig rig(device, curve, points, scalars, n, 0, 0);
  MsmBench r;
  for (int i = 0; i < warmup; ++i) rig.run();
  HIPX(hipStreamSynchronize(rig.st));
  // pass 1: whole-pipeline time (plan + engine), host-blocking once per MSM as in a proof
  r.ms_per_msm = time_on(rig.st, iters, [&] { rig.run(); }) / iters;
  // pass 2: per-launch events around the bucket-accumulate kernel
  rig.eng->set_instrument(true);
  MsmEngine::Stats s;
  for (int i = 0; i < std::min(iters, 8); ++i) rig.run();
  HIPX(hipStreamSynchronize(rig.st));
  rig.eng->collect(s);
  r.ms_accumulate = (float)(s.accumulate_ms / std::max<uint64_t>(1, s.launches));
  r.mixed_adds = s.mixed_adds / std::max<uint64_t>(1, s.launches);
  r.tasks = s.tasks / std::max<uint64_t>(1, s.launches);
  r.c = rig.prm.c;
  r.windows = rig.prm.windows;
  r.depth = rig.prm.depth;
  r.table_ms = rig.table_ms;
  if (out && is_inf) rig.result(out, is_inf);
  return r;
}

float bench_plan(int device, const uint8_t* scalars, size_t n, int c, int dense, int warmup, int iters) {
  if (n == 0 || iters <= 0) throw ZkpError(ZKP_ERR_INVALID_ARG, "bench_plan: n and iters must be > 0");
  HIPX(hipSetDevice(device));
  Stream st(hipStreamNonBlocking);
  const MsmParams prm = make_params(n, c, 0);
  MsmPlan plan(n, prm, st);
  plan.set_dense(dense != 0);
  DevBuf<> d(n * 8);
  HIPX(hipMemcpyAsync(d, scalars, n * 32, hipMemcpyHostToDevice, st));
  for (int i = 0; i < warmup; ++i) plan.build(d, n);
  HIPX(hipStreamSynchronize(st));
  return time_on(st, iters, [&] { plan.build(d, n); }) / iters;
}

float bench_ntt(int device, int log_n, int count, int warmup, int iters) {
  if (iters <= 0) throw ZkpError(ZKP_ERR_INVALID_ARG, "bench_ntt: iters must be > 0");
  if (count < 1 || count > 3) throw ZkpError(ZKP_ERR_INVALID_ARG, "bench_ntt: 1..3 vectors");
  if (log_n < 0 || log_n > 27) throw ZkpError(ZKP_ERR_INVALID_ARG, "bench_ntt: log_n out of range");
  HIPX(hipSetDevice(device));
  Stream st(hipStreamNonBlocking);
  const size_t n = size_t(1) << log_n;
  NttEngine eng(log_n, st);
  DevBuf<> d(n * 8 * count);
  std::vector<uint32_t> seed(n * 8);
  uint64_t x = 0x5A4B5032;
  for (auto& v : seed) {  // uniform-ish Fr-sized values
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    v = (uint32_t)(x >> 32);
  }
  for (size_t i = 0; i < n; ++i) seed[i * 8 + 7] &= 0x0fffffffu;
  uint32_t* vecs[3];
  for (int v = 0; v < count; ++v) {
    vecs[v] = d + (size_t)v * n * 8;
    HIPX(hipMemcpyAsync(vecs[v], seed.data(), n * 32, hipMemcpyHostToDevice, st));
  }
  HIPX(hipStreamSynchronize(st));  // seed is released at the end of the scope
  for (int i = 0; i < warmup; ++i) eng.coset_extend_batch(vecs, count);
  return time_on(st, iters, [&] { eng.coset_extend_batch(vecs, count); }) / iters;
}

void ntt_fr(int device, uint8_t* data, size_t n, int mode) {
  if (n == 0 || (n & (n - 1))) throw ZkpError(ZKP_ERR_INVALID_ARG, "NTT size must be a power of two");
  HIPX(hipSetDevice(device));
  Stream st(hipStreamNonBlocking);
  NttEngine eng(lg_ceil(n), st);
  DevBuf<> d(n * 8);
  HIPX(hipMemcpyAsync(d, data, n * 32, hipMemcpyHostToDevice, st));
  launch_fr_to_dev(d, n, st);
  if (mode == 0)
    eng.forward(d);
  else if (mode == 1)
    eng.inverse(d);
  else
    eng.coset_extend(d);
  launch_fr_from_dev(d, n, st);
  HIPX(hipMemcpyAsync(data, d, n * 32, hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
}

}  // namespace zkp
