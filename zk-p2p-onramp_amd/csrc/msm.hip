// Pippenger MSM engine for BN254 G1/G2 on gfx950.  See msm.hpp for the pipeline.
#include "msm.hpp"

#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "curve.hpp"
#include "msm_kernels.hpp"
#include "hip_check.hpp"

namespace zkp {

namespace {

constexpr int TPB = 256;

inline unsigned grid_for(size_t n, int tpb = TPB) { return (unsigned)((n + tpb - 1) / tpb); }

__device__ __forceinline__ uint32_t lane_rank(uint64_t m) {  // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// row t of the base table from row t-1: 2^c * P, affine.  One launch per row keeps
// every launch short (~T-1 launches of n threads at zkey load).
template <class F>
__global__ __launch_bounds__(TPB) void k_extend_row(uint32_t* __restrict__ table, uint32_t n, int dbl, int t) {
  msmk::extend_row<F>(blockIdx.x * TPB + threadIdx.x, table, n, dbl, t);
}

// the mask of the finite bases of row 0 (BaseMask): thread i tests base i (PW words: all zero = the
// point at infinity, in the zkey's form and in the device's), a wave's ballot gives two mask words;
// count += the finite bases
template <int PW>
__global__ __launch_bounds__(TPB) void k_present(const uint32_t* __restrict__ row0, uint32_t n,
                                                 uint32_t* __restrict__ bits, uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * TPB + threadIdx.x;
  uint32_t any = 0;
  if (i < n) {
    const uint4* p = reinterpret_cast<const uint4*>(row0 + (size_t)i * PW);
#pragma unroll
    for (int q = 0; q < PW / 4; ++q) {
      const uint4 v = p[q];
      any |= v.x | v.y | v.z | v.w;
    }
  }
  const uint64_t m = __ballot(any != 0);
  const uint32_t lane = threadIdx.x & 63;
  if ((lane & 31) == 0 && i < n) bits[i >> 5] = (uint32_t)(m >> lane);
  if (lane == 0 && m) atomicAdd(count, (uint32_t)__popcll(m));
}
__global__ __launch_bounds__(TPB) void k_mask_or(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                 uint32_t nw, uint32_t* __restrict__ out,
                                                 uint32_t* __restrict__ count) {
  const uint32_t j = blockIdx.x * TPB + threadIdx.x;
  if (j >= nw) return;
  const uint32_t v = a[j] | b[j];
  out[j] = v;
  if (v) atomicAdd(count, (uint32_t)__popc(v));
}
// PlanMembership: memb[i] = bit p when plan p is used and scalar i is in its mask (no mask: every one);
// a wave's ballot gives two words of the mask of the scalars with any bit, count += those
struct MembBits {
  const uint32_t* bits[PlanMembership::NPLAN];
  uint32_t all;  // plans without a mask (every scalar belongs)
  uint32_t use;
};
__global__ __launch_bounds__(TPB) void k_membership(MembBits in, uint32_t n, uint8_t* __restrict__ memb,
                                                    uint32_t* __restrict__ any, uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * TPB + threadIdx.x;
  uint32_t tag = 0;
  if (i < n) {
#pragma unroll
    for (int p = 0; p < PlanMembership::NPLAN; ++p) {
      if (!(in.use >> p & 1)) continue;
      const uint32_t bit = (in.all >> p & 1) ? 1u : (in.bits[p][i >> 5] >> (i & 31)) & 1u;
      tag |= bit << p;
    }
    memb[i] = (uint8_t)tag;
  }
  const uint64_t m = __ballot(tag != 0);
  const uint32_t lane = threadIdx.x & 63;
  if ((lane & 31) == 0 && i < n) any[i >> 5] = (uint32_t)(m >> lane);
  if (lane == 0 && m) atomicAdd(count, (uint32_t)__popcll(m));
}

// G2 (Fq2) accumulation and bucket merges (the wide finish kernels): without a bound the
// compiler takes 256 VGPRs + AGPRs (one wave per SIMD, nothing to hide the mad-chain
// latency); two waves per SIMD (a few spilled dwords; accumulation measured 5.24 -> 4.55 ms
// per 6.4 M-point G2 MSM)
// (G1: no bound, 118 VGPRs and four waves per SIMD; 3 / 5 / 6 waves measured slower, profiles/acc_waves_r03.txt)
template <class F>
struct AccWaves {
  static constexpr int value = FWords<F>::W == 16 ? 2 : 1;
};
template <class F>
struct MergeWaves {
  static constexpr int value = FWords<F>::W == 16 ? 2 : 1;
};
template <class F>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(AccWaves<F>::value))) void k_accumulate(const uint32_t* __restrict__ points,
                                                    const uint32_t* __restrict__ vals,
                                                    const uint32_t* __restrict__ start,
                                                    const uint32_t* __restrict__ end,
                                                    const uint32_t* __restrict__ off, uint32_t nb, uint32_t S,
                                                    const uint32_t* __restrict__ perm, uint32_t* __restrict__ out) {
  msmk::accumulate<F>(blockIdx.x * TPB + threadIdx.x, points, vals, start, end, off, nb, S, perm, out);
}

// accumulate-task order by length, longest first (a counting sort over the S + 1 lengths): the
// lanes of a wave then run chains of equal length -- without it every bucket's short last task
// idles the lanes beside it (~7 % of the uniform-scalar H accumulation at S = 32)
__global__ __launch_bounds__(TPB) void k_tlen_count(const uint32_t* __restrict__ start, const uint32_t* __restrict__ end,
                                                    const uint32_t* __restrict__ off, uint32_t nb, uint32_t S,
                                                    uint32_t* __restrict__ hist) {
  extern __shared__ uint32_t h[];  // S + 1 counters
  for (uint32_t k = threadIdx.x; k <= S; k += TPB) h[k] = 0;
  __syncthreads();
  const uint32_t t = blockIdx.x * TPB + threadIdx.x;
  if (t < off[nb]) atomicAdd(&h[S - msmk::task_len(t, start, end, off, nb, S)], 1u);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k <= S; k += TPB) hist[(size_t)k * gridDim.x + blockIdx.x] = h[k];
}
__global__ __launch_bounds__(TPB) void k_tlen_scatter(const uint32_t* __restrict__ start,
                                                      const uint32_t* __restrict__ end,
                                                      const uint32_t* __restrict__ off, uint32_t nb, uint32_t S,
                                                      const uint32_t* __restrict__ hoff, uint32_t* __restrict__ perm) {
  extern __shared__ uint32_t cur[];  // S + 1 cursors
  for (uint32_t k = threadIdx.x; k <= S; k += TPB) cur[k] = hoff[(size_t)k * gridDim.x + blockIdx.x];
  __syncthreads();
  const uint32_t t = blockIdx.x * TPB + threadIdx.x;
  if (t < off[nb]) perm[atomicAdd(&cur[S - msmk::task_len(t, start, end, off, nb, S)], 1u)] = t;
}
template <class F>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(MergeWaves<F>::value))) void k_merge_heavy(const uint32_t* __restrict__ src,
                                                     const uint32_t* __restrict__ off,
                                                     const uint32_t* __restrict__ hoff, uint32_t nb, uint32_t S2,
                                                     int lvl, uint32_t* __restrict__ dst) {
  msmk::merge_heavy<F>(blockIdx.x * TPB + threadIdx.x, src, off, hoff, nb, S2, lvl, dst);
}
template <class F>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(MergeWaves<F>::value))) void k_merge_final(const uint32_t* __restrict__ part0,
                                                     const uint32_t* __restrict__ part1,
                                                     const uint32_t* __restrict__ off, uint32_t nb, uint32_t S2,
                                                     int levels, uint32_t* __restrict__ buckets) {
  msmk::merge_final<F>(blockIdx.x * TPB + threadIdx.x, part0, part1, off, nb, S2, levels, buckets);
}
template <class F>
__global__ __launch_bounds__(TPB) void k_rowcol_chain(const uint32_t* __restrict__ buckets, const msmk::RowCol rc,
                                                      uint32_t* __restrict__ part, uint32_t* __restrict__ sums) {
  msmk::rowcol_chain<F>(blockIdx.x * TPB + threadIdx.x, buckets, rc, part, sums);
}
template <class F>
__global__ __launch_bounds__(TPB) void k_rowcol_tree(const uint32_t* __restrict__ part, const msmk::RowCol rc,
                                                     uint32_t* __restrict__ sums) {
  msmk::rowcol_tree<F>(blockIdx.x * TPB + threadIdx.x, part, rc, sums);
}
template <class F>
__global__ __launch_bounds__(TPB) void k_reduce_segments(const uint32_t* __restrict__ buckets, uint32_t G,
                                                         uint32_t half, uint32_t M, uint32_t* __restrict__ s_out,
                                                         uint32_t* __restrict__ t_out) {
  msmk::reduce_segments<F>(blockIdx.x * TPB + threadIdx.x, buckets, G, half, M, s_out, t_out);
}
template <class F>
__global__ __launch_bounds__(TPB) void k_subset_first(const uint32_t* __restrict__ s_in,
                                                      const uint32_t* __restrict__ t_in, uint32_t G, uint32_t lgP,
                                                      uint32_t fan, uint32_t* __restrict__ out) {
  msmk::subset_first<F>(blockIdx.x * TPB + threadIdx.x, s_in, t_in, G, lgP, fan, out);
}
// (no waves-per-SIMD bound: a latency-bound tree, one wave per SIMD suffices; bounding the G2 variant
// to two waves spills ~290 dwords)
template <class F>
__global__ __launch_bounds__(msmk::TREE_TPB) void k_subset_tree_first(
    const uint32_t* __restrict__ s_in, const uint32_t* __restrict__ t_in, uint32_t lgP, uint32_t nch,
    uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[msmk::XyzzLimbs<F>::N * (msmk::TREE_TPB / 2)];
  msmk::subset_tree_first<F>(s_in, t_in, lgP, nch, blockIdx.y, blockIdx.x, lds, out);
}
template <class F>
__global__ __launch_bounds__(msmk::TREE_TPB) void k_subset_tree_next(
    const uint32_t* __restrict__ in, uint32_t n_in, uint32_t n_out, uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[msmk::XyzzLimbs<F>::N * (msmk::TREE_TPB / 2)];
  msmk::subset_tree_next<F>(in, n_in, n_out, blockIdx.y, blockIdx.x, lds, out);
}

// count (or, with rank != nullptr, claim a slot for) one entry in LDS counter h[b]; lanes of a
// wave that all hit the same counter (the skewed buckets of 0/1 witness values) use one atomic
__device__ __forceinline__ uint32_t lds_claim(uint32_t* h, uint32_t b, bool valid) {
  const uint64_t m = __ballot(valid);
  if (!m) return 0;
  const int leader = __builtin_ctzll(m);
  const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)b, leader);
  const uint64_t same = __ballot(valid && b == b0);
  if (same == m) {
    uint32_t base = 0;
    if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(&h[b0], (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
    return base + lane_rank(m);
  }
  return valid ? atomicAdd(&h[b], 1u) : 0u;
}

#include "hsort_kernels.hpp"

// heavy-merge grid bound per level: heavy c > S2  =>  ceil(c/S2) <= 2c/S2
inline size_t level_bound(size_t bound, int S2) { return 2 * bound / S2 + 1; }

template <class F>
void run_accumulate(const MsmPlan& plan, const MsmBases& bases, uint32_t* part_a, hipStream_t st, hipEvent_t ev0,
                    hipEvent_t ev1) {
  const MsmParams& prm = plan.params();
  const uint32_t nb = (uint32_t)prm.buckets();
  if (ev0) HIPX(hipEventRecord(ev0, st));
  if (plan.entries() > 0)
    hipLaunchKernelGGL(k_accumulate<F>, dim3(grid_for(plan.max_tasks_now())), dim3(TPB), 0, st, bases.data(),
                       plan.vals(), plan.bstart(), plan.bend(), plan.task_off(), nb, (uint32_t)prm.S, plan.perm(),
                       part_a);
  if (ev1) HIPX(hipEventRecord(ev1, st));
  HIPX(hipGetLastError());
}

// the first level's geometry for the engine's kernels
inline msmk::RowCol rowcol_for(const MsmParams& p) {
  return msmk::rowcol_make((uint32_t)p.groups, (uint32_t)p.U(), (uint32_t)p.V(), msmk::ROWCOL_CHAIN, msmk::ROWCOL_SPAN);
}

template <class F>
void run_finish(const MsmPlan& plan, uint32_t* part_a, uint32_t* part_b, uint32_t* buckets, uint32_t* rc_part,
                uint32_t* rc_sums, uint32_t* seg_s, uint32_t* seg_t, uint32_t* const sub[2], uint32_t* d_out,
                hipStream_t st) {
  const MsmParams& prm = plan.params();
  const uint32_t nb = (uint32_t)prm.buckets();
  const size_t xyzz_bytes = 16 * (size_t)FWords<F>::W;
  size_t bound = plan.max_tasks_now();
  for (int lv = 0; lv < plan.merge_levels() && plan.entries() > 0; ++lv) {
    bound = level_bound(bound, prm.S2);
    const uint32_t* src = (lv & 1) ? part_b : part_a;
    uint32_t* dst = (lv & 1) ? part_a : part_b;
    hipLaunchKernelGGL(k_merge_heavy<F>, dim3(grid_for(bound)), dim3(TPB), 0, st, src, plan.task_off(),
                       plan.level_off(lv), nb, (uint32_t)prm.S2, lv, dst);
  }
  hipLaunchKernelGGL(k_merge_final<F>, dim3(grid_for(nb)), dim3(TPB), 0, st, part_a, part_b, plan.task_off(), nb,
                     (uint32_t)prm.S2, plan.merge_levels(), buckets);
  // bucket reduction, first level: every group's row and column sums (chains, then a shuffle tree)
  const msmk::RowCol rc = rowcol_for(prm);
  hipLaunchKernelGGL(k_rowcol_chain<F>, dim3(grid_for((size_t)rc.row_parts() + rc.col_parts())), dim3(TPB), 0, st,
                     buckets, rc, rc_part, rc_sums);
  hipLaunchKernelGGL(k_rowcol_tree<F>, dim3(grid_for((size_t)rc.row_lanes() + rc.col_lanes())), dim3(TPB), 0, st,
                     rc_part, rc, rc_sums);
  // second level, over the G = 2 * groups sub-groups of V points: segments, then the K = lgP + 1 subset
  // sums per sub-group
  const uint32_t G = (uint32_t)prm.subgroups(), V = (uint32_t)prm.V();
  const uint32_t M = (uint32_t)prm.M, lgP = (uint32_t)prm.lgP(), K = (uint32_t)prm.K();
  hipLaunchKernelGGL(k_reduce_segments<F>, dim3(grid_for((size_t)G * (V / M))), dim3(TPB), 0, st, rc_sums, G, V, M,
                     seg_s, seg_t);
  // workgroup LDS trees: 2 * TREE_TPB values per workgroup and launch level
  int cur = 0;
  constexpr uint32_t CH = 2 * msmk::TREE_TPB;
  uint32_t n = ((1u << lgP) + CH - 1) / CH;
  if ((size_t)G * K * n <= msmk::TREE_FIRST_MAX) {  // about one round of workgroups: the tree from the inputs
    hipLaunchKernelGGL(k_subset_tree_first<F>, dim3(n, G * K), dim3(msmk::TREE_TPB), 0, st, seg_s, seg_t, lgP, n,
                       sub[0]);
  } else {  // many inputs: a full-lane fan-in chain level first (short: the trees above it take the
            // rest), then trees
    const uint32_t cf = msmk::TREE_CHAIN_FAN;
    n = (((1u << lgP) + 2 * cf - 1) / (2 * cf));
    hipLaunchKernelGGL(k_subset_first<F>, dim3(grid_for((size_t)G * K * n)), dim3(TPB), 0, st, seg_s, seg_t, G, lgP,
                       cf, sub[0]);
  }
  while (n > 1) {
    const uint32_t next = (n + CH - 1) / CH;
    hipLaunchKernelGGL(k_subset_tree_next<F>, dim3(next, G * K), dim3(msmk::TREE_TPB), 0, st, sub[cur], n, next,
                       sub[cur ^ 1]);
    cur ^= 1;
    n = next;
  }
  HIPX(hipGetLastError());
  HIPX(hipMemcpyAsync(d_out, sub[cur], (size_t)G * K * xyzz_bytes, hipMemcpyDeviceToDevice, st));
}

}  // namespace

// ------------------------------------------------------------------ MsmBases

MsmBases::MsmBases(Curve curve, size_t n, int c, int depth) : curve_(curve), n_(n), c_(c), depth_(depth) {
  if (depth < 1 || c < 2) throw std::runtime_error("MsmBases: bad parameters");
  if ((size_t)depth * std::max<size_t>(n, 1) >= (size_t(1) << 31))
    throw std::runtime_error("MsmBases: depth * n must stay below 2^31 (31-bit base indices)");
  bytes_ = bytes_for(curve, n, depth);
  d_ = DevBuf<>(bytes_ / 4);
}

MsmBases::MsmBases(Curve curve, const uint32_t* points, size_t n, int c)
    : curve_(curve), n_(n), c_(c), depth_(1), view_(points) {
  if (c < 2 || !points) throw std::runtime_error("MsmBases: bad parameters");
  if (std::max<size_t>(n, 1) >= (size_t(1) << 31))
    throw std::runtime_error("MsmBases: depth * n must stay below 2^31 (31-bit base indices)");
}

namespace {

// the count of a mask just enqueued on st comes to the host; a mask with every bit set is dropped,
// any other gets its index list (built on the host: once per table, at load)
void settle_mask(BaseMask& m, const uint32_t* d_count, size_t n, hipStream_t st) {
  uint32_t cnt = 0;
  HIPX(hipGetLastError());
  HIPX(hipMemcpyAsync(&cnt, d_count, 4, hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  m.count = cnt;
  if (cnt == n) {
    m.bits.reset();
    return;
  }
  if (cnt == 0) {  // nothing to list: a plan still sees a mask, of no scalars
    m.index = DevBuf<>(1);
    return;
  }
  std::vector<uint32_t> bits((n + 31) / 32), idx;
  HIPX(hipMemcpy(bits.data(), m.bits, bits.size() * 4, hipMemcpyDeviceToHost));
  idx.reserve(cnt);
  for (size_t w = 0; w < bits.size(); ++w)
    for (uint32_t v = bits[w]; v; v &= v - 1) idx.push_back((uint32_t)(w * 32 + __builtin_ctz(v)));
  if (idx.size() != cnt) throw std::runtime_error("MSM: mask and its count disagree");
  m.index = DevBuf<>(cnt);
  HIPX(hipMemcpy(m.index, idx.data(), (size_t)cnt * 4, hipMemcpyHostToDevice));
}

}  // namespace

void MsmBases::extend(hipStream_t st) {
  if (view_) throw std::runtime_error("MsmBases: a view has no rows to derive");
  mask_ = BaseMask{};
  if (n_ == 0) return;
  mask_.bits = DevBuf<>((n_ + 31) / 32);
  DevBuf<> cnt(1);
  HIPX(hipMemsetAsync(cnt, 0, 4, st));
  if (curve_ == Curve::G1)
    hipLaunchKernelGGL(k_present<16>, dim3(grid_for(n_)), dim3(TPB), 0, st, d_, (uint32_t)n_, mask_.bits, cnt);
  else
    hipLaunchKernelGGL(k_present<32>, dim3(grid_for(n_)), dim3(TPB), 0, st, d_, (uint32_t)n_, mask_.bits, cnt);
  for (int t = 1; t < depth_; ++t) {
    if (curve_ == Curve::G1)
      hipLaunchKernelGGL(k_extend_row<Fq>, dim3(grid_for(n_)), dim3(TPB), 0, st, d_, (uint32_t)n_, c_, t);
    else
      hipLaunchKernelGGL(k_extend_row<Fq2>, dim3(grid_for(n_)), dim3(TPB), 0, st, d_, (uint32_t)n_, c_, t);
  }
  settle_mask(mask_, cnt, n_, st);
}

BaseMask mask_union(const MsmBases& a, const MsmBases& b, hipStream_t st) {
  if (a.n() != b.n()) throw std::runtime_error("MSM: mask union of tables of different sizes");
  BaseMask m;
  m.count = a.n();
  if (!a.present() || !b.present()) return m;
  const size_t nw = (a.n() + 31) / 32;
  m.bits = DevBuf<>(nw);
  DevBuf<> cnt(1);
  HIPX(hipMemsetAsync(cnt, 0, 4, st));
  hipLaunchKernelGGL(k_mask_or, dim3(grid_for(nw)), dim3(TPB), 0, st, a.present(), b.present(), (uint32_t)nw,
                     m.bits, cnt);
  settle_mask(m, cnt, a.n(), st);
  return m;
}

PlanMembership plan_membership(const uint32_t* const bits[PlanMembership::NPLAN],
                               const size_t count[PlanMembership::NPLAN], const bool use[PlanMembership::NPLAN],
                               size_t n, hipStream_t st) {
  PlanMembership r;
  r.any.count = n;
  MembBits in{};
  for (int p = 0; p < PlanMembership::NPLAN; ++p) {
    if (!use[p]) continue;
    in.use |= 1u << p;
    in.bits[p] = bits[p];
    if (!bits[p]) in.all |= 1u << p;
    r.count[p] = bits[p] ? count[p] : n;
  }
  if (n == 0) {
    r.any.count = 0;
    return r;
  }
  r.memb = DevBuf<uint8_t>(n);
  r.any.bits = DevBuf<>((n + 31) / 32);
  DevBuf<> cnt(1);
  HIPX(hipMemsetAsync(cnt, 0, 4, st));
  hipLaunchKernelGGL(k_membership, dim3(grid_for(n)), dim3(TPB), 0, st, in, (uint32_t)n, r.memb, r.any.bits, cnt);
  settle_mask(r.any, cnt, n, st);
  return r;
}

// ------------------------------------------------------------------ MsmPlan

MsmSortScratch::MsmSortScratch(size_t max_n_, size_t max_present, const MsmParams& prm_, int nplans_)
    : prm(prm_), nplans(nplans_), max_n(std::max<size_t>(max_n_, 1)) {
  if (nplans < 1 || nplans > PlanMembership::NPLAN) throw std::invalid_argument("MSM: plans of a shared build");
  if (prm.c < MsmParams::MIN_C || prm.c > MsmParams::MAX_C || prm.windows > HS_STAGE / HS_TPB)
    throw std::invalid_argument("MSM: window bits outside the plan's range");
  if (max_n * prm.depth >= (size_t(1) << 31)) throw std::runtime_error("MSM size too large for 31-bit base indices");
  nbuckets = prm.buckets();
  max_entries = prm.max_entries(max_n, max_present);
  if (max_entries >= 0xffffffffull) throw std::runtime_error("MSM size too large for 32-bit entry indices");
  max_tasks = prm.max_tasks(max_entries);
  merge_levels = msm_merge_levels(max_n, prm);
  cnt = DevBuf<>(nbuckets + 1);
  const size_t ntl = (size_t)(prm.S + 1) * grid_for(max_tasks);
  tl_hist = DevBuf<>(ntl);
  tl_off = DevBuf<>(ntl);
  if (merge_levels > 0) lvl_tsum = DevBuf<>((size_t)merge_levels * scan_tiles_for(nbuckets + 1));
  // bucket-key bits kb = b1 (bin) + b2 (sub-bin) + b3 (bucket in sub-bin): b3 = 5 for the one-
  // workgroup-per-sub-bin pass C (k_hs_fine), up to 9 (tiled pass C) when kb > 23 (c > 20 with
  // several bucket groups); b1, b2 <= 9
  int kb = 1;
  while ((size_t(1) << kb) < nbuckets) ++kb;
  b3 = std::max(std::min(kb, HS_B3), kb - HS_MAX_B1 - HS_MAX_B2);
  b2 = (kb - b3) / 2;
  const int b1 = kb - b3 - b2;
  if (b1 > HS_MAX_B1 || b2 > HS_MAX_B2 || b3 > HS_MAX_B2)
    throw std::invalid_argument("MSM: too many buckets for the bucket sort (window bits x bucket groups)");
  nbins = (uint32_t)((nbuckets + (size_t(1) << (b2 + b3)) - 1) >> (b2 + b3));
  k = std::max(1, std::min(4, HS_STAGE / (HS_TPB * prm.windows)));
  if (k == 3) k = 2;
  const uint32_t nblk = (uint32_t)((max_n + k * HS_TPB - 1) / (k * HS_TPB));
  const size_t nh3 = (tiles3(max_entries) << b3) + 1;
  toff3 = DevBuf<>((size_t)nq() + 1);
  // a shared build keeps HS_NPLAN count arrays, stride3 apart, whether or not every plan is there
  stride3 = nh3;
  const size_t nh3_all = nplans > 1 ? nh3 * HS_NPLAN : nh3;
  if (nh3_all >= 0xffffffffull) throw std::runtime_error("MSM size too large for the sort's scans");
  hist3 = DevBuf<>(nh3_all);
  off3 = DevBuf<>(nh3_all);
  if (nplans > 1) binbase = DevBuf<>(nbins + 1);
  const size_t nh = (size_t)nbins * nblk, nh2 = tiles2(max_entries) << b2;
  hist = DevBuf<>(nh);
  blkoff = DevBuf<>(nh);
  toff = DevBuf<>(nbins + 1);
  hist2 = DevBuf<>(nh2);
  off2 = DevBuf<>(nh2);
  subbase = DevBuf<>((size_t)nq() + 1);
  ent_a = DevBuf<uint2>(max_entries);
  ent_b = DevBuf<uint2>(max_entries);
  const size_t scan_n = std::max(std::max(std::max(nbuckets + 1, nh3_all), std::max(nh2, ntl)), nh);
  tsum = DevBuf<>(scan_tiles_for(scan_n) + 1);
}

size_t MsmSortScratch::tiles2(size_t total) const { return (total + HS_TILE - 1) / HS_TILE + nbins; }
size_t MsmSortScratch::tiles3(size_t total) const { return (total + HS_TILE - 1) / HS_TILE + nq(); }

MsmPlan::MsmPlan(size_t max_n, const MsmParams& prm, hipStream_t stream, size_t max_present,
                 std::shared_ptr<MsmSortScratch> scratch)
    : prm_(prm), max_n_(std::max<size_t>(max_n, 1)), stream_(stream), sc_(std::move(scratch)) {
  if (!sc_) sc_ = std::make_shared<MsmSortScratch>(max_n_, max_present, prm_);
  nbuckets_ = prm_.buckets();
  max_entries_ = prm_.max_entries(max_n_, max_present);
  const MsmParams& q = sc_->prm;
  if (q.c != prm_.c || q.windows != prm_.windows || q.depth != prm_.depth || q.S != prm_.S || sc_->max_n < max_n_ ||
      sc_->max_entries < max_entries_)
    throw std::runtime_error("MSM: sort scratch built for other parameters or fewer entries");
  max_tasks_ = prm_.max_tasks(max_entries_);
  merge_levels_ = sc_->merge_levels;
  vals_sorted_ = DevBuf<>(max_entries_);
  bstart_ = DevBuf<>(nbuckets_ + 1);
  bend_ = DevBuf<>(nbuckets_ + 1);
  off_task_ = DevBuf<>(nbuckets_ + 1);
  perm_ = DevBuf<>(max_tasks_);
  if (merge_levels_ > 0) lvl_all_ = DevBuf<>((size_t)merge_levels_ * (nbuckets_ + 1));
  hs_binbase_ = DevBuf<>(sc_->nbins + 1);
  ready_ = Event(false);
}

namespace {

// pass A's kernels for K scalars per thread, with (MASK) or without an index list of the scalars to
// visit; TAG: every entry carries the plans it belongs to (a shared build)
template <bool MASK>
auto hs_count1_for(int k) {
  return k == 4 ? k_hs_count1<4, MASK> : (k == 2 ? k_hs_count1<2, MASK> : k_hs_count1<1, MASK>);
}
template <bool MASK, bool TAG>
auto hs_scatter1_for(int k) {
  return k == 4 ? k_hs_scatter1<4, MASK, TAG> : (k == 2 ? k_hs_scatter1<2, MASK, TAG> : k_hs_scatter1<1, MASK, TAG>);
}

// Passes A and B of the three-pass LDS-staged bucket sort (hsort_kernels.hpp), enqueued on st.  Pass A
// visits the m scalars that `index` lists (null: all n, m = n) and drops their zero digits; memb (a
// shared build's membership table, null for one plan) tags every entry with its plans; skew takes the
// wave-aggregated LDS claims of pass B (whole waves of one sub-bin: the 0/1-heavy witness).  Leaves
// the entries by sub-bin in sc.ent_b, the sub-bins' bases in sc.subbase and the bins' in binbase
// (nbins + 1 words, the last one the entry count).
void sort_passes_ab(MsmSortScratch& sc, const uint32_t* scalars, size_t n, const uint32_t* index, size_t m,
                    const uint8_t* memb, bool skew, uint32_t* binbase, hipStream_t st) {
  const MsmParams& prm = sc.prm;
  const int W = prm.windows, k = sc.k, b3 = sc.b3, sh1 = sc.b2 + b3;
  const uint32_t nbins = sc.nbins, nsub = 1u << sc.b2;
  const uint32_t nblk = (uint32_t)((m + k * HS_TPB - 1) / (k * HS_TPB));
  uint2* ea = sc.ent_a;
  // A: digits -> bins
  auto count1 = index ? hs_count1_for<true>(k) : hs_count1_for<false>(k);
  hipLaunchKernelGGL(count1, dim3(nblk), dim3(HS_TPB), 0, st, scalars, (uint32_t)n, index, (uint32_t)m, prm.c, W,
                     prm.depth, sh1, nbins, sc.hist);
  scan_nolookback(sc.hist, sc.blkoff, (size_t)nbins * nblk, sc.tsum, st);
  hipLaunchKernelGGL(k_hs_binbase, dim3(1), dim3(512), 0, st, sc.blkoff, sc.hist, nbins, nblk, binbase, sc.toff);
  auto scatter1 = memb ? (index ? hs_scatter1_for<true, true>(k) : hs_scatter1_for<false, true>(k))
                       : (index ? hs_scatter1_for<true, false>(k) : hs_scatter1_for<false, false>(k));
  const size_t lds1 = (size_t)k * HS_TPB * W * 8 + (size_t)nbins * 8;
  hipLaunchKernelGGL(scatter1, dim3(nblk), dim3(HS_TPB), lds1, st, scalars, (uint32_t)n, index, (uint32_t)m, prm.c, W,
                     prm.depth, sh1, nbins, sc.blkoff, ea, memb);
  // B: bins -> sub-bins (tiles past the used ones exit; their counters stay zero)
  const size_t tiles = sc.tiles2((uint32_t)(m * W)), nh2 = tiles << sc.b2;
  HIPX(hipMemsetAsync(sc.hist2, 0, nh2 * 4, st));
  hipLaunchKernelGGL((skew ? k_hs_count2<true> : k_hs_count2<false>), dim3((unsigned)tiles), dim3(HS_TPB), 0, st, ea,
                     binbase, sc.toff, nbins, b3, nsub, sc.hist2);
  scan_nolookback(sc.hist2, sc.off2, nh2, sc.tsum, st);
  hipLaunchKernelGGL(k_hs_subbase, dim3(grid_for(sc.nq() + 1)), dim3(HS_TPB), 0, st, sc.off2, binbase, sc.toff, nbins,
                     nsub, sc.subbase);
  hipLaunchKernelGGL((skew ? k_hs_scatter2<true, false> : k_hs_scatter2<false, false>), dim3((unsigned)tiles),
                     dim3(HS_TPB), 0, st, ea, binbase, sc.toff, nbins, b3, nsub, sc.off2, sc.ent_b.get(), nullptr);
}

// the opening of the tiled pass C (pass B one level down: no workgroup takes more than HS_TILE
// entries): the sub-bins' tile offsets and `words` zeroed counters for the sc.tiles3() tiles
void open_tiled_pass_c(MsmSortScratch& sc, size_t words, hipStream_t st) {
  hipLaunchKernelGGL(k_hs_subtiles, dim3(1), dim3(SC_TPB), 0, st, sc.subbase, sc.nq(), sc.toff3);
  HIPX(hipMemsetAsync(sc.hist3, 0, words * 4, st));
}

}  // namespace

void MsmPlan::build(const uint32_t* scalars, size_t n, const uint32_t* present, size_t n_present) {
  if (n > max_n_) throw std::runtime_error("MSM: n exceeds plan capacity");
  if (!present) n_present = n;
  if (n_present > n) throw std::runtime_error("MSM: more finite bases than scalars");
  if (n_present * prm_.windows > max_entries_) throw std::runtime_error("MSM: finite bases exceed plan capacity");
  n_ = n;
  MsmSortScratch& sc = *sc_;
  const uint32_t nb = (uint32_t)nbuckets_, nq = sc.nq();
  const int b3 = sc.b3;
  hipStream_t st = stream_;
  // total_ = n * W (with a mask: its count * W) bounds the nonzero digits (the accumulate grid: threads
  // past the last task exit), so nothing waits on the host; the exact count stays on the device
  // (entries_dev)
  total_ = (uint32_t)(n_present * prm_.windows);
  hs_built_ = false;
  if (total_ != 0) {
    // zero digits and the scalars whose base is at infinity are dropped in pass A (it visits only the
    // mask's index list).  Dense plans (uniform scalars: the H MSM) group their sub-bins with one
    // workgroup each (k_hs_fine); compacted plans (the witness: whole waves of one bin / sub-bin /
    // bucket) take the wave-aggregated LDS claims and the tiled pass C, as do keys with more than 5
    // bucket bits per sub-bin
    sort_passes_ab(sc, scalars, n, present, n_present, nullptr, !dense_, hs_binbase_, st);
    const uint2* eb = sc.ent_b;
    // C: sub-bins -> buckets, bounds and task counts
    if (dense_ && b3 <= HS_B3) {
      hipLaunchKernelGGL(k_hs_fine, dim3(nq), dim3(HS_FINE_TPB), 0, st, eb, sc.subbase, nq, b3, nb, (uint32_t)prm_.S,
                         vals_sorted_, bstart_, bend_, sc.cnt);
    } else {
      const uint32_t nf = 1u << b3;
      const size_t tiles3 = sc.tiles3(total_), nh3 = tiles3 << b3;
      open_tiled_pass_c(sc, nh3, st);
      hipLaunchKernelGGL(k_hs_count2<true>, dim3((unsigned)tiles3), dim3(HS_TPB), 0, st, eb, sc.subbase, sc.toff3, nq,
                         0, nf, sc.hist3);
      scan_nolookback(sc.hist3, sc.off3, nh3, sc.tsum, st);
      hipLaunchKernelGGL((k_hs_scatter2<true, true>), dim3((unsigned)tiles3), dim3(HS_TPB), 0, st, eb, sc.subbase,
                         sc.toff3, nq, 0, nf, sc.off3, nullptr, vals_sorted_);
      hipLaunchKernelGGL(k_hs_bounds3, dim3(grid_for((size_t)nb + 1)), dim3(HS_TPB), 0, st, sc.toff3, sc.off3,
                         sc.subbase, b3, nb, (uint32_t)prm_.S, bstart_, bend_, sc.cnt);
    }
    hs_built_ = true;
  }
  build_tail(total_ == 0);
}

void MsmPlan::build_tail(bool empty) {
  MsmSortScratch& sc = *sc_;
  hipStream_t st = stream_;
  const uint32_t nb = (uint32_t)nbuckets_;
  if (empty) {
    HIPX(hipMemsetAsync(bstart_, 0, (nbuckets_ + 1) * 4, st));
    HIPX(hipMemsetAsync(bend_, 0, (nbuckets_ + 1) * 4, st));
    HIPX(hipMemsetAsync(sc.cnt, 0, (nbuckets_ + 1) * 4, st));
  }
  // accumulate-task offsets and the heavy-bucket merge levels' offsets (look-back-free scans: they
  // run beside the accumulations of the other streams)
  scan_nolookback(sc.cnt, off_task_, nbuckets_ + 1, sc.tsum, st);
  max_tasks_now_ = prm_.max_tasks(total_);
  if (total_ > 0) {
    // accumulate-task order by length, longest first
    const unsigned nblk = grid_for(max_tasks_now_);
    const size_t lds = (size_t)(prm_.S + 1) * 4, nh = (size_t)(prm_.S + 1) * nblk;
    hipLaunchKernelGGL(k_tlen_count, dim3(nblk), dim3(TPB), lds, st, bstart_, bend_, off_task_, nb, (uint32_t)prm_.S,
                       sc.tl_hist);
    scan_nolookback(sc.tl_hist, sc.tl_off, nh, sc.tsum, st);
    hipLaunchKernelGGL(k_tlen_scatter, dim3(nblk), dim3(TPB), lds, st, bstart_, bend_, off_task_, nb,
                       (uint32_t)prm_.S, sc.tl_off, perm_);
  }
  if (merge_levels_ > 0 && total_ > 0) {
    const uint32_t nt = (uint32_t)scan_tiles_for(nbuckets_ + 1);
    hipLaunchKernelGGL(k_lvl_tiles, dim3(nt), dim3(SC_TPB), 0, st, off_task_, nb, (uint32_t)prm_.S2, merge_levels_,
                       nt, sc.lvl_tsum);
    hipLaunchKernelGGL(k_lvl_top, dim3(merge_levels_), dim3(SC_TPB), 0, st, sc.lvl_tsum, nt);
    hipLaunchKernelGGL(k_lvl_apply, dim3(nt), dim3(SC_TPB), 0, st, off_task_, nb, (uint32_t)prm_.S2, merge_levels_,
                       nt, sc.lvl_tsum, lvl_all_);
  }
  HIPX(hipGetLastError());
  HIPX(hipEventRecord(ready_, st));
}

void MsmPlan::build_shared(MsmPlan* const plans[PlanMembership::NPLAN], const uint32_t* scalars, size_t n,
                           const PlanMembership& mem) {
  static_assert(PlanMembership::NPLAN == HS_NPLAN, "the tag bits of the sort's entries");
  MsmPlan* first = nullptr;
  uint32_t pmask = 0;
  for (int p = 0; p < HS_NPLAN; ++p) {
    MsmPlan* pl = plans[p];
    if (!pl) continue;
    if (!first) first = pl;
    if (pl->sc_ != first->sc_ || pl->stream_ != first->stream_ || pl->dense_)
      throw std::runtime_error("MSM: a shared build takes compacted plans of one scratch and one stream");
    if (n > pl->max_n_) throw std::runtime_error("MSM: n exceeds plan capacity");
    if (mem.count[p] > n || mem.count[p] * pl->prm_.windows > pl->max_entries_)
      throw std::runtime_error("MSM: finite bases exceed plan capacity");
    pl->n_ = n;
    pl->total_ = (uint32_t)(mem.count[p] * pl->prm_.windows);
    pl->hs_built_ = false;
    if (pl->total_) pmask |= 1u << p;
  }
  if (!first) return;
  MsmSortScratch& sc = *first->sc_;
  const MsmParams& prm = first->prm_;
  const uint32_t* index = mem.any.list();
  const size_t n_any = mem.any.bits ? mem.any.count : n;
  if (sc.nplans < 2 || n_any > n || n_any * prm.windows > sc.max_entries)
    throw std::runtime_error("MSM: sort scratch not built for this shared build");
  hipStream_t st = first->stream_;
  if (pmask) {
    // passes A and B as in build(), over the union of the plans' scalars and with the plans' tag in
    // every entry; pass C (tiled) per plan
    sort_passes_ab(sc, scalars, n, index, n_any, mem.memb.get(), true, sc.binbase, st);
    const uint32_t nb = (uint32_t)first->nbuckets_, nq = sc.nq(), nbins = sc.nbins;
    const int b3 = sc.b3;
    const uint32_t nf = 1u << b3;
    const uint2* eb = sc.ent_b;
    // every plan's array: its tiles' counts and one word more (k_hs_count3), all scanned as one
    const size_t tiles3 = sc.tiles3((uint32_t)(n_any * prm.windows)), stride = (tiles3 << b3) + 1;
    if (stride > sc.stride3) throw std::runtime_error("MSM: sort scratch too small for this shared build");
    open_tiled_pass_c(sc, stride * HS_NPLAN, st);
    hipLaunchKernelGGL(k_hs_count3, dim3((unsigned)tiles3), dim3(HS_TPB), 0, st, eb, sc.subbase, sc.toff3, nq, nf, pmask,
                       stride, sc.hist3);
    scan_nolookback(sc.hist3, sc.off3, stride * HS_NPLAN, sc.tsum, st);
    HsPlanOut out{};
    for (int p = 0; p < HS_NPLAN; ++p)
      if (pmask >> p & 1) out.v[p] = plans[p]->vals_sorted_;
    hipLaunchKernelGGL(k_hs_scatter3, dim3((unsigned)tiles3), dim3(HS_TPB), 0, st, eb, sc.subbase, sc.toff3, nq, nf, pmask,
                       stride, sc.off3, out);
    for (int p = 0; p < HS_NPLAN; ++p) {
      if (!(pmask >> p & 1)) continue;
      MsmPlan& pl = *plans[p];
      hipLaunchKernelGGL(k_hs_bounds3p, dim3(grid_for((size_t)nb + 1)), dim3(HS_TPB), 0, st, sc.toff3,
                         sc.off3 + p * stride, nq, b3, nb, (uint32_t)prm.S, pl.bstart_, pl.bend_, sc.cnt,
                         pl.hs_binbase_ + nbins);
      pl.hs_built_ = true;
      pl.build_tail(false);
    }
  }
  for (int p = 0; p < HS_NPLAN; ++p)
    if (plans[p] && !(pmask >> p & 1)) plans[p]->build_tail(true);
}

// ------------------------------------------------------------------ MsmEngine

MsmEngine::MsmEngine(Curve curve, const MsmParams& prm, size_t max_n, hipStream_t stream)
    : curve_(curve), prm_(prm), max_n_(std::max<size_t>(max_n, 1)), stream_(stream) {
  fwords_ = curve_fwords(curve);
  nbuckets_ = prm_.buckets();
  max_tasks_ = prm_.max_tasks(max_n_ * prm_.windows);
  const size_t xyzz_words = 4 * (size_t)fwords_;
  part_a_ = DevBuf<>(max_tasks_ * xyzz_words);
  part_b_ = DevBuf<>(max_tasks_ * xyzz_words);
  buckets_ = DevBuf<>(nbuckets_ * xyzz_words);
  const msmk::RowCol rc = rowcol_for(prm_);
  rc_part_ = DevBuf<>(((size_t)rc.row_parts() + rc.col_parts()) * xyzz_words);
  rc_ = DevBuf<>((size_t)prm_.subgroups() * prm_.V() * xyzz_words);
  const size_t P = (size_t)prm_.V() / prm_.M, nseg = (size_t)prm_.subgroups() * P;
  seg_s_ = DevBuf<>(nseg * xyzz_words);
  seg_t_ = DevBuf<>(nseg * xyzz_words);
  const size_t n1 = prm_.out_points() * std::max((P + 2 * msmk::TREE_CHAIN_FAN - 1) / (2 * msmk::TREE_CHAIN_FAN),
                                                 (P + 2 * msmk::TREE_TPB - 1) / (2 * msmk::TREE_TPB));
  for (int i = 0; i < 2; ++i) sub_[i] = DevBuf<>(n1 * xyzz_words);
  for (auto& e : ev_) e[0] = Event(true), e[1] = Event(true);
  h_counts_ = PinnedBuf<uint32_t>(2 * MAX_PENDING);
}

void MsmEngine::collect(Stats& s) {
  for (int i = 0; i < pending_; ++i) {
    float ms = 0;
    HIPX(hipEventElapsedTime(&ms, ev_[i][0], ev_[i][1]));
    const uint32_t adds = h_total_dev_[i] ? h_counts_[MAX_PENDING + i] : h_total_[i];
    s.accumulate_ms += ms;
    s.launches += 1;
    s.mixed_adds += adds;
    s.tasks += h_counts_[i];
    s.per_launch.push_back({ms, adds, h_blocks_[i]});
  }
  pending_ = 0;
}

void MsmEngine::accumulate(const MsmPlan& plan, const MsmBases& bases) {
  const MsmParams& p = plan.params();
  if (p.c != prm_.c || p.depth != prm_.depth || p.windows != prm_.windows)
    throw std::runtime_error("MSM: plan and engine parameters differ");
  if (bases.c() != p.c || bases.depth() != p.depth || bases.curve() != curve_)
    throw std::runtime_error("MSM: base table does not match the plan (c, depth, curve)");
  if (bases.n() != plan.n()) throw std::runtime_error("MSM: base table size differs from the scalar count");
  if (plan.n() > max_n_) throw std::runtime_error("MSM: n exceeds engine capacity");
  HIPX(hipStreamWaitEvent(stream_, plan.ready(), 0));
  const int slot = (instrument_ && pending_ < MAX_PENDING && plan.entries() > 0) ? pending_++ : -1;
  hipEvent_t e0 = slot >= 0 ? ev_[slot][0].get() : nullptr, e1 = slot >= 0 ? ev_[slot][1].get() : nullptr;
  if (curve_ == Curve::G1)
    run_accumulate<Fq>(plan, bases, part_a_, stream_, e0, e1);
  else
    run_accumulate<Fq2>(plan, bases, part_a_, stream_, e0, e1);
  if (slot >= 0) {
    h_total_[slot] = plan.entries();  // every nonzero digit is one mixed addition
    h_blocks_[slot] = (uint32_t)grid_for(plan.max_tasks_now());
    h_total_dev_[slot] = plan.entries_dev() != nullptr;
    if (h_total_dev_[slot])  // hand-sorted plans: the exact count, not the grid bound n * W
      HIPX(hipMemcpyAsync(&h_counts_[MAX_PENDING + slot], plan.entries_dev(), 4, hipMemcpyDeviceToHost, stream_));
    HIPX(hipMemcpyAsync(&h_counts_[slot], plan.task_off() + plan.params().buckets(), 4, hipMemcpyDeviceToHost,
                        stream_));
  }
}

void MsmEngine::finish(const MsmPlan& plan, uint32_t* d_out, hipStream_t st) {
  if (!st) st = stream_;
  uint32_t* const sub[2] = {sub_[0], sub_[1]};
  if (curve_ == Curve::G1)
    run_finish<Fq>(plan, part_a_, part_b_, buckets_, rc_part_, rc_, seg_s_, seg_t_, sub, d_out, st);
  else
    run_finish<Fq2>(plan, part_a_, part_b_, buckets_, rc_part_, rc_, seg_s_, seg_t_, sub, d_out, st);
}

void MsmEngine::run(const MsmPlan& plan, const MsmBases& bases, uint32_t* d_out) {
  accumulate(plan, bases);
  finish(plan, d_out, stream_);
}

}  // namespace zkp
