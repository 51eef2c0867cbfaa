// Pippenger multi-scalar multiplication over BN254 G1 / G2 on gfx950.
//
// Replaces ffjavascript ``G1.multiExpAffine`` / ``G2.multiExpAffine``
// (g1m/g2m_multiexpAffine_chunk) as called five times by
// snarkjs ``groth16_prove``.  Result is bit-identical as a group element; the
// algorithm is a GPU re-design, not a translation.  Three objects:
//
//  MsmBases  (per point set, built once at zkey load, resident in HBM)
//     depth T rows of the affine bases: row t = 2^(c*t) * P_i.  With T = W
//     (the default: 288 GB of HBM pays for it) every window of a scalar lands
//     in ONE shared set of 2^(c-1) buckets, so the per-window bucket reduction
//     and the host Horner fold disappear; with T < W the W windows fall into
//     G = ceil(W/T) bucket groups, folded by Horner with shift c*T.
//
//  MsmPlan   (per scalar vector and set of finite bases, per proof; shared by every MSM over the
//     same scalars and the same finite bases -- B1 and the G2 MSM B2 share the witness's plan B)
//     0. mask   : a scalar whose base is the point at infinity (MsmBases::present) emits no digit
//     1. digits : the nonzero signed c-bit digits as (key = group*2^(c-1) + |d|-1,
//                 val = (t*n + i) | sign<<31), computed from the scalars inside
//     2. sort   : the hand-written three-pass LDS-staged bucket sort (hsort_kernels.hpp)
//     3. bounds : bucket [start, end) ranges, accumulate-task offsets (tasks of
//                 <= S entries never straddle a bucket), the task order by length and
//                 the offsets of the heavy-bucket merge levels.
//     Plans over the same scalars that differ only in their masks (a proof's witness plans B, A, C)
//     come from one build_shared: steps 1 and 2 once over the union, the entries tagged by plan.
//     build and build_shared enqueue the sort's first two passes (digits -> bins -> sub-bins) through
//     one driver in msm.hip; only the last pass (sub-bins -> buckets, bounds) differs between them.
//
//  MsmEngine (per curve and stream: partial sums, buckets, reduction tree)
//     4. accumulate: one thread per task, mixed XYZZ additions of gathered bases;
//                 every thread does the same bounded work whatever the scalar
//                 distribution (0/1-heavy witnesses put most points in one bucket).
//     5. merge  : buckets with more than 2*S2 task partials are folded by segmented
//                 merge levels that skip the light buckets; one thread per bucket
//                 sums what is left.
//     6. reduce : per group, with the 2^(c-1) buckets as U rows of V = 2^ceil((c-1)/2) (k = u V + v),
//                 sum_k (k+1) B_k = V sum_u u rho_u + sum_v (v+1) kappa_v  from the row sums rho_u and
//                 the column sums kappa_v: two additions per bucket (a chain per thread, then a
//                 shuffle tree per wave).  The two weighted sums over <= V points each (sub-groups
//                 2g: rho_1.., 2g+1: kappa) are sum_p T_p + M sum_b 2^b Q_b from segment running
//                 sums (S_p, T_p over M points) and bit-subset sums Q_b = sum_{p: bit b} S_p.
//     7. out    : 2G x K points (XYZZ, device layout); the host applies the 2^b, M, V and group
//                 (2^(c T g)) weights by Horner (msm_fold).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "hip_raii.hpp"

namespace zkp {

// the rounded-up base-2 logarithm: the least l with 2^l >= n (0 for n <= 1)
inline int lg_ceil(size_t n) {
  int l = 0;
  while ((size_t(1) << l) < n) ++l;
  return l;
}

struct MsmParams {
  int c = 16;        // window bits
  int windows = 16;  // W = ceil(255 / c)   (254-bit scalars + the signed-digit carry)
  int depth = 16;    // T: precomputed rows per base
  int groups = 1;    // G = ceil(W / T) bucket groups
  int S = 32;        // max entries per accumulate task
  int S2 = 4;        // fan-in of a heavy-bucket merge level (short chains: latency-bound)
  int M = 4;         // row / column sums per reduction segment (running sums)
  // bits the windows cover: 255 = any scalar below r plus the signed-digit carry.  A caller whose
  // scalars are all below 2^b passes b + 1 and gets ceil((b + 1) / c) windows: no digits, buckets or
  // reductions for the windows above (zkey_verify.hip: 128-bit coefficients, 129)
  int scalar_bits = 255;
  // c_override / depth_override: 0 = automatic.  Window bits must lie in [MIN_C, MAX_C]: W <= 32
  // windows keep a scalar block's digits in one LDS stage of the bucket sort, and the bucket key
  // (group and bucket bits, <= 27) splits into its three passes (hsort_kernels.hpp).
  static constexpr int MIN_C = 8, MAX_C = 24;
  static MsmParams make(size_t n, int c_override = 0, int depth_override = 0, int scalar_bits = 255) {
    MsmParams p;
    if (scalar_bits < 1 || scalar_bits > 255) throw std::invalid_argument("MSM scalar bits must be within 1..255");
    p.scalar_bits = scalar_bits;
    const int lg = lg_ceil(n);
    // one bucket set of 2^(c-1) buckets against n*W entries: c = lg - 4 keeps every bucket ~8*W
    // entries deep and the bucket reduction (2^c full adds) small; 20 bits caps the automatic choice
    p.c = c_override > 0 ? c_override : (lg - 4 < MIN_C ? MIN_C : (lg - 4 > 20 ? 20 : lg - 4));
    if (p.c < MIN_C || p.c > MAX_C)
      throw std::invalid_argument("MSM window bits must be within " + std::to_string(MIN_C) + ".." +
                                  std::to_string(MAX_C) + " (got " + std::to_string(p.c) + ")");
    p.windows = (scalar_bits + p.c - 1) / p.c;
    p.depth = depth_override > 0 ? (depth_override < p.windows ? depth_override : p.windows) : p.windows;
    p.groups = (p.windows + p.depth - 1) / p.depth;
    if (p.M > p.V()) p.M = p.V();
    return p;
  }
  size_t half() const { return size_t(1) << (c - 1); }
  size_t buckets() const { return (size_t)groups * half(); }
  // capacities: the entries of max_n scalars of which at most max_present emit digits, and the
  // accumulate tasks of so many entries (every bucket's last task may be a short one)
  size_t max_entries(size_t max_n, size_t max_present) const {
    return std::max<size_t>(std::min(max_present, max_n), 1) * windows;
  }
  size_t max_tasks(size_t entries) const { return (entries + S - 1) / S + buckets(); }
  // a group's buckets as U rows of V: bucket k = u V + v, V = 2^ceil((c-1)/2) >= U
  int lgV() const { return c / 2; }
  int V() const { return 1 << lgV(); }
  int U() const { return 1 << (c - 1 - lgV()); }
  // every group reduces to two sub-groups of V points (its row sums, then its column sums), each of
  // which leaves lgP subset sums Q_b and sum_p T_p (P = V / M segments): K points
  int subgroups() const { return 2 * groups; }
  int lg_m() const { return lg_ceil((size_t)M); }
  int lgP() const { return lgV() - lg_m(); }
  int K() const { return lgP() + 1; }
  size_t out_points() const { return (size_t)subgroups() * K(); }
};

// Window bits for a DENSE plan (hand-written bucket sort) near c.  The top window of a 254-bit
// scalar holds only 254 - (W - 1) c digit bits: for c = 18, 19, 21 (2, 7, 2 bits) all n of its
// digits fall into a handful of buckets, i.e. into one or a few sub-bins of the sort's pass C,
// which gives every sub-bin ONE workgroup -- measured 1.3 ms for that kernel alone at 2^20
// points and c = 18 (0.05 ms at c = 20), +13 ms per Venmo proof at c = 21
// (273c6e8:tools/gpu/experiments/r2_hsort_c*.sh).  Keep c whose top window spans >= 12 bits (>= 128
// sub-bins), trying c+1, c-1, c+2, ... within [8, 20]; below 2^17 points one workgroup per
// sub-bin copes (n entries at most), so c stays.
inline int dense_window_bits(int c, size_t n) {
  auto top = [](int cc) { return 254 - ((255 + cc - 1) / cc - 1) * cc; };
  if (n < (size_t(1) << 17) || top(c) >= 12) return c;
  for (int d = 1; d <= 6; ++d) {
    if (c + d <= 20 && top(c + d) >= 12) return c + d;
    if (c - d >= 8 && top(c - d) >= 12) return c - d;
  }
  return c;
}
// the automatic window bits of a plan over n uniform scalars (the prover's H plan, the kernel-level
// MSMs, the ptau sums): lg n - 3 within [8, 20], moved off a collapsed top window
inline int h_window_bits(size_t n) { return dense_window_bits(std::min(20, std::max(8, lg_ceil(n) - 3)), n); }

// words per coordinate element: G1 -> Fq (8 words), G2 -> Fq2 (16 words)
enum class Curve { G1 = 1, G2 = 2 };

inline int curve_fwords(Curve c) { return c == Curve::G1 ? 8 : 16; }

// The finite bases of a table as a device bitset: bit i & 31 of word i / 32 is set when base i is not
// the point at infinity (all-zero coordinates).  A zkey holds an infinity base for every signal that no
// A (or B) linear combination mentions; a plan built with the mask emits no digit for those, so the
// accumulation never spends a wave's full addition on lanes that add nothing.  `index` lists the set
// bits in order (index[j] = the j-th finite base): a masked plan's pass A visits `count` scalars through
// it instead of testing n bits, so its cost follows the finite bases, not the signals.  Empty (no bits,
// no index, both null) when every base is finite: a plan then runs its unmasked kernels and reads
// neither.
struct BaseMask {
  DevBuf<> bits, index;
  size_t count = 0;  // finite bases (n when there is no mask)
  const uint32_t* data() const { return bits ? bits.get() : nullptr; }
  const uint32_t* list() const { return index ? index.get() : nullptr; }
};

// Precomputed base table: rows() x n affine points (device layout, Montgomery R'=2^261).
class MsmBases {
 public:
  MsmBases(Curve curve, size_t n, int c, int depth);
  // a view, not a table: n points that already lie in HBM in device layout, depth 1, nothing owned and
  // no mask (a base at infinity costs its lane an addition).  Lets one resident array serve base sets
  // that overlap (ptau_verify.hip: points [k, k + m) and [k + 1, k + m + 1) under one plan).
  MsmBases(Curve curve, const uint32_t* points, size_t n, int c);
  // row 0 (n points): the caller fills it (device layout), then extend() derives rows 1..T-1 and the
  // mask of the finite bases from row 0 (it waits for the stream once: the count comes to the host)
  uint32_t* row0() { return d_; }
  void extend(hipStream_t st);
  // the finite bases (null: all of them) and how many they are, once extend() has run
  const uint32_t* present() const { return mask_.data(); }
  const uint32_t* present_index() const { return mask_.list(); }
  size_t present_count() const { return mask_.bits ? mask_.count : n_; }
  const uint32_t* data() const { return view_ ? view_ : d_.get(); }
  size_t n() const { return n_; }
  int c() const { return c_; }
  int depth() const { return depth_; }
  Curve curve() const { return curve_; }
  size_t bytes() const { return bytes_; }
  static size_t bytes_for(Curve curve, size_t n, int depth) {
    return (size_t)depth * (n ? n : 1) * 8 * curve_fwords(curve);
  }

 private:
  Curve curve_;
  size_t n_;
  int c_, depth_;
  size_t bytes_ = 0;
  DevBuf<> d_;
  const uint32_t* view_ = nullptr;
  BaseMask mask_;
};

// the bases finite in a or in b (two tables over the same n signals whose MSMs share one plan: the
// zkey's B1 and B2); no mask when either table has none.  Waits for the stream once.
BaseMask mask_union(const MsmBases& a, const MsmBases& b, hipStream_t st);

// Which of up to NPLAN plans over the same n scalars each scalar belongs to (MsmPlan::build_shared):
// memb[i] has bit p set when scalar i's base is finite in plan p's mask; `any` masks the scalars with
// at least one bit (its index list is what the shared pass A visits; no mask when that is all of them).
struct PlanMembership {
  static constexpr int NPLAN = 3;
  DevBuf<uint8_t> memb;
  BaseMask any;
  size_t count[NPLAN] = {};  // scalars with bit p
  size_t bytes() const { return memb.count() + (any.bits.count() + any.index.count()) * 4; }
};
// bits[p]: plan p's mask over n scalars (BaseMask::data; null: every scalar belongs) with count[p] set
// bits; use[p] false: no plan p (its bit stays clear).  Built on the device; waits for the stream once.
PlanMembership plan_membership(const uint32_t* const bits[PlanMembership::NPLAN],
                               const size_t count[PlanMembership::NPLAN], const bool use[PlanMembership::NPLAN],
                               size_t n, hipStream_t st);

// The bucket sort's working memory and geometry: entries, histograms, tile offsets and scan sums,
// 16 of a plan's ~20 bytes per entry.  Nothing reads it once MsmPlan::build has enqueued its last
// kernel, so plans with the same parameters that build back to back on ONE stream share one.
struct MsmSortScratch {
  // max_n scalars of which at most max_present emit digits; nplans > 1: the scratch of a shared build
  // (MsmPlan::build_shared) of so many plans, whose pass C keeps its counts per plan
  MsmSortScratch(size_t max_n, size_t max_present, const MsmParams& prm, int nplans = 1);
  MsmParams prm;
  int nplans = 1;
  size_t stride3 = 0;  // words between the plans' pass-C count arrays
  DevBuf<> binbase;    // a shared build's bin bases (one plan's live in the plan: the entry count)
  size_t max_n, max_entries, max_tasks, nbuckets;
  int merge_levels = 0;
  int b2 = 0, b3 = 0, k = 1;  // sub-bin / bucket bits of the key, scalars per thread in pass A
  uint32_t nbins = 0;
  uint32_t nq() const { return nbins << b2; }  // sub-bins
  // workgroups (tiles) of pass B and of the tiled pass C over `total` entries: every bin / sub-bin may
  // end in a partial tile
  size_t tiles2(size_t total) const;
  size_t tiles3(size_t total) const;
  DevBuf<> cnt, tl_hist, tl_off, lvl_tsum;
  DevBuf<> toff3, hist3, off3;
  DevBuf<> hist, blkoff, toff, hist2, off2, subbase;
  DevBuf<uint2> ent_a, ent_b;  // (key, base|sign) entries
  DevBuf<> tsum;               // tile sums of the look-back-free scans
};

class MsmPlan {
 public:
  // max_present: the most scalars that can emit digits (a mask's count; default all max_n), which
  // sizes the plan's outputs; scratch: shared sort memory (see MsmSortScratch), or the plan's own
  MsmPlan(size_t max_n, const MsmParams& prm, hipStream_t stream, size_t max_present = ~size_t(0),
          std::shared_ptr<MsmSortScratch> scratch = nullptr);
  // scalars: device, 8 LE 32-bit words each (standard form, any value < 2^256: reduced below r
  // when loaded, msm_kernels.hpp load_scalar, so W = ceil(255 / c) windows always hold the carry).
  // present: the index list of a base table's mask over the same n (BaseMask::list; null = none) with
  // n_present entries: a scalar it does not list counts as zero.
  // Enqueues on the plan's stream, never blocks the host (the exact entry count stays on the
  // device: entries_dev()); records ready() at the end.
  void build(const uint32_t* scalars, size_t n, const uint32_t* present = nullptr, size_t n_present = 0);
  // One build for up to PlanMembership::NPLAN compacted plans over the same scalars (null: no plan p)
  // that share one scratch (made for so many plans) and one stream: the digits are computed and
  // sorted once over the scalars of mem.any, every entry tagged with the plans it belongs to; the
  // last pass writes each plan's bucket-ordered words.  Every plan ends as build() with its own mask
  // would leave it (the same outputs, the exact entry count; order inside a bucket is unspecified in
  // both) and records its ready(): the plans with entries in the order of the array, then the empty ones.
  static void build_shared(MsmPlan* const plans[PlanMembership::NPLAN], const uint32_t* scalars, size_t n,
                           const PlanMembership& mem);
  // dense (uniform scalars, e.g. the H MSM's: nearly every digit is nonzero and the buckets evenly
  // filled): pass C of the sort takes one workgroup per sub-bin; otherwise (the 0/1-heavy witness:
  // whole waves of entries in one bucket) wave-aggregated LDS claims and a tiled pass C
  void set_dense(bool d) { dense_ = d; }
  bool dense() const { return dense_; }
  const MsmParams& params() const { return prm_; }
  hipEvent_t ready() const { return ready_; }
  hipStream_t stream() const { return stream_; }
  size_t n() const { return n_; }
  size_t max_n() const { return max_n_; }
  // entries the accumulate grid is sized for: the bound n * W, or the mask's count * W (the exact
  // count stays on the device)
  uint32_t entries() const { return total_; }
  // device word holding the exact nonzero-digit count once ready() (nullptr for an empty plan)
  const uint32_t* entries_dev() const { return hs_built_ ? hs_binbase_ + sc_->nbins : nullptr; }
  int merge_levels() const { return merge_levels_; }

  // device results (read-only once ready())
  const uint32_t* vals() const { return vals_sorted_; }
  const uint32_t* bstart() const { return bstart_; }
  const uint32_t* bend() const { return bend_; }
  const uint32_t* task_off() const { return off_task_; }
  const uint32_t* perm() const { return perm_; }  // task order (by length)
  const uint32_t* level_off(int lv) const { return lvl_all_ + (size_t)lv * (nbuckets_ + 1); }
  size_t max_tasks_now() const { return max_tasks_now_; }
  size_t max_tasks() const { return max_tasks_; }

 private:
  // what follows the sort: an empty plan's bounds (empty) or the task offsets, the task order and the
  // merge levels' offsets from the bucket bounds and task counts; records ready()
  void build_tail(bool empty);
  MsmParams prm_;
  size_t max_n_, n_ = 0;
  hipStream_t stream_;
  Event ready_;
  size_t nbuckets_ = 0, max_entries_ = 0, max_tasks_ = 0, max_tasks_now_ = 0;
  int merge_levels_ = 0;
  uint32_t total_ = 0;
  // what the engines read: base|sign words in bucket order (the accumulation's input), bucket
  // bounds, task offsets and order, merge level l's offsets (lvl_all_ + l * (buckets + 1)), and the
  // bin bases whose last word is the entry count
  DevBuf<> vals_sorted_;
  DevBuf<> bstart_, bend_, off_task_;
  DevBuf<> lvl_all_;
  DevBuf<> perm_;  // accumulate-task order by length (longest first)
  DevBuf<> hs_binbase_;
  bool dense_ = false;
  bool hs_built_ = false;
  // the three-pass LDS-staged bucket sort's memory (hsort_kernels.hpp)
  std::shared_ptr<MsmSortScratch> sc_;
};

class MsmEngine {
 public:
  MsmEngine(Curve curve, const MsmParams& prm, size_t max_n, hipStream_t stream);

  // sum_i s_i * P_i for the plan's scalars over the bases (bases.n() == plan.n(),
  // same c and depth).  Waits for plan.ready() on the engine's stream, enqueues
  // everything there; the 2G x K sub-group sums (XYZZ, device layout, window_words() words)
  // land in d_out (device).  Nothing is synchronised.
  void run(const MsmPlan& plan, const MsmBases& bases, uint32_t* d_out);
  // the same in two phases: accumulate() on the engine's stream (bucket-task partial sums),
  // finish() (merges + reduction + output) on stream `st` (0 = the engine's), which the
  // caller must order after accumulate(), e.g. by an event; lets a stream run the next
  // MSM's accumulation while another finishes this one
  void accumulate(const MsmPlan& plan, const MsmBases& bases);
  void finish(const MsmPlan& plan, uint32_t* d_out, hipStream_t st = nullptr);
  size_t window_words() const { return window_words_for(curve_, prm_); }
  static size_t window_words_for(Curve c, const MsmParams& p) { return p.out_points() * 4 * curve_fwords(c); }

  // Kernel instrumentation (HIP events on this engine's stream).  When enabled,
  // every run() brackets the bucket-accumulate kernel with events; collect()
  // must be called after the stream is synchronised.
  struct Launch {
    float ms;       // HIP events on the engine's stream around the launch
    uint32_t adds;  // nonzero digits it accumulated (mixed additions)
    uint32_t blocks;  // workgroups of the launch (matches a kernel trace's grid size / TPB)
  };
  struct Stats {
    double accumulate_ms = 0;  // summed over launches
    uint64_t launches = 0;
    uint64_t mixed_adds = 0;   // nonzero (point, window) digits processed
    uint64_t tasks = 0;
    std::vector<Launch> per_launch;  // every collected launch, in order
  };
  void set_instrument(bool on) { instrument_ = on; }
  void collect(Stats& s);
  const MsmParams& params() const { return prm_; }
  Curve curve() const { return curve_; }
  hipStream_t stream() const { return stream_; }

 private:
  Curve curve_;
  MsmParams prm_;
  size_t max_n_;
  hipStream_t stream_;
  size_t nbuckets_ = 0, max_tasks_ = 0;
  int fwords_;
  DevBuf<> part_a_, part_b_, buckets_;
  DevBuf<> rc_part_, rc_;  // row / column chain partials; the 2G sub-groups of V row and column sums
  DevBuf<> seg_s_, seg_t_, sub_[2];
  static constexpr int MAX_PENDING = 16;
  bool instrument_ = false;
  int pending_ = 0;
  Event ev_[MAX_PENDING][2];
  PinnedBuf<uint32_t> h_counts_;  // pinned: tasks per pending run, then entries per pending run
  uint32_t h_total_[MAX_PENDING] = {};
  bool h_total_dev_[MAX_PENDING] = {};
  uint32_t h_blocks_[MAX_PENDING] = {};  // entries copied from the device (h_counts_[MAX_PENDING + i])
};

// merge levels needed for n points with the given params (worst case: one bucket of
// a group receives a digit of every window of the group)
inline int msm_merge_levels(size_t max_n, const MsmParams& prm) {
  size_t m = ((max_n ? max_n : 1) * (size_t)prm.depth + prm.S - 1) / prm.S;
  int levels = 0;
  while (m > 2 * (size_t)prm.S2) {
    m = (m + prm.S2 - 1) / prm.S2;
    ++levels;
  }
  return levels;
}

}  // namespace zkp
