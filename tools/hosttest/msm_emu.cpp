// CPU replay of the MSM pipeline (msm_kernels.hpp per-thread bodies, same
// parameters as MsmEngine) for debugging without a GPU.
// usage: msm_emu <g1|g2> <file: points(zkey layout)|scalars> <n> [c] [depth] [--task S] [--seg M] [--events]
//   -> prints the affine result (decimal); c, depth 0 = automatic
//   --task S, --seg M: the accumulate task size and the reduction's segment size (as ZKP_MSM task_h= /
//     seg= set them; the kernel-level entry points run with S = 48, device_pipeline.hip apply_task_options)
//   --events: a `geometry` line before the result, and after it one `event <stage> <dbl> <cancel> <acc_inf>
//     <q_inf>` line per stage: how often the additions of that stage took an exceptional branch (curve.hpp ZKP_XYZZ_EVENT)
// The per-thread bodies are the shared templates.  The two device-only reductions (the shuffle butterfly
// rowcol_tree and the workgroup LDS trees) are restated as host loops that pair the operands in the
// device's order; their additions are the shared xyzz_add.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

// events per (stage, kind): the stage is set before each loop below, the kind comes from the hook
static std::vector<std::string> g_stage_names;
static std::vector<std::array<unsigned long long, 4>> g_events;
static int g_stage = 0, g_reduce_stage[2] = {0, 0};
static int stage_id(const std::string& name) {
  for (size_t i = 0; i < g_stage_names.size(); ++i)
    if (g_stage_names[i] == name) return (int)i;
  g_stage_names.push_back(name);
  g_events.push_back({0, 0, 0, 0});
  return (int)g_stage_names.size() - 1;
}
static void set_stage(const std::string& name) { g_stage = stage_id(name); }
static inline void emu_event(int kind) { ++g_events[g_stage][kind]; }
enum { EMU_REDUCE_R = 0, EMU_REDUCE_T = 1 };
#define ZKP_XYZZ_EVENT(kind) ::emu_event((int)(kind))
#define ZKP_MSM_STAGE(tag) (::g_stage = ::g_reduce_stage[EMU_##tag])
#include "../../zk-p2p-onramp_amd/csrc/msm_kernels.hpp"
#include "../../zk-p2p-onramp_amd/csrc/msm.hpp"
#include "../../zk-p2p-onramp_amd/csrc/host_ec.hpp"
using namespace zkp;

struct Overrides {
  int c = 0, depth = 0, task = 0, seg = 0;
  bool events = false;
};

// the workgroup's sum of its TREE_TPB threads' values, in the order of msmk::wg_tree_sum: at level sh
// thread t < sh adds the value of thread t + sh
template <class F>
static Xyzz<F> host_wg_tree_sum(std::vector<Xyzz<F>>& v, const std::string& stage) {
  for (int sh = msmk::TREE_TPB / 2; sh >= 1; sh >>= 1) {
    set_stage(stage + ".lds." + std::to_string(sh));
    for (int t = 0; t < sh; ++t) xyzz_add(v[t], v[t + sh]);
  }
  return v[0];
}

// one tree launch (msmk::subset_tree_first / subset_tree_next): value(seg, i) is value i of the cnt(seg)
// values of sum seg; chunk sums -> out[seg * nch + chunk].  Thread t of a chunk loads values t and
// TREE_TPB + t of the chunk's 2 * TREE_TPB.
template <class F, class Cnt, class Val>
static void host_tree_level(uint32_t nseg, uint32_t nch, Cnt cnt, Val value, const std::string& stage, uint32_t* out) {
  std::vector<Xyzz<F>> v(msmk::TREE_TPB);
  for (uint32_t seg = 0; seg < nseg; ++seg)
    for (uint32_t chunk = 0; chunk < nch; ++chunk) {
      for (auto& x : v) x = xyzz_inf<F>();
      for (int h = 0; h < 2; ++h) {
        set_stage(stage + ".load" + std::to_string(h));
        for (uint32_t t = 0; t < (uint32_t)msmk::TREE_TPB; ++t) {
          const uint32_t i = chunk * 2 * msmk::TREE_TPB + (uint32_t)h * msmk::TREE_TPB + t;
          if (i < cnt(seg)) xyzz_add(v[t], value(seg, i));
        }
      }
      store_xyzz(out, (size_t)seg * nch + chunk, host_wg_tree_sum(v, stage));
    }
}

template <class F, class HF>
static host::Jac<HF> run(std::vector<uint32_t>& pts, std::vector<uint32_t>& sc, uint32_t n, const Overrides& ovr) {
  constexpr int FW = FWords<F>::W;
  // convert points to device layout
  for (size_t i = 0; i < pts.size() / 8; ++i) {
    Fq x = load_fe<FqCfg>(&pts[i * 8]);
    x = mul(x, fe_const<FqCfg>(Conv::FQ_ZKEY_TO_DEV));
    store_fe(&pts[i * 8], x);
  }
  MsmParams prm = MsmParams::make(std::max<uint32_t>(n, 1), ovr.c, ovr.depth);
  if (ovr.task > 0) prm.S = ovr.task;
  if (ovr.seg > 0 && ovr.seg <= prm.V()) prm.M = ovr.seg;  // as apply_task_options
  const uint32_t W = prm.windows, T = prm.depth, G = prm.groups, half = 1u << (prm.c - 1), nb = G * half;
  // base table rows 1..T-1 (as MsmBases::extend)
  std::vector<uint32_t> table((size_t)T * n * 2 * FW);
  std::copy(pts.begin(), pts.begin() + (size_t)n * 2 * FW, table.begin());
  for (uint32_t t = 1; t < T; ++t)
    for (uint32_t i = 0; i < n; ++i) msmk::extend_row<F>(i, table.data(), n, prm.c, (int)t);
  // the nonzero digits (window-major, point order); the device sort groups them by bucket in another order
  std::vector<std::vector<std::pair<uint32_t, uint32_t>>> per(W);
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t s[9];
    msmk::load_scalar(sc.data(), i, s);
    uint32_t carry = 0, key, val;
    for (uint32_t w = 0; w < W; ++w)
      if (msmk::digit_entry(s, (int)w, prm.c, (int)T, n, i, carry, key, val)) per[w].push_back({key, val});
  }
  std::vector<uint32_t> ks, vs;
  for (auto& v : per)
    for (auto& e : v) ks.push_back(e.first), vs.push_back(e.second);
  // stable sort on the whole bucket key (group and bucket bits), as the bucket sort groups them
  std::vector<uint32_t> idx(ks.size());
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return ks[a] < ks[b]; });
  { std::vector<uint32_t> k2(ks.size()), v2(ks.size()); for (size_t i = 0; i < idx.size(); ++i) { k2[i] = ks[idx[i]]; v2[i] = vs[idx[i]]; } ks.swap(k2); vs.swap(v2); }
  const uint32_t total2 = (uint32_t)ks.size();
  std::vector<uint32_t> st(nb + 1, 0), en(nb + 1, 0), cnt(nb + 1), off(nb + 1);
  for (uint32_t i = 0; i < total2; ++i) {  // bucket [start, end) and ceil(len / S) tasks (as k_hs_fine / k_hs_bounds3)
    if (i == 0 || ks[i - 1] != ks[i]) st[ks[i]] = i;
    if (i == total2 - 1 || ks[i + 1] != ks[i]) en[ks[i]] = i + 1;
  }
  for (uint32_t b = 0; b <= nb; ++b) cnt[b] = b == nb ? 0u : (en[b] - st[b] + prm.S - 1) / prm.S;
  uint32_t acc = 0;
  for (uint32_t b = 0; b <= nb; ++b) { off[b] = acc; acc += cnt[b]; }
  const uint32_t ntask = off[nb];
  std::vector<uint32_t> part((size_t)(ntask + 1) * 4 * FW);
  set_stage("accumulate");
  for (uint32_t t = 0; t < ntask; ++t) msmk::accumulate<F>(t, table.data(), vs.data(), st.data(), en.data(), off.data(), nb, prm.S, nullptr, part.data());
  // heavy-bucket merge levels (as MsmPlan::build + MsmEngine::run)
  const int levels = msm_merge_levels(std::max<uint32_t>(n, 1), prm);
  std::vector<uint32_t> part1(part.size()), hcnt(nb + 1), hoff(nb + 1);
  for (int lv = 0; lv < levels; ++lv) {
    for (uint32_t b = 0; b <= nb; ++b) msmk::heavy_counts(b, off.data(), nb, prm.S2, lv, hcnt.data());
    uint32_t a2 = 0;
    for (uint32_t b = 0; b <= nb; ++b) { hoff[b] = a2; a2 += hcnt[b]; }
    const uint32_t* src = (lv & 1) ? part1.data() : part.data();
    uint32_t* dst = (lv & 1) ? part.data() : part1.data();
    set_stage("merge_heavy." + std::to_string(lv));
    for (uint32_t t = 0; t < hoff[nb]; ++t) msmk::merge_heavy<F>(t, src, off.data(), hoff.data(), nb, prm.S2, lv, dst);
  }
  std::vector<uint32_t> buckets((size_t)nb * 4 * FW);
  set_stage("merge_final");
  for (uint32_t b = 0; b < nb; ++b)
    msmk::merge_final<F>(b, part.data(), part1.data(), off.data(), nb, prm.S2, levels, buckets.data());
  // reduction, first level (as run_finish): the row and column partials by rowcol_chain with the engine's
  // chain lengths, then every sum from its partials in the order of the shuffle butterfly rowcol_tree
  // (lane l of a sum adds partials 2l and 2l + 1, then at level m the value of lane l ^ m: every lane
  // computes its own sum, lane 0 stores), placed by rowcol_slot.  The lanes of row 0, which has no
  // slot, hold infinity.
  const uint32_t U = prm.U(), V = prm.V(), G2 = prm.subgroups();
  const msmk::RowCol rc = msmk::rowcol_make(G, U, V, msmk::ROWCOL_CHAIN, msmk::ROWCOL_SPAN);
  const uint32_t nparts = rc.row_parts() + rc.col_parts();
  std::vector<uint32_t> rpart((size_t)nparts * 4 * FW, 0xdeadbeefu), xs((size_t)G2 * V * 4 * FW, 0xdeadbeefu);
  set_stage("rowcol_chain.row");
  for (uint32_t id = 0; id < rc.row_parts(); ++id) msmk::rowcol_chain<F>(id, buckets.data(), rc, rpart.data(), xs.data());
  set_stage("rowcol_chain.col");
  for (uint32_t id = rc.row_parts(); id < nparts; ++id) msmk::rowcol_chain<F>(id, buckets.data(), rc, rpart.data(), xs.data());
  std::vector<Xyzz<F>> lane(64);
  for (uint32_t seg = 0; seg < G * (U + V); ++seg) {
    const uint32_t slot = msmk::rowcol_slot(seg, rc);
    const bool col = seg >= G * U;
    const std::string name = col ? "rowcol_tree.col" : "rowcol_tree.row";
    const uint32_t n = col ? rc.nc() : rc.nr(), e = n >= 2 ? 2u : 1u, lanes = n / e;
    const size_t p0 = col ? (size_t)rc.row_parts() + (size_t)(seg - G * U) * n : (size_t)seg * n;
    set_stage(name + ".pair");
    for (uint32_t l = 0; l < lanes; ++l) {
      lane[l] = xyzz_inf<F>();
      if (slot == msmk::ROWCOL_NONE) continue;
      lane[l] = load_xyzz<F>(rpart.data(), p0 + (size_t)l * e);
      if (e == 2) xyzz_add(lane[l], load_xyzz<F>(rpart.data(), p0 + (size_t)l * e + 1));
    }
    for (uint32_t m = 1; m < lanes; m <<= 1) {
      set_stage(name + ".bfly." + std::to_string(m));
      const std::vector<Xyzz<F>> before(lane.begin(), lane.begin() + lanes);
      for (uint32_t l = 0; l < lanes; ++l) xyzz_add(lane[l], before[l ^ m]);
    }
    if (slot != msmk::ROWCOL_NONE) store_xyzz(xs.data(), slot, lane[0]);
  }
  // second level over the 2G sub-groups of V points: segments, then the K subset sums by the launches
  // run_finish chooses: workgroup trees from the segment sums, or first a chain level of fan-in
  // TREE_CHAIN_FAN, then tree levels until one value per sum is left
  const uint32_t M = prm.M, lgP = prm.lgP(), K = prm.K(), P = V / M;
  std::vector<uint32_t> ss((size_t)G2 * P * 4 * FW), tt(ss.size());
  g_reduce_stage[EMU_REDUCE_R] = stage_id("reduce_segments.R");
  g_reduce_stage[EMU_REDUCE_T] = stage_id("reduce_segments.T");
  for (uint32_t id = 0; id < G2 * P; ++id) msmk::reduce_segments<F>(id, xs.data(), G2, V, M, ss.data(), tt.data());
  constexpr uint32_t CH = 2 * msmk::TREE_TPB;
  uint32_t nn = (P + CH - 1) / CH;
  const bool tree_first = (size_t)G2 * K * nn <= msmk::TREE_FIRST_MAX;
  std::vector<uint32_t> sub, sub2;
  if (tree_first) {
    sub.resize((size_t)G2 * K * nn * 4 * FW);
    host_tree_level<F>(
        G2 * K, nn, [&](uint32_t seg) { return seg % K < lgP ? P / 2 : P; },
        [&](uint32_t seg, uint32_t i) {
          const uint32_t g = seg / K, b = seg % K;
          if (b == lgP) return load_xyzz<F>(tt.data(), (size_t)g * P + i);
          const uint32_t p = ((i >> b) << (b + 1)) | (1u << b) | (i & ((1u << b) - 1));
          return load_xyzz<F>(ss.data(), (size_t)g * P + p);
        },
        "subset_tree", sub.data());
  } else {
    const uint32_t cf = msmk::TREE_CHAIN_FAN;
    nn = msmk::subset_n1(lgP, cf);
    sub.resize((size_t)G2 * K * nn * 4 * FW);
    set_stage("subset_first");
    for (uint32_t id = 0; id < G2 * K * nn; ++id) msmk::subset_first<F>(id, ss.data(), tt.data(), G2, lgP, cf, sub.data());
  }
  const uint32_t first_n = nn;
  while (nn > 1) {
    const uint32_t next = (nn + CH - 1) / CH;
    sub2.assign((size_t)G2 * K * next * 4 * FW, 0);
    host_tree_level<F>(
        G2 * K, next, [&](uint32_t) { return nn; },
        [&](uint32_t seg, uint32_t i) { return load_xyzz<F>(sub.data(), (size_t)seg * nn + i); }, "subset_next",
        sub2.data());
    sub.swap(sub2);
    nn = next;
  }
  if (ovr.events)
    std::printf("geometry c=%d windows=%d depth=%d groups=%d U=%u V=%u Lr=%u Lc=%u nr=%u nc=%u M=%u P=%u S=%d S2=%d "
                "levels=%d first=%s chunks=%u\n",
                prm.c, prm.windows, prm.depth, prm.groups, U, V, rc.Lr, rc.Lc, rc.nr(), rc.nc(), M, P, prm.S, prm.S2,
                levels, tree_first ? "tree" : "chain", first_n);
  // host fold (same as device_pipeline.hip msm_fold)
  auto ld = [&](uint32_t w) {
    const uint32_t* p = sub.data() + (size_t)w * 4 * FW;
    if constexpr (FW == 8)
      return host::jac_from_xyzz(host::fq_from_dev(p), host::fq_from_dev(p + 8), host::fq_from_dev(p + 16), host::fq_from_dev(p + 24));
    else {
      auto f2 = [](const uint32_t* q) { return host::Fq2{host::fq_from_dev(q), host::fq_from_dev(q + 8)}; };
      return host::jac_from_xyzz(f2(p), f2(p + 16), f2(p + 32), f2(p + 48));
    }
  };
  auto subgroup = [&](uint32_t s) {
    host::Jac<HF> a = lgP > 0 ? ld(s * K + lgP - 1) : host::Jac<HF>::inf();
    for (int b = (int)lgP - 2; b >= 0; --b) a = host::jac_add(host::jac_dbl(a), ld(s * K + b));
    for (int i = 0; i < prm.lg_m(); ++i) a = host::jac_dbl(a);
    return host::jac_add(a, ld(s * K + lgP));
  };
  auto group = [&](uint32_t g) {
    host::Jac<HF> a = subgroup(2 * g);
    for (int i = 0; i < prm.lgV(); ++i) a = host::jac_dbl(a);
    return host::jac_add(a, subgroup(2 * g + 1));
  };
  host::Jac<HF> r = group(G - 1);
  for (int g = (int)G - 2; g >= 0; --g) {
    for (int i = 0; i < prm.c * (int)T; ++i) r = host::jac_dbl(r);
    r = host::jac_add(r, group(g));
  }
  return r;
}

static void print_events() {
  for (size_t i = 0; i < g_stage_names.size(); ++i)
    printf("event %s %llu %llu %llu %llu\n", g_stage_names[i].c_str(), g_events[i][0], g_events[i][1], g_events[i][2],
           g_events[i][3]);
}

int main(int argc, char** argv) {
  std::vector<const char*> pos;
  Overrides ovr;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--events")) ovr.events = true;
    else if (!strcmp(argv[i], "--task") && i + 1 < argc) ovr.task = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--seg") && i + 1 < argc) ovr.seg = atoi(argv[++i]);
    else pos.push_back(argv[i]);
  }
  if (pos.size() < 3) {
    fprintf(stderr, "usage: msm_emu <g1|g2> <file> <n> [c] [depth] [--task S] [--seg M] [--events]\n");
    return 2;
  }
  bool g2 = std::string(pos[0]) == "g2";
  FILE* f = fopen(pos[1], "rb");
  if (!f) return 1;
  uint32_t n = atoi(pos[2]);
  ovr.c = pos.size() > 3 ? atoi(pos[3]) : 0, ovr.depth = pos.size() > 4 ? atoi(pos[4]) : 0;
  size_t pw = g2 ? 32 : 16;
  std::vector<uint32_t> pts(n * pw), sc(n * 8 + 8);
  if (fread(pts.data(), 4, pts.size(), f) != pts.size()) return 1;
  if (fread(sc.data(), 4, n * 8, f) != n * 8) return 1;
  if (!g2) {
    auto a = host::jac_to_aff(run<Fq, host::Fq>(pts, sc, n, ovr));
    if (a.inf) { printf("inf\n"); if (ovr.events) print_events(); return 0; }
    auto x = a.x.to_std(), y = a.y.to_std();
    printf("%s %s\n", host::u256_to_dec(x).c_str(), host::u256_to_dec(y).c_str());
  } else {
    auto a = host::jac_to_aff(run<Fq2, host::Fq2>(pts, sc, n, ovr));
    if (a.inf) { printf("inf\n"); if (ovr.events) print_events(); return 0; }
    printf("%s %s %s %s\n", host::u256_to_dec(a.x.c0.to_std()).c_str(), host::u256_to_dec(a.x.c1.to_std()).c_str(),
           host::u256_to_dec(a.y.c0.to_std()).c_str(), host::u256_to_dec(a.y.c1.to_std()).c_str());
  }
  if (ovr.events) print_events();
  return 0;
}
