// The device pipeline of a proof and its helpers (see device_pipeline.hpp).
#include "device_pipeline.hpp"

#include <sched.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <future>
#include <type_traits>

#include "qap.hpp"

namespace zkp {

// ------------------------------------------------------------------ shared helpers

template <class F>
static F f_from_dev(const uint32_t* w) {
  if constexpr (std::is_same_v<F, HFq2>) return HFq2{host::fq_from_dev(w), host::fq_from_dev(w + 8)};
  else return host::fq_from_dev(w);
}

template <class F>
Jac<F> msm_fold(const uint32_t* win, const MsmParams& p) {
  constexpr int FW = sizeof(F) == sizeof(HFq) ? 8 : 16;
  auto load = [&](size_t k) {
    const uint32_t* q = win + k * 4 * FW;
    return host::jac_from_xyzz(f_from_dev<F>(q), f_from_dev<F>(q + FW), f_from_dev<F>(q + 2 * FW),
                               f_from_dev<F>(q + 3 * FW));
  };
  // sub-group s (K points): sum_p T_p + M sum_b 2^b Q_b; group g: its column sums' sub-group plus V times
  // its row sums'
  const int K = p.K(), lgP = p.lgP();
  auto sub = [&](int s) {
    Jac<F> acc = lgP > 0 ? load((size_t)s * K + lgP - 1) : Jac<F>::inf();
    for (int b = lgP - 2; b >= 0; --b) acc = host::jac_add(host::jac_dbl(acc), load((size_t)s * K + b));
    for (int i = 0; i < p.lg_m(); ++i) acc = host::jac_dbl(acc);
    return host::jac_add(acc, load((size_t)s * K + lgP));
  };
  auto group = [&](int g) {
    Jac<F> acc = sub(2 * g);
    for (int i = 0; i < p.lgV(); ++i) acc = host::jac_dbl(acc);
    return host::jac_add(acc, sub(2 * g + 1));
  };
  Jac<F> r = group(p.groups - 1);
  for (int g = p.groups - 2; g >= 0; --g) {
    for (int i = 0; i < p.c * p.depth; ++i) r = host::jac_dbl(r);
    r = host::jac_add(r, group(g));
  }
  return r;
}
template Jac<HFq> msm_fold<HFq>(const uint32_t*, const MsmParams&);
template Jac<HFq2> msm_fold<HFq2>(const uint32_t*, const MsmParams&);

void put_fq(const HFq& x, uint8_t* out) { host::u256_to_le(x.to_std(), out); }

bool jac_to_bytes_g1(const Jac<HFq>& p, uint8_t* out) {
  std::memset(out, 0, 64);
  auto a = host::jac_to_aff(p);
  if (!a.inf) put_fq(a.x, out), put_fq(a.y, out + 32);
  return !a.inf;
}
bool jac_to_bytes_g2(const Jac<HFq2>& p, uint8_t* out) {
  std::memset(out, 0, 128);
  auto a = host::jac_to_aff(p);
  if (!a.inf) put_fq(a.x.c0, out), put_fq(a.x.c1, out + 32), put_fq(a.y.c0, out + 64), put_fq(a.y.c1, out + 96);
  return !a.inf;
}

// host cores this process may use: the affinity mask, capped by a cgroup v2 CPU quota (the GPU boxes
// show 256 CPUs to nproc but allow 16)
static int host_cores() {
  static const int n = [] {
    int c = (int)std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) c = CPU_COUNT(&set);
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char q[32] = {0};
      long per = 0;
      if (std::fscanf(f, "%31s %ld", q, &per) == 2 && std::strcmp(q, "max") != 0 && per > 0) {
        const long quota = std::atol(q);
        if (quota > 0) c = std::min(c, (int)std::max(1L, (quota + per / 2) / per));
      }
      std::fclose(f);
    }
    return std::max(1, c);
  }();
  return n;
}

int env_int(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return (v && *v) ? std::atoi(v) : dflt;
}

int env_int_range(const char* name, int dflt, int lo, int hi) {
  const char* v = std::getenv(name);
  if (!v || !*v) return dflt;
  char* stop = nullptr;
  const long x = std::strtol(v, &stop, 10);
  if (*stop || x < lo || x > hi)
    throw ZkpError(ZKP_ERR_INVALID_ARG, std::string(name) + ": an integer within " + std::to_string(lo) + ".." +
                                            std::to_string(hi) + " (got '" + v + "')");
  return (int)x;
}

MsmOptions msm_options() {
  MsmOptions o;
  const char* e = std::getenv("ZKP_MSM");
  if (!e) return o;
  std::string spec(e);
  size_t at = 0;
  while (at < spec.size()) {
    size_t end = spec.find(',', at);
    if (end == std::string::npos) end = spec.size();
    const std::string item = spec.substr(at, end - at);
    at = end + 1;
    if (item.empty()) continue;
    const size_t eq = item.find('=');
    if (eq == std::string::npos) throw ZkpError(ZKP_ERR_INVALID_ARG, "ZKP_MSM: '" + item + "' is not key=value");
    const std::string key = item.substr(0, eq), val = item.substr(eq + 1);
    if (key == "plan") {
      if (val != "dense" && val != "compact") throw ZkpError(ZKP_ERR_INVALID_ARG, "ZKP_MSM: plan=dense|compact");
      o.dense = val == "dense" ? 1 : 0;
      continue;
    }
    if (key == "wsel") {
      if (val != "first" && val != "second" && val != "auto")
        throw ZkpError(ZKP_ERR_INVALID_ARG, "ZKP_MSM: wsel=first|second|auto");
      o.wsel = val == "first" ? 1 : (val == "second" ? 2 : 0);
      continue;
    }
    if (key == "sparse") {
      if (val != "0" && val != "1") throw ZkpError(ZKP_ERR_INVALID_ARG, "ZKP_MSM: sparse=0|1");
      o.sparse = val == "1" ? 1 : 0;
      continue;
    }
    if (key == "share" || key == "cgate") {
      if (val != "0" && val != "1") throw ZkpError(ZKP_ERR_INVALID_ARG, "ZKP_MSM: " + key + "=0|1");
      (key == "share" ? o.share : o.cgate) = val == "1" ? 1 : 0;
      continue;
    }
    char* stop = nullptr;
    const long v = std::strtol(val.c_str(), &stop, 10);
    if (val.empty() || *stop || v <= 0 || v > (1 << 20))
      throw ZkpError(ZKP_ERR_INVALID_ARG, "ZKP_MSM: bad value in '" + item + "'");
    int* dst = key == "w" ? &o.w : key == "h" ? &o.h : key == "depth" ? &o.depth : key == "task_w" ? &o.task_w
             : key == "task_h" ? &o.task_h : key == "seg" ? &o.seg : key == "w2" ? &o.w2
             : key == "wsets" ? &o.wsets : nullptr;
    if (!dst) throw ZkpError(ZKP_ERR_INVALID_ARG, "ZKP_MSM: unknown key '" + key + "'");
    if (key == "seg" && (v & (v - 1))) throw ZkpError(ZKP_ERR_INVALID_ARG, "ZKP_MSM: seg must be a power of two");
    if (key == "wsets" && v > 2) throw ZkpError(ZKP_ERR_INVALID_ARG, "ZKP_MSM: wsets=1|2");
    *dst = (int)v;
  }
  return o;
}

MsmParams make_params(size_t n, int c, int depth, int scalar_bits) {
  try {
    return MsmParams::make(n, c, depth, scalar_bits);
  } catch (const std::invalid_argument& x) {
    throw ZkpError(ZKP_ERR_INVALID_ARG, x.what());
  }
}

void apply_task_options(MsmParams& p, int task, const MsmOptions& o) {
  p.S = task > 0 ? task : 48;
  if (o.seg > 0 && o.seg <= p.V()) p.M = o.seg;
}

// MSM parameters for a prover: window bits automatic (ZKP_MSM w= / h= override); table depth = W
// (one bucket set) unless the tables would not fit in half of the free HBM, then the largest depth
// that does (ZKP_MSM depth= overrides).
static void choose_msm_params(size_t n_w, size_t n_h, const MsmOptions& o, MsmParams& pw, MsmParams& ph) {
  // measured on the Venmo shape (273c6e8:tools/gpu/experiments/sweep_c2.sh): the witness MSMs (70 % of the
  // digits of a 0/1-heavy witness are single entries) prefer one bit less than lg n - 4, the
  // uniform-scalar H MSM one bit more (fewer windows; the bucket reduction is cheap), moved off the
  // widths whose top window collapses into a few buckets (dense_window_bits)
  const int cw = o.w ? o.w : std::min(20, std::max(8, lg_ceil(n_w) - 5));
  const int ch = o.h ? o.h : h_window_bits(n_h);
  auto tune = [&] { apply_task_options(pw, o.task_w, o), apply_task_options(ph, o.task_h, o); };
  pw = make_params(n_w, cw, o.depth);
  ph = make_params(n_h, ch, o.depth);
  tune();
  if (o.depth > 0) return;
  size_t free_b = 0, total_b = 0;
  HIPX(hipMemGetInfo(&free_b, &total_b));
  const size_t row_w = n_w * (3 * 64 + 128), row_h = n_h * 64;
  const size_t budget = free_b / 2;
  int depth = std::max(pw.windows, ph.windows);
  while (depth > 1 && (size_t)std::min(depth, pw.windows) * row_w + (size_t)std::min(depth, ph.windows) * row_h > budget)
    --depth;
  pw = make_params(n_w, cw, depth);
  ph = make_params(n_h, ch, depth);
  tune();
}

void fill_bases(MsmBases& b, const uint8_t* src, size_t count, size_t at, hipStream_t st) {
  const size_t pw = b.curve() == Curve::G1 ? 16 : 32;  // words per point
  if (at) HIPX(hipMemsetAsync(b.row0(), 0, at * pw * 4, st));  // leading infinity points
  if (count) {
    HIPX(hipMemcpyAsync(b.row0() + at * pw, src, count * pw * 4, hipMemcpyHostToDevice, st));
    launch_convert_fq_zkey(b.row0() + at * pw, count * pw / 8, st);
  }
  b.extend(st);
}

// [lo, hi) of slice `part` when n items are cut into nparts contiguous ranges.  With
// ZKP_SPLIT_BALANCE=1 (a split proof with the distributed quotient) and G = nparts > 3, the parts
// that extend a quotient vector (0..2: rank v % G extends vector v) get weight max(1, 11 - G) and
// the others 11: with one coset extension costing r = 1/8 of the proof's MSM work M (S24: ~6.6 of
// ~53 ms), Q + M s_q = M s_o and 3 s_q + (G - 3) s_o = 1 give s_q = (11 - G) / (8 G),
// s_o = 11 / (8 G).  lo = n W_<k / W in integers (zkp_amd.dist.split_range and
// oracle.groth16.split_range compute the same).
static void split_range(size_t n, int part, int nparts, size_t& lo, size_t& hi) {
  const char* e = std::getenv("ZKP_SPLIT_BALANCE");
  if (!(e && std::atoi(e) == 1) || nparts <= 3) {
    lo = n * (size_t)part / (size_t)nparts;
    hi = n * (size_t)(part + 1) / (size_t)nparts;
    return;
  }
  const size_t wq = (size_t)std::max(1, 11 - nparts);
  auto cum = [&](int k) { return wq * (size_t)std::min(k, 3) + (size_t)11 * (size_t)std::max(k - 3, 0); };
  const size_t total = cum(nparts);
  lo = n * cum(part) / total;
  hi = n * cum(part + 1) / total;
}

// ------------------------------------------------------------------ device pipeline

DevicePipeline::DevicePipeline(int dev, const ZkeyParsed& z, int part, int nparts, const DevicePipeline* share)
    : dev_(dev), hdr_(z.hdr) {
  HIPX(hipSetDevice(dev_));
  // s0 carries the critical path (quotient -> H plan -> H MSM): highest priority, so the
  // A/B1/C (s2) and B2 (s1) MSMs fill the CUs it leaves idle instead of delaying it
  int prio_lo = 0, prio_hi = 0;
  HIPX(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  s0_ = Stream(hipStreamNonBlocking, prio_hi);
  s1_ = Stream(hipStreamNonBlocking, prio_lo);
  s2_ = Stream(hipStreamNonBlocking, prio_lo);
  // s3 runs every MSM's finish (merges + reduction: short latency-bound launches) at high
  // priority, so they slip in between the long accumulations instead of queueing behind them
  s3_ = Stream(hipStreamNonBlocking, prio_hi);
  for (int i = 0; i < EV_COUNT; ++i) ev_[i] = Event(i != EV_G2_ACC);
  const ZkeyHeader& h = hdr_;
  const size_t nd_all = h.domain_size, c0 = (size_t)h.n_public + 1;  // first witness index with a C base
  split_range(h.n_vars, part, nparts, wlo_, whi_);
  split_range(h.domain_size, part, nparts, hlo_, hhi_);
  const size_t nv = whi_ - wlo_, nd = hhi_ - hlo_;
  const MsmOptions opt = msm_options();
  MsmParams pw, ph;
  choose_msm_params(nv, nd, opt, pw, ph);
  wsel_opt_ = opt.wsel;
  sparse_ = opt.sparse != 0;
  share_ = opt.share != 0;
  cgate_ = opt.cgate != 0;
  // base tables: A, B1, C, B2 indexed by witness signal (C's first nPublic+1 bases are
  // infinity, so one witness plan serves all four), H by domain index
  auto build_wtables = [&](WSet& w) {
    w.ta = std::make_shared<MsmBases>(Curve::G1, nv, w.pw.c, w.pw.depth);
    w.tb1 = std::make_shared<MsmBases>(Curve::G1, nv, w.pw.c, w.pw.depth);
    w.tc = std::make_shared<MsmBases>(Curve::G1, nv, w.pw.c, w.pw.depth);
    w.tb2 = std::make_shared<MsmBases>(Curve::G2, nv, w.pw.c, w.pw.depth);
    fill_bases(*w.ta, z.bf.sec[5].ptr + wlo_ * 64, nv, 0, s0_);
    fill_bases(*w.tb1, z.bf.sec[6].ptr + wlo_ * 64, nv, 0, s0_);
    fill_bases(*w.tb2, z.bf.sec[7].ptr + wlo_ * 128, nv, 0, s0_);
    const size_t cfirst = std::max(wlo_, c0);  // first witness index of the slice with a C base
    const size_t lead = std::min(cfirst, whi_) - wlo_;
    const size_t cnt = whi_ > cfirst ? whi_ - cfirst : 0;
    fill_bases(*w.tc, cnt ? z.bf.sec[8].ptr + (cfirst - c0) * 64 : nullptr, cnt, lead, s0_);
    w.mb = std::make_shared<BaseMask>(mask_union(*w.tb1, *w.tb2, s0_));
    // the shared build's membership table, for the plans build_engines will make: one per slot with a
    // mask, and one for the slots without (the first of them)
    if (sparse_ && share_) {
      const uint32_t* bits[NPLAN] = {w.mb->data(), w.ta->present(), w.tc->present()};
      const size_t cnt[NPLAN] = {w.mb->count, w.ta->present_count(), w.tc->present_count()};
      bool use[NPLAN], unmasked = false;
      int nuse = 0;
      for (int p = 0; p < NPLAN; ++p) {
        use[p] = bits[p] || !unmasked;
        if (!bits[p]) unmasked = true;
        nuse += use[p];
      }
      if (nuse > 1) w.memb = std::make_shared<PlanMembership>(plan_membership(bits, cnt, use, nv, s0_));
    }
  };
  if (share) {
    if (share->dev_ != dev_ || share->wlo_ != wlo_ || share->whi_ != whi_ || share->hlo_ != hlo_ ||
        share->hhi_ != hhi_)
      throw ZkpError(ZKP_ERR_INTERNAL, "shared base tables of another device or slice");
    nws_ = share->wset2_tables_ ? 2 : 1;
    for (int k = 0; k < nws_; ++k) {
      const WSet& o = share->ws_[k];
      ws_[k].pw = o.pw, ws_[k].ta = o.ta, ws_[k].tb1 = o.tb1, ws_[k].tc = o.tc, ws_[k].tb2 = o.tb2;
      ws_[k].mb = o.mb, ws_[k].memb = o.memb;
    }
    th_ = share->th_;
    // the H plan and engine must read th_ with the parameters it was built with: a sibling's own
    // choose_msm_params can pick another depth when less HBM is free by now
    ph = share->plan_h_->params();
    if (th_->c() != ph.c || th_->depth() != ph.depth)
      throw ZkpError(ZKP_ERR_INTERNAL, "shared H table built with other parameters");
  } else {
    ws_[0].pw = pw;
    build_wtables(ws_[0]);
    th_ = std::make_shared<MsmBases>(Curve::G1, nd, ph.c, ph.depth);
    fill_bases(*th_, z.bf.sec[9].ptr + hlo_ * 64, nd, 0, s0_);
    // the second witness configuration (round 5): c = w + 2 bits, one bucket set,
    // for witnesses whose values are mostly >= 2^32 (all-uniform: c = 20 is ~7 % faster than 18 on the
    // Venmo shape, profiles/wsweep_r04.txt); full provers only, and only where its tables fit in half
    // of the HBM still free (the Venmo key: +26.6 GB)
    const int c2 = opt.w2 ? opt.w2 : std::min(24, pw.c + 2);
    if (nparts == 1 && opt.wsets == 2 && c2 != pw.c) {
      HIPX(hipStreamSynchronize(s0_));
      size_t free_b = 0, total_b = 0;
      HIPX(hipMemGetInfo(&free_b, &total_b));
      const MsmParams p2 = make_params(nv, c2, 0);
      if ((size_t)p2.windows * nv * (3 * 64 + 128) <= free_b / 2) {
        ws_[1].pw = make_params(nv, c2, p2.windows);
        apply_task_options(ws_[1].pw, opt.task_w, opt);
        build_wtables(ws_[1]);
        nws_ = 2;
      }
    }
  }
  for (int m = 0; m < 2; ++m) {
    const Csr& c = z.csr[m];
    rowptr_[m] = DevBuf<>(c.rowptr.size());
    HIPX(hipMemcpyAsync(rowptr_[m], c.rowptr.data(), c.rowptr.size() * 4, hipMemcpyHostToDevice, s0_));
    col_[m] = DevBuf<>(std::max<size_t>(c.col.size(), 1));
    val_[m] = DevBuf<>(std::max<size_t>(c.val.size(), 8));
    if (!c.col.empty()) {
      HIPX(hipMemcpyAsync(col_[m], c.col.data(), c.col.size() * 4, hipMemcpyHostToDevice, s0_));
      HIPX(hipMemcpyAsync(val_[m], c.val.data(), c.val.size() * 4, hipMemcpyHostToDevice, s0_));
      launch_convert_coefs(val_[m], c.col.size(), s0_);
    }
  }
  // witness upload slots: each has its own copy stream, so a proof's
  // witness H2D runs outside the compute lock and overlaps the proof in flight, and its own pinned
  // staging buffer and copy threads (upload()); allocated on the slot's first host-witness upload
  // (ensure_upload_slot) except slot 0 of a device's first full pipeline (below), so split provers and
  // staged-only sibling pipelines hold no pinned staging or copy threads
  for (auto& b : abc_) b = DevBuf<>(nd_all * 8);
  pscal_ = DevBuf<>(nd_all * 8);
  ntt_ = std::make_unique<NttEngine>((int)h.log_domain, s0_);
  // the witness plan feeds A/B1/C on s2 and B2 on s1; they overlap the quotient on s0, which then
  // plans and runs the H MSM.  The witness plan runs on the high-priority finish stream s3 (ahead
  // of its G1 finishes), so its sort passes are not starved by the quotient's NTTs on s0: the
  // witness accumulations start ~5 ms earlier; proof 26.69 -> 26.58 ms (profiles/wplan_r03.txt)
  nv_ = nv;
  build_engines(ws_[0]);
  plan_h_ = std::make_unique<MsmPlan>(nd, ph, s0_);
  // H scalars are uniform (quotient evaluations): dense plan (one workgroup per sub-bin)
  plan_h_->set_dense(true);
  g1h_ = std::make_unique<MsmEngine>(Curve::G1, ph, nd, s0_);
  winh_ = g1h_->window_words();
  // the second witness configuration's plan and engines (~6 GB at the Venmo shape) come later
  // (add_second_wset), after every pipeline of the prover holds its essentials; the group-sum slots
  // are sized for both
  wset2_tables_ = nws_ > 1;
  nws_ = 1;
  wina_ = ws_[0].g1[0]->window_words();
  win2_ = ws_[0].g2->window_words();
  if (wset2_tables_) {
    const MsmParams& p2 = ws_[1].pw;
    wina_ = std::max(wina_, MsmEngine::window_words_for(Curve::G1, p2));
    win2_ = std::max(win2_, MsmEngine::window_words_for(Curve::G2, p2));
  }
  dwin_ = DevBuf<>(win_total());
  hwin_ = PinnedBuf<uint32_t>(win_total());
  // a full prover's first upload slot exists from load on, so a one-shot prover's first host-witness
  // proof does not pay its ~410 MB of HBM, ~220 MB of pinned memory, streams and copy threads, and an
  // out-of-memory surfaces here rather than at prove time; the second slot stays lazy, and
  // so does every slot of a pipeline that shares another one's tables (ZKP_INFLIGHT siblings, the
  // repeated ordinals of a rehearsal: their HBM goes to the second witness configuration first)
  if (nparts == 1 && !share) ensure_upload_slot(0);
  HIPX(hipStreamSynchronize(s0_));
}

void DevicePipeline::build_engines(WSet& w) {
  const bool sp = sparse_;
  w.mask[PL_B] = sp ? w.mb->list() : nullptr;
  w.mask[PL_A] = sp ? w.ta->present_index() : nullptr;
  w.mask[PL_C] = sp ? w.tc->present_index() : nullptr;
  w.present[PL_B] = w.mask[PL_B] ? w.mb->count : nv_;
  w.present[PL_A] = w.mask[PL_A] ? w.ta->present_count() : nv_;
  w.present[PL_C] = w.mask[PL_C] ? w.tc->present_count() : nv_;
  // the sort's scratch (16 of a plan's ~20 bytes per entry) once, sized for the fullest plan; every
  // plan's own outputs by its mask's count
  // (a shared build sorts the union of the plans' signals: nearly the fullest plan's, C's, at the Venmo key)
  const bool shared = sp && share_ && w.memb;
  w.shared_build = shared;
  const size_t most = std::max(w.present[PL_B], std::max(w.present[PL_A], w.present[PL_C]));
  auto scratch = std::make_shared<MsmSortScratch>(
      nv_, shared ? (w.memb->any.bits ? w.memb->any.count : nv_) : most, w.pw, shared ? (int)NPLAN : 1);
  for (int p = 0; p < NPLAN; ++p) {
    w.plan[p] = nullptr;
    for (int q = 0; q < p && !w.mask[p]; ++q)
      if (!w.mask[q]) {
        w.plan[p] = w.plan[q];
        break;
      }
    if (w.plan[p]) continue;
    w.own[p] = std::make_unique<MsmPlan>(nv_, w.pw, s3_, w.present[p], scratch);
    w.plan[p] = w.own[p].get();
  }
  for (auto& g : w.g1) g = std::make_unique<MsmEngine>(Curve::G1, w.pw, nv_, s2_);
  w.g2 = std::make_unique<MsmEngine>(Curve::G2, w.pw, nv_, s1_);
}

void DevicePipeline::add_second_wset() {
  if (!wset2_tables_ || nws_ > 1) return;
  HIPX(hipSetDevice(dev_));
  try {
    build_engines(ws_[1]);
    nws_ = 2;
  } catch (const HipError& e) {
    if (e.code != hipErrorOutOfMemory) throw;
    (void)hipGetLastError();
    ws_[1].drop_engines();
  }
}

int DevicePipeline::acquire_upload() {
  std::unique_lock<std::mutex> lk(upmu_);
  upcv_.wait(lk, [&] {
    for (bool b : upbusy_)
      if (!b) return true;
    return false;
  });
  for (int k = 0; k < NUP; ++k)
    if (!upbusy_[k]) {
      upbusy_[k] = true;
      return k;
    }
  return 0;  // unreachable
}

void DevicePipeline::ensure_upload_slot(int k) {
  if (up_[k]) return;
  const size_t stage_words = std::max<size_t>(wt_chunks(hdr_.n_vars), 1) * wt_chunk_words();
  // (each piece only if missing: a failed first attempt leaves no leak behind the next one)
  if (!upstage_[k]) upstage_[k] = DevBuf<>(stage_words);
  if (!uph_[k]) uph_[k] = PinnedBuf<uint8_t>(stage_words * 4);
  if (!sup_[k]) sup_[k] = Stream(hipStreamNonBlocking);
  for (int j = 0; j + 1 < NDMA; ++j) {
    if (!sdma_[k][j]) sdma_[k][j] = Stream(hipStreamNonBlocking);
    if (!evdma_[k][j]) evdma_[k][j] = Event(false);
  }
  for (auto& t : copiers_[k])
    if (!t) t = std::make_unique<JobThread>();
  up_[k] = DevBuf<>(std::max<size_t>((size_t)hdr_.n_vars * 8, 8));  // last: marks the slot ready
}

float DevicePipeline::upload(int k, const WtnsView& w, uint64_t* pcie_bytes) {
  HIPX(hipSetDevice(dev_));
  const auto t0 = std::chrono::steady_clock::now();
  ensure_upload_slot(k);
  const uint32_t n = hdr_.n_vars;
  const uint32_t nch = wt_chunks(n);
  const size_t chw = wt_chunk_words();
  const uint8_t* src = w.values;
  uint32_t* pin = reinterpret_cast<uint32_t*>(uph_[k].get());
  hipStream_t st = sup_[k];
  std::exception_ptr errs[NCOPY];
  std::atomic<uint64_t> sent{0};
  std::atomic<uint32_t> large{0};
  // encode threads: every usable host core for a lone upload (the single-proof latency path), the
  // cores shared out among concurrent uploads (an 8-GPU batch has up to 16 at once: 8 groups of 16
  // threads encode 705 Venmo witnesses/s on a 16-core quota, of 2 threads 1,096/s;
  // profiles/host_capacity_r05.json)
  struct Active {
    Active() { ++uploads_active_; }
    ~Active() { --uploads_active_; }
  } active;
  const int T = std::max(2, std::min(NCOPY, host_cores() / std::max(1, uploads_active_.load())));
  // chunk c's DMA goes to stream c % NDMA: one copy queue serialises the ~100 chunk copies with
  // ~10 us between them (rocprofv3 --memory-copy-trace: 2.7 ms for 62 MB), parallel queues overlap
  // those gaps and each other's transfers
  auto dma_stream = [&](uint32_t c) { return (c % NDMA) == 0 ? st : sdma_[k][c % NDMA - 1].get(); };
  auto part = [&](int t) {
    try {
      HIPX(hipSetDevice(dev_));
      uint32_t nl = 0;
      for (uint32_t c = (uint32_t)t; c < nch; c += (uint32_t)T) {
        const size_t words = wt_encode_chunk(src, n, c, pin + (size_t)c * chw, &nl);
        HIPX(hipMemcpyAsync(upstage_[k] + (size_t)c * chw, pin + (size_t)c * chw, words * 4, hipMemcpyHostToDevice,
                            dma_stream(c)));
        sent += words * 4;
      }
      large += nl;
    } catch (...) {
      errs[t] = std::current_exception();
    }
  };
  for (int t = 1; t < T; ++t) copiers_[k][t - 1]->start([&, t] { part(t); });
  part(0);
  for (int t = 1; t < T; ++t) copiers_[k][t - 1]->wait();
  for (auto& e : errs)
    if (e) {
      (void)hipStreamSynchronize(st);
      for (int j = 0; j + 1 < NDMA; ++j) (void)hipStreamSynchronize(sdma_[k][j]);
      std::rethrow_exception(e);
    }
  // one expansion after every chunk's DMA has been enqueued (the other copy queues joined by events
  // recorded here, after every encode thread has enqueued its copies)
  for (int j = 0; j + 1 < NDMA; ++j) {
    HIPX(hipEventRecord(evdma_[k][j], sdma_[k][j]));
    HIPX(hipStreamWaitEvent(st, evdma_[k][j], 0));
  }
  launch_witness_unpack(upstage_[k], 0, n, up_[k], st);
  HIPX(hipStreamSynchronize(st));
  if (pcie_bytes) *pcie_bytes = sent.load();
  up_large_[k] = n ? (double)large.load() / n : 0.0;
  return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

DevicePipeline::MsmOut DevicePipeline::prove_uploaded(int k, float h2d_ms, const EarlyFn& early) {
  std::lock_guard<std::mutex> lk(mu_);
  HIPX(hipSetDevice(dev_));
  maybe_inject_fault();
  record_no_transfer();
  MsmOut o = prove_dev(up_[k], early, pick_wset(up_large_[k]));
  o.ms[0] = h2d_ms;
  return o;
}

void DevicePipeline::enqueue_quotient(const uint32_t* d_wit) {
  const ZkeyHeader& h = hdr_;
  launch_build_abc(rowptr_[0], col_[0], val_[0], rowptr_[1], col_[1], val_[1], d_wit, h.domain_size, abc_[0],
                   abc_[1], abc_[2], s0_);
  HIPX(hipEventRecord(ev_[EV_ABC], s0_));
  // one vector per launch, not coset_extend_batch: the batched passes (3x the workgroups at s0's
  // high priority) finish the quotient ~1.8 ms sooner but crowd out the G2 and witness
  // accumulations that fill the per-vector launches' last-round gaps -- -4 % proofs/s, +0.5 ms
  // latency on one box, 4 alternating rounds (profiles/ntt_batch_ab_r04.txt)
  for (auto& b : abc_) ntt_->coset_extend(b);
  launch_join_abc(abc_[0], abc_[1], abc_[2], h.domain_size, pscal_, s0_);
  HIPX(hipEventRecord(ev_[EV_QUOT], s0_));
}

void DevicePipeline::stage(int slot, const WtnsView& w) {
  std::lock_guard<std::mutex> lk(mu_);
  HIPX(hipSetDevice(dev_));
  if (slot < 0 || slot > 4096) throw ZkpError(ZKP_ERR_INVALID_ARG, "bad staging slot");
  if ((size_t)slot >= slots_.size()) slots_.resize(slot + 1);
  if (!slots_[slot]) slots_[slot] = DevBuf<>((size_t)hdr_.n_vars * 8);
  if ((size_t)slot >= slot_large_.size()) slot_large_.resize(slot + 1, 0.0);
  HIPX(hipMemcpyAsync(slots_[slot], w.values, (size_t)hdr_.n_vars * 32, hipMemcpyHostToDevice, s0_));
  // the share of values >= 2^32 (pick_wset), counted while the copy runs
  size_t nl = 0;
  for (size_t i = 0; i < hdr_.n_vars; ++i) {
    const uint8_t* v = w.values + 32 * i;
    uint32_t w1;
    uint64_t hi[3];
    std::memcpy(&w1, v + 4, 4);
    std::memcpy(hi, v + 8, 24);
    nl += (w1 | hi[0] | hi[1] | hi[2]) != 0;
  }
  slot_large_[slot] = hdr_.n_vars ? (double)nl / hdr_.n_vars : 0.0;
  HIPX(hipStreamSynchronize(s0_));
}

void DevicePipeline::set_instrument(bool on) {
  std::lock_guard<std::mutex> lk(mu_);
  for (int k = 0; k < nws_; ++k) {
    for (auto& g : ws_[k].g1) g->set_instrument(on);
    ws_[k].g2->set_instrument(on);
  }
  g1h_->set_instrument(on);
  stats_g1_ = MsmEngine::Stats{};
  stats_g2_ = MsmEngine::Stats{};
  launches_.clear();
}

void DevicePipeline::collect_kind(MsmEngine& e, int kind, MsmEngine::Stats& agg) {
  MsmEngine::Stats s;
  e.collect(s);
  agg.accumulate_ms += s.accumulate_ms, agg.launches += s.launches, agg.mixed_adds += s.mixed_adds;
  agg.tasks += s.tasks;
  for (const auto& l : s.per_launch)
    if (launches_.size() < 65536) launches_.push_back({(double)kind, (double)l.adds, (double)l.ms, (double)l.blocks});
}

void DevicePipeline::quotient(const WtnsView& w, uint8_t* out) {
  UploadSlot slot(this);
  upload(slot.k, w);
  std::lock_guard<std::mutex> lk(mu_);
  HIPX(hipSetDevice(dev_));
  enqueue_quotient(up_[slot.k]);
  HIPX(hipMemcpyAsync(out, pscal_, (size_t)hdr_.domain_size * 32, hipMemcpyDeviceToHost, s0_));
  HIPX(hipStreamSynchronize(s0_));
}

void DevicePipeline::quotient_part_staged(int slot, int mask, void* const* dst) {
  std::shared_lock<std::shared_mutex> sl(stage_mu_);
  std::lock_guard<std::mutex> lk(mu_);
  HIPX(hipSetDevice(dev_));
  const uint32_t* d = slot_ptr(slot);
  const ZkeyHeader& h = hdr_;
  launch_build_abc(rowptr_[0], col_[0], val_[0], rowptr_[1], col_[1], val_[1], d, h.domain_size, abc_[0], abc_[1],
                   abc_[2], s0_);
  uint32_t* sel[3];
  int cnt = 0;
  for (int v = 0; v < 3; ++v) {
    if (!(mask >> v & 1)) continue;
    if (!dst[v]) throw ZkpError(ZKP_ERR_INVALID_ARG, "quotient part: null destination");
    sel[cnt++] = abc_[v];
  }
  if (cnt) ntt_->coset_extend_batch(sel, cnt);
  for (int v = 0; v < 3; ++v)
    if (mask >> v & 1)
      HIPX(hipMemcpyAsync(dst[v], abc_[v], (size_t)h.domain_size * 32, hipMemcpyDeviceToDevice, s0_));
  HIPX(hipStreamSynchronize(s0_));
}

DevicePipeline::MsmOut DevicePipeline::prove_ext_staged(int slot, const void* const* abc) {
  std::shared_lock<std::shared_mutex> sl(stage_mu_);
  std::lock_guard<std::mutex> lk(mu_);
  HIPX(hipSetDevice(dev_));
  const uint32_t* d = slot_ptr(slot);
  for (int v = 0; v < 3; ++v)
    if (!abc[v]) throw ZkpError(ZKP_ERR_INVALID_ARG, "partial prove: null quotient slice");
  record_no_transfer();
  for (int v = 0; v < 3; ++v) ext_abc_[v] = static_cast<const uint32_t*>(abc[v]);
  struct ClearExt {  // ext_abc_ is set for this proof only, however it ends
    const uint32_t** p;
    ~ClearExt() { p[0] = p[1] = p[2] = nullptr; }
  } clear_ext{ext_abc_};
  return prove_dev(d);
}

DevicePipeline::MsmOut DevicePipeline::prove(const WtnsView& w, const EarlyFn& early) {
  UploadSlot slot(this);
  uint64_t bytes = 0;
  const float ms = upload(slot.k, w, &bytes);
  MsmOut o = prove_uploaded(slot.k, ms, early);
  o.pcie_mb = (float)(bytes * 1e-6);
  return o;
}

DevicePipeline::MsmOut DevicePipeline::prove_staged(int slot, const EarlyFn& early) {
  std::shared_lock<std::shared_mutex> sl(stage_mu_);
  return prove_resident(slot_ptr(slot), early, slot_large(slot));
}

DevicePipeline::MsmOut DevicePipeline::prove_resident(const uint32_t* d_wit, const EarlyFn& early, double large_frac) {
  std::lock_guard<std::mutex> lk(mu_);
  HIPX(hipSetDevice(dev_));
  record_no_transfer();
  return prove_dev(d_wit, early, pick_wset(large_frac));
}

void DevicePipeline::record_no_transfer() {
  HIPX(hipEventRecord(ev_[EV_H2D_BEGIN], s0_));
  HIPX(hipEventRecord(ev_[EV_H2D_END], s0_));
}

struct DevicePipeline::ProofRun {
  WSet& ws;  // the witness configuration the proof takes
  int wset;
  const uint32_t* d_wit;
  uint32_t *wa, *wh, *wb2;  // the group sums' slots in dwin_: A | B1 | C, H, B2
  int g2first;              // g2first_, off under ZKP_SERIAL
  bool cgate;               // cgate_, off under ZKP_SERIAL
  // opened by enqueue_g1 once plan B is enqueued, by enqueue_g2 once EV_G2_ACC is recorded (g2first)
  // and by enqueue_h once EV_QUOT is recorded (cgate)
  Gate planned, g2acc, quot;
  std::exception_ptr err[3];  // of enqueue_g1, enqueue_g2, enqueue_h
};

// s3: the witness plans B, A, C (one per mask of finite bases, each MSM takes its table's).  With
// ZKP_MSM share=1 (default) ONE build fills the three plans (MsmPlan::build_shared), so all are ready
// before the quotient ends; share=0 builds B, A, C back to back.
// s2: the G1 accumulations A, B1, C back to back; s3 finishes each (merges + reduction: latency-bound
// chains) while s2 accumulates the next.  A starts when the G2 accumulation ends: the G2 finish (a
// latency-bound chain on the low-priority s1) then runs beside A, B1 and C instead of waiting out the
// H accumulation and sharing the proof's tail with the H finish (+0.4 %, 7 of 8 alternated pairs:
// profiles/g2_first_ab_r06.txt).  cgate=1 holds C's accumulation until the quotient is done (EV_QUOT).
void DevicePipeline::enqueue_g1(ProofRun& r) {
  WSet& ws = r.ws;
  try {
    HIPX(hipSetDevice(dev_));
    HIPX(hipStreamWaitEvent(s2_, ev_[EV_H2D_END], 0));
    HIPX(hipEventRecord(ev_[EV_G1_BEGIN], s2_));
    HIPX(hipStreamWaitEvent(ws.plan[PL_B]->stream(), ev_[EV_H2D_END], 0));
    if (ws.shared_build) {  // one build fills every plan
      MsmPlan* own[NPLAN];
      for (int p = 0; p < NPLAN; ++p) own[p] = ws.own[p].get();
      MsmPlan::build_shared(own, r.d_wit + wlo_ * 8, whi_ - wlo_, *ws.memb);
      r.planned.open();
    } else {
      for (int p = 0; p < NPLAN; ++p) {
        if (ws.own[p]) ws.own[p]->build(r.d_wit + wlo_ * 8, whi_ - wlo_, ws.mask[p], ws.present[p]);
        if (p == PL_B) r.planned.open();
      }
    }
    const MsmBases* tabs[3] = {ws.ta.get(), ws.tb1.get(), ws.tc.get()};
    const MsmPlan* plans[3] = {ws.plan[PL_A], ws.plan[PL_B], ws.plan[PL_C]};
    for (int m = 0; m < 3; ++m) {
      if (r.g2first && m == r.g2first - 1) {
        r.g2acc.wait();
        HIPX(hipStreamWaitEvent(s2_, ev_[EV_G2_ACC], 0));
      }
      if (r.cgate && m == 2) {  // C fills the window of the H plan's sort
        r.quot.wait();
        HIPX(hipStreamWaitEvent(s2_, ev_[EV_QUOT], 0));
      }
      ws.g1[m]->accumulate(*plans[m], *tabs[m]);
      HIPX(hipEventRecord(ev_[EV_ACC_A + m], s2_));
      HIPX(hipStreamWaitEvent(s3_, ev_[EV_ACC_A + m], 0));
      ws.g1[m]->finish(*plans[m], r.wa + m * wina_, s3_);
      if (serial_) {  // profiling: no overlap between the finish and the next accumulation
        HIPX(hipEventRecord(ev_[EV_FINISH], s3_));
        HIPX(hipStreamWaitEvent(s2_, ev_[EV_FINISH], 0));
      }
    }
    HIPX(hipEventRecord(ev_[EV_G1_END], s3_));
  } catch (...) {
    r.err[0] = std::current_exception();
    r.planned.fail(r.err[0]);
  }
}

// s1: the G2 MSM B2 on plan B, once that plan is enqueued (s1 then waits on its ready()): the G2
// accumulation comes first in the proof
void DevicePipeline::enqueue_g2(ProofRun& r) {
  WSet& ws = r.ws;
  try {
    r.planned.wait();
    HIPX(hipSetDevice(dev_));
    if (serial_) HIPX(hipStreamWaitEvent(s1_, ev_[EV_G1_END], 0));
    HIPX(hipEventRecord(ev_[EV_G2_BEGIN], s1_));
    // the finish on s1 too: s3 is in-order, the G1 finishes must not queue behind it (gating the
    // G2 finish on the H plan, on either stream, measured +0.9 ms: profiles/g2_finish_r03.txt)
    ws.g2->accumulate(*ws.plan[PL_B], *ws.tb2);
    if (r.g2first) {
      HIPX(hipEventRecord(ev_[EV_G2_ACC], s1_));
      r.g2acc.open();
    }
    ws.g2->finish(*ws.plan[PL_B], r.wb2, s1_);
    HIPX(hipEventRecord(ev_[EV_G2_END], s1_));
  } catch (...) {
    r.err[1] = std::current_exception();
    r.g2acc.fail(r.err[1]);
  }
}

// s0: quotient (buildABC, 3 coset NTTs, joinABC), H plan, H MSM
void DevicePipeline::enqueue_h(ProofRun& r) {
  try {
    if (serial_) HIPX(hipStreamWaitEvent(s0_, ev_[EV_G2_END], 0));
    if (ext_abc_[0]) {  // distributed quotient: only the join of this domain slice
      HIPX(hipEventRecord(ev_[EV_ABC], s0_));
      launch_join_abc(ext_abc_[0], ext_abc_[1], ext_abc_[2], (uint32_t)(hhi_ - hlo_), pscal_ + hlo_ * 8, s0_);
      HIPX(hipEventRecord(ev_[EV_QUOT], s0_));
    } else {
      enqueue_quotient(r.d_wit);
    }
    r.quot.open();
    plan_h_->build(pscal_ + hlo_ * 8, hhi_ - hlo_);
    g1h_->run(*plan_h_, *th_, r.wh);
  } catch (...) {
    r.err[2] = std::current_exception();
    r.quot.fail(r.err[2]);
  }
}

DevicePipeline::MsmOut DevicePipeline::prove_dev(const uint32_t* d_wit, const EarlyFn& early, int wsel) {
  const int wset = wsel < nws_ ? wsel : 0;
  // group-sum layout in dwin_ (slots sized for the larger witness configuration): A | B1 | C
  // (engines ws.g1) | H (g1h) | B2 (ws.g2)
  uint32_t* wh = dwin_ + 3 * wina_;
  ProofRun r{ws_[wset], wset, d_wit, dwin_, wh, wh + winh_, serial_ ? 0 : g2first_, !serial_ && cgate_};
  // Nothing here blocks on the device (a plan's exact digit count stays there), but a proof enqueues
  // a few hundred launches, so each stream is fed from its own host thread; the G2 thread starts first
  // and waits for plan B to be enqueued.  ZKP_SERIAL=1 (profiling only) chains the three streams so
  // every kernel runs alone.
  if (serial_) {
    enqueue_g1(r);
    if (!r.err[0]) enqueue_g2(r);
    if (!r.err[0] && !r.err[1]) enqueue_h(r);
  } else {
    jt_g2_.start([&] { enqueue_g2(r); });
    jt_g1_.start([&] { enqueue_g1(r); });
    enqueue_h(r);
    jt_g1_.wait();
    jt_g2_.wait();
  }
  for (auto& e : r.err)
    if (e) {
      (void)hipDeviceSynchronize();  // let every enqueued kernel drain before buffers are reused
      std::rethrow_exception(e);
    }
  return collect_proof(r, early);
}

DevicePipeline::MsmOut DevicePipeline::collect_proof(const ProofRun& r, const EarlyFn& early) {
  WSet& ws = r.ws;
  HIPX(hipEventRecord(ev_[EV_H_END], s0_));
  // the witness MSMs' group sums (A | B1 | C, B2) go to the host as soon as their finishes end
  // (s3 holds the G1 finishes; it waits for the G2 finish), so the host folds them and the caller
  // blinds A, B and the r/s part of C (`early`) while the H MSM still runs; only C + H, the
  // affine conversions and the H fold remain after the device is done
  HIPX(hipStreamWaitEvent(s3_, ev_[EV_G2_END], 0));
  HIPX(hipMemcpyAsync(hwin_, dwin_, 3 * wina_ * 4, hipMemcpyDeviceToHost, s3_));
  HIPX(hipMemcpyAsync(hwin_ + 3 * wina_ + winh_, r.wb2, ws.g2->window_words() * 4, hipMemcpyDeviceToHost, s3_));
  HIPX(hipEventRecord(ev_[EV_WIT_COPIED], s3_));
  HIPX(hipMemcpyAsync(hwin_ + 3 * wina_, r.wh, winh_ * 4, hipMemcpyDeviceToHost, s0_));
  HIPX(hipEventRecord(ev_[EV_H_COPIED], s0_));
  MsmOut o;
  const MsmParams& pa = ws.g1[0]->params();
  const MsmParams& ph = g1h_->params();
  HIPX(hipEventSynchronize(ev_[EV_WIT_COPIED]));
  o.a = msm_fold<HFq>(hwin_, pa);
  o.b1 = msm_fold<HFq>(hwin_ + wina_, pa);
  o.c = msm_fold<HFq>(hwin_ + 2 * wina_, pa);
  o.b2 = msm_fold<HFq2>(hwin_ + 3 * wina_ + winh_, pa);
  if (early) {
    try {
      early(o);
    } catch (...) {
      (void)hipStreamSynchronize(s0_);  // the H MSM and its copy still run: drain before rethrowing
      (void)hipStreamSynchronize(s3_);
      throw;
    }
  }
  HIPX(hipStreamSynchronize(s0_));
  HIPX(hipStreamSynchronize(s3_));
  for (int m = 0; m < 3; ++m) collect_kind(*ws.g1[m], m, stats_g1_);
  collect_kind(*g1h_, 3, stats_g1_);
  collect_kind(*ws.g2, 4, stats_g2_);
  o.wset = r.wset;
  o.h = msm_fold<HFq>(hwin_ + 3 * wina_, ph);
  HIPX(hipEventElapsedTime(&o.ms[0], ev_[EV_H2D_BEGIN], ev_[EV_H2D_END]));  // wtns H2D
  HIPX(hipEventElapsedTime(&o.ms[1], ev_[EV_H2D_END], ev_[EV_ABC]));  // buildABC
  HIPX(hipEventElapsedTime(&o.ms[2], ev_[EV_ABC], ev_[EV_QUOT]));  // NTT + join
  HIPX(hipEventElapsedTime(&o.ms[3], ev_[EV_G1_BEGIN], ev_[EV_G1_END]));  // witness plan + G1 MSMs A, B1, C (s2)
  HIPX(hipEventElapsedTime(&o.ms[4], ev_[EV_G2_BEGIN], ev_[EV_G2_END]));  // G2 MSM (s1)
  HIPX(hipEventElapsedTime(&o.ms[5], ev_[EV_QUOT], ev_[EV_H_END]));  // H plan + G1 MSM H (s0)
  return o;
}

}  // namespace zkp
