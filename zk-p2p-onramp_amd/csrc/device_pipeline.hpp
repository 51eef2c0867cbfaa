// The device side of one proof: DevicePipeline (one per device and proof in flight: base tables,
// streams, plans, engines, buffers, witness upload slots) and the helpers it shares with the Prover
// (prover.hip) and the kernel-level entry points (kernel_api.hip).
#pragma once
#include <array>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <vector>

#include "hip_check.hpp"
#include "hip_raii.hpp"
#include "prover.hpp"

namespace zkp {

using host::Affine;
using host::Jac;
using host::U256;
using HFq = host::Fq;
using HFq2 = host::Fq2;
using HFr = host::Fr;

// ------------------------------------------------------------------ shared helpers

// fold an MSM engine output (device XYZZ layout, G x K points: per group the lgP subset
// sums Q_b then sum_p T_p) into the MSM value:
//   R_g = sum_p T_p + M * sum_b 2^b Q_b,   result = sum_g 2^(c T g) R_g   (Horner both)
// (F = HFq for G1, HFq2 for G2)
template <class F>
Jac<F> msm_fold(const uint32_t* win, const MsmParams& p);

// standard-form LE encodings: a field element (32 bytes), an affine point (64 / 128 bytes; the point
// at infinity is all zero and returns false)
void put_fq(const HFq& x, uint8_t* out);
bool jac_to_bytes_g1(const Jac<HFq>& p, uint8_t* out);
bool jac_to_bytes_g2(const Jac<HFq2>& p, uint8_t* out);

int env_int(const char* name, int dflt);
// the same for a knob with a range: anything but an integer within [lo, hi] is a ZKP_ERR_INVALID_ARG
int env_int_range(const char* name, int dflt, int lo, int hi);

// MSM tuning options: ONE environment variable read when a prover (or a kernel-level MSM) is built,
// ZKP_MSM = "key=value[,key=value...]" (empty / unset: automatic everything):
//   w=<bits>  h=<bits>    window bits of the witness plan / the H plan and the kernel-level MSMs (8..24)
//   depth=<rows>          base-table rows T per point (1..W; default W, or the largest depth whose
//                         tables fit half of the free HBM)
//   task_w=<n> task_h=<n> entries per bucket-accumulation task of either plan (default 48 / 48)
//   seg=<n>               buckets per bucket-reduction segment (a power of two; default 4)
//   plan=dense|compact    the plan variant of the kernel-level MSMs (zkp_msm_*; default dense)
// A malformed value or an unknown key is a ZKP_ERR_INVALID_ARG: a typo never silently tunes nothing.
//   w2=<bits>             window bits of the second witness plan (default w + 2; full provers only)
//   wsets=1|2             witness-MSM configurations kept resident (default 2: w and w2)
//   wsel=first|second|auto  which one a proof takes (default auto: by the witness's share of values
//                         >= 2^32, DevicePipeline::pick_wset)
//   sparse=0|1            1 (default): a scalar whose base is the point at infinity emits no digit -- a
//                         prover builds one witness plan per distinct mask of finite bases (B1 and B2
//                         share one); 0: one unmasked witness plan for all four MSMs
//   share=0|1             1 (default): a proof's witness plans come from ONE build (MsmPlan::build_shared:
//                         the digits computed and sorted once, every entry tagged with its plans); 0: one
//                         build per plan, back to back
//   cgate=0|1             1: the witness accumulation C starts only when the quotient is done (it fills the
//                         window of the H plan's sort); 0 (default): as soon as its plan is ready
struct MsmOptions {
  int w = 0, h = 0, depth = 0, task_w = 0, task_h = 0, seg = 0, w2 = 0, wsets = 2;
  int dense = 1;
  int wsel = 0;  // 0 auto, 1 first, 2 second
  int sparse = 1;
  int share = 1;
  int cgate = 0;
};
MsmOptions msm_options();

// MsmParams::make with its std::invalid_argument as a ZKP_ERR_INVALID_ARG
MsmParams make_params(size_t n, int c, int depth, int scalar_bits = 255);

// the task size (task = the plan's task_w / task_h option, 0: the default of 48 entries) and the
// reduction segment (seg=) of a plan.
// H-plan tasks of <= 48 entries (the uniform quotient scalars fill every bucket evenly, ~208 entries at
// the Venmo shape: 5 task partials per bucket instead of 7, so the latency-bound merge_final at the end
// of the proof folds fewer): +0.7 % and +0.9 % proofs/s over 32, 7 of 7 alternated rounds on two boxes
// (profiles/task_size_ab_r05.txt).  Witness-plan tasks of <= 48 too since the G2 accumulation runs first
// (round 6): +0.6 / +1.0 % over 32 on two boxes, every alternated pair; 96 ties, 128 and 192 lose
// (profiles/task_w_ab_r06.txt)
void apply_task_options(MsmParams& p, int task, const MsmOptions& o);

// upload `count` zkey points (snarkjs LEM layout) into row 0 of a base table at point
// offset `at`, convert to the device Montgomery form, then derive the shifted rows
void fill_bases(MsmBases& b, const uint8_t* src, size_t count, size_t at, hipStream_t st);

// A long-lived host thread that runs one job at a time (the per-proof G1 / G2 enqueue jobs of a
// pipeline: no thread creation on the proof's critical path)
class JobThread {
 public:
  JobThread() : th_([this] { loop(); }) {}
  ~JobThread() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    th_.join();
  }
  void start(std::function<void()> f) {
    {
      std::lock_guard<std::mutex> lk(m_);
      job_ = std::move(f);
      done_ = false;
    }
    cv_.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [&] { return done_; });
  }

 private:
  void loop() {
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
      cv_.wait(lk, [&] { return stop_ || job_; });
      if (!job_) return;  // stop with no job pending
      std::function<void()> f = std::move(job_);
      job_ = nullptr;
      lk.unlock();
      f();  // the jobs catch their own exceptions
      lk.lock();
      done_ = true;
      cv_.notify_all();
    }
  }
  std::mutex m_;
  std::condition_variable cv_;
  std::function<void()> job_;
  bool stop_ = false, done_ = true;
  std::thread th_;  // last: started once the state above exists
};

// A one-shot hand-off between two of a proof's host threads: the consumer's wait() blocks until the
// producer opens the gate, or rethrows what the producer failed it with.  fail() after open() does
// nothing: a producer that throws once the consumer may run keeps the error to itself.
class Gate {
 public:
  void open() { p_.set_value(), opened_ = true; }
  void fail(const std::exception_ptr& e) {
    if (!opened_) p_.set_exception(e);
  }
  void wait() { f_.get(); }

 private:
  std::promise<void> p_;
  std::shared_future<void> f_ = p_.get_future().share();
  bool opened_ = false;
};

// ------------------------------------------------------------------ device pipeline

class DevicePipeline {
 public:
  // part / nparts: this pipeline holds only slice `part` of every point section (the
  // point-range split of one proof over several GPUs); 0 / 1 = all
  // share: another pipeline of the same device and slice whose base tables (the ~38 GB of
  // precomputed points) this one uses instead of building its own (ZKP_INFLIGHT > 1: several
  // proofs in flight per device, each with its own streams, plans, engines and buffers)
  DevicePipeline(int dev, const ZkeyParsed& z, int part = 0, int nparts = 1, const DevicePipeline* share = nullptr);
  // the members release themselves in reverse order of declaration: the streams last
  ~DevicePipeline() { (void)hipSetDevice(dev_); }

  // the second witness configuration's plan and engines, this pipeline's own: with many pipelines on
  // one GPU (ZKP_INFLIGHT, a multi-device rehearsal) HBM can run out here, and the pipeline then keeps
  // the first configuration only (the shared tables stay).  Called by the Prover once every pipeline
  // is built.
  void add_second_wset();

  struct MsmOut {
    Jac<HFq> a, b1, c, h;
    Jac<HFq2> b2;
    float ms[6];
    float pcie_mb = 0;  // witness transfer payload (prove() from a host witness)
    int wset = 0;       // the witness configuration the proof took (pick_wset)
  };
  // called with a, b1, c, b2 folded (h not yet) while the H MSM still runs on the device
  using EarlyFn = std::function<void(const MsmOut&)>;

  // ---- witness upload slots.  acquire_upload() blocks until one of the NUP slots is free;
  // upload() copies a witness into it (the calling thread waits for it, the compute streams do
  // not); prove_uploaded() then runs the proof on it under the compute lock.  Two callers (two
  // zkp_prove threads, or the two batch workers of a device) thus overlap one proof's upload with
  // the other's compute.
  int acquire_upload();
  void release_upload(int k) {
    {
      std::lock_guard<std::mutex> lk(upmu_);
      upbusy_[k] = false;
    }
    upcv_.notify_one();
  }
  struct UploadSlot {  // RAII: one acquired upload slot
    DevicePipeline* d;
    int k;
    explicit UploadSlot(DevicePipeline* dp) : d(dp), k(dp->acquire_upload()) {}
    ~UploadSlot() { d->release_upload(k); }
  };
  // the resources of upload slot k, created on its first use (the caller holds slot k)
  void ensure_upload_slot(int k);
  // H2D of a witness (pageable host memory, 32 B per signal) into slot k.  PCIe is the limit (a
  // 205 MB witness: ~4.3 ms at ~48 GB/s through pinned memory), so the transfer is COMPACT: NCOPY
  // host threads encode chunks of 64K signals (qap.hpp WT_*: per block of 64, the values >= 2^32 as
  // 32 B, the others as their low word, plus a 12-byte block meta) straight into the slot's pinned
  // buffer and enqueue each chunk's DMA (pinned -> HBM staging, the slot's copy stream) as soon as it
  // is encoded, so encoding and PCIe overlap; one kernel then expands the chunks into the 32-B
  // witness layout.  A 0/1-heavy witness moves ~2.5x fewer bytes; an all-uniform one as many plus the
  // meta.  Returns the wall time (ms).
  float upload(int k, const WtnsView& w, uint64_t* pcie_bytes = nullptr);
  MsmOut prove_uploaded(int k, float h2d_ms, const EarlyFn& early = {});
  // test hook (ZKP_TEST_FAIL, read by Prover): this pipeline
  // reports a device failure on its (after+1)-th proof and every later one
  void set_fault_injection(int after) { fail_after_ = after; }
  bool healthy() const { return healthy_.load(); }
  void mark_failed() { healthy_.store(false); }
  int device() const { return dev_; }

  // quotient (rows A4..A8) from a device-resident witness; result scalars in pscal_
  void enqueue_quotient(const uint32_t* d_wit);

  // keep a witness resident in HBM slot `slot` (benchmarks: timing without PCIe)
  // Staging slots are written under stage_mu_ held exclusively, and read (slot lookup AND the whole
  // proof that reads the slot, on this pipeline or a ZKP_INFLIGHT sibling) under stage_mu_ shared:
  // restaging waits for the proofs that read the old witness.  Lock order: stage_mu_, then mu_.
  std::unique_lock<std::shared_mutex> lock_stage() { return std::unique_lock<std::shared_mutex>(stage_mu_); }
  void stage(int slot, const WtnsView& w);  // caller holds lock_stage()
  double slot_large(int slot) const {       // caller holds the staging lock (shared)
    return slot >= 0 && (size_t)slot < slot_large_.size() ? slot_large_[slot] : 0.0;
  }
  const uint32_t* slot_ptr(int slot) const {
    if (slot < 0 || (size_t)slot >= slots_.size() || !slots_[slot])
      throw ZkpError(ZKP_ERR_INVALID_ARG, "staging slot is empty");
    return slots_[slot];
  }

  void set_instrument(bool on);
  void stats(MsmEngine::Stats& g1, MsmEngine::Stats& g2) {
    std::lock_guard<std::mutex> lk(mu_);
    g1 = stats_g1_;
    g2 = stats_g2_;
  }
  // every instrumented accumulate launch since set_instrument(true): {kind, adds, ms}, kind 0..2 the
  // witness MSMs A, B1, C (G1), 3 the H MSM (G1), 4 the witness MSM B2 (G2)
  void launch_records(std::vector<std::array<double, 4>>& out) {
    std::lock_guard<std::mutex> lk(mu_);
    out.insert(out.end(), launches_.begin(), launches_.end());
  }
  void msm_params(MsmParams& pw, MsmParams& ph, MsmParams* pw2 = nullptr) const {
    pw = ws_[0].pw;
    ph = plan_h_->params();
    if (pw2) *pw2 = nws_ > 1 ? ws_[1].pw : MsmParams{};
  }
  int witness_sets() const { return nws_; }
  size_t table_bytes() const {
    size_t b = th_->bytes();
    for (int k = 0; k < (wset2_tables_ ? 2 : 1); ++k)  // resident tables, whether or not this pipeline's engines use them
      b += ws_[k].ta->bytes() + ws_[k].tb1->bytes() + ws_[k].tc->bytes() + ws_[k].tb2->bytes();
    return b;
  }
  // the witness configuration a proof takes: the second (wider windows) when the witness's share of
  // values >= 2^32 is above WSET2_LARGE_FRAC (each such value carries a digit in every window; 0/1 and
  // other small values only one or two), unless ZKP_MSM wsel= fixes it
  int pick_wset(double large_frac) const {
    if (nws_ < 2 || wsel_opt_ == 1) return 0;
    if (wsel_opt_ == 2) return 1;
    return large_frac > WSET2_LARGE_FRAC ? 1 : 0;
  }
  static constexpr double WSET2_LARGE_FRAC = 0.55;

  void quotient(const WtnsView& w, uint8_t* out);

  // Distributed quotient of a split proof, stage 1: buildABC on the
  // witness in `slot`, then the coset extension (rows A5-A7) of the vectors in mask (bit 0
  // A, 1 B, 2 C) only, each copied whole (domain x 32 bytes, device layout: Montgomery
  // 2^261, 8 packed words) to dst[v], device memory on this device.  Returns when done.
  void quotient_part_staged(int slot, int mask, void* const* dst);

  // stage 2: this slice's partial sums with the H scalars joined (row A8) from abc[0..2] =
  // the coset evaluations of A, B, C at this part's domain slice (device memory, ready)
  MsmOut prove_ext_staged(int slot, const void* const* abc);

  MsmOut prove(const WtnsView& w, const EarlyFn& early = {});

  MsmOut prove_staged(int slot, const EarlyFn& early = {});
  // shared hold of this (first) pipeline's staging slots for a proof that reads one of them
  std::shared_lock<std::shared_mutex> hold_stage() { return std::shared_lock<std::shared_mutex>(stage_mu_); }

  // a proof of a witness already resident on this GPU: this pipeline's staging slot, or a
  // ZKP_INFLIGHT sibling's (staged witnesses live in the device's first pipeline)
  MsmOut prove_resident(const uint32_t* d_wit, const EarlyFn& early = {}, double large_frac = 0.0);
  // claimed by a staged caller (Prover::prove_staged spreads concurrent callers over the pipelines)
  std::atomic<bool> staged_busy{false};

  // the whole device pipeline on a resident witness (caller holds mu_, EV_H2D_BEGIN / _END recorded):
  // starts the three enqueue jobs (enqueue_g1, enqueue_g2, enqueue_h), then collect_proof
  MsmOut prove_dev(const uint32_t* d_wit, const EarlyFn& early = {}, int wsel = 0);

 private:
  int dev_;
  size_t wlo_ = 0, whi_ = 0, hlo_ = 0, hhi_ = 0;  // witness / domain slice held by this pipeline
  bool serial_ = env_int("ZKP_SERIAL", 0) == 1;  // profiling: no stream overlap
  ZkeyHeader hdr_;
  Stream s0_, s1_, s2_, s3_;  // first: destroyed after everything enqueued on them
  // g2first_ = k: witness accumulation k - 1 (1: the first, A) waits for EV_G2_ACC; ZKP_G2FIRST=0 lets
  // A, B1, C run beside the G2 accumulation from the start
  int g2first_ = env_int_range("ZKP_G2FIRST", 1, 0, 3);
  // ZKP_MSM cgate=1: the last witness accumulation (C) waits for EV_QUOT, so it runs in the window of the
  // H plan's sort instead of beside the quotient's NTTs; 0: as soon as its plan is ready
  bool cgate_ = false;
  // a proof's events: the stage times of MsmOut::ms are differences of the timed ones
  enum Ev {
    EV_H2D_BEGIN,  // s0, recorded by the caller of prove_dev: the witness transfer (ms[0])
    EV_H2D_END,    // s0: start of the proof; s2 and the witness plan's stream wait for it
    EV_ABC,        // s0: buildABC done (ms[1])
    EV_QUOT,       // s0: coset NTTs + joinABC done (ms[2]); the H plan and MSM follow (ms[5])
    EV_H_END,      // s0: H MSM done
    EV_H_COPIED,   // s0: H group sums on the host
    EV_G2_END,     // s1: G2 MSM done (ms[4]); s3's copy of the witness MSMs' sums waits for it
    EV_G2_BEGIN,   // s1
    EV_G1_END,     // s3: the last G1 witness finish (ms[3])
    EV_G1_BEGIN,   // s2
    EV_ACC_A,      // s2: accumulation A, B1, C done (the next two too); its finish on s3 waits for it
    EV_ACC_B1,
    EV_ACC_C,
    EV_FINISH,      // s3: a G1 finish done (ZKP_SERIAL only: the next accumulation waits for it)
    EV_WIT_COPIED,  // s3: A, B1, C, B2 group sums on the host
    EV_G2_ACC,      // s1, no timing: the G2 accumulation's end (g2first_)
    EV_COUNT
  };
  Event ev_[EV_COUNT];
  JobThread jt_g1_, jt_g2_;  // host threads feeding s2 (witness plan, G1 MSMs) and s1 (G2 MSM)
  // one witness-MSM configuration: window bits, base tables and the mask of the bases finite in B1 or
  // B2 (shared by the pipelines of one device), plans and engines (per pipeline).  A witness plan per
  // distinct mask of finite bases, in the order the accumulations take them: B (B2 then B1), A, C;
  // tables without a mask (and all of them under ZKP_MSM sparse=0) share one unmasked plan.  The
  // plans share the sort's scratch on one stream: one shared build fills them all (ZKP_MSM share=1), or
  // they build back to back (share=0).
  enum { PL_B, PL_A, PL_C, NPLAN };
  struct WSet {
    MsmParams pw;
    std::shared_ptr<MsmBases> ta, tb1, tc, tb2;
    std::shared_ptr<BaseMask> mb;
    // which plans each signal belongs to and the signals of any (ZKP_MSM share=1 with more than one plan)
    std::shared_ptr<PlanMembership> memb;
    std::unique_ptr<MsmPlan> own[NPLAN];  // own[p]: built for slot p (null: slot p uses an earlier one)
    MsmPlan* plan[NPLAN] = {};            // the plan each slot takes
    const uint32_t* mask[NPLAN] = {};  // each slot's index list of finite bases (null: no mask)
    size_t present[NPLAN] = {};
    bool shared_build = false;  // one MsmPlan::build_shared fills the plans (sparse, share=1 and a membership table)
    std::unique_ptr<MsmEngine> g1[3], g2;  // g1: A, B1, C
    void drop_engines() {
      for (int p = 0; p < NPLAN; ++p) own[p].reset(), plan[p] = nullptr;
      for (auto& g : g1) g.reset();
      g2.reset();
    }
  };
  WSet ws_[2];
  int nws_ = 1, wsel_opt_ = 0;
  bool sparse_ = true;         // ZKP_MSM sparse=
  bool share_ = true;          // ZKP_MSM share=
  bool wset2_tables_ = false;  // this device holds the second configuration's tables (add_second_wset)
  size_t nv_ = 0;              // witness signals of this pipeline's slice
  void build_engines(WSet& w);
  // one proof's enqueue state (device_pipeline.hip) and its three jobs, one per host thread and stream
  // family: the witness plans and the G1 MSMs A, B1, C (s3, s2), the G2 MSM B2 (s1), the quotient and
  // the H MSM (s0).  Each records its own failure in the proof's err[] slot.
  struct ProofRun;
  void enqueue_g1(ProofRun& r);
  void enqueue_g2(ProofRun& r);
  void enqueue_h(ProofRun& r);
  // what follows the jobs: the group sums to the host, the folds (`early` once A, B1, C, B2 are
  // folded), the engines' statistics and the stage times
  MsmOut collect_proof(const ProofRun& r, const EarlyFn& early);
  // EV_H2D_BEGIN / _END of a proof without a witness transfer
  void record_no_transfer();
  std::shared_ptr<MsmBases> th_;  // shared by the pipelines of one device
  DevBuf<> rowptr_[2], col_[2], val_[2];
  static constexpr int NUP = 2;    // witness upload slots (double buffering)
  static constexpr int NCOPY = 16;  // host threads per upload at most (compact encoding into pinned memory, DMA enqueues)
  static inline std::atomic<int> uploads_active_{0};  // uploads in progress in this process (all pipelines)
  DevBuf<> up_[NUP];              // the witness slots (32 B per signal)
  DevBuf<> upstage_[NUP];         // compact chunk regions (HBM)
  PinnedBuf<uint8_t> uph_[NUP];   // pinned staging of each slot: compact chunk regions

  Stream sup_[NUP];
  static constexpr int NDMA = 4;  // copy queues per upload slot (sup_ and NDMA - 1 more)
  Stream sdma_[NUP][NDMA > 1 ? NDMA - 1 : 1];
  Event evdma_[NUP][NDMA > 1 ? NDMA - 1 : 1];
  std::unique_ptr<JobThread> copiers_[NUP][NCOPY - 1];  // after the slot's streams: joined before those go
  std::mutex upmu_;
  std::condition_variable upcv_;
  bool upbusy_[NUP] = {false, false};
  std::atomic<bool> healthy_{true};
  int fail_after_ = -1, proofs_done_ = 0;
  void maybe_inject_fault() {
    if (fail_after_ >= 0 && proofs_done_++ >= fail_after_) {
      healthy_.store(false);
      throw HipError(hipErrorLaunchFailure, "injected device failure (ZKP_TEST_FAIL)", __FILE__, __LINE__);
    }
  }
  DevBuf<> abc_[3];
  DevBuf<> pscal_;
  const uint32_t* ext_abc_[3] = {nullptr, nullptr, nullptr};  // set only inside prove_ext_staged
  std::unique_ptr<NttEngine> ntt_;
  std::unique_ptr<MsmPlan> plan_h_;
  std::unique_ptr<MsmEngine> g1h_;
  size_t wina_ = 0, winh_ = 0, win2_ = 0;  // group-sum slot sizes (max over the witness configurations)
  size_t win_total() const { return 3 * wina_ + winh_ + win2_; }
  DevBuf<> dwin_;
  PinnedBuf<uint32_t> hwin_;
  std::mutex mu_;
  std::shared_mutex stage_mu_;  // staging slots (see stage())
  std::vector<DevBuf<>> slots_;
  std::vector<double> slot_large_;     // per staging slot: share of witness values >= 2^32
  double up_large_[NUP] = {0.0, 0.0};  // per upload slot, of the witness last uploaded
  MsmEngine::Stats stats_g1_, stats_g2_;
  std::vector<std::array<double, 4>> launches_;  // {kind, adds, ms, workgroups} per instrumented launch (capped)
  void collect_kind(MsmEngine& e, int kind, MsmEngine::Stats& agg);
};

}  // namespace zkp
