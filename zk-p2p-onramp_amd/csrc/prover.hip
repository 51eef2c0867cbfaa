// Groth16 prover core (see prover.hpp).
#include "prover.hpp"

#include <sys/random.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <thread>

#include "device_pipeline.hpp"
#include "host_pairing.hpp"

namespace zkp {

// parsing (parse_binfile, parse_wtns, parse_zkey): zkey_parse.cpp, host-only (sanitizer-tested)

static U256 scalar_or_random(const uint8_t* s32) {
  U256 v;
  if (s32) {
    v = host::u256_from_le(s32);
    while (host::u256_geq(v, host::FR_DESC.mod)) host::u256_sub(v, host::FR_DESC.mod);
    return v;
  }
  for (;;) {
    uint8_t b[32];
    size_t got = 0;
    while (got < 32) {
      ssize_t k = getrandom(b + got, 32 - got, 0);
      if (k <= 0) throw ZkpError(ZKP_ERR_INTERNAL, "getrandom failed");
      got += (size_t)k;
    }
    b[31] &= 0x3f;  // 254 bits
    v = host::u256_from_le(b);
    if (!host::u256_geq(v, host::FR_DESC.mod)) return v;
  }
}

// ------------------------------------------------------------------ Prover

Prover::Prover(const uint8_t* zkey, size_t len, const std::vector<int>& devices, int part, int nparts)
    : part_(part), nparts_(nparts) {
  if (nparts < 1 || part < 0 || part >= nparts) throw ZkpError(ZKP_ERR_INVALID_ARG, "bad part / nparts");
  if (nparts > 1 && devices.size() > 1) throw ZkpError(ZKP_ERR_INVALID_ARG, "a partial prover runs on one device");
  ZkeyParsed z = parse_zkey(zkey, len);
  hdr_ = z.hdr;
  int ndev = 0;
  HIPX(hipGetDeviceCount(&ndev));
  if (ndev <= 0) throw ZkpError(ZKP_ERR_DEVICE, "no HIP device available");
  std::vector<int> devs = devices.empty() ? std::vector<int>{0} : devices;
  // ZKP_INFLIGHT = k > 1: k pipelines per device sharing its base tables, so zkp_prove_batch
  // (one worker per pipeline) and concurrent zkp_prove callers keep k proofs in flight per GPU
  // devs_ holds inflight_ consecutive pipelines per entry of `devices`; the staged entry points'
  // dev_index names an entry of `devices` (its first pipeline).  An ordinal listed twice (a
  // multi-device rehearsal on one GPU) shares the base tables of its first listing.
  inflight_ = std::max(1, std::min(4, env_int("ZKP_INFLIGHT", 1)));
  for (int d : devs)
    if (d < 0 || d >= ndev) throw ZkpError(ZKP_ERR_INVALID_ARG, "device ordinal out of range");
  ndevices_ = (int)devs.size();
  devs_.resize((size_t)ndevices_ * inflight_);
  // the first listing of every ordinal builds its base tables (upload + row derivation, ~2 s
  // for the Venmo key): one host thread per GPU, so an 8-GPU load takes as long as one
  std::vector<int> owner(ndevices_, -1);  // entry whose tables entry e shares (-1: builds its own)
  for (int e = 0; e < ndevices_; ++e)
    for (int f = 0; f < e && owner[e] < 0; ++f)
      if (devs[f] == devs[e] && owner[f] < 0) owner[e] = f;
  {
    std::vector<std::exception_ptr> errs(ndevices_);
    std::vector<std::thread> th;
    for (int e = 0; e < ndevices_; ++e)
      if (owner[e] < 0)
        th.emplace_back([&, e] {
          try {
            devs_[(size_t)e * inflight_] = std::make_unique<DevicePipeline>(devs[e], z, part, nparts);
          } catch (...) {
            errs[e] = std::current_exception();
          }
        });
    for (auto& t : th) t.join();
    for (auto& x : errs)
      if (x) std::rethrow_exception(x);
  }
  for (int e = 0; e < ndevices_; ++e) {
    const DevicePipeline* first = devs_[(size_t)(owner[e] < 0 ? e : owner[e]) * inflight_].get();
    if (owner[e] >= 0) devs_[(size_t)e * inflight_] = std::make_unique<DevicePipeline>(devs[e], z, part, nparts, first);
    for (int k = 1; k < inflight_; ++k)
      devs_[(size_t)e * inflight_ + k] = std::make_unique<DevicePipeline>(devs[e], z, part, nparts, first);
  }
  for (auto& d : devs_) d->add_second_wset();
  // test hooks (never set in production): verify-before-return default, a corrupted H partial
  // (exercises verify-before-return), an injected device failure (exercises the batch re-queue)
  {
    const int v = env_int("ZKP_VERIFY", 2);
    verify_.store(v >= 0 && v <= 2 ? v : 2);
  }
  corrupt_h_ = env_int("ZKP_TEST_CORRUPT_H", 0);
  // ZKP_TEST_FAIL="<pipeline>:<after>": that pipeline reports a device failure from its (after+1)-th proof on
  if (const char* f = std::getenv("ZKP_TEST_FAIL")) {
    int fp = -1, after = 0;
    if (std::sscanf(f, "%d:%d", &fp, &after) == 2 && fp >= 0 && fp < (int)devs_.size())
      devs_[fp]->set_fault_injection(after);
  }
}

// next healthy pipeline in round-robin order (a pipeline that hit a HIP error is skipped)
DevicePipeline& Prover::pick_device() {
  const size_t nd = devs_.size();
  const unsigned start = rr_.fetch_add(1);
  for (size_t i = 0; i < nd; ++i) {
    DevicePipeline& d = *devs_[(start + i) % nd];
    if (d.healthy()) return d;
  }
  throw ZkpError(ZKP_ERR_DEVICE, "every device of this prover has failed");
}

Prover::~Prover() = default;

// a HIP error on one pipeline retires every pipeline of its device: the error may be sticky
// device state that the ZKP_INFLIGHT siblings share
// (a logical device = one entry of the device list and its inflight_ pipelines)
void Prover::retire_device(const DevicePipeline& failed) {
  size_t at = 0;
  while (at < devs_.size() && devs_[at].get() != &failed) ++at;
  const size_t first = at / inflight_ * inflight_;
  for (size_t i = first; i < first + inflight_ && i < devs_.size(); ++i) devs_[i]->mark_failed();
}

// snarkjs groth16_prove's blinding, in two phases: everything but piH
// (assemble_pre: runs while the H MSM is still on the device) and C + piH + the encoding.
struct Blinded {
  Jac<HFq> Cpart;  // piC' + s A + r B1 - (r s) delta1
  Affine<HFq> a;   // A and B are final here: converted to affine before piH exists
  Affine<HFq2> b;
};
static Blinded assemble_pre(const ZkeyHeader& h, const DevicePipeline::MsmOut& m, const uint8_t* r32,
                            const uint8_t* s32) {
  const U256 r = scalar_or_random(r32), s = scalar_or_random(s32);
  const Jac<HFq> alpha1 = host::jac_from_aff(h.alpha1), beta1 = host::jac_from_aff(h.beta1),
                 delta1 = host::jac_from_aff(h.delta1);
  const Jac<HFq2> beta2 = host::jac_from_aff(h.beta2), delta2 = host::jac_from_aff(h.delta2);
  Blinded o;
  // A = piA' + alpha1 + r delta1
  const Jac<HFq> A = host::jac_add(host::jac_add(m.a, alpha1), host::jac_mul(delta1, r));
  // B = piB' + beta2 + s delta2 ; B1 = piB1' + beta1 + s delta1
  const Jac<HFq2> B = host::jac_add(host::jac_add(m.b2, beta2), host::jac_mul(delta2, s));
  Jac<HFq> B1 = host::jac_add(host::jac_add(m.b1, beta1), host::jac_mul(delta1, s));
  // C = piC' + piH + s A + r B1 - (r s) delta1
  HFr rs = HFr::from_std(r) * HFr::from_std(s);
  U256 nrs = rs.neg().to_std();
  Jac<HFq> C = m.c;
  C = host::jac_add(C, host::jac_mul(A, s));
  C = host::jac_add(C, host::jac_mul(B1, r));
  o.Cpart = host::jac_add(C, host::jac_mul(delta1, nrs));
  o.a = host::jac_to_aff(A);
  o.b = host::jac_to_aff(B);
  return o;
}
static void assemble_post(const ZkeyHeader& h, const Blinded& bl, const Jac<HFq>& piH, const WtnsView& w,
                          zkp_proof* out) {
  const Affine<HFq>& a = bl.a;
  const Affine<HFq2>& b = bl.b;
  auto c = host::jac_to_aff(host::jac_add(bl.Cpart, piH));
  put_fq(a.x, out->pi_a[0]);
  put_fq(a.y, out->pi_a[1]);
  put_fq(b.x.c0, out->pi_b[0][0]);
  put_fq(b.x.c1, out->pi_b[0][1]);
  put_fq(b.y.c0, out->pi_b[1][0]);
  put_fq(b.y.c1, out->pi_b[1][1]);
  put_fq(c.x, out->pi_c[0]);
  put_fq(c.y, out->pi_c[1]);
  out->n_public = h.n_public;
  if (out->public_signals && out->public_capacity)
    std::memcpy(out->public_signals, w.values + 32, (size_t)std::min(h.n_public, out->public_capacity) * 32);
}
static void assemble(const ZkeyHeader& h, const DevicePipeline::MsmOut& m, const WtnsView& w, const uint8_t* r32,
                     const uint8_t* s32, zkp_proof* out) {
  assemble_post(h, assemble_pre(h, m, r32, s32), m.h, w, out);
}

// test hook ZKP_TEST_CORRUPT_H: the H MSM result off by one generator, as a silent device error would
static Jac<HFq> maybe_corrupt(const Jac<HFq>& h, bool on) {
  if (!on) return h;
  const Affine<HFq> g{HFq::one(), HFq::one() + HFq::one(), false};  // (1, 2)
  return host::jac_add(h, host::jac_from_aff(g));
}

float Prover::verify_or_throw(const WtnsView& w, const zkp_proof* out) const {
  const auto t0 = std::chrono::steady_clock::now();
  if (hdr_.ic.size() != (size_t)hdr_.n_public + 1)
    throw ZkpError(ZKP_ERR_FORMAT, "verify: the zkey has no IC section (nPublic + 1 points)");
  host::VerifyingKey vk;
  vk.alpha1 = hdr_.alpha1;
  vk.beta2 = hdr_.beta2;
  vk.gamma2 = hdr_.gamma2;
  vk.delta2 = hdr_.delta2;
  vk.ic = hdr_.ic.data();
  vk.n_public = (int)hdr_.n_public;
  std::vector<U256> pub(hdr_.n_public);
  for (uint32_t i = 0; i < hdr_.n_public; ++i) pub[i] = host::u256_from_le(w.values + 32 * (size_t)(i + 1));
  auto fq = [](const uint8_t* b) { return HFq::from_std(host::u256_from_le(b)); };
  const Affine<HFq> a{fq(out->pi_a[0]), fq(out->pi_a[1]), false};
  const Affine<HFq2> b{HFq2{fq(out->pi_b[0][0]), fq(out->pi_b[0][1])}, HFq2{fq(out->pi_b[1][0]), fq(out->pi_b[1][1])},
                       false};
  const Affine<HFq> c{fq(out->pi_c[0]), fq(out->pi_c[1]), false};
  if (!host::groth16_verify(vk, pub.data(), a, b, c))
    throw ZkpError(ZKP_ERR_INTERNAL,
                   "proof failed verify-before-return (pairing check against the zkey's verification key): not "
                   "returned; the device result is suspect");
  return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static WtnsView check_wtns(const ZkeyHeader& h, const uint8_t* wtns, size_t len) {
  WtnsView w = parse_wtns(wtns, len);
  if (w.n_witness != h.n_vars)
    throw ZkpError(ZKP_ERR_WITNESS_LENGTH, "Invalid witness length. Circuit: " + std::to_string(h.n_vars) +
                                               ", witness: " + std::to_string(w.n_witness));
  return w;
}

static bool all_zero(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (p[i]) return false;
  return true;
}
static HFq fq_from_std_bytes(const uint8_t* p) {
  U256 v = host::u256_from_le(p);
  if (host::u256_geq(v, host::FQ_DESC.mod)) throw ZkpError(ZKP_ERR_INVALID_ARG, "partial: coordinate out of range");
  return HFq::from_std(v);
}
static Jac<HFq> g1_from_bytes(const uint8_t* p) {
  if (all_zero(p, 64)) return Jac<HFq>::inf();
  return host::jac_from_aff(Affine<HFq>{fq_from_std_bytes(p), fq_from_std_bytes(p + 32), false});
}
static Jac<HFq2> g2_from_bytes(const uint8_t* p) {
  if (all_zero(p, 128)) return Jac<HFq2>::inf();
  return host::jac_from_aff(Affine<HFq2>{HFq2{fq_from_std_bytes(p), fq_from_std_bytes(p + 32)},
                                         HFq2{fq_from_std_bytes(p + 64), fq_from_std_bytes(p + 96)}, false});
}
static void msm_out_to_partial(const DevicePipeline::MsmOut& m, int part, int nparts, zkp_partial* out) {
  jac_to_bytes_g1(m.a, out->a);
  jac_to_bytes_g1(m.b1, out->b1);
  jac_to_bytes_g1(m.c, out->c);
  jac_to_bytes_g1(m.h, out->h);
  jac_to_bytes_g2(m.b2, out->b2);
  out->part = (uint32_t)part;
  out->nparts = (uint32_t)nparts;
}

// a proof's stage times into Prover::last_ms_ (the caller holds tmu_); host_ms = {host assembly, total
// wall, verify-before-return}, which stay as they are when not given
static void record_timings(float* last_ms, const DevicePipeline::MsmOut& m, const float* host_ms = nullptr) {
  for (int i = 0; i < 5; ++i) last_ms[i] = m.ms[i];
  last_ms[7] = m.ms[5];
  last_ms[9] = m.pcie_mb;
  last_ms[10] = (float)m.wset;
  if (host_ms) last_ms[5] = host_ms[0], last_ms[6] = host_ms[1], last_ms[8] = host_ms[2];
}

void Prover::require_full() const {
  if (nparts_ != 1)
    throw ZkpError(ZKP_ERR_INVALID_ARG, "this prover holds one point range (part " + std::to_string(part_) + " of " +
                                            std::to_string(nparts_) + "): use zkp_prove_partial + zkp_proof_combine");
}

void Prover::prove_partial(const uint8_t* wtns, size_t len, zkp_partial* out) {
  WtnsView w = check_wtns(hdr_, wtns, len);
  DevicePipeline::MsmOut m = devs_[0]->prove(w);
  msm_out_to_partial(m, part_, nparts_, out);
  std::lock_guard<std::mutex> lk(tmu_);
  record_timings(last_ms_, m);
}

void Prover::prove_partial_staged(int slot, zkp_partial* out) {
  DevicePipeline::MsmOut m = devs_[0]->prove_staged(slot);
  msm_out_to_partial(m, part_, nparts_, out);
  std::lock_guard<std::mutex> lk(tmu_);
  record_timings(last_ms_, m);
}

void Prover::quotient_part_staged(int slot, int mask, void* const* dst) {
  if (mask < 0 || mask > 7) throw ZkpError(ZKP_ERR_INVALID_ARG, "quotient part: mask must be within 0..7");
  devs_[0]->quotient_part_staged(slot, mask, dst);
}

void Prover::prove_partial_ext_staged(int slot, const void* const* abc, zkp_partial* out) {
  DevicePipeline::MsmOut m = devs_[0]->prove_ext_staged(slot, abc);
  msm_out_to_partial(m, part_, nparts_, out);
  std::lock_guard<std::mutex> lk(tmu_);
  record_timings(last_ms_, m);
}

void proof_combine(const uint8_t* zkey, size_t len, const zkp_partial* parts, int nparts, const uint8_t* wtns,
                   size_t wlen, const uint8_t* r32, const uint8_t* s32, zkp_proof* out) {
  if (nparts < 1) throw ZkpError(ZKP_ERR_INVALID_ARG, "no partials");
  ZkeyParsed z = parse_zkey(zkey, len, false);
  WtnsView w = check_wtns(z.hdr, wtns, wlen);
  std::vector<int> seen(nparts, 0);
  DevicePipeline::MsmOut m;
  m.a = m.b1 = m.c = m.h = Jac<HFq>::inf();
  m.b2 = Jac<HFq2>::inf();
  for (int i = 0; i < nparts; ++i) {
    const zkp_partial& p = parts[i];
    if ((int)p.nparts != nparts || p.part >= p.nparts || seen[p.part]++)
      throw ZkpError(ZKP_ERR_INVALID_ARG, "partials must be parts 0..nparts-1 of one split, each exactly once");
    m.a = host::jac_add(m.a, g1_from_bytes(p.a));
    m.b1 = host::jac_add(m.b1, g1_from_bytes(p.b1));
    m.c = host::jac_add(m.c, g1_from_bytes(p.c));
    m.h = host::jac_add(m.h, g1_from_bytes(p.h));
    m.b2 = host::jac_add(m.b2, g2_from_bytes(p.b2));
  }
  assemble(z.hdr, m, w, r32, s32, out);
}

void Prover::prove(const uint8_t* wtns, size_t len, const uint8_t* r32, const uint8_t* s32, zkp_proof* out) {
  require_full();
  auto t0 = std::chrono::steady_clock::now();
  WtnsView w = check_wtns(hdr_, wtns, len);
  DevicePipeline& d = pick_device();
  DevicePipeline::MsmOut m;
  Blinded bl;
  try {
    m = d.prove(w, [&](const DevicePipeline::MsmOut& o) { bl = assemble_pre(hdr_, o, r32, s32); });
  } catch (const HipError&) {
    retire_device(d);
    throw;
  }
  auto t1 = std::chrono::steady_clock::now();
  assemble_post(hdr_, bl, maybe_corrupt(m.h, corrupt_h_ == 1), w, out);
  auto t2 = std::chrono::steady_clock::now();
  using ms = std::chrono::duration<float, std::milli>;
  const float host_ms[3] = {ms(t2 - t1).count(), ms(t2 - t0).count(), verify() ? verify_or_throw(w, out) : 0.f};
  std::lock_guard<std::mutex> lk(tmu_);
  record_timings(last_ms_, m, host_ms);
}

// Batch scheduler: a shared queue of witness indices; two
// worker threads per device pipeline (one uploads the next witness into a free upload slot
// while the other's proof computes), per-proof status, and re-queue on device failure: a
// worker whose device raises a HIP error puts its witness back at the head of the queue
// and retires the device; the other devices finish the batch.  A witness that is itself
// invalid (format, length, curve) fails alone.
zkp_status Prover::prove_batch(const uint8_t* const* wtns, const size_t* lens, int n, const uint8_t* const* r32s,
                               const uint8_t* const* s32s, zkp_proof* outs, zkp_status* statuses,
                               std::string* first_error) {
  require_full();
  std::vector<zkp_status> st(n, ZKP_ERR_INTERNAL);
  std::vector<std::string> msg(n);
  std::mutex qm;
  std::condition_variable qcv;
  std::deque<int> q;
  for (int i = 0; i < n; ++i) q.push_back(i);
  int outstanding = n;
  const size_t nd = devs_.size();
  auto live_devices = [&] {
    size_t k = 0;
    for (auto& d : devs_) k += d->healthy() ? 1 : 0;
    return k;
  };
  auto finish = [&](int i, zkp_status s, const std::string& m) {
    std::lock_guard<std::mutex> lk(qm);
    st[i] = s;
    msg[i] = m;
    --outstanding;
    qcv.notify_all();
  };
  auto worker = [&](size_t di) {
    DevicePipeline& d = *devs_[di];
    for (;;) {
      int i;
      {
        std::unique_lock<std::mutex> lk(qm);
        qcv.wait(lk, [&] { return !q.empty() || outstanding == 0 || !d.healthy(); });
        if (q.empty() || !d.healthy()) return;
        i = q.front();
        q.pop_front();
      }
      WtnsView w;
      try {
        w = check_wtns(hdr_, wtns[i], lens[i]);
      } catch (const ZkpError& e) {
        finish(i, e.status, e.what());
        continue;
      }
      try {
        Blinded bl;
        DevicePipeline::MsmOut m = d.prove(w, [&](const DevicePipeline::MsmOut& o) {
          bl = assemble_pre(hdr_, o, r32s ? r32s[i] : nullptr, s32s ? s32s[i] : nullptr);
        });
        assemble_post(hdr_, bl, maybe_corrupt(m.h, corrupt_h_ == 1 || (corrupt_h_ == 2 && (i & 1))), w, &outs[i]);
        if (verify_batch()) verify_or_throw(w, &outs[i]);  // on the worker thread: overlaps the next proof
        finish(i, ZKP_OK, "");
      } catch (const HipError& e) {
        retire_device(d);  // every pipeline of that device (ZKP_INFLIGHT siblings share its state)
        std::lock_guard<std::mutex> lk(qm);
        if (live_devices() > 0) {
          q.push_front(i);  // re-queue on a healthy device
        } else {            // nothing left to run on: fail this and everything queued
          st[i] = ZKP_ERR_DEVICE;
          msg[i] = e.what();
          --outstanding;
          while (!q.empty()) {
            st[q.front()] = ZKP_ERR_DEVICE;
            msg[q.front()] = std::string("no healthy device left: ") + e.what();
            q.pop_front();
            --outstanding;
          }
        }
        qcv.notify_all();
        return;
      } catch (const ZkpError& e) {
        finish(i, e.status, e.what());
      } catch (const std::bad_alloc&) {
        finish(i, ZKP_ERR_OUT_OF_MEMORY, "host out of memory");
      } catch (const std::exception& e) {
        finish(i, ZKP_ERR_INTERNAL, e.what());
      }
    }
  };
  if (live_devices() == 0) {
    for (int i = 0; i < n; ++i) st[i] = ZKP_ERR_DEVICE, msg[i] = "every device of this prover has failed";
  } else {
    std::vector<std::thread> th;
    for (size_t di = 0; di < nd; ++di)
      for (int k = 0; k < 2; ++k) th.emplace_back(worker, di);
    for (auto& t : th) t.join();
  }
  zkp_status first = ZKP_OK;
  for (int i = 0; i < n; ++i) {
    if (statuses) statuses[i] = st[i];
    if (st[i] != ZKP_OK && first == ZKP_OK) {
      first = st[i];
      if (first_error) *first_error = "proof " + std::to_string(i) + ": " + msg[i];
    }
  }
  return first;
}

void Prover::quotient(const uint8_t* wtns, size_t len, uint8_t* out) {
  WtnsView w = check_wtns(hdr_, wtns, len);
  devs_[0]->quotient(w, out);
}

void Prover::timings(float* ms, int n) const {
  std::lock_guard<std::mutex> lk(tmu_);
  for (int i = 0; i < n && i < 11; ++i) ms[i] = last_ms_[i];
}

DevicePipeline& Prover::staged_pipeline(int dev_index) const {
  if (dev_index < 0 || dev_index >= ndevices_)
    throw ZkpError(ZKP_ERR_INVALID_ARG, "device index " + std::to_string(dev_index) + " out of range (the prover has " +
                                            std::to_string(ndevices_) + " devices)");
  return *devs_[(size_t)dev_index * inflight_];
}

void Prover::stage(int dev, int slot, const uint8_t* wtns, size_t len) {
  DevicePipeline& d = staged_pipeline(dev);
  WtnsView w = check_wtns(hdr_, wtns, len);
  auto ex = d.lock_stage();  // no staged proof of this device reads a slot or its public signals now
  d.stage(slot, w);
  std::lock_guard<std::mutex> lk(smu_);
  if (staged_pub_.size() < (size_t)ndevices_) staged_pub_.resize(ndevices_);
  auto& v = staged_pub_[dev];
  if ((size_t)slot >= v.size()) v.resize(slot + 1);
  v[slot].assign(w.values, w.values + (size_t)(hdr_.n_public + 1) * 32);
}

void Prover::prove_staged(int dev, int slot, const uint8_t* r32, const uint8_t* s32, zkp_proof* out) {
  require_full();
  DevicePipeline& base = staged_pipeline(dev);
  auto staged = base.hold_stage();  // the slot stays valid and unchanged until the proof is done
  const uint32_t* d_wit = base.slot_ptr(slot);
  const double large_frac = base.slot_large(slot);
  // concurrent staged callers on one device take its idle ZKP_INFLIGHT pipelines (the staged
  // witnesses live in the first one; the others read them in place); with none idle the call
  // queues on the first pipeline
  DevicePipeline* d = &base;
  bool claimed = false;
  for (int k = 0; k < inflight_ && !claimed; ++k) {
    DevicePipeline* c = devs_[(size_t)dev * inflight_ + k].get();
    bool idle = false;
    if (c->staged_busy.compare_exchange_strong(idle, true)) d = c, claimed = true;
  }
  struct Release {
    DevicePipeline* d;
    bool on;
    ~Release() {
      if (on) d->staged_busy.store(false);
    }
  } release{d, claimed};
  auto t0 = std::chrono::steady_clock::now();
  Blinded bl;
  DevicePipeline::MsmOut m = d->prove_resident(
      d_wit, [&](const DevicePipeline::MsmOut& o) { bl = assemble_pre(hdr_, o, r32, s32); }, large_frac);
  auto t1 = std::chrono::steady_clock::now();
  WtnsView w;
  {
    std::lock_guard<std::mutex> lk(smu_);
    w.values = staged_pub_[dev][slot].data();
    w.n_witness = hdr_.n_vars;
  }
  assemble_post(hdr_, bl, maybe_corrupt(m.h, corrupt_h_ == 1), w, out);
  auto t2 = std::chrono::steady_clock::now();
  using ms = std::chrono::duration<float, std::milli>;
  const float host_ms[3] = {ms(t2 - t1).count(), ms(t2 - t0).count(), verify() ? verify_or_throw(w, out) : 0.f};
  std::lock_guard<std::mutex> lk(tmu_);
  record_timings(last_ms_, m, host_ms);
}

Prover::StagedView Prover::staged_view(int dev, int slot) const {
  DevicePipeline& base = staged_pipeline(dev);
  StagedView v;
  v.hold = base.hold_stage();
  v.ptr = base.slot_ptr(slot);
  v.n_signals = hdr_.n_vars;
  v.device = base.device();
  return v;
}

void Prover::set_instrument(bool on) {
  for (auto& d : devs_) d->set_instrument(on);
}

void Prover::msm_config(double* out, int n) const {
  MsmParams pw, ph, pw2;
  devs_[0]->msm_params(pw, ph, &pw2);
  const bool two = devs_[0]->witness_sets() > 1;
  const double v[10] = {(double)pw.c, (double)pw.depth, (double)pw.groups, (double)ph.c,
                        (double)ph.depth, (double)ph.groups, (double)devs_[0]->table_bytes(),
                        two ? (double)pw2.c : 0.0, two ? (double)pw2.depth : 0.0, two ? (double)pw2.groups : 0.0};
  for (int i = 0; i < n && i < 10; ++i) out[i] = v[i];
}

void Prover::kernel_stats(double* out, int n) const {
  MsmEngine::Stats a{}, b{};
  for (auto& d : devs_) {
    MsmEngine::Stats x, y;
    d->stats(x, y);
    a.accumulate_ms += x.accumulate_ms, a.launches += x.launches, a.mixed_adds += x.mixed_adds, a.tasks += x.tasks;
    b.accumulate_ms += y.accumulate_ms, b.launches += y.launches, b.mixed_adds += y.mixed_adds, b.tasks += y.tasks;
  }
  const double v[8] = {a.accumulate_ms, (double)a.launches, (double)a.mixed_adds, (double)a.tasks,
                       b.accumulate_ms, (double)b.launches, (double)b.mixed_adds, (double)b.tasks};
  for (int i = 0; i < n && i < 8; ++i) out[i] = v[i];
}

int Prover::launch_records(double* out, int max_records) const {
  std::vector<std::array<double, 4>> all;
  for (auto& d : devs_) d->launch_records(all);
  const int n = (int)std::min<size_t>(all.size(), (size_t)std::max(0, max_records));
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 4; ++j) out[4 * i + j] = all[i][j];
  return (int)all.size();
}

}  // namespace zkp
