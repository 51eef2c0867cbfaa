// `wtns check` on the device (wtns_check.hpp; the per-lane bodies are wtns_check_kernels.hpp).
//
// Per term the constraint kernels read 32 B of coefficient, 4 B of wire index and 32 B of witness (a
// gather), 68 B in all, plus 12 B of row pointers per constraint; nothing but the fail bitmap is written.
#include "wtns_check.hpp"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "device_pipeline.hpp"
#include "hip_check.hpp"
#include "hip_raii.hpp"
#include "prover.hpp"
#include "wtns_check_kernels.hpp"

namespace zkp {

namespace {

using wcheck::Outcome;
constexpr int TPB = 256;
constexpr int CTPB = 1024;  // k_collect's one workgroup
inline unsigned grid_for(size_t n, int per_block = TPB) { return (unsigned)((n + per_block - 1) / per_block); }

// Constraints of at least this many terms (A + B + C) take a wavefront each.  A lane of the short kernel
// holds its 63 neighbours for as long as its own rows last, so one row of hundreds of terms among rows of
// three costs the wavefront hundreds of term times; a wavefront of its own costs the constraint three
// strided passes and three 6-step butterflies.  Measured (tools/bench_wtns_check.py --sweep: 1 % of the terms
// in rows of one length L among 4-term constraints, profiles/wtns_check.json): the two paths tie between
// L = 12 and L = 16 (14 to 18 terms with the other two sides), the wavefront wins by 10-12 % at L = 24 and by
// 2.8-3.3x at L = 254; below 12 the lane wins.  DESIGN.md §8j.
constexpr uint32_t LONG_TERMS = 24;

// standard-form coefficient -> coef * 2^522: two Montgomery products by 2^522 (each multiplies by 2^261)
__global__ __launch_bounds__(TPB) void k_convert_r1cs_coefs(uint32_t* __restrict__ vals, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  store_fe(vals + i * 8, to_mont(to_mont(load_fe<FrCfg>(vals + i * 8))));
}

__global__ void k_reset(Outcome* __restrict__ out) {
  const uint32_t t = threadIdx.x;
  if (t < (uint32_t)wcheck::MAX_LISTED) out->bad[t] = 0;
  if (t == 0) {
    out->n_bad = 0;
    out->n_listed = 0;
    out->first_unreduced = wcheck::NONE;
    out->w0_not_one = 0;
  }
}

// one lane per signal: below r, and signal 0 is 1.  atomicMin: the lowest index whatever the order
__global__ __launch_bounds__(TPB) void k_scan_witness(const uint32_t* __restrict__ w, uint32_t n, Outcome* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const uint4* q = reinterpret_cast<const uint4*>(w + i * 8);
  const uint4 a = q[0], b = q[1];
  const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  if (wcheck::not_reduced(v)) atomicMin(&out->first_unreduced, (uint32_t)i);
  if (i == 0 && !wcheck::is_one(v)) out->w0_not_one = 1;
}

__device__ __forceinline__ void mark(uint32_t* __restrict__ bits, uint32_t c) { atomicOr(&bits[c >> 5], 1u << (c & 31u)); }

// ids: the constraints of this path, ascending (null: all of 0 .. n_ids - 1)
__global__ __launch_bounds__(TPB) void k_check_short(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col,
                                                     const uint32_t* __restrict__ val, const uint32_t* __restrict__ w,
                                                     const uint32_t* __restrict__ ids, uint32_t n_ids,
                                                     uint32_t* __restrict__ bits) {
  const size_t k = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (k >= n_ids) return;
  const uint32_t c = ids ? ids[k] : (uint32_t)k;
  if (wcheck::short_lane_fails(rowptr, col, val, w, c)) mark(bits, c);
}

__device__ __forceinline__ Fr from_lane(const Fr& x, int off) {
  Fr o;
#pragma unroll
  for (int i = 0; i < NL; ++i) o.v[i] = (uint32_t)__shfl_xor((int)x.v[i], off, wcheck::WAVE);
  return o;
}

// a wavefront per constraint; a whole wavefront leaves together, so every lane that stays takes part
// in the exchanges
__global__ __launch_bounds__(TPB) void k_check_long(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col,
                                                    const uint32_t* __restrict__ val, const uint32_t* __restrict__ w,
                                                    const uint32_t* __restrict__ ids, uint32_t n_ids,
                                                    uint32_t* __restrict__ bits) {
  const size_t wave = ((size_t)blockIdx.x * TPB + threadIdx.x) / wcheck::WAVE;
  const uint32_t lane = threadIdx.x % wcheck::WAVE;
  if (wave >= n_ids) return;
  const uint32_t c = ids[wave];
  auto row = [&](int m) {  // every lane ends with the whole row's sum
    Fr p = wcheck::long_lane_partial(rowptr, col, val, w, c, m, lane);
    for (int off = wcheck::WAVE / 2; off >= 1; off >>= 1) p = wcheck::pair_sum(p, from_lane(p, off));
    return p;
  };
  const Fr a = row(0), b = row(1), cc = row(2);
  if (lane == 0 && !wcheck::satisfied(a, b, cc)) mark(bits, c);
}

// The fail bitmap -> count and the lowest failing indices, ascending, by ONE workgroup and without
// atomics: the result depends on the bitmap alone.  First the count: every thread sums the bits of its
// strided 16-byte pieces (independent loads, no barrier in the loop; nquads = the bitmap's words / 4, the
// bitmap being padded with zero words), then a tree.  A good witness ends here.  Otherwise the workgroup
// walks the bitmap in tiles of CTPB words in order; a tile with a set bit ranks its words by a prefix sum
// of their counts and writes them at their ranks, until the list holds min(16, n_bad) entries.
__global__ __launch_bounds__(CTPB) void k_collect(const uint32_t* __restrict__ bits, uint32_t nquads,
                                                  Outcome* __restrict__ out) {
  __shared__ uint32_t scan[CTPB];
  __shared__ uint32_t s_listed;
  const uint32_t t = threadIdx.x;
  uint32_t mine = 0;
  const uint4* q = reinterpret_cast<const uint4*>(bits);
  for (uint32_t i = t; i < nquads; i += CTPB) {
    const uint4 v = q[i];
    mine += wcheck::popcount32(v.x) + wcheck::popcount32(v.y) + wcheck::popcount32(v.z) + wcheck::popcount32(v.w);
  }
  scan[t] = mine;
  if (t == 0) s_listed = 0;
  __syncthreads();
  for (uint32_t off = CTPB / 2; off >= 1; off >>= 1) {
    if (t < off) scan[t] += scan[t + off];
    __syncthreads();
  }
  const uint32_t n_bad = scan[0];
  const uint32_t want = min(n_bad, (uint32_t)wcheck::MAX_LISTED);
  __syncthreads();
  if (t == 0) {
    out->n_bad = n_bad;
    out->n_listed = want;
  }
  const uint64_t nwords = (uint64_t)nquads * 4;
  // s_listed changes between barriers only, so every thread takes the same turns
  for (uint64_t base = 0; base < nwords && s_listed < want; base += CTPB) {
    const uint64_t i = base + t;
    const uint32_t word = i < nwords ? bits[i] : 0u;
    const uint32_t pc = wcheck::popcount32(word);
    if (!__syncthreads_or(pc != 0)) continue;
    scan[t] = pc;
    __syncthreads();
    for (uint32_t off = 1; off < (uint32_t)CTPB; off <<= 1) {
      const uint32_t below = t >= off ? scan[t - off] : 0u;
      __syncthreads();
      scan[t] += below;
      __syncthreads();
    }
    const uint32_t listed = s_listed;
    wcheck::collect_word(word, (uint32_t)i, listed + scan[t] - pc, out->bad);
    const uint32_t tile = scan[CTPB - 1];
    __syncthreads();
    if (t == 0) s_listed = listed + min(tile, (uint32_t)wcheck::MAX_LISTED);
    __syncthreads();
  }
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

CheckTimings& check_timings() {
  thread_local CheckTimings t;
  return t;
}

uint32_t check_long_terms() {
  const char* e = std::getenv("ZKP_WTNS_CHECK_LONG");
  if (!e || !*e) return LONG_TERMS;
  char* stop = nullptr;
  const unsigned long long v = std::strtoull(e, &stop, 10);
  if (*stop || v > 0xffffffffull) throw ZkpError(ZKP_ERR_INVALID_ARG, "ZKP_WTNS_CHECK_LONG: not a term count");
  return (uint32_t)v;
}

void check_wtns_header(const R1csCsr& csr, const uint8_t* wtns, size_t len) {
  const WtnsView w = parse_wtns(wtns, len);
  if (w.n_witness != csr.n_wires)
    throw ZkpError(ZKP_ERR_WITNESS_LENGTH, "Invalid witness length. Circuit: " + std::to_string(csr.n_wires) +
                                               ", witness: " + std::to_string(w.n_witness));
}

struct WitnessChecker::Dev {
  Stream st;
  Event ev[3];
  DevBuf<> rowptr, col, val, ids_short, ids_long, wit, bits;
  DevBuf<Outcome> out;
  PinnedBuf<Outcome> hout;
  uint32_t n_short = 0, n_long = 0, nwords = 0;
  bool all_short = true;
};

R1csCsr parse_r1cs_or_throw(const uint8_t* r1cs, size_t len, double* parse_ms) {
  const auto t0 = std::chrono::steady_clock::now();
  R1csCsr csr;
  std::string err;
  const zkp_status s = parse_r1cs(r1cs, len, csr, err);
  if (s != ZKP_OK) throw ZkpError(s, err);
  if (parse_ms) *parse_ms = ms_since(t0);
  return csr;
}

WitnessChecker::WitnessChecker(int device, R1csCsr&& csr, double parse_ms) : dev_(device) {
  const auto t_all = std::chrono::steady_clock::now();
  auto t0 = t_all;
  n_wires_ = csr.n_wires;
  n_public_ = csr.n_public();
  n_constraints_ = csr.n_constraints;
  n_terms_ = csr.n_terms();
  // the rows by length, on the host
  const uint32_t lt = long_terms_ = check_long_terms();
  std::vector<uint32_t> ids_short, ids_long;
  for (uint32_t c = 0; c < n_constraints_; ++c)
    if (lt && csr.rowptr[(size_t)c * 3 + 3] - csr.rowptr[(size_t)c * 3] >= lt) ids_long.push_back(c);
  if (!ids_long.empty()) {
    ids_short.reserve(n_constraints_ - ids_long.size());
    size_t k = 0;
    for (uint32_t c = 0; c < n_constraints_; ++c) {
      if (k < ids_long.size() && ids_long[k] == c) ++k;
      else ids_short.push_back(c);
    }
  }
  n_long_ = (uint32_t)ids_long.size();
  parse_ms += ms_since(t0);

  t0 = std::chrono::steady_clock::now();
  HIPX(hipSetDevice(dev_));
  d_ = std::make_unique<Dev>();
  Dev& d = *d_;
  d.st = Stream(hipStreamNonBlocking);
  for (auto& e : d.ev) e = Event(true);
  d.n_long = n_long_;
  d.all_short = ids_long.empty();
  d.n_short = d.all_short ? n_constraints_ : (uint32_t)ids_short.size();
  d.nwords = (uint32_t)(((uint64_t)n_constraints_ + 127) / 128 * 4);  // whole 16-byte pieces (k_collect)
  auto up = [&](DevBuf<>& b, const std::vector<uint32_t>& v) {
    b = DevBuf<>(std::max<size_t>(v.size(), 1));
    if (!v.empty()) HIPX(hipMemcpyAsync(b, v.data(), v.size() * 4, hipMemcpyHostToDevice, d.st));
  };
  up(d.rowptr, csr.rowptr);
  up(d.col, csr.col);
  up(d.val, csr.val);
  up(d.ids_short, ids_short);
  up(d.ids_long, ids_long);
  d.wit = DevBuf<>((size_t)n_wires_ * 8);
  d.bits = DevBuf<>(std::max<uint32_t>(d.nwords, 1));
  d.out = DevBuf<Outcome>(1);
  d.hout = PinnedBuf<Outcome>(1);
  if (n_terms_) {
    hipLaunchKernelGGL(k_convert_r1cs_coefs, dim3(grid_for(n_terms_)), dim3(TPB), 0, d.st, d.val.get(), (size_t)n_terms_);
    HIPX(hipGetLastError());
  }
  HIPX(hipStreamSynchronize(d.st));  // the host vectors go away with csr
  CheckTimings& t = check_timings();
  t = CheckTimings{};
  t.parse_ms = parse_ms;
  t.upload_ms = ms_since(t0);
  t.total_ms = t.parse_ms + t.upload_ms;
}

WitnessChecker::~WitnessChecker() {
  if (d_) (void)hipSetDevice(dev_);
}

void WitnessChecker::check(const uint8_t* wtns, size_t len, zkp_check_result* res, std::string& msg) {
  const auto t0 = std::chrono::steady_clock::now();
  const WtnsView w = parse_wtns(wtns, len);
  if (w.n_witness != n_wires_)
    throw ZkpError(ZKP_ERR_WITNESS_LENGTH, "Invalid witness length. Circuit: " + std::to_string(n_wires_) +
                                               ", witness: " + std::to_string(w.n_witness));
  std::lock_guard<std::mutex> lk(mu_);
  HIPX(hipSetDevice(dev_));
  Dev& d = *d_;
  HIPX(hipEventRecord(d.ev[0], d.st));
  HIPX(hipMemcpyAsync(d.wit, w.values, (size_t)n_wires_ * 32, hipMemcpyHostToDevice, d.st));
  run(d.wit, true, res, msg);
  check_timings().total_ms = ms_since(t0);
}

void WitnessChecker::check_staged(Prover& p, int dev_index, int slot, zkp_check_result* res, std::string& msg) {
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> lk(mu_);
  // the hold a staged proof takes: the slot's copy is complete and nobody restages it until we are done.
  // Proofs of the same slot only read it too, so they may run beside the check.
  const Prover::StagedView v = p.staged_view(dev_index, slot);
  if (v.device != dev_)
    throw ZkpError(ZKP_ERR_INVALID_ARG, "the checker is on device " + std::to_string(dev_) + ", the staged witness on device " +
                                            std::to_string(v.device));
  if (v.n_signals != n_wires_)
    throw ZkpError(ZKP_ERR_INVALID_ARG, "the staged witness has " + std::to_string(v.n_signals) + " signals, the r1cs " +
                                            std::to_string(n_wires_) + " wires");
  HIPX(hipSetDevice(dev_));
  HIPX(hipEventRecord(d_->ev[0], d_->st));
  run(v.ptr, false, res, msg);
  check_timings().total_ms = ms_since(t0);
}

// caller holds mu_, has selected the device and recorded ev[0] (and enqueued the copy, if any) on the stream
void WitnessChecker::run(const uint32_t* d_wit, bool copied, zkp_check_result* res, std::string& msg) {
  Dev& d = *d_;
  const hipStream_t st = d.st;
  HIPX(hipEventRecord(d.ev[1], st));
  // every counter and flag starts afresh
  HIPX(hipMemsetAsync(d.bits, 0, (size_t)std::max<uint32_t>(d.nwords, 1) * 4, st));
  hipLaunchKernelGGL(k_reset, dim3(1), dim3(64), 0, st, d.out.get());
  hipLaunchKernelGGL(k_scan_witness, dim3(grid_for(n_wires_)), dim3(TPB), 0, st, d_wit, n_wires_, d.out.get());
  if (d.n_short)
    hipLaunchKernelGGL(k_check_short, dim3(grid_for(d.n_short)), dim3(TPB), 0, st, d.rowptr.get(), d.col.get(), d.val.get(),
                       d_wit, d.all_short ? (const uint32_t*)nullptr : d.ids_short.get(), d.n_short, d.bits.get());
  if (d.n_long)
    hipLaunchKernelGGL(k_check_long, dim3(grid_for(d.n_long, TPB / wcheck::WAVE)), dim3(TPB), 0, st, d.rowptr.get(),
                       d.col.get(), d.val.get(), d_wit, d.ids_long.get(), d.n_long, d.bits.get());
  if (d.nwords) hipLaunchKernelGGL(k_collect, dim3(1), dim3(CTPB), 0, st, d.bits.get(), d.nwords / 4, d.out.get());
  HIPX(hipGetLastError());
  HIPX(hipMemcpyAsync(d.hout.get(), d.out.get(), sizeof(Outcome), hipMemcpyDeviceToHost, st));
  HIPX(hipEventRecord(d.ev[2], st));
  HIPX(hipStreamSynchronize(st));
  float copy_ms = 0, kernel_ms = 0;
  HIPX(hipEventElapsedTime(&copy_ms, d.ev[0], d.ev[1]));
  HIPX(hipEventElapsedTime(&kernel_ms, d.ev[1], d.ev[2]));
  CheckTimings& t = check_timings();
  t = CheckTimings{};
  t.copy_ms = copied ? copy_ms : 0.0;
  t.kernel_ms = kernel_ms;

  const Outcome& o = *d.hout.get();
  std::memset(res, 0, sizeof(*res));
  res->n_constraints = n_constraints_;
  if (o.w0_not_one) {
    msg = "INVALID: signal 0 is not 1";
  } else if (o.first_unreduced != wcheck::NONE) {
    msg = "INVALID: signal " + std::to_string(o.first_unreduced) + " is not reduced";
  } else if (o.n_bad) {
    res->n_bad = o.n_bad;
    res->n_listed = o.n_listed;
    for (uint32_t k = 0; k < o.n_listed && k < (uint32_t)wcheck::MAX_LISTED; ++k) res->bad[k] = o.bad[k];
    res->first_bad = o.bad[0];
    msg = "INVALID: constraint " + std::to_string(res->first_bad) + " is not satisfied (" + std::to_string(res->n_bad) +
          " of " + std::to_string(n_constraints_) + " fail)";
  } else {
    res->valid = 1;
    msg = "OK";
  }
}

}  // namespace zkp
