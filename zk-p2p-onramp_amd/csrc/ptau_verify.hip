// Device side of `powersoftau verify` (ptau_verify.hpp): the point sections of a ptau file.
//
// Every section (2-6, 12-15 when present) is uploaded once and stays in HBM: section k + 1 uploads on a
// second stream while section k is checked.  In order:
//   1. k_check_points over every section, k_g2_subgroup over the G2 sections (3, 6, 13);
//   2. the singular points (host, from the file's bytes);
//   3. powers: with coefficients r_i, A = sum r_i P_i and B = sum r_i P_(i+1) must satisfy
//      e(A, tauG2[1]) = e(B, G2).  One plan per chunk of ZKP_VERIFY_CHUNK coefficients runs against two
//      views of the resident section, at point offsets 0 and 1 (MsmBases views: nothing is copied);
//   4. the Lagrange sections: sum_i rho_i lX_i == sum_j s_j X_j with s_j = sum_p iFFT_p(rho^(p))_j, one
//      129-bit plan over the 2N - 1 Lagrange points and one 255-bit plan over the N tau points, each
//      shared by the three G1 vectors and the G2 vector.
// The coefficients are 128-bit (k_rlc_coeffs, one stream per verification): the plans of 3 and of the
// Lagrange side of 4 cover 129 bits at depth T = 1.  Chunk sums are folded (msm_fold) and added on the host.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "curve.hpp"
#include "device_pipeline.hpp"
#include "g2_subgroup_kernels.hpp"
#include "mpc.hpp"
#include "points_through.hpp"
#include "ptau_verify.hpp"
#include "qap.hpp"
#include "spans.hpp"
#include "zkey_verify.hpp"

namespace zkp {

namespace {

constexpr int SUB_TPB = 128;
constexpr int TPB = 256;
unsigned grid(size_t n, int tpb) { return (unsigned)((n + tpb - 1) / tpb); }

// One thread per point: [r]P with the scalar in registers, the same digits in every lane.  out[0] += the
// points outside the subgroup, out[1] = min(out[1], base + i) over them.
__global__ __launch_bounds__(SUB_TPB) void k_g2_subgroup(const uint32_t* __restrict__ pts, size_t n, uint64_t base,
                                                         unsigned long long* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * SUB_TPB + threadIdx.x;
  if (i >= n) return;
  if (!g2sub::in_subgroup(pts, i)) {
    atomicAdd(&out[0], 1ull);
    atomicMin(&out[1], (unsigned long long)(base + i));
  }
}

// s[i] += t[i], i < n (Fr, device layout)
__global__ __launch_bounds__(TPB) void k_fr_add_into(uint32_t* __restrict__ s, const uint32_t* __restrict__ t, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  store_fe(s + i * 8, add(load_fe<FrCfg>(s + i * 8), load_fe<FrCfg>(t + i * 8)));
}

thread_local PtauVerifyTimings g_timings;

void require_free(size_t bytes) {
  size_t free_b = 0, total_b = 0;
  HIPX(hipMemGetInfo(&free_b, &total_b));
  if (bytes > free_b)
    throw ZkpError(ZKP_ERR_OUT_OF_MEMORY, "ptau verify: the working set of " + std::to_string(bytes >> 20) +
                                              " MiB does not fit in " + std::to_string(free_b >> 20) + " MiB of free HBM");
}

// one sum per base set
struct Sum {
  Jac<HFq> g1 = Jac<HFq>::inf();
  Jac<HFq2> g2 = Jac<HFq2>::inf();
};
struct BaseSet {
  Curve curve;
  const uint32_t* pts;  // resident, device layout
};

// sum_i scalar_i * base_i over resident base sets that share the scalars: per chunk of at most CH scalars
// one plan, one engine run per set against a view of the set's chunk.  Depth 1 (the bases are used once).
class SumRunner {
 public:
  SumRunner(size_t max_n, int scalar_bits, bool g2, hipStream_t st, Spans& sp, PtauVerifyTimings& t)
      : st_(st), sp_(sp), t_(t), ch_(std::max<size_t>(1, std::min(max_n, verify_chunk_points()))) {
    const int c = scalar_bits == 129 ? rlc_window_bits(ch_) : h_window_bits(ch_);
    prm_ = make_params(ch_, c, 1, scalar_bits);
    const MsmOptions opt = msm_options();
    apply_task_options(prm_, opt.task_h, opt);
    plan_ = std::make_unique<MsmPlan>(ch_, prm_, st);
    plan_->set_dense(true);
    eng1_ = std::make_unique<MsmEngine>(Curve::G1, prm_, ch_, st);
    if (g2) eng2_ = std::make_unique<MsmEngine>(Curve::G2, prm_, ch_, st);
    ww_ = MsmEngine::window_words_for(Curve::G2, prm_);
    ds_ = DevBuf<>(ch_ * 8);
    dwin_ = DevBuf<>(MAX_SETS * ww_);
    hwin_ = PinnedBuf<uint32_t>(MAX_SETS * ww_);
  }
  // a generous bound of what a runner allocates: the plan's ~36 bytes per (scalar, window) entry, the
  // engines' task partials and buckets (XYZZ: 128 / 256 bytes)
  static size_t bytes_bound(size_t max_n, int scalar_bits) {
    const size_t ch = std::max<size_t>(1, std::min(max_n, verify_chunk_points()));
    const size_t entries = ch * (size_t)((scalar_bits + 7) / 8);
    return entries * 36 + (entries / 16 + (size_t(1) << 21)) * 384 * 2 + ch * 32;
  }
  // scalars: n resident 8-word standard-form values, or null: coefficients first_index .. + n - 1 of seed32.
  // out[k] += the sum over sets[k] (its points 0 .. n - 1).
  void run(const uint32_t* scalars, const uint8_t* seed32, uint64_t first_index, size_t n, const std::vector<BaseSet>& sets,
           Sum* out, double* acc_ms) {
    if (sets.size() > MAX_SETS) throw ZkpError(ZKP_ERR_INTERNAL, "ptau verify: too many base sets");
    for (size_t at = 0; at < n; at += ch_) {
      const size_t m = std::min(ch_, n - at);
      const uint32_t* sc = scalars ? scalars + at * 8 : ds_.get();
      if (!scalars) {
        sp_.begin(st_);
        rlc_coeffs_resident(seed32, first_index + at, m, ds_, st_);
        sp_.end(st_, &t_.coeffs_ms);
      }
      sp_.begin(st_);
      plan_->build(sc, m);
      sp_.end(st_, &t_.plan_ms);
      sp_.begin(st_);
      for (size_t k = 0; k < sets.size(); ++k) {
        const bool g2 = sets[k].curve == Curve::G2;
        const MsmBases view(sets[k].curve, sets[k].pts + at * (g2 ? 32 : 16), m, prm_.c);
        (g2 ? *eng2_ : *eng1_).run(*plan_, view, dwin_ + k * ww_);
      }
      sp_.end(st_, acc_ms);
      HIPX(hipMemcpyAsync(hwin_, dwin_, sets.size() * ww_ * 4, hipMemcpyDeviceToHost, st_));
      HIPX(hipStreamSynchronize(st_));
      const auto t0 = std::chrono::steady_clock::now();
      for (size_t k = 0; k < sets.size(); ++k) {
        if (sets[k].curve == Curve::G2)
          out[k].g2 = host::jac_add(out[k].g2, msm_fold<HFq2>(hwin_ + k * ww_, prm_));
        else
          out[k].g1 = host::jac_add(out[k].g1, msm_fold<HFq>(hwin_ + k * ww_, prm_));
      }
      t_.fold_ms += wall_ms(t0);
      ++t_.chunks;
    }
  }

 private:
  static constexpr size_t MAX_SETS = 4;
  hipStream_t st_;
  Spans& sp_;
  PtauVerifyTimings& t_;
  size_t ch_, ww_ = 0;
  MsmParams prm_;
  std::unique_ptr<MsmPlan> plan_;
  std::unique_ptr<MsmEngine> eng1_, eng2_;
  DevBuf<> ds_, dwin_;
  PinnedBuf<uint32_t> hwin_;
};

template <class F>
bool same_jac(const Jac<F>& a, const Jac<F>& b) {
  const Affine<F> x = host::jac_to_aff(a), y = host::jac_to_aff(b);
  return x.inf == y.inf && (x.inf || (x.x == y.x && x.y == y.y));
}

// zkey-layout bytes (Montgomery 2^256, the host's own form) -> host points; canonical, checked before
Affine<HFq> g1_of(const uint8_t* p) {
  return Affine<HFq>{HFq::raw(host::u256_from_le(p)), HFq::raw(host::u256_from_le(p + 32)), false};
}
Affine<HFq2> g2_of(const uint8_t* p) {
  return Affine<HFq2>{HFq2{HFq::raw(host::u256_from_le(p)), HFq::raw(host::u256_from_le(p + 32))},
                      HFq2{HFq::raw(host::u256_from_le(p + 64)), HFq::raw(host::u256_from_le(p + 96))}, false};
}
void g1_bytes(const Affine<HFq>& a, uint8_t* out) {
  host::u256_to_le(a.x.v, out), host::u256_to_le(a.y.v, out + 32);
}
void g2_bytes(const Affine<HFq2>& a, uint8_t* out) {
  host::u256_to_le(a.x.c0.v, out), host::u256_to_le(a.x.c1.v, out + 32);
  host::u256_to_le(a.y.c0.v, out + 64), host::u256_to_le(a.y.c1.v, out + 96);
}
bool all_zero(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (p[i]) return false;
  return true;
}

}  // namespace

PtauFile parse_ptau(const uint8_t* ptau, size_t len) {
  const BinFile bf = parse_binfile(ptau, len, "ptau", 1);
  PtauFile f;
  for (int id = 0; id < 16; ++id) f.sec[id] = bf.sec[id];
  if (!f.sec[1].ptr) throw ZkpError(ZKP_ERR_FORMAT, "ptau: missing section 1");
  if (f.sec[1].len < 4) throw ZkpError(ZKP_ERR_FORMAT, "ptau: bad header (section 1)");
  uint32_t n8;
  std::memcpy(&n8, f.sec[1].ptr, 4);
  if (n8 != 32 || f.sec[1].len < 4 + 32 + 4 + 4) throw ZkpError(ZKP_ERR_FORMAT, "ptau: bad header (section 1): n8 must be 32");
  if (std::memcmp(f.sec[1].ptr + 4, host::FQ_DESC.mod.w, 32) != 0) throw ZkpError(ZKP_ERR_CURVE, "ptau: curve is not bn128");
  std::memcpy(&f.power, f.sec[1].ptr + 36, 4);
  std::memcpy(&f.ceremony_power, f.sec[1].ptr + 40, 4);
  // power 0 has no tau*G1[1], tau*G2[1]: nothing could be checked
  if (f.power < 1 || f.power > 28) throw ZkpError(ZKP_ERR_FORMAT, "ptau: power must be within 1..28 (section 1)");
  if (f.ceremony_power < f.power) throw ZkpError(ZKP_ERR_FORMAT, "ptau: ceremonyPower below power (section 1)");
  const size_t N = f.N(), nlag = 2 * N - 1;
  auto sized = [&](int id, size_t want) {
    if (!f.sec[id].ptr) throw ZkpError(ZKP_ERR_FORMAT, "ptau: missing section " + std::to_string(id));
    if (f.sec[id].len != want)
      throw ZkpError(ZKP_ERR_FORMAT, "ptau: section " + std::to_string(id) + " has " + std::to_string(f.sec[id].len) +
                                         " bytes, its power wants " + std::to_string(want));
  };
  sized(2, nlag * 64), sized(3, N * 128), sized(4, N * 64), sized(5, N * 64), sized(6, 128);
  if (!f.sec[7].ptr) throw ZkpError(ZKP_ERR_FORMAT, "ptau: missing section 7");
  if (f.sec[7].len < 4) throw ZkpError(ZKP_ERR_FORMAT, "ptau: section 7 has no contribution count");
  int have = 0;
  for (int id = 12; id <= 15; ++id) have += f.sec[id].ptr ? 1 : 0;
  if (have) {
    for (int id = 12; id <= 15; ++id) sized(id, nlag * (id == 13 ? 128 : 64));
    f.lagrange = true;
  }
  return f;
}

namespace {

const char* section_name(int id) {
  switch (id) {
    case 2: return "tauG1";
    case 3: return "tauG2";
    case 4: return "alphaTauG1";
    case 5: return "betaTauG1";
    default: return "betaG2";
  }
}

}  // namespace

PtauVerifyTimings& ptau_verify_timings() { return g_timings; }

void g2_subgroup_resident(const uint32_t* d_points, size_t n, uint64_t base, unsigned long long* bad, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_g2_subgroup, dim3(grid(n, SUB_TPB)), dim3(SUB_TPB), 0, st, d_points, n, base, bad);
  HIPX(hipGetLastError());
}

void g2_subgroup_check(int device, const uint8_t* points, size_t n, uint64_t* n_bad, uint64_t* first_bad) {
  *n_bad = 0, *first_bad = SUBGROUP_NO_BAD;
  if (!n) return;
  HIPX(hipSetDevice(device));
  points_through(verify_chunk_points(), 128, 0, points, n, nullptr, n_bad, first_bad,
                 [](const uint32_t* d, size_t m, uint64_t base, uint32_t*, unsigned long long* bad, hipStream_t st) {
                   g2_subgroup_resident(d, m, base, bad, st);
                 });
}

PairSums rlc_pairs(int device, bool g2, const uint8_t* seed32, uint64_t first_index, const uint8_t* points, size_t n) {
  PairSums r;
  if (n <= 1) return r;
  if (first_index > (uint64_t(1) << 62) || (uint64_t)n > (uint64_t(1) << 31))
    throw ZkpError(ZKP_ERR_INVALID_ARG, "rlc pairs: index or count out of range");
  HIPX(hipSetDevice(device));
  const size_t pb = g2 ? 128 : 64;
  require_free(n * pb + SumRunner::bytes_bound(n - 1, 129) + (size_t(64) << 20));
  Stream st(hipStreamNonBlocking);
  DevBuf<> d(n * pb / 4);
  DevBuf<unsigned long long> dbad(2);
  HIPX(hipMemcpyAsync(d, points, n * pb, hipMemcpyHostToDevice, st));
  points_bad_reset(dbad, st);
  points_check_resident(g2, d, n, 0, dbad, st);
  unsigned long long hbad[2];
  HIPX(hipMemcpyAsync(hbad, dbad, 16, hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  if (hbad[0]) throw ZkpError(ZKP_ERR_INVALID_ARG, "rlc pairs: point " + std::to_string(hbad[1]) + " is not on the curve");
  launch_convert_fq_zkey(d, n * (g2 ? 4 : 2), st);
  Spans sp;
  PtauVerifyTimings t;
  double acc = 0;
  SumRunner run(n - 1, 129, g2, st, sp, t);
  const Curve cv = g2 ? Curve::G2 : Curve::G1;
  Sum out[2];
  run.run(nullptr, seed32, first_index, n - 1, {BaseSet{cv, d}, BaseSet{cv, d + pb / 4}}, out, &acc);
  sp.collect();
  r.a1 = out[0].g1, r.b1 = out[1].g1, r.a2 = out[0].g2, r.b2 = out[1].g2;
  return r;
}

bool ptau_verify_sections(int device, const uint8_t* ptau, size_t len, const uint8_t* seed32, std::string& msg) {
  const auto t_begin = std::chrono::steady_clock::now();
  PtauVerifyTimings t;
  Spans sp;
  auto verdict = [&](bool ok, const std::string& m) {
    sp.collect();
    msg = m;
    t.total_ms = wall_ms(t_begin);
    g_timings = t;
    return ok;
  };
  auto bad = [&](const std::string& m) { return verdict(false, m); };

  const PtauFile f = parse_ptau(ptau, len);
  const size_t N = f.N(), nlag = 2 * N - 1;
  if (f.lagrange && f.power > 27) throw ZkpError(ZKP_ERR_INVALID_ARG, "ptau verify: Lagrange sections above power 27 are not supported");
  std::vector<int> ids = {2, 3, 4, 5, 6};
  if (f.lagrange) ids.insert(ids.end(), {12, 13, 14, 15});
  uint8_t seed[32];
  if (seed32)
    std::memcpy(seed, seed32, 32);
  else
    os_random(seed, 32);
  t.parse_ms = wall_ms(t_begin);

  // ---- device: the working set first
  HIPX(hipSetDevice(device));
  size_t need = size_t(64) << 20;
  for (int id : ids) need += f.sec[id].len;
  need += SumRunner::bytes_bound(nlag, 129);
  if (f.lagrange) need += SumRunner::bytes_bound(N, 255) + 3 * N * 32;
  require_free(need);
  Stream st(hipStreamNonBlocking), sx(hipStreamNonBlocking);  // compute; uploads
  DevBuf<> dsec[16];
  for (int id : ids) dsec[id] = DevBuf<>(f.sec[id].len / 4);
  DevBuf<unsigned long long> dbad(2 * 32);  // [2 id]: curve, [2 (16 + id)]: subgroup
  PinnedBuf<unsigned long long> hbad(2 * 32);

  // ---- 1. points: section k + 1 uploads (sx) while section k is checked (st)
  {
    std::vector<Event> up;
    for (size_t k = 0; k < ids.size(); ++k) up.emplace_back(false);
    auto upload = [&](size_t k) {
      const auto t0 = std::chrono::steady_clock::now();
      HIPX(hipMemcpyAsync(dsec[ids[k]], f.sec[ids[k]].ptr, f.sec[ids[k]].len, hipMemcpyHostToDevice, sx));
      HIPX(hipEventRecord(up[k], sx));
      t.upload_ms += wall_ms(t0);
    };
    upload(0);
    for (size_t k = 0; k < ids.size(); ++k) {
      const int id = ids[k];
      HIPX(hipStreamWaitEvent(st, up[k], 0));
      points_bad_reset(dbad.get() + 2 * id, st);
      points_bad_reset(dbad.get() + 2 * (16 + id), st);
      sp.begin(st);
      points_check_resident(PtauFile::is_g2(id), dsec[id], f.points(id), 0, dbad.get() + 2 * id, st);
      sp.end(st, &t.check_ms);
      if (PtauFile::is_g2(id)) {
        sp.begin(st);
        g2_subgroup_resident(dsec[id], f.points(id), 0, dbad.get() + 2 * (16 + id), st);
        sp.end(st, &t.subgroup_ms);
      }
      if (k + 1 < ids.size()) upload(k + 1);
    }
    HIPX(hipMemcpyAsync(hbad, dbad, 2 * 32 * 8, hipMemcpyDeviceToHost, st));
    HIPX(hipStreamSynchronize(st));
    HIPX(hipStreamSynchronize(sx));  // no upload still reads the caller's buffer
    for (int id : ids)
      if (hbad[2 * id])
        return bad("section " + std::to_string(id) + " point " + std::to_string(hbad[2 * id + 1]) + " is not on the curve");
    for (int id : ids)
      if (PtauFile::is_g2(id) && hbad[2 * (16 + id)])
        return bad("section " + std::to_string(id) + " point " + std::to_string(hbad[2 * (16 + id) + 1]) +
                   " is not in the subgroup");
  }

  // ---- 2. singular points
  const Affine<HFq> g1gen{HFq::from_std(U256{{1, 0, 0, 0}}), HFq::from_std(U256{{2, 0, 0, 0}}), false};
  const Affine<HFq2> g2gen = g2_generator();
  {
    uint8_t g1b[64], g2b[128];
    g1_bytes(g1gen, g1b), g2_bytes(g2gen, g2b);
    if (std::memcmp(f.sec[2].ptr, g1b, 64) != 0) return bad("First element of tau*G1 section must be the generator");
    if (std::memcmp(f.sec[3].ptr, g2b, 128) != 0) return bad("First element of tau*G2 section must be the generator");
    if (all_zero(f.sec[2].ptr + 64, 64)) return bad("Second element of tau*G1 section is the point at infinity");
    if (all_zero(f.sec[3].ptr + 128, 128)) return bad("Second element of tau*G2 section is the point at infinity");
    if (all_zero(f.sec[4].ptr, 64)) return bad("First element of alpha*tau*G1 section is the point at infinity");
    if (all_zero(f.sec[5].ptr, 64)) return bad("First element of beta*tau*G1 section is the point at infinity");
    if (all_zero(f.sec[6].ptr, 128)) return bad("beta*G2 is the point at infinity");
  }
  const Affine<HFq> tau_g1_1 = g1_of(f.sec[2].ptr + 64), beta_g1 = g1_of(f.sec[5].ptr);
  const Affine<HFq2> tau_g2_1 = g2_of(f.sec[3].ptr + 128), beta_g2 = g2_of(f.sec[6].ptr);

  // ---- every section to the device layout, in place
  sp.begin(st);
  for (int id : ids) launch_convert_fq_zkey(dsec[id], f.points(id) * (PtauFile::is_g2(id) ? 4 : 2), st);
  sp.end(st, &t.plan_ms);

  // ---- 3. powers
  auto pairing = [&](auto&& check) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = check();
    t.pairing_ms += wall_ms(t0);
    return ok;
  };
  uint64_t first = 0;
  {
    SumRunner run(nlag - 1, 129, true, st, sp, t);
    for (int id : {2, 3, 4, 5}) {
      const size_t pairs = f.points(id) - 1;
      const Curve cv = id == 3 ? Curve::G2 : Curve::G1;
      Sum s[2];
      run.run(nullptr, seed, first, pairs, {BaseSet{cv, dsec[id]}, BaseSet{cv, dsec[id] + (id == 3 ? 32 : 16)}}, s,
              &t.acc_pairs_ms);
      first += pairs;
      const bool ok = pairing([&] {
        return id == 3 ? same_ratio(g1gen, tau_g1_1, host::jac_to_aff(s[0].g2), host::jac_to_aff(s[1].g2))
                       : same_ratio(host::jac_to_aff(s[0].g1), host::jac_to_aff(s[1].g1), g2gen, tau_g2_1);
      });
      if (!ok) return bad(std::string(section_name(id)) + " section. Powers do not match");
    }
  }
  if (!pairing([&] { return same_ratio(g1gen, beta_g1, g2gen, beta_g2); })) return bad("betaG2 does not match betaTauG1");
  if (!f.lagrange) return verdict(true, "OK");

  // ---- 4. Lagrange sections: coefficient first + i for flat index i, shared by the four vectors
  const int lag_id[4] = {12, 13, 14, 15}, tau_id[4] = {2, 3, 4, 5};
  std::vector<BaseSet> lag_sets, tau_sets;
  for (int v = 0; v < 4; ++v) {
    lag_sets.push_back(BaseSet{v == 1 ? Curve::G2 : Curve::G1, dsec[lag_id[v]]});
    tau_sets.push_back(BaseSet{v == 1 ? Curve::G2 : Curve::G1, dsec[tau_id[v]]});
  }
  SumRunner run129(nlag, 129, true, st, sp, t), run255(N, 255, true, st, sp, t);
  DevBuf<> ds(N * 8), dtmp(N * 8), dstd(N * 8);
  std::vector<std::unique_ptr<NttEngine>> ntts((size_t)f.power + 1);
  // level p's scalars iFFT_p(rho^(p)) (device layout) into dtmp
  auto level_scalars = [&](int p) {
    const size_t n = (size_t)1 << p;
    rlc_coeffs_resident(seed, first + n - 1, n, dtmp, st);
    launch_fr_to_dev(dtmp, n, st);
    if (p > 0) {
      if (!ntts[p]) ntts[p] = std::make_unique<NttEngine>(p, st);
      ntts[p]->inverse(dtmp);
    }
  };
  sp.begin(st);
  HIPX(hipMemsetAsync(ds, 0, N * 32, st));
  for (int p = 0; p <= (int)f.power; ++p) {
    const size_t n = (size_t)1 << p;
    level_scalars(p);
    hipLaunchKernelGGL(k_fr_add_into, dim3(grid(n, TPB)), dim3(TPB), 0, st, ds.get(), dtmp.get(), n);
    HIPX(hipGetLastError());
  }
  HIPX(hipMemcpyAsync(dstd, ds, N * 32, hipMemcpyDeviceToDevice, st));
  launch_fr_from_dev(dstd, N, st);
  sp.end(st, &t.ntt_ms);
  Sum lhs[4], rhs[4];
  run129.run(nullptr, seed, first, nlag, lag_sets, lhs, &t.acc_lag_ms);
  run255.run(dstd, nullptr, 0, N, tau_sets, rhs, &t.acc_tau_ms);
  for (int v = 0; v < 4; ++v) {
    if (v == 1 ? same_jac(lhs[v].g2, rhs[v].g2) : same_jac(lhs[v].g1, rhs[v].g1)) continue;
    // the smallest failing level of this vector
    for (int p = 0; p <= (int)f.power; ++p) {
      const size_t n = (size_t)1 << p;
      const size_t pw = v == 1 ? 32 : 16;
      Sum l, r;
      run129.run(nullptr, seed, first + n - 1, n, {BaseSet{lag_sets[v].curve, lag_sets[v].pts + (n - 1) * pw}}, &l,
                 &t.acc_lag_ms);
      level_scalars(p);
      launch_fr_from_dev(dtmp, n, st);
      run255.run(dtmp, nullptr, 0, n, {tau_sets[v]}, &r, &t.acc_tau_ms);
      if (!(v == 1 ? same_jac(l.g2, r.g2) : same_jac(l.g1, r.g1)))
        return bad("Lagrange section " + std::to_string(lag_id[v]) + " does not match section " +
                   std::to_string(tau_id[v]) + " at level " + std::to_string(p));
    }
    // the whole differs but no level does: the sums above are wrong, not the file
    throw ZkpError(ZKP_ERR_INTERNAL, "ptau verify: Lagrange section " + std::to_string(lag_id[v]) + " fails as a whole but at no level");
  }
  return verdict(true, "OK");
}

}  // namespace zkp
