// `snarkjs zkey export bellman | zkey bellman contribute | zkey import bellman` on the GPU; zkey_bellman.hpp has
// the file format and the change of basis of the H section.  Every per-point pass streams through the two slots
// of ptau_stream.hpp in chunks of ZKP_PTAU_CHUNK points (convert_pass: decode, point check, scaling, encode).
//
// export bellman      section 9 through the forward group FFT (group_fft, the kernels of gfft_kernels.hpp), then
//                     with IC, L, A, B1, B2: upload the zkey-layout chunk, k_check_points, k_scale_powers with
//                     first = -2, ratio = w2 (H) or k_encode_points (the rest), download into the file.
// bellman contribute  upload the uncompressed chunk, k_decode_points, k_check_points; H and L go through
//                     k_scale_powers with first = k^-1, ratio = 1 and its uncompressed stream into the new file;
//                     the other sections are only checked and their bytes copied.
// import bellman      upload the uncompressed chunk, k_decode_points, k_check_points; H goes through
//                     k_scale_powers with first = -1/2, ratio = w2^-1, gains B_(n-1) = infinity and goes through
//                     the inverse group FFT into section 9; L becomes section 8; IC, A, B1, B2 are compared with
//                     the old key's sections.
//
// The transform reads and writes host memory (group_fft / group_ifft), so the H section crosses the bus twice
// more than a fused pass would: 2 x 512 MB at the Venmo shape beside a transform of seconds.
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "consts.hpp"
#include "hip_check.hpp"
#include "hip_raii.hpp"
#include "host_ec.hpp"
#include "prover.hpp"
#include "ptau_stream.hpp"
#include "spans.hpp"
#include "zkey_bellman.hpp"

namespace zkp {

using namespace pstream;

namespace {

thread_local BellmanTimings g_timings;

using HFr = host::Fr;

HFr root_of_unity(int p) {  // Fr.w[p]
  host::U256 v;
  for (int i = 0; i < 4; ++i) v.w[i] = (uint64_t)FR_ROOTS_W[p][2 * i] | (uint64_t)FR_ROOTS_W[p][2 * i + 1] << 32;
  return HFr::from_std(v);
}

// a host point in the zkey layout (host::Fq holds the Montgomery 2^256 form the file stores; infinity: zeros)
void put_g1_lem(uint8_t* o, const host::Affine<host::Fq>& p) {
  std::memset(o, 0, 64);
  if (!p.inf) host::u256_to_le(p.x.v, o), host::u256_to_le(p.y.v, o + 32);
}
void put_g2_lem(uint8_t* o, const host::Affine<host::Fq2>& p) {
  std::memset(o, 0, 128);
  if (p.inf) return;
  host::u256_to_le(p.x.c0.v, o), host::u256_to_le(p.x.c1.v, o + 32);
  host::u256_to_le(p.y.c0.v, o + 64), host::u256_to_le(p.y.c1.v, o + 96);
}

void put32be(uint8_t* o, uint32_t v) { o[0] = (uint8_t)(v >> 24), o[1] = (uint8_t)(v >> 16), o[2] = (uint8_t)(v >> 8), o[3] = (uint8_t)v; }

Job make_job(const char* name, bool g2, size_t n, const uint8_t* in, uint8_t* out, uint8_t* out_enc) {
  Job j{0, g2, n, in, out, {}, {}, out_enc};
  j.name = name;
  return j;
}
void set_scale(Job& j, const HFr& first, const HFr& ratio) {
  j.scale = true;
  words_of(first.to_std(), j.first), words_of(ratio.to_std(), j.ratio);
}

// the pass over jobs on `device`, its device and transfer times into t
void run_pass(int device, const std::vector<Job>& jobs, size_t ch, int wb, const Convert& cv, BellmanTimings& t,
              double BellmanTimings::*scaling) {
  HIPX(hipSetDevice(device));
  Slot slot[2];
  make_slots(slot, jobs, ch, false);
  Spans sp;
  PtauChallengeTimings pt;
  convert_pass(slot, jobs, chunks_of(jobs, ch), wb, cv, sp, pt);
  for (Slot& s : slot) HIPX(hipStreamSynchronize(s.st));
  sp.collect();
  t.upload_ms += pt.upload_ms, t.decode_ms += pt.decode_ms, t.check_ms += pt.parse_check_ms;
  t.*scaling += pt.g1_ms + pt.g2_ms;
  t.encode_ms += pt.encode_ms, t.download_ms += pt.download_ms, t.chunks += pt.chunks;
}

// the sections of a key that the file carries, validated beyond parse_zkey: sections 3 and 10
struct KeyView {
  ZkeyParsed z;
  MpcParams mpc;
  size_t n_ic, n_l, n;
};
KeyView read_key(const uint8_t* zkey, size_t len) {
  KeyView k{parse_zkey(zkey, len, false), {}, 0, 0, 0};
  const Section* s = k.z.bf.sec;
  const ZkeyHeader& hd = k.z.hdr;
  for (int id : {3, 5, 6, 7, 8, 9, 10})
    if (!s[id].ptr) throw ZkpError(ZKP_ERR_FORMAT, "zkey: missing section " + std::to_string(id));
  k.n_ic = (size_t)hd.n_public + 1, k.n = hd.domain_size;
  if (hd.n_vars < k.n_ic) throw ZkpError(ZKP_ERR_FORMAT, "zkey: fewer signals than public inputs");
  k.n_l = (size_t)hd.n_vars - k.n_ic;
  const uint64_t want[10] = {0, 0, 0, k.n_ic * 64, 0, (uint64_t)hd.n_vars * 64, (uint64_t)hd.n_vars * 64, (uint64_t)hd.n_vars * 128,
                             k.n_l * 64, k.n * 64};
  for (int id : {3, 5, 6, 7, 8, 9})
    if (s[id].len != want[id])
      throw ZkpError(ZKP_ERR_FORMAT, "zkey: section " + std::to_string(id) + " has " + std::to_string(s[id].len) +
                                         " bytes, its header wants " + std::to_string(want[id]));
  if (hd.log_domain > 27) throw ZkpError(ZKP_ERR_FORMAT, "zkey: domain above 2^27");
  k.mpc = read_mpc(s[10].ptr, s[10].len);
  return k;
}

// bytes of the file of a key with these counts and nc contributions; the offsets of its parts in at[]:
// IC, H, L, A, B1, B2 (their first point), csHash, the contribution count
size_t file_layout(size_t n_ic, size_t n, size_t n_l, size_t n_vars, size_t nc, size_t (&at)[8]) {
  size_t o = MPCPARAMS_HEADER;
  const size_t cnt[6] = {n_ic, n - 1, n_l, n_vars, n_vars, n_vars};
  for (int k = 0; k < 6; ++k) at[k] = o + 4, o += 4 + cnt[k] * (k == 5 ? 128 : 64);
  at[6] = o, o += 64;
  at[7] = o, o += 4 + nc * MPCPARAMS_CONTRIBUTION;
  return o;
}

}  // namespace

BellmanTimings& zkey_bellman_timings() { return g_timings; }

std::vector<uint8_t> zkey_export_bellman(int device, const uint8_t* zkey, size_t len) {
  const auto t_begin = std::chrono::steady_clock::now();
  BellmanTimings t;
  // ---- everything that can be refused without the device
  const KeyView k = read_key(zkey, len);
  const Section* s = k.z.bf.sec;
  const ZkeyHeader& hd = k.z.hdr;
  const size_t ch = ptau_chunk_points();
  const int wb = window_bits();
  size_t at[8];
  std::vector<uint8_t> out(file_layout(k.n_ic, k.n, k.n_l, hd.n_vars, k.mpc.contributions.size(), at));
  mpcparams_header(hd.alpha1, hd.beta1, hd.beta2, hd.gamma2, hd.delta1, hd.delta2, out.data());
  const size_t cnt[6] = {k.n_ic, k.n - 1, k.n_l, hd.n_vars, hd.n_vars, hd.n_vars};
  for (int i = 0; i < 6; ++i) put32be(out.data() + at[i] - 4, (uint32_t)cnt[i]);
  std::memcpy(out.data() + at[6], k.mpc.cs_hash, 64);
  put32be(out.data() + at[7], (uint32_t)k.mpc.contributions.size());
  for (size_t i = 0; i < k.mpc.contributions.size(); ++i)
    mpcparams_put_contribution(k.mpc.contributions[i], out.data() + at[7] + 4 + i * MPCPARAMS_CONTRIBUTION);
  t.parse_ms = wall_ms(t_begin);
  // ---- H: sum_j w^(ij) H_j, all n of them; the pass below scales the first n - 1 and drops the last
  std::vector<uint8_t> hf(k.n * 64);
  group_fft(device, false, s[9].ptr, (int)hd.log_domain, hf.data(), &t.transform_ms);
  // ---- the sections
  std::vector<Job> jobs;
  jobs.push_back(make_job("IC", false, cnt[0], s[3].ptr, nullptr, out.data() + at[0]));
  jobs.push_back(make_job("H", false, cnt[1], hf.data(), nullptr, out.data() + at[1]));
  const HFr two = HFr::from_std(host::U256{{2, 0, 0, 0}});
  set_scale(jobs.back(), two.neg(), root_of_unity((int)hd.log_domain + 1));
  jobs.push_back(make_job("L", false, cnt[2], s[8].ptr, nullptr, out.data() + at[2]));
  jobs.push_back(make_job("A", false, cnt[3], s[5].ptr, nullptr, out.data() + at[3]));
  jobs.push_back(make_job("B1", false, cnt[4], s[6].ptr, nullptr, out.data() + at[4]));
  jobs.push_back(make_job("B2", true, cnt[5], s[7].ptr, nullptr, out.data() + at[5]));
  run_pass(device, jobs, ch, wb, Convert{false, true, "zkey: "}, t, &BellmanTimings::coset_ms);
  t.total_ms = wall_ms(t_begin);
  g_timings = t;
  return out;
}

std::vector<uint8_t> zkey_bellman_contribute(int device, const uint8_t* challenge, size_t len, ChaChaRng& rng, uint8_t* hash64) {
  const auto t_begin = std::chrono::steady_clock::now();
  BellmanTimings t;
  // ---- everything that can be refused without the device
  const MpcParamsFile f = mpcparams_parse(challenge, len);
  const size_t ch = ptau_chunk_points();
  const int wb = window_bits();
  const host::Affine<host::Fq> alpha1 = mpcparams_g1(f.header, "alpha1"), beta1 = mpcparams_g1(f.header + 64, "beta1");
  const host::Affine<host::Fq2> beta2 = mpcparams_g2(f.header + 128, "beta2"), gamma2 = mpcparams_g2(f.header + 256, "gamma2");
  const host::Affine<host::Fq> delta1 = mpcparams_g1(f.header + MPCPARAMS_DELTA1_AT, "delta1");
  const host::Affine<host::Fq2> delta2 = mpcparams_g2(f.header + MPCPARAMS_DELTA2_AT, "delta2");
  MpcParams m = mpcparams_read_mpc(f);
  // ---- the secret and its proof of knowledge, as zkey contribute draws them
  uint8_t k32[32];
  mpc_contribute(m, rng, delta1, 0, std::string(), nullptr, 0, 0, k32);
  const HFr kinv = HFr::from_std(host::u256_from_le(k32)).inv();
  // ---- the new file: the old one with the new deltas and one contribution more
  std::vector<uint8_t> out(len + MPCPARAMS_CONTRIBUTION);
  std::memcpy(out.data(), challenge, len);
  const MpcContribution& c = m.contributions.back();
  mpcparams_header(alpha1, beta1, beta2, gamma2, c.delta_after, mpc_g2_times(delta2, k32), out.data());
  put32be(out.data() + (f.contributions - 4 - challenge), f.n_contributions + 1);
  mpcparams_put_contribution(c, out.data() + len);
  if (hash64) {
    Blake2b h;
    h.update(out.data() + len, MPCPARAMS_CONTRIBUTION);
    h.final(hash64);
  }
  t.parse_ms = wall_ms(t_begin);
  // ---- every point checked; H and L times k^-1
  auto dst = [&](const uint8_t* p) { return out.data() + (p - challenge); };
  std::vector<Job> jobs;
  jobs.push_back(make_job("IC", false, f.n_ic, f.ic, nullptr, nullptr));
  jobs.push_back(make_job("H", false, f.n_h, f.h, nullptr, dst(f.h)));
  set_scale(jobs.back(), kinv, HFr::one());
  jobs.push_back(make_job("L", false, f.n_l, f.l, nullptr, dst(f.l)));
  set_scale(jobs.back(), kinv, HFr::one());
  jobs.push_back(make_job("A", false, f.n_vars, f.a, nullptr, nullptr));
  jobs.push_back(make_job("B1", false, f.n_vars, f.b1, nullptr, nullptr));
  jobs.push_back(make_job("B2", true, f.n_vars, f.b2, nullptr, nullptr));
  run_pass(device, jobs, ch, wb, Convert{true, true, "mpcparams: "}, t, &BellmanTimings::scale_ms);
  t.total_ms = wall_ms(t_begin);
  g_timings = t;
  return out;
}

std::vector<uint8_t> zkey_import_bellman(int device, const uint8_t* old_zkey, size_t len, const uint8_t* response,
                                         size_t response_len, const char* name) {
  const auto t_begin = std::chrono::steady_clock::now();
  BellmanTimings t;
  // ---- everything that can be refused without the device
  const KeyView k = read_key(old_zkey, len);
  const Section* s = k.z.bf.sec;
  const ZkeyHeader& hd = k.z.hdr;
  const MpcParamsFile f = mpcparams_parse(response, response_len);
  const size_t ch = ptau_chunk_points();
  const int wb = window_bits();
  auto refuse = [](const std::string& m) { return ZkpError(ZKP_ERR_FORMAT, "mpcparams: " + m); };
  auto counts = [&](const char* what, uint64_t got, uint64_t want) {
    if (got != want)
      throw refuse(std::string(what) + " has " + std::to_string(got) + " points, the key wants " + std::to_string(want));
  };
  counts("IC", f.n_ic, k.n_ic), counts("H", f.n_h, k.n - 1), counts("L", f.n_l, k.n_l), counts("A", f.n_vars, hd.n_vars);
  if (std::memcmp(f.cs_hash, k.mpc.cs_hash, 64) != 0) throw refuse("csHash is not the key's");
  const size_t nc = k.mpc.contributions.size();
  if (f.n_contributions != nc + 1)
    throw refuse("contributions: the response has " + std::to_string(f.n_contributions) + ", the key has " + std::to_string(nc) +
                 " and wants exactly one more");
  for (size_t i = 0; i < nc; ++i) {
    uint8_t rec[MPCPARAMS_CONTRIBUTION];
    mpcparams_put_contribution(k.mpc.contributions[i], rec);
    if (std::memcmp(rec, f.contributions + i * MPCPARAMS_CONTRIBUTION, MPCPARAMS_CONTRIBUTION) != 0)
      throw refuse("contribution " + std::to_string(i) + " is not the key's");
  }
  {
    uint8_t hdr[MPCPARAMS_HEADER];
    mpcparams_header(hd.alpha1, hd.beta1, hd.beta2, hd.gamma2, hd.delta1, hd.delta2, hdr);
    const char* hname[4] = {"alpha1", "beta1", "beta2", "gamma2"};
    const size_t hat[5] = {0, 64, 128, 256, 384};
    for (int i = 0; i < 4; ++i)
      if (std::memcmp(hdr + hat[i], f.header + hat[i], hat[i + 1] - hat[i]) != 0) throw refuse(std::string(hname[i]) + " is not the key's");
  }
  const uint8_t* last = f.contributions + nc * MPCPARAMS_CONTRIBUTION;
  MpcContribution c;
  {
    const std::string what = "contribution " + std::to_string(nc);
    c.delta_after = mpcparams_g1(last, what + " deltaAfter");
    c.g1_s = mpcparams_g1(last + 64, what + " g1_s");
    c.g1_sx = mpcparams_g1(last + 128, what + " g1_sx");
    c.g2_spx = mpcparams_g2(last + 192, what + " g2_spx");
    std::memcpy(c.transcript, last + 320, 64);
    c.type = 0;
    if (name && *name) c.params = mpc_name_params(name);
  }
  if (std::memcmp(f.header + MPCPARAMS_DELTA1_AT, last, 64) != 0) throw refuse("delta1 is not the new contribution's deltaAfter");
  const host::Affine<host::Fq2> delta2 = mpcparams_g2(f.header + MPCPARAMS_DELTA2_AT, "delta2");
  // ---- the new key: the old one with sections 2, 8, 9 and 10 rewritten
  std::vector<uint8_t> out(old_zkey, old_zkey + len);
  auto off = [&](int id) { return (size_t)(s[id].ptr - old_zkey); };
  {
    const size_t d1 = off(2) + 4 + 32 + 4 + 32 + 12 + 64 + 64 + 128 + 128;
    put_g1_lem(out.data() + d1, c.delta_after), put_g2_lem(out.data() + d1 + 64, delta2);
  }
  t.parse_ms = wall_ms(t_begin);
  // ---- the sections: H scaled into hs (B_(n-1) = infinity stays zero), L into section 8, the rest compared
  std::vector<uint8_t> hs(k.n * 64, 0), ic(k.n_ic * 64), a((size_t)hd.n_vars * 64), b1((size_t)hd.n_vars * 64),
      b2((size_t)hd.n_vars * 128);
  std::vector<Job> jobs;
  jobs.push_back(make_job("IC", false, f.n_ic, f.ic, ic.data(), nullptr));
  jobs.push_back(make_job("H", false, f.n_h, f.h, hs.data(), nullptr));
  const HFr two = HFr::from_std(host::U256{{2, 0, 0, 0}});
  set_scale(jobs.back(), two.neg().inv(), root_of_unity((int)hd.log_domain + 1).inv());
  jobs.push_back(make_job("L", false, f.n_l, f.l, out.data() + off(8), nullptr));
  jobs.push_back(make_job("A", false, f.n_vars, f.a, a.data(), nullptr));
  jobs.push_back(make_job("B1", false, f.n_vars, f.b1, b1.data(), nullptr));
  jobs.push_back(make_job("B2", true, f.n_vars, f.b2, b2.data(), nullptr));
  run_pass(device, jobs, ch, wb, Convert{true, false, "mpcparams: "}, t, &BellmanTimings::coset_ms);
  auto t0 = std::chrono::steady_clock::now();
  auto same = [&](const char* what, const std::vector<uint8_t>& got, int id, size_t pb) {
    if (std::memcmp(got.data(), s[id].ptr, got.size()) == 0) return;
    size_t i = 0;
    while (std::memcmp(got.data() + i * pb, s[id].ptr + i * pb, pb) == 0) ++i;
    throw refuse(std::string(what) + " point " + std::to_string(i) + " is not the key's");
  };
  same("IC", ic, 3, 64), same("A", a, 5, 64), same("B1", b1, 6, 64), same("B2", b2, 7, 128);
  t.parse_ms += wall_ms(t0);
  group_ifft(device, false, hs.data(), (int)hd.log_domain, out.data() + off(9), &t.transform_ms);
  t0 = std::chrono::steady_clock::now();
  MpcParams m = k.mpc;
  m.contributions.push_back(std::move(c));
  binfile_replace_section(out, 10, write_mpc(m));
  t.parse_ms += wall_ms(t0);
  t.total_ms = wall_ms(t_begin);
  g_timings = t;
  return out;
}

}  // namespace zkp
