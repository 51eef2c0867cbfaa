// `snarkjs powersoftau export challenge | challenge contribute | import response` (reference
// circuit/scripts/generate_keys_phase1.sh:12-14) on the GPU; ptau_challenge.hpp has the formats.  All three
// stream the sections through the two slots of ptau_stream.hpp in chunks of ZKP_PTAU_CHUNK points.
//
// export challenge      upload the zkey-layout chunk, k_encode_points (uncompressed stream only), download
//                       into the challenge file; a host thread hashes the file in order and the result must be
//                       the challenge that section 7 implies.
// challenge contribute  upload the uncompressed chunk, k_decode_points (-> zkey layout), k_check_points,
//                       k_scale_powers with the compressed stream as its only output, download into the
//                       response file; the hash of the challenge file runs beside it on a host thread, and
//                       only the key's three G2 points wait for it.
// import response       upload the compressed chunk, k_decompress_points (-> zkey layout for the new file and
//                       uncompressed for the next-challenge hash), download both.  One pass: the response
//                       hash, with which the next-challenge hash begins, is the hash of the response file
//                       itself, which the hashing thread computes from the input before it takes the chunks.
//
// The passes, the slots and the kernels of the three are ptau_stream.hip; this unit holds the commands and the
// kernel-level entries of ptau_challenge.hpp.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <future>
#include <string>
#include <thread>
#include <vector>

#include "hip_check.hpp"
#include "hip_raii.hpp"
#include "host_ec.hpp"
#include "prover.hpp"
#include "ptau_challenge.hpp"
#include "ptau_decompress_kernels.hpp"
#include "ptau_stream.hpp"
#include "ptau_verify.hpp"
#include "spans.hpp"

namespace zkp {

using namespace pstream;

namespace {

template <class F>
__global__ __launch_bounds__(TPB) void k_field_sqrt(const uint32_t* __restrict__ in, size_t n, pdec::Consts k,
                                                    uint32_t* __restrict__ out, uint8_t* __restrict__ is_square) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  pdec::sqrt_lane<F>(in, k, out, is_square, i);
}

thread_local PtauChallengeTimings g_timings;

// points of section id at power N
size_t section_points(int id, size_t N) { return id == 2 ? 2 * N - 1 : id == 6 ? 1 : N; }

// What an old file must be for export and import: parsed, section 7 read, not truncated.  -> whether it has
// a contribution (then its last challenge and response hash are set)
bool read_old(const PtauFile& f, const char* verb, uint8_t challenge[64], uint8_t response[64]) {
  const bool have = ptau_last_hashes(f.sec[7].ptr, f.sec[7].len, challenge, response);
  if (f.power < f.ceremony_power)
    throw ZkpError(ZKP_ERR_INVALID_ARG, std::string("ptau: cannot ") + verb + " a truncated file");
  return have;
}

}  // namespace

PtauChallengeTimings& ptau_challenge_timings() { return g_timings; }

void points_decompress(int device, bool g2, const uint8_t* compressed, size_t n, uint8_t* out_lem, uint64_t* n_bad,
                       uint64_t* first_bad) {
  points_to_zkey(device, g2, true, compressed, n, out_lem, n_bad, first_bad);
}

void points_from_uncompressed(int device, bool g2, const uint8_t* bytes, size_t n, uint8_t* out_lem, uint64_t* n_bad,
                              uint64_t* first_bad) {
  points_to_zkey(device, g2, false, bytes, n, out_lem, n_bad, first_bad);
}

void field_sqrt(int device, bool fq2, const uint8_t* in, size_t n, uint8_t* out, uint8_t* is_square) {
  const size_t eb = fq2 ? 64 : 32;
  for (size_t i = 0; i < n * (eb / 32); ++i)
    if (host::u256_geq(host::u256_from_le(in + 32 * i), host::FQ_DESC.mod))
      throw ZkpError(ZKP_ERR_INVALID_ARG, "field sqrt: element " + std::to_string(i / (eb / 32)) + " has a coordinate >= p");
  const size_t ch = ptau_chunk_points();
  if (!n) return;
  pdec::Consts k;
  pdec::fill_consts(k, false);
  HIPX(hipSetDevice(device));
  const size_t CH = std::min(n, ch);
  DevBuf<> din(CH * eb / 4), dout(CH * eb / 4);
  DevBuf<uint8_t> dsq(CH);
  Stream st(hipStreamNonBlocking);
  for (size_t at = 0; at < n; at += CH) {
    const size_t m = std::min(CH, n - at);
    HIPX(hipMemcpyAsync(din, in + at * eb, m * eb, hipMemcpyHostToDevice, st));
    if (fq2)
      hipLaunchKernelGGL(k_field_sqrt<Fq2>, dim3(grid(m)), dim3(TPB), 0, st, din.get(), m, k, dout.get(), dsq.get());
    else
      hipLaunchKernelGGL(k_field_sqrt<Fq>, dim3(grid(m)), dim3(TPB), 0, st, din.get(), m, k, dout.get(), dsq.get());
    HIPX(hipGetLastError());
    HIPX(hipMemcpyAsync(out + at * eb, dout, m * eb, hipMemcpyDeviceToHost, st));
    HIPX(hipMemcpyAsync(is_square + at, dsq, m, hipMemcpyDeviceToHost, st));
    HIPX(hipStreamSynchronize(st));
  }
}

std::vector<uint8_t> ptau_export_challenge(int device, const uint8_t* ptau, size_t len) {
  const auto t_begin = std::chrono::steady_clock::now();
  PtauChallengeTimings t;
  // ---- everything that can be refused without the device
  const PtauFile f = parse_ptau(ptau, len);
  uint8_t challenge[64], last_response[64];
  const bool have = read_old(f, "export the challenge of", challenge, last_response);
  const size_t ch = ptau_chunk_points();
  t.parse_check_ms = wall_ms(t_begin);
  if (!have) Blake2b().final(last_response);
  const size_t N = f.N();
  std::vector<uint8_t> out(384 * N + 128);
  std::memcpy(out.data(), last_response, 64);
  std::vector<Job> jobs;
  {
    uint8_t* o = out.data() + 64;
    for (int id = 2; id <= 6; ++id) {
      jobs.push_back(Job{id, PtauFile::is_g2(id), f.points(id), f.sec[id].ptr, nullptr, {}, {}, o});
      o += f.sec[id].len;
    }
  }
  const std::vector<Chunk> chunks = chunks_of(jobs, ch);
  // a file without contributions answers first_challenge(ceremonyPower): hashed beside the rest
  std::future<void> first;
  if (!have)
    first = std::async(std::launch::async, [&] {
      const auto h0 = std::chrono::steady_clock::now();
      ptau_first_challenge(f.ceremony_power, challenge);
      t.challenge_ms = wall_ms(h0);
    });
  HIPX(hipSetDevice(device));
  Slot slot[2];
  make_slots(slot, jobs, ch, false);
  for (Slot& s : slot) s.henc = PinnedBuf<uint8_t>(s.hlem.count());
  Spans sp;
  uint8_t got[64];
  {
    Blake2b h;
    HashThread ht;
    ht.th = std::thread([&] {
      const auto h0 = std::chrono::steady_clock::now();
      h.update(last_response, 64);
      ht.feed.drain(h);
      t.next_challenge_ms = wall_ms(h0);
    });
    encode_pass(slot, jobs, chunks, ht.feed, sp, t, true);
    t.chunks = chunks.size();
    ht.finish();
    h.final(got);
  }
  for (Slot& s : slot) HIPX(hipStreamSynchronize(s.st));
  sp.collect();
  if (first.valid()) first.get();
  if (std::memcmp(got, challenge, 64) != 0)
    throw ZkpError(ZKP_ERR_FORMAT, "ptau: sections 2-6 do not hash to the last contribution's nextChallenge");
  t.total_ms = wall_ms(t_begin);
  g_timings = t;
  return out;
}

std::vector<uint8_t> ptau_challenge_contribute(int device, const uint8_t* challenge, size_t len, ChaChaRng& rng) {
  const auto t_begin = std::chrono::steady_clock::now();
  PtauChallengeTimings t;
  // ---- the power is read from the length
  size_t N = 0;
  if (len >= 128 && (len - 128) % 384 == 0) N = (len - 128) / 384;
  if (N < 2 || N > (size_t(1) << 28) || (N & (N - 1)))
    throw ZkpError(ZKP_ERR_FORMAT, "challenge: a file of " + std::to_string(len) +
                                       " bytes is not 384 * 2^power + 128 with power within 1..28");
  const size_t ch = ptau_chunk_points();
  const int wb = window_bits();
  t.parse_check_ms = wall_ms(t_begin);
  // ---- the secrets and the G1 half of the key: nothing here needs the challenge hash
  auto t0 = std::chrono::steady_clock::now();
  const PtauDraw draw = ptau_draw(rng);
  t.key_ms = wall_ms(t0);
  std::vector<uint8_t> out(192 * N + 864);
  std::vector<Job> jobs;
  {
    const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    uint32_t tau[8], alpha[8], beta[8];
    words_of(draw.prv[0], tau), words_of(draw.prv[1], alpha), words_of(draw.prv[2], beta);
    const uint8_t* in = challenge + 64;
    uint8_t* o = out.data() + 64;
    auto job = [&](int id, const uint32_t (&first)[8], const uint32_t (&ratio)[8]) {
      const size_t n = section_points(id, N), pb = PtauFile::is_g2(id) ? 128 : 64;
      Job j{id, PtauFile::is_g2(id), n, in, nullptr, {}, {}, o};
      std::memcpy(j.first, first, 32), std::memcpy(j.ratio, ratio, 32);
      jobs.push_back(j);
      in += n * pb, o += n * pb / 2;
    };
    job(2, one, tau), job(3, one, tau), job(4, alpha, tau), job(5, beta, tau), job(6, beta, one);
  }
  const std::vector<Chunk> chunks = chunks_of(jobs, ch);
  // ---- the hash of the challenge file beside the device work
  uint8_t hash[64];
  std::future<void> hashed = std::async(std::launch::async, [&] {
    const auto h0 = std::chrono::steady_clock::now();
    Blake2b h;
    h.update(challenge, len);
    h.final(hash);
    t.challenge_ms = wall_ms(h0);
  });
  HIPX(hipSetDevice(device));
  Slot slot[2];
  make_slots(slot, jobs, ch, true);
  Spans sp;
  decode_scale_pass(slot, jobs, chunks, wb, sp, t);
  for (Slot& s : slot) HIPX(hipStreamSynchronize(s.st));
  sp.collect();
  hashed.get();
  // ---- the key's G2 points answer the challenge hash
  t0 = std::chrono::steady_clock::now();
  std::memcpy(out.data(), hash, 64);
  uint8_t key_lem[768];
  ptau_key_forms(draw, hash, key_lem, out.data() + out.size() - 768);
  t.key_ms += wall_ms(t0);
  t.total_ms = wall_ms(t_begin);
  g_timings = t;
  return out;
}

std::vector<uint8_t> ptau_import_response(int device, const uint8_t* ptau, size_t len, const uint8_t* response,
                                          size_t response_len, const char* name) {
  const auto t_begin = std::chrono::steady_clock::now();
  PtauChallengeTimings t;
  // ---- everything that can be refused without the device
  const PtauFile f = parse_ptau(ptau, len);
  uint8_t challenge[64], last_response[64];
  const bool have = read_old(f, "import a response into", challenge, last_response);
  const size_t N = f.N();
  if (response_len != 192 * N + 864) throw ZkpError(ZKP_ERR_FORMAT, "response: size of the contribution is invalid");
  const size_t ch = ptau_chunk_points();
  t.parse_check_ms = wall_ms(t_begin);
  if (!have) {
    const auto h0 = std::chrono::steady_clock::now();
    ptau_first_challenge(f.ceremony_power, challenge);
    t.challenge_ms = wall_ms(h0);
  }
  if (std::memcmp(response, challenge, 64) != 0)
    throw ZkpError(ZKP_ERR_FORMAT, "response: this contribution is not based on the previous hash");
  const uint8_t* key_u = response + response_len - 768;
  uint8_t key_lem[768];
  auto t0 = std::chrono::steady_clock::now();
  ptau_key_from_uncompressed(key_u, key_lem);
  t.key_ms = wall_ms(t0);
  // ---- the output file: sections 1-6 laid out, 7 appended at the end
  std::vector<uint8_t> out;
  uint8_t* sec_out[8] = {};
  ptau_layout(f, out, sec_out);
  std::vector<Job> jobs;
  {
    const uint8_t* in = response + 64;
    for (int id = 2; id <= 6; ++id) {
      jobs.push_back(Job{id, PtauFile::is_g2(id), f.points(id), in, sec_out[id], {}, {}, nullptr});
      in += f.sec[id].len / 2;
    }
  }
  const std::vector<Chunk> chunks = chunks_of(jobs, ch);
  // ---- one pass beside the hashes: the response file's own (its state before the key is the record's
  // partial hash, its end the response hash), then the next challenge over the uncompressed chunks
  HIPX(hipSetDevice(device));
  Slot slot[2];
  make_slots(slot, jobs, ch, true);
  Spans sp;
  Blake2b partial, next;
  uint8_t response_hash[64];
  {
    HashThread ht;
    ht.th = std::thread([&] {
      auto h0 = std::chrono::steady_clock::now();
      partial.update(response, response_len - 768);
      Blake2b whole = partial;
      whole.update(key_u, 768);
      whole.final(response_hash);
      t.partial_hash_ms = wall_ms(h0);
      h0 = std::chrono::steady_clock::now();
      next.update(response_hash, 64);
      ht.feed.drain(next);
      t.next_challenge_ms = wall_ms(h0);
    });
    decompress_pass(slot, jobs, chunks, ht.feed, sp, t);
    ht.finish();
  }
  for (Slot& s : slot) HIPX(hipStreamSynchronize(s.st));
  sp.collect();
  // ---- the record
  uint8_t five[448], again[64];
  std::memcpy(five, sec_out[2] + 64, 64), std::memcpy(five + 64, sec_out[3] + 128, 128);
  std::memcpy(five + 192, sec_out[4], 64), std::memcpy(five + 256, sec_out[5], 64), std::memcpy(five + 320, sec_out[6], 128);
  std::vector<uint8_t> rec = ptau_record_of_key(key_lem, key_u, five, partial, 0, name, nullptr, 0, 0, again);
  next.final(rec.data() + PTAU_RECORD_NEXT_AT);
  ptau_append_section7(f, out, rec);
  t.total_ms = wall_ms(t_begin);
  g_timings = t;
  return out;
}

}  // namespace zkp
