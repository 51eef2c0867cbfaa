// Setup acceleration, phase 1 start: `snarkjs powersoftau contribute <in> <out>` and `powersoftau beacon`
// (reference circuit/scripts/generate_keys_phase1.sh:8,10,18) on the GPU.  A contribution multiplies every
// point of sections 2-5 by its own scalar,
//   tauG1[i] tau^i,  tauG2[i] tau^i,  alphaTauG1[i] alpha tau^i,  betaTauG1[i] beta tau^i,  betaG2 beta
// (5 * 2^power - 1 variable-base, variable-scalar multiplications, 2^power of them in G2), appends a record to
// section 7 and writes sections 1-7; sections 12-15 of the input are dropped (the contribution invalidates
// them) and any other id is not copied.  The byte-level model is tests/helpers/ptau_model.py contribute.
//
// A truncated file (power < ceremonyPower) is refused: the next challenge hashes the sections of the whole
// ceremony, which such a file no longer holds.
//
// Pass 1 (k_scale_powers).  The sections stream through the device in chunks of ZKP_PTAU_CHUNK points on two
// slots, each with its own stream and buffers: while one chunk computes, the next uploads and the previous
// one downloads.  A chunk is checked (k_check_points: canonical and on the curve), scaled, and leaves as the
// zkey-layout bytes of the file and as the compressed form the partial hash reads.  A host thread hashes the
// compressed chunks in order while the device works on later ones.
//
// Pass 2 (k_encode_points).  nextChallenge = Blake2b(responseHash || the new sections uncompressed), and
// responseHash continues the FINISHED partial hash over the key: its first block cannot be compressed before
// pass 1 and its hash are done, so the two hashes cannot run side by side.  The uncompressed bytes are
// therefore made in a second pass over the file's new sections (upload, encode, download: memory traffic
// only) instead of being kept for the whole file beside it; a second host thread hashes them in order.
// The same holds at the start: a file without contributions answers first_challenge(ceremonyPower), which the
// partial hash begins with; the thread that runs the partial hash computes it first.
//
// The working set is the two slots' chunk buffers, on the device and pinned on the host.  The passes, the
// slots and the kernels are ptau_stream.hip; this unit holds the two commands and points_scale_powers.
#include <chrono>
#include <cstring>
#include <future>
#include <string>
#include <thread>
#include <vector>

#include "hip_check.hpp"
#include "host_ec.hpp"
#include "prover.hpp"
#include "ptau_contribute.hpp"
#include "ptau_stream.hpp"
#include "ptau_verify.hpp"
#include "spans.hpp"

namespace zkp {

using namespace pstream;

namespace {

thread_local PtauContributeTimings g_timings;

// a 256-bit LE value reduced mod r, as standard-form words
void reduced_words(const uint8_t* le32, uint32_t (&w)[8]) {
  host::U256 v = host::u256_from_le(le32);
  while (host::u256_geq(v, host::FR_DESC.mod)) host::u256_sub(v, host::FR_DESC.mod);
  words_of(v, w);
}

}  // namespace

PtauContributeTimings& ptau_contribute_timings() { return g_timings; }

void points_scale_powers(int device, bool g2, const uint8_t* points, size_t n, const uint8_t* first32,
                         const uint8_t* ratio32, uint8_t* out) {
  const size_t ch = ptau_chunk_points();
  const int wb = window_bits();
  if (!n) return;
  std::vector<Job> jobs(1);
  jobs[0] = Job{0, g2, n, points, out, {}, {}, nullptr};
  reduced_words(first32, jobs[0].first);
  reduced_words(ratio32, jobs[0].ratio);
  HIPX(hipSetDevice(device));
  Slot slot[2];
  make_slots(slot, jobs, ch, false);
  Spans sp;
  PtauContributeTimings t;
  scale_pass(slot, jobs, chunks_of(jobs, ch), wb, nullptr, ZKP_ERR_INVALID_ARG, "scale powers: ", sp, t);
}

std::vector<uint8_t> ptau_contribute(int device, const uint8_t* ptau, size_t len, ChaChaRng& rng, uint32_t type,
                                     const char* name, const uint8_t* beacon, size_t beacon_len,
                                     uint32_t num_iterations_exp) {
  const auto t_begin = std::chrono::steady_clock::now();
  PtauContributeTimings t;
  // ---- everything that can be refused without the device
  const PtauFile f = parse_ptau(ptau, len);
  uint8_t challenge[64];
  const bool have_challenge = ptau_last_challenge(f.sec[7].ptr, f.sec[7].len, challenge);
  if (f.power < f.ceremony_power) throw ZkpError(ZKP_ERR_INVALID_ARG, "ptau: cannot contribute to a truncated file");
  if (type == 1 && num_iterations_exp > 63) throw ZkpError(ZKP_ERR_INVALID_ARG, "beacon: numIterationsExp must be <= 63");
  if (type == 1 && beacon_len > 255) throw ZkpError(ZKP_ERR_INVALID_ARG, "beacon: hash longer than 255 bytes");
  const size_t ch = ptau_chunk_points();
  const int wb = window_bits();
  t.parse_check_ms = wall_ms(t_begin);
  // ---- the secrets and the G1 half of the key: nothing here needs the challenge
  auto t0 = std::chrono::steady_clock::now();
  const PtauDraw draw = ptau_draw(rng);
  t.key_ms = wall_ms(t0);
  // ---- the output file: sections 1-6 laid out, 7 appended at the end
  const size_t N = f.N();
  std::vector<uint8_t> out;
  uint8_t* sec_out[8] = {};
  ptau_layout(f, out, sec_out);
  std::vector<Job> jobs;
  {
    const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    uint32_t tau[8], alpha[8], beta[8];
    words_of(draw.prv[0], tau), words_of(draw.prv[1], alpha), words_of(draw.prv[2], beta);
    auto job = [&](int id, size_t n, const uint32_t (&first)[8], const uint32_t (&ratio)[8]) {
      Job j{id, PtauFile::is_g2(id), n, f.sec[id].ptr, sec_out[id], {}, {}, nullptr};
      std::memcpy(j.first, first, 32), std::memcpy(j.ratio, ratio, 32);
      jobs.push_back(j);
    };
    job(2, 2 * N - 1, one, tau), job(3, N, one, tau), job(4, N, alpha, tau), job(5, N, beta, tau), job(6, 1, beta, one);
  }
  const std::vector<Chunk> chunks = chunks_of(jobs, ch);
  // ---- pass 1 beside the partial hash
  HIPX(hipSetDevice(device));
  Slot slot[2];
  make_slots(slot, jobs, ch, true);
  Spans sp;
  Blake2b partial;
  std::promise<void> challenge_ready;
  std::future<void> challenge_known = challenge_ready.get_future();
  HashThread ht1;
  ht1.th = std::thread([&] {
    auto h0 = std::chrono::steady_clock::now();
    try {
      if (!have_challenge) ptau_first_challenge(f.ceremony_power, challenge);
    } catch (...) {  // out of memory: handed to the caller's thread
      challenge_ready.set_exception(std::current_exception());
      ht1.feed.end();
      return;
    }
    t.challenge_ms = wall_ms(h0);
    challenge_ready.set_value();
    h0 = std::chrono::steady_clock::now();
    partial.update(challenge, 64);
    ht1.feed.drain(partial);
    t.partial_hash_ms = wall_ms(h0);
  });
  scale_pass(slot, jobs, chunks, wb, &ht1.feed, ZKP_ERR_FORMAT, "ptau: ", sp, t);
  challenge_known.get();
  ht1.finish();
  // ---- the record
  uint8_t five[448], response[64];
  std::memcpy(five, sec_out[2] + 64, 64), std::memcpy(five + 64, sec_out[3] + 128, 128);
  std::memcpy(five + 192, sec_out[4], 64), std::memcpy(five + 256, sec_out[5], 64), std::memcpy(five + 320, sec_out[6], 128);
  t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> rec = ptau_record(draw, challenge, five, partial, type, name, beacon, beacon_len, num_iterations_exp, response);
  t.key_ms += wall_ms(t0);
  // ---- pass 2 beside the next-challenge hash
  {
    Blake2b next;
    HashThread ht2;
    ht2.th = std::thread([&] {
      const auto h0 = std::chrono::steady_clock::now();
      next.update(response, 64);
      ht2.feed.drain(next);
      t.next_challenge_ms = wall_ms(h0);
    });
    encode_pass(slot, jobs, chunks, ht2.feed, sp, t);
    ht2.finish();
    next.final(rec.data() + PTAU_RECORD_NEXT_AT);
  }
  for (Slot& s : slot) HIPX(hipStreamSynchronize(s.st));
  sp.collect();
  ptau_append_section7(f, out, rec);
  t.total_ms = wall_ms(t_begin);
  g_timings = t;
  return out;
}

}  // namespace zkp
