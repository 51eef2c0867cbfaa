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
// The working set is the two slots' chunk buffers, on the device and pinned on the host.
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <future>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "hip_check.hpp"
#include "hip_raii.hpp"
#include "host_ec.hpp"
#include "prover.hpp"
#include "ptau_contribute.hpp"
#include "ptau_scale_kernels.hpp"
#include "ptau_stream.hpp"
#include "ptau_verify.hpp"
#include "spans.hpp"
#include "zkey_verify.hpp"

namespace zkp {

using pscale::Powers;
using namespace pstream;

namespace {

// window bits of the ladder (gfft::scale): 2 measured 24 % (G1) and 44 % (G2) faster than 1 at power 20
// (profiles/ptau_contribute.json); ZKP_PTAU_WINDOW=1|2 overrides the default
constexpr int DEFAULT_WINDOW = 2;
constexpr int TPB = 128;
unsigned grid(size_t n) { return (unsigned)((n + TPB - 1) / TPB); }

// One thread per point: out_i = (base * ratio^i) * in_i as the streams that are asked for (null: skipped).
template <class F, int WB>
__global__ __launch_bounds__(TPB) void k_scale_powers(const uint32_t* __restrict__ in, size_t n, Powers pw,
                                                      uint32_t* __restrict__ lem, uint32_t* __restrict__ u,
                                                      uint32_t* __restrict__ c) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const Xyzz<F> r = pscale::scale_lane<F, WB>(in, pw, i);
  pscale::encode_xyzz<F>(r, pw.to_zkey, lem, u, c, i);
}

struct alignas(16) ToZkey {
  uint32_t w[8];
};

// One thread per zkey-layout point (canonical): its other encodings
template <class F>
__global__ __launch_bounds__(TPB) void k_encode_points(const uint32_t* __restrict__ in, size_t n, ToZkey k,
                                                       uint32_t* __restrict__ lem, uint32_t* __restrict__ u,
                                                       uint32_t* __restrict__ c) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  pscale::encode_lem<F>(in, k.w, lem, u, c, i);
}

}  // namespace

int pstream::window_bits() {
  const char* e = std::getenv("ZKP_PTAU_WINDOW");
  if (!e || !*e) return DEFAULT_WINDOW;
  if ((e[0] != '1' && e[0] != '2') || e[1])
    throw ZkpError(ZKP_ERR_INVALID_ARG, std::string("ZKP_PTAU_WINDOW: 1 or 2 (got '") + e + "')");
  return e[0] - '0';
}

namespace {

void launch_scale(bool g2, int wb, const uint32_t* in, size_t n, const Powers& pw, uint32_t* lem, uint32_t* u, uint32_t* c,
                  hipStream_t st) {
  if (!n) return;
  const dim3 g(grid(n)), b(TPB);
  if (g2 && wb == 2)
    hipLaunchKernelGGL((k_scale_powers<Fq2, 2>), g, b, 0, st, in, n, pw, lem, u, c);
  else if (g2)
    hipLaunchKernelGGL((k_scale_powers<Fq2, 1>), g, b, 0, st, in, n, pw, lem, u, c);
  else if (wb == 2)
    hipLaunchKernelGGL((k_scale_powers<Fq, 2>), g, b, 0, st, in, n, pw, lem, u, c);
  else
    hipLaunchKernelGGL((k_scale_powers<Fq, 1>), g, b, 0, st, in, n, pw, lem, u, c);
  HIPX(hipGetLastError());
}

void launch_encode(bool g2, const uint32_t* in, size_t n, const ToZkey& k, uint32_t* lem, uint32_t* u, uint32_t* c,
                   hipStream_t st) {
  if (!n) return;
  if (g2)
    hipLaunchKernelGGL(k_encode_points<Fq2>, dim3(grid(n)), dim3(TPB), 0, st, in, n, k, lem, u, c);
  else
    hipLaunchKernelGGL(k_encode_points<Fq>, dim3(grid(n)), dim3(TPB), 0, st, in, n, k, lem, u, c);
  HIPX(hipGetLastError());
}

double wall_ms(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

thread_local PtauContributeTimings g_timings;

// a 256-bit LE value reduced mod r, as standard-form words
void reduced_words(const uint8_t* le32, uint32_t (&w)[8]) {
  host::U256 v = host::u256_from_le(le32);
  while (host::u256_geq(v, host::FR_DESC.mod)) host::u256_sub(v, host::FR_DESC.mod);
  for (int i = 0; i < 4; ++i) w[2 * i] = (uint32_t)v.w[i], w[2 * i + 1] = (uint32_t)(v.w[i] >> 32);
}
void words_of(const host::U256& v, uint32_t (&w)[8]) {
  for (int i = 0; i < 4; ++i) w[2 * i] = (uint32_t)v.w[i], w[2 * i + 1] = (uint32_t)(v.w[i] >> 32);
}

}  // namespace

void HashFeed::publish(const uint8_t* p, size_t len) {
  {
    std::lock_guard<std::mutex> g(m_);
    items_.push_back({p, len});
  }
  cv_.notify_all();
}
void HashFeed::close() {
  {
    std::lock_guard<std::mutex> g(m_);
    closed_ = true;
  }
  cv_.notify_all();
}
void HashFeed::wait_consumed(size_t k) {
  std::unique_lock<std::mutex> g(m_);
  cv_.wait(g, [&] { return done_ > k || ended_; });
}
void HashFeed::end() {
  {
    std::lock_guard<std::mutex> g(m_);
    ended_ = true;
  }
  cv_.notify_all();
}
void HashFeed::drain(Blake2b& h) {
  for (;;) {
    std::pair<const uint8_t*, size_t> it;
    {
      std::unique_lock<std::mutex> g(m_);
      cv_.wait(g, [&] { return done_ < items_.size() || closed_; });
      if (done_ == items_.size()) return;
      it = items_[done_];
    }
    h.update(it.first, it.second);
    {
      std::lock_guard<std::mutex> g(m_);
      ++done_;
    }
    cv_.notify_all();
  }
}

std::vector<Chunk> pstream::chunks_of(const std::vector<Job>& jobs, size_t ch) {
  std::vector<Chunk> v;
  for (size_t j = 0; j < jobs.size(); ++j)
    for (size_t at = 0; at < jobs[j].n; at += ch) v.push_back(Chunk{(int)j, at, std::min(ch, jobs[j].n - at)});
  return v;
}

void pstream::make_slots(Slot (&slot)[2], const std::vector<Job>& jobs, size_t ch, bool hashes) {
  size_t bytes = 0;
  for (const Job& j : jobs) bytes = std::max(bytes, std::min(ch, j.n) * (j.g2 ? 128 : 64));
  for (Slot& s : slot) {
    s.st = Stream(hipStreamNonBlocking);
    s.a = DevBuf<>(bytes / 4), s.b = DevBuf<>(bytes / 4);
    s.dbad = DevBuf<unsigned long long>(2);
    s.hlem = PinnedBuf<uint8_t>(bytes);
    s.hbad = PinnedBuf<unsigned long long>(2);
    s.done = Event(false);
    if (hashes) s.c = DevBuf<>(bytes / 8), s.henc = PinnedBuf<uint8_t>(bytes);
  }
}

// Pass 1 over the chunks (ptau_stream.hpp)
void pstream::scale_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, int wb,
                         HashFeed* feed, zkp_status bad_status, const char* bad_prefix, Spans& sp, PtauContributeTimings& t,
                         double* decode_ms) {
  bool enc = feed != nullptr;
  for (const Job& j : jobs) enc = enc || j.out_enc;
  auto finish = [&](size_t k) {
    const auto t0 = std::chrono::steady_clock::now();
    Slot& s = slot[k % 2];
    const Chunk& c = chunks[k];
    const Job& j = jobs[c.job];
    const size_t pb = j.g2 ? 128 : 64;
    HIPX(hipEventSynchronize(s.done));
    if (s.hbad[0])
      throw ZkpError(bad_status, std::string(bad_prefix) + (j.id ? "section " + std::to_string(j.id) + " " : "") + "point " +
                                     std::to_string(s.hbad[1]) + " is not on the curve");
    if (j.out) std::memcpy(j.out + c.start * pb, s.hlem.get(), c.m * pb);
    if (j.out_enc) std::memcpy(j.out_enc + c.start * pb / 2, s.henc.get(), c.m * pb / 2);
    if (feed) feed->publish(s.henc.get(), c.m * pb / 2);
    t.download_ms += wall_ms(t0);
  };
  for (size_t k = 0; k < chunks.size(); ++k) {
    Slot& s = slot[k % 2];
    const Chunk& c = chunks[k];
    const Job& j = jobs[c.job];
    const size_t pb = j.g2 ? 128 : 64;
    if (feed && k >= 2) feed->wait_consumed(k - 2);  // the slot's compressed bytes have been hashed
    Powers pw;
    pscale::fill_powers(pw, j.first, j.ratio, c.start);
    {
      const auto t0 = std::chrono::steady_clock::now();
      HIPX(hipMemcpyAsync(decode_ms ? s.b : s.a, j.in + c.start * pb, c.m * pb, hipMemcpyHostToDevice, s.st));
      t.upload_ms += wall_ms(t0);
    }
    points_bad_reset(s.dbad, s.st);
    if (decode_ms) {  // b is free until the scaling writes it: the staging buffer of the uncompressed bytes
      sp.begin(s.st);
      launch_decode(j.g2, s.b, c.m, c.start, s.a, s.dbad, s.st);
      sp.end(s.st, decode_ms);
    }
    sp.begin(s.st);
    points_check_resident(j.g2, s.a, c.m, c.start, s.dbad, s.st);
    sp.end(s.st, &t.parse_check_ms);
    sp.begin(s.st);
    launch_scale(j.g2, wb, s.a, c.m, pw, j.out ? s.b.get() : nullptr, nullptr, enc ? s.c.get() : nullptr, s.st);
    sp.end(s.st, j.g2 ? &t.g2_ms : &t.g1_ms);
    HIPX(hipMemcpyAsync(s.hbad.get(), s.dbad.get(), 16, hipMemcpyDeviceToHost, s.st));
    if (j.out) HIPX(hipMemcpyAsync(s.hlem.get(), s.b.get(), c.m * pb, hipMemcpyDeviceToHost, s.st));
    if (enc) HIPX(hipMemcpyAsync(s.henc.get(), s.c.get(), c.m * pb / 2, hipMemcpyDeviceToHost, s.st));
    HIPX(hipEventRecord(s.done, s.st));
    ++t.chunks;
    if (k >= 1) finish(k - 1);
  }
  if (!chunks.empty()) finish(chunks.size() - 1);
}

// Pass 2: the new sections uncompressed, to the hashing thread (ptau_stream.hpp)
void pstream::encode_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, HashFeed& feed,
                          Spans& sp, PtauContributeTimings& t, bool from_in) {
  ToZkey tz;
  pscale::fill_to_zkey(tz.w);
  auto finish = [&](size_t k) {
    const auto t0 = std::chrono::steady_clock::now();
    Slot& s = slot[k % 2];
    const Chunk& c = chunks[k];
    const Job& j = jobs[c.job];
    const size_t pb = j.g2 ? 128 : 64;
    HIPX(hipEventSynchronize(s.done));
    if (j.out_enc) std::memcpy(j.out_enc + c.start * pb, s.henc.get(), c.m * pb);
    feed.publish(s.henc.get(), c.m * pb);
    t.download_ms += wall_ms(t0);
  };
  for (size_t k = 0; k < chunks.size(); ++k) {
    Slot& s = slot[k % 2];
    const Chunk& c = chunks[k];
    const Job& j = jobs[c.job];
    const size_t pb = j.g2 ? 128 : 64;
    if (k >= 2) feed.wait_consumed(k - 2);
    {
      const auto t0 = std::chrono::steady_clock::now();
      HIPX(hipMemcpyAsync(s.a, (from_in ? j.in : j.out) + c.start * pb, c.m * pb, hipMemcpyHostToDevice, s.st));
      t.upload_ms += wall_ms(t0);
    }
    sp.begin(s.st);
    launch_encode(j.g2, s.a, c.m, tz, nullptr, s.b, nullptr, s.st);
    sp.end(s.st, &t.encode_ms);
    HIPX(hipMemcpyAsync(s.henc.get(), s.b.get(), c.m * pb, hipMemcpyDeviceToHost, s.st));
    HIPX(hipEventRecord(s.done, s.st));
    if (k >= 1) finish(k - 1);
  }
  if (!chunks.empty()) finish(chunks.size() - 1);
}

void pstream::ptau_layout(const PtauFile& f, std::vector<uint8_t>& out, uint8_t* (&sec_out)[8]) {
  size_t body = 12 + 12 + f.sec[1].len;
  for (int id = 2; id <= 6; ++id) body += 12 + f.sec[id].len;
  out.reserve(body + 12 + f.sec[7].len + 2048);  // section 7 with its new record is appended: no reallocation
  out.resize(body);
  uint8_t* o = out.data();
  auto put32 = [&](uint32_t x) { std::memcpy(o, &x, 4), o += 4; };
  auto put64 = [&](uint64_t x) { std::memcpy(o, &x, 8), o += 8; };
  std::memcpy(o, "ptau", 4), o += 4;
  put32(1), put32(7);
  put32(1), put64(f.sec[1].len);
  std::memcpy(o, f.sec[1].ptr, f.sec[1].len), o += f.sec[1].len;
  for (int id = 2; id <= 6; ++id) {
    put32((uint32_t)id), put64(f.sec[id].len);
    sec_out[id] = o, o += f.sec[id].len;
  }
}

// section 7: the count, the earlier records, the new one
void pstream::ptau_append_section7(const PtauFile& f, std::vector<uint8_t>& out, const std::vector<uint8_t>& rec) {
  const size_t old = f.sec[7].len - 4, s7 = 4 + old + rec.size();
  uint32_t count;
  std::memcpy(&count, f.sec[7].ptr, 4);
  ++count;
  const uint32_t id = 7;
  const uint64_t l64 = s7;
  auto app = [&](const void* p, size_t n) { out.insert(out.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
  app(&id, 4), app(&l64, 8), app(&count, 4), app(f.sec[7].ptr + 4, old), app(rec.data(), rec.size());
}

PtauContributeTimings& ptau_contribute_timings() { return g_timings; }

size_t ptau_chunk_points() {
  constexpr size_t DEFAULT = size_t(1) << 22, MAX = size_t(1) << 26;
  const char* e = std::getenv("ZKP_PTAU_CHUNK");
  if (!e) return DEFAULT;
  char* stop = nullptr;
  const long long v = std::strtoll(e, &stop, 10);
  if (!*e || *stop || v < 1 || (unsigned long long)v > MAX)
    throw ZkpError(ZKP_ERR_INVALID_ARG, "ZKP_PTAU_CHUNK: points per chunk must be an integer within 1.." +
                                            std::to_string(MAX) + " (got '" + e + "')");
  return (size_t)v;
}

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
