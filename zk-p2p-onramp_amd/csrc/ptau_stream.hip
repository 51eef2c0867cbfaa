// The streaming of the ptau sections (ptau_stream.hpp): the feed to the hashing threads, the chunks and the two
// slots, the one loop that runs a pass over them (run_chunks), the four passes as what they enqueue per chunk
// and what they deliver from a finished slot, and the per-point kernels they launch.  The per-lane bodies are
// ptau_scale_kernels.hpp and ptau_decompress_kernels.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "hip_check.hpp"
#include "points_through.hpp"
#include "ptau_decompress_kernels.hpp"
#include "ptau_scale_kernels.hpp"
#include "ptau_stream.hpp"
#include "zkey_verify.hpp"

namespace zkp {

using pscale::Powers;
using namespace pstream;

namespace {

// window bits of the ladder (gfft::scale): 2 measured 24 % (G1) and 44 % (G2) faster than 1 at power 20
// (profiles/ptau_contribute.json); ZKP_PTAU_WINDOW=1|2 overrides the default
constexpr int DEFAULT_WINDOW = 2;

struct alignas(16) ToZkey {
  uint32_t w[8];
};

__device__ __forceinline__ void count_bad(unsigned long long* bad, uint64_t index) {
  atomicAdd(&bad[0], 1ull);
  atomicMin(&bad[1], (unsigned long long)index);
}

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

// One thread per zkey-layout point (canonical): its other encodings
template <class F>
__global__ __launch_bounds__(TPB) void k_encode_points(const uint32_t* __restrict__ in, size_t n, ToZkey k,
                                                       uint32_t* __restrict__ lem, uint32_t* __restrict__ u,
                                                       uint32_t* __restrict__ c) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  pscale::encode_lem<F>(in, k.w, lem, u, c, i);
}

// One thread per uncompressed point: its zkey layout (zeros and counted if refused)
template <class F>
__global__ __launch_bounds__(TPB) void k_decode_points(const uint32_t* __restrict__ in, size_t n, uint64_t base, ToZkey k,
                                                       uint32_t* __restrict__ lem, unsigned long long* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  if (pdec::decode_lane<F>(in, k.w, lem, i)) count_bad(bad, base + i);
}

// One thread per compressed point: y by a square root, then the streams that are asked for
template <class F>
__global__ __launch_bounds__(TPB) void k_decompress_points(const uint32_t* __restrict__ in, size_t n, uint64_t base,
                                                           pdec::Consts k, uint32_t* __restrict__ lem,
                                                           uint32_t* __restrict__ u, unsigned long long* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  if (pdec::decompress_lane<F>(in, k, lem, u, i)) count_bad(bad, base + i);
}

void launch_scale(bool g2, int wb, const uint32_t* in, size_t n, const Powers& pw, uint32_t* lem, uint32_t* u, uint32_t* c,
                  hipStream_t st) {
  if (!n) return;
  const auto k = g2 ? (wb == 2 ? k_scale_powers<Fq2, 2> : k_scale_powers<Fq2, 1>)
                    : (wb == 2 ? k_scale_powers<Fq, 2> : k_scale_powers<Fq, 1>);
  hipLaunchKernelGGL(k, dim3(grid(n)), dim3(TPB), 0, st, in, n, pw, lem, u, c);
  HIPX(hipGetLastError());
}

void launch_encode(bool g2, const uint32_t* in, size_t n, const ToZkey& k, uint32_t* lem, uint32_t* u, uint32_t* c,
                   hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL((g2 ? k_encode_points<Fq2> : k_encode_points<Fq>), dim3(grid(n)), dim3(TPB), 0, st, in, n, k, lem, u, c);
  HIPX(hipGetLastError());
}

// n uncompressed points at d_in -> zkey layout at d_lem; bad[0] += the refused points, bad[1] = min(bad[1],
// base + i) over them
void launch_decode(bool g2, const uint32_t* d_in, size_t n, uint64_t base, uint32_t* d_lem, unsigned long long* bad,
                   hipStream_t st) {
  if (!n) return;
  ToZkey k;
  pscale::fill_to_zkey(k.w);
  hipLaunchKernelGGL((g2 ? k_decode_points<Fq2> : k_decode_points<Fq>), dim3(grid(n)), dim3(TPB), 0, st, d_in, n, base, k,
                     d_lem, bad);
  HIPX(hipGetLastError());
}

void launch_decompress(bool g2, const uint32_t* in, size_t n, uint64_t base, const pdec::Consts& k, uint32_t* lem,
                       uint32_t* u, unsigned long long* bad, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL((g2 ? k_decompress_points<Fq2> : k_decompress_points<Fq>), dim3(grid(n)), dim3(TPB), 0, st, in, n, base,
                     k, lem, u, bad);
  HIPX(hipGetLastError());
}

// what a pass that counts bad points throws for the first of them: "<prefix>[section <id> ]point <i><cause>"
// (a job with a name: "<prefix><name> point <i><cause>")
struct Refusal {
  zkp_status status;
  const char* prefix;
  const char* cause;
};

// The two-slot loop.  Chunk k takes slot k % 2 once the hashing thread has consumed chunk k - 2 (whose
// bytes the slot's pinned buffer still held); enqueue(s, j, c) puts the chunk's upload, kernels and downloads
// on s.st.  Chunk k - 1 is finished while k computes: its event waited for, refused if the pass counts bad
// points (refusal) and it had one, else deliver(s, j, c) takes the slot's host buffers into the job's
// outputs and to the feed.  count: whether the chunks add to t.chunks.
template <class Enqueue, class Deliver>
void run_chunks(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, HashFeed* feed,
                const Refusal* refusal, PtauContributeTimings& t, bool count, Enqueue enqueue, Deliver deliver) {
  auto finish = [&](size_t k) {
    const auto t0 = std::chrono::steady_clock::now();
    Slot& s = slot[k % 2];
    const Chunk& c = chunks[k];
    const Job& j = jobs[c.job];
    HIPX(hipEventSynchronize(s.done));
    if (refusal && s.hbad[0])
      throw ZkpError(refusal->status, std::string(refusal->prefix) +
                                          (j.name ? std::string(j.name) + " " : j.id ? "section " + std::to_string(j.id) + " " : "") +
                                          "point " + std::to_string(s.hbad[1]) + refusal->cause);
    deliver(s, j, c);
    t.download_ms += wall_ms(t0);
  };
  for (size_t k = 0; k < chunks.size(); ++k) {
    Slot& s = slot[k % 2];
    const Chunk& c = chunks[k];
    if (feed && k >= 2) feed->wait_consumed(k - 2);
    enqueue(s, jobs[c.job], c);
    HIPX(hipEventRecord(s.done, s.st));
    if (count) ++t.chunks;
    if (k >= 1) finish(k - 1);
  }
  if (!chunks.empty()) finish(chunks.size() - 1);
}

void upload(Slot& s, uint32_t* dst, const uint8_t* src, size_t bytes, PtauContributeTimings& t) {
  const auto t0 = std::chrono::steady_clock::now();
  HIPX(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s.st));
  t.upload_ms += wall_ms(t0);
}

// The two scaling passes.  head(s, j, c) brings the chunk into s.a in the zkey layout; then the point check, the
// scaling into b (if the job keeps the zkey layout) and c (if the compressed stream is hashed or kept), the downloads.
template <class Head>
void scaling_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, int wb, HashFeed* feed,
                  const Refusal& refusal, Spans& sp, PtauContributeTimings& t, Head head) {
  bool enc = feed != nullptr;
  for (const Job& j : jobs) enc = enc || j.out_enc;
  run_chunks(
      slot, jobs, chunks, feed, &refusal, t, true,
      [&](Slot& s, const Job& j, const Chunk& c) {
        Powers pw;
        pscale::fill_powers(pw, j.first, j.ratio, c.start);
        head(s, j, c);
        sp.begin(s.st);
        points_check_resident(j.g2, s.a, c.m, c.start, s.dbad, s.st);
        sp.end(s.st, &t.parse_check_ms);
        sp.begin(s.st);
        launch_scale(j.g2, wb, s.a, c.m, pw, j.out ? s.b.get() : nullptr, nullptr, enc ? s.c.get() : nullptr, s.st);
        sp.end(s.st, j.g2 ? &t.g2_ms : &t.g1_ms);
        HIPX(hipMemcpyAsync(s.hbad.get(), s.dbad.get(), 16, hipMemcpyDeviceToHost, s.st));
        if (j.out) HIPX(hipMemcpyAsync(s.hlem.get(), s.b.get(), c.m * j.pb(), hipMemcpyDeviceToHost, s.st));
        if (enc) HIPX(hipMemcpyAsync(s.henc.get(), s.c.get(), c.m * j.pb() / 2, hipMemcpyDeviceToHost, s.st));
      },
      [&](Slot& s, const Job& j, const Chunk& c) {
        if (j.out) std::memcpy(j.out + c.start * j.pb(), s.hlem.get(), c.m * j.pb());
        if (j.out_enc) std::memcpy(j.out_enc + c.start * j.pb() / 2, s.henc.get(), c.m * j.pb() / 2);
        if (feed) feed->publish(s.henc.get(), c.m * j.pb() / 2);
      });
}

}  // namespace

int pstream::window_bits() {
  const char* e = std::getenv("ZKP_PTAU_WINDOW");
  if (!e || !*e) return DEFAULT_WINDOW;
  if ((e[0] != '1' && e[0] != '2') || e[1])
    throw ZkpError(ZKP_ERR_INVALID_ARG, std::string("ZKP_PTAU_WINDOW: 1 or 2 (got '") + e + "')");
  return e[0] - '0';
}

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

template <class F>
void HashFeed::change(F f) {
  {
    std::lock_guard<std::mutex> g(m_);
    f();
  }
  cv_.notify_all();
}
void HashFeed::publish(const uint8_t* p, size_t len) { change([&] { items_.push_back({p, len}); }); }
void HashFeed::close() { change([&] { closed_ = true; }); }
void HashFeed::end() { change([&] { ended_ = true; }); }
void HashFeed::wait_consumed(size_t k) {
  std::unique_lock<std::mutex> g(m_);
  cv_.wait(g, [&] { return done_ > k || ended_; });
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
    change([&] { ++done_; });
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
  for (const Job& j : jobs) bytes = std::max(bytes, std::min(ch, j.n) * j.pb());
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

void pstream::scale_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, int wb,
                         HashFeed* feed, zkp_status bad_status, const char* bad_prefix, Spans& sp, PtauContributeTimings& t) {
  scaling_pass(slot, jobs, chunks, wb, feed, Refusal{bad_status, bad_prefix, " is not on the curve"}, sp, t,
               [&](Slot& s, const Job& j, const Chunk& c) {
                 upload(s, s.a, j.in + c.start * j.pb(), c.m * j.pb(), t);
                 points_bad_reset(s.dbad, s.st);
               });
}

void pstream::decode_scale_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, int wb,
                                Spans& sp, PtauChallengeTimings& t) {
  scaling_pass(slot, jobs, chunks, wb, nullptr, Refusal{ZKP_ERR_FORMAT, "challenge: ", " is not on the curve"}, sp, t,
               [&](Slot& s, const Job& j, const Chunk& c) {
                 // b is free until the scaling writes it: the staging buffer of the uncompressed bytes
                 upload(s, s.b, j.in + c.start * j.pb(), c.m * j.pb(), t);
                 points_bad_reset(s.dbad, s.st);
                 sp.begin(s.st);
                 launch_decode(j.g2, s.b, c.m, c.start, s.a, s.dbad, s.st);
                 sp.end(s.st, &t.decode_ms);
               });
}

void pstream::convert_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, int wb,
                           const Convert& cv, Spans& sp, PtauChallengeTimings& t) {
  ToZkey tz;
  pscale::fill_to_zkey(tz.w);
  const Refusal refusal{ZKP_ERR_FORMAT, cv.prefix, " is not on the curve"};
  auto dest = [&](const Job& j) { return cv.out_u ? j.out_enc : j.out; };
  run_chunks(
      slot, jobs, chunks, nullptr, &refusal, t, true,
      [&](Slot& s, const Job& j, const Chunk& c) {
        const size_t bytes = c.m * j.pb();
        if (cv.in_u) {
          // b is free until the result is written to it: the staging buffer of the uncompressed bytes
          upload(s, s.b, j.in + c.start * j.pb(), bytes, t);
          points_bad_reset(s.dbad, s.st);
          sp.begin(s.st);
          launch_decode(j.g2, s.b, c.m, c.start, s.a, s.dbad, s.st);
          sp.end(s.st, &t.decode_ms);
        } else {
          upload(s, s.a, j.in + c.start * j.pb(), bytes, t);
          points_bad_reset(s.dbad, s.st);
        }
        sp.begin(s.st);
        points_check_resident(j.g2, s.a, c.m, c.start, s.dbad, s.st);
        sp.end(s.st, &t.parse_check_ms);
        HIPX(hipMemcpyAsync(s.hbad.get(), s.dbad.get(), 16, hipMemcpyDeviceToHost, s.st));
        if (!dest(j)) return;
        const uint32_t* src = s.b;
        if (j.scale) {
          Powers pw;
          pscale::fill_powers(pw, j.first, j.ratio, c.start);
          sp.begin(s.st);
          launch_scale(j.g2, wb, s.a, c.m, pw, cv.out_u ? nullptr : s.b.get(), cv.out_u ? s.b.get() : nullptr, nullptr, s.st);
          sp.end(s.st, j.g2 ? &t.g2_ms : &t.g1_ms);
        } else if (cv.out_u) {
          sp.begin(s.st);
          launch_encode(j.g2, s.a, c.m, tz, nullptr, s.b, nullptr, s.st);
          sp.end(s.st, &t.encode_ms);
        } else {
          src = s.a;
        }
        HIPX(hipMemcpyAsync(s.hlem.get(), src, bytes, hipMemcpyDeviceToHost, s.st));
      },
      [&](Slot& s, const Job& j, const Chunk& c) {
        if (dest(j)) std::memcpy(dest(j) + c.start * j.pb(), s.hlem.get(), c.m * j.pb());
      });
}

void pstream::encode_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, HashFeed& feed,
                          Spans& sp, PtauContributeTimings& t, bool from_in) {
  ToZkey tz;
  pscale::fill_to_zkey(tz.w);
  run_chunks(
      slot, jobs, chunks, &feed, nullptr, t, false,
      [&](Slot& s, const Job& j, const Chunk& c) {
        upload(s, s.a, (from_in ? j.in : j.out) + c.start * j.pb(), c.m * j.pb(), t);
        sp.begin(s.st);
        launch_encode(j.g2, s.a, c.m, tz, nullptr, s.b, nullptr, s.st);
        sp.end(s.st, &t.encode_ms);
        HIPX(hipMemcpyAsync(s.henc.get(), s.b.get(), c.m * j.pb(), hipMemcpyDeviceToHost, s.st));
      },
      [&](Slot& s, const Job& j, const Chunk& c) {
        if (j.out_enc) std::memcpy(j.out_enc + c.start * j.pb(), s.henc.get(), c.m * j.pb());
        feed.publish(s.henc.get(), c.m * j.pb());
      });
}

void pstream::decompress_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, HashFeed& feed,
                              Spans& sp, PtauChallengeTimings& t) {
  pdec::Consts k1, k2;
  pdec::fill_consts(k1, false), pdec::fill_consts(k2, true);
  const Refusal refusal{ZKP_ERR_FORMAT, "response: ", " is not a point of the curve"};
  run_chunks(
      slot, jobs, chunks, &feed, &refusal, t, true,
      [&](Slot& s, const Job& j, const Chunk& c) {
        upload(s, s.c, j.in + c.start * j.pb() / 2, c.m * j.pb() / 2, t);
        points_bad_reset(s.dbad, s.st);
        sp.begin(s.st);
        launch_decompress(j.g2, s.c, c.m, c.start, j.g2 ? k2 : k1, s.b, s.a, s.dbad, s.st);
        sp.end(s.st, j.g2 ? &t.decomp_g2_ms : &t.decomp_g1_ms);
        HIPX(hipMemcpyAsync(s.hbad.get(), s.dbad.get(), 16, hipMemcpyDeviceToHost, s.st));
        HIPX(hipMemcpyAsync(s.hlem.get(), s.b.get(), c.m * j.pb(), hipMemcpyDeviceToHost, s.st));
        HIPX(hipMemcpyAsync(s.henc.get(), s.a.get(), c.m * j.pb(), hipMemcpyDeviceToHost, s.st));
      },
      [&](Slot& s, const Job& j, const Chunk& c) {
        std::memcpy(j.out + c.start * j.pb(), s.hlem.get(), c.m * j.pb());
        feed.publish(s.henc.get(), c.m * j.pb());
      });
}

void pstream::points_to_zkey(int device, bool g2, bool compressed, const uint8_t* in, size_t n, uint8_t* out, uint64_t* n_bad,
                             uint64_t* first_bad) {
  *n_bad = 0, *first_bad = POINTS_NO_BAD;
  const size_t pb = g2 ? 128 : 64, ch = ptau_chunk_points();  // read, and refused, even when there is no point
  if (!n) return;
  HIPX(hipSetDevice(device));
  pdec::Consts k;
  pdec::fill_consts(k, g2);
  points_through(ch, compressed ? pb / 2 : pb, pb, in, n, out, n_bad, first_bad,
                 [&](const uint32_t* d_in, size_t m, uint64_t base, uint32_t* d_out, unsigned long long* bad, hipStream_t st) {
                   if (compressed)
                     launch_decompress(g2, d_in, m, base, k, d_out, nullptr, bad, st);
                   else
                     launch_decode(g2, d_in, m, base, d_out, bad, st);
                 });
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

}  // namespace zkp
