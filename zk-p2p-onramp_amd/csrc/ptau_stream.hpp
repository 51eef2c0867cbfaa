// The chunked two-slot streaming that `powersoftau contribute` / `beacon` (ptau_contribute.hip) and `export
// challenge` / `challenge contribute` / `import response` (ptau_challenge.hip) share: sections cut into chunks
// of ZKP_PTAU_CHUNK points, two slots with their own stream, device and pinned buffers, and host threads that
// hash the chunks in order while the device works on later ones.  Everything declared here, and
// ptau_chunk_points (ptau_contribute.hpp), is defined in ptau_stream.hip, with the per-point kernels the
// passes launch; the two command units call into it and not into each other.
#pragma once
#include <condition_variable>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "hip_raii.hpp"
#include "mpc.hpp"
#include "prover.hpp"
#include "ptau_challenge.hpp"
#include "ptau_contribute.hpp"
#include "ptau_verify.hpp"
#include "spans.hpp"

namespace zkp {
namespace pstream {

// one thread per point
constexpr int TPB = 128;
inline unsigned grid(size_t n) { return (unsigned)((n + TPB - 1) / TPB); }

// Byte ranges handed from the pipeline to one hashing thread, in order.  The producer publishes chunk k and
// may reuse its buffer once consumed() > k.
class HashFeed {
 public:
  void publish(const uint8_t* p, size_t len);
  void close();
  void wait_consumed(size_t k);  // until chunk k has been hashed (or the consumer has given up)
  void end();                    // the consumer leaves: nobody waits for it any more
  void drain(Blake2b& h);        // the consumer: every published range into h, until close()

 private:
  template <class F>
  void change(F f);  // f under the lock, then every waiter looks again
  std::mutex m_;
  std::condition_variable cv_;
  std::vector<std::pair<const uint8_t*, size_t>> items_;
  size_t done_ = 0;
  bool closed_ = false, ended_ = false;
};

// closes the feed and joins its thread on every way out
struct HashThread {
  HashFeed feed;
  std::thread th;
  ~HashThread() { finish(); }
  void finish() {
    feed.close();
    if (th.joinable()) th.join();
  }
};

struct Job {  // one section
  int id;
  bool g2;
  size_t n;
  const uint8_t* in;  // zkey layout; decode_scale_pass: uncompressed; decompress_pass: compressed
  uint8_t* out;       // zkey layout (null: not wanted)
  uint32_t first[8], ratio[8];
  uint8_t* out_enc = nullptr;  // the pass's encoded stream, if it is kept and not only hashed
  const char* name = nullptr;  // convert_pass: what a refusal calls the section ("<name> point <i>")
  bool scale = false;          // convert_pass: whether the points are multiplied by first * ratio^i
  size_t pb() const { return g2 ? 128 : 64; }  // bytes of a point in the zkey layout
};
struct Chunk {
  int job;
  size_t start, m;
};

struct Slot {
  DevBuf<> a, b, c;  // full-size, full-size, half-size (compressed) point buffers
  DevBuf<unsigned long long> dbad;
  PinnedBuf<uint8_t> hlem, henc;
  PinnedBuf<unsigned long long> hbad;
  Event done;
  Stream st;  // last: drained before the buffers go
};

std::vector<Chunk> chunks_of(const std::vector<Job>& jobs, size_t ch);
void make_slots(Slot (&slot)[2], const std::vector<Job>& jobs, size_t ch, bool hashes);
int window_bits();  // ZKP_PTAU_WINDOW

// a standard-form scalar as Job::first / ratio hold it
inline void words_of(const host::U256& v, uint32_t (&w)[8]) {
  for (int i = 0; i < 4; ++i) w[2 * i] = (uint32_t)v.w[i], w[2 * i + 1] = (uint32_t)(v.w[i] >> 32);
}

// The four passes, each through the one two-slot loop (run_chunks, ptau_stream.hip).  A pass that refuses a
// point throws while the other slot is busy and the hashing thread waits on its feed: the caller's HashThread,
// declared after its slots, closes and joins, then each Slot drains its stream.

// Upload, point check, scale; the zkey-layout bytes into each job's out (if any), the compressed bytes to the
// hashing thread (if feed) and into out_enc (if any).  bad_status: what a point off the curve is (with its
// message).
void scale_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, int wb, HashFeed* feed,
                zkp_status bad_status, const char* bad_prefix, Spans& sp, PtauContributeTimings& t);
// The same over jobs whose `in` is the uncompressed form, which k_decode_points turns into the zkey layout
// first; a point it refuses counts like one off the curve (ZKP_ERR_FORMAT "challenge: ...")
void decode_scale_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, int wb, Spans& sp,
                       PtauChallengeTimings& t);
// Zkey-layout points (each job's out; from_in: its in) uncompressed, into out_enc (if any) and to the
// hashing thread.  Its chunks are not counted: it is the second pass over a file whose first pass counted them.
void encode_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, HashFeed& feed, Spans& sp,
                 PtauContributeTimings& t, bool from_in = false);
// The compressed sections: upload, decompress; the zkey-layout bytes into each job's out, the uncompressed
// bytes to the hashing thread.  A refused point is ZKP_ERR_FORMAT "response: ...".
void decompress_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, HashFeed& feed,
                     Spans& sp, PtauChallengeTimings& t);

// The MPCParams passes of zkey_bellman.hip.  Each job's `in` is uncompressed (in_u) or in the zkey layout; every
// point is decoded (in_u) and checked, a job with `scale` multiplied by first * ratio^i, and the result leaves
// uncompressed into out_enc (out_u) or in the zkey layout into out.  A job without that output is only checked.
// A refused point is ZKP_ERR_FORMAT "<prefix><name> point <i> is not on the curve".
struct Convert {
  bool in_u, out_u;
  const char* prefix;
};
void convert_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, int wb, const Convert& cv,
                  Spans& sp, PtauChallengeTimings& t);

// ptau_challenge.hpp's points_decompress (compressed: k_decompress_points) and points_from_uncompressed
// (k_decode_points): chunks of ZKP_PTAU_CHUNK points on one stream (points_through.hpp)
void points_to_zkey(int device, bool g2, bool compressed, const uint8_t* in, size_t n, uint8_t* out, uint64_t* n_bad,
                    uint64_t* first_bad);

// The new file of a contribution to f: the header and sections 1-6 laid out in `out` (2-6 to be filled at
// sec_out[id]), with room reserved for section 7; then section 7 with `rec` appended to f's records
void ptau_layout(const PtauFile& f, std::vector<uint8_t>& out, uint8_t* (&sec_out)[8]);
void ptau_append_section7(const PtauFile& f, std::vector<uint8_t>& out, const std::vector<uint8_t>& rec);

}  // namespace pstream
}  // namespace zkp
