// The chunked two-slot streaming that `powersoftau contribute` / `beacon` (ptau_contribute.hip) and `export
// challenge` / `challenge contribute` / `import response` (ptau_challenge.hip) share: sections cut into chunks
// of ZKP_PTAU_CHUNK points, two slots with their own stream, device and pinned buffers, and host threads that
// hash the chunks in order while the device works on later ones.  Defined in ptau_contribute.hip.
#pragma once
#include <condition_variable>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "hip_raii.hpp"
#include "mpc.hpp"
#include "prover.hpp"
#include "ptau_contribute.hpp"
#include "ptau_verify.hpp"
#include "spans.hpp"

namespace zkp {
namespace pstream {

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
  const uint8_t* in;  // zkey layout; scale_pass with decode: uncompressed; decompress: compressed
  uint8_t* out;       // zkey layout (null: not wanted)
  uint32_t first[8], ratio[8];
  uint8_t* out_enc = nullptr;  // the pass's encoded stream, if it is kept and not only hashed
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

// Upload, point check, scale; the zkey-layout bytes into each job's out (if any), the compressed bytes to the
// hashing thread (if feed) and into out_enc (if any).  decode_ms != null: a job's `in` is the uncompressed
// form, which k_decode_points (ptau_challenge.hip) turns into the zkey layout first; a point it refuses
// counts like one off the curve.  bad_status: what such a point is (with its message).
void scale_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, int wb, HashFeed* feed,
                zkp_status bad_status, const char* bad_prefix, Spans& sp, PtauContributeTimings& t,
                double* decode_ms = nullptr);
// Zkey-layout points (each job's out; from_in: its in) uncompressed, into out_enc (if any) and to the
// hashing thread
void encode_pass(Slot (&slot)[2], const std::vector<Job>& jobs, const std::vector<Chunk>& chunks, HashFeed& feed, Spans& sp,
                 PtauContributeTimings& t, bool from_in = false);

// k_decode_points on a stream (ptau_challenge.hip): n uncompressed points at d_in -> zkey layout at d_lem;
// bad[0] += the refused points, bad[1] = min(bad[1], base + i) over them
void launch_decode(bool g2, const uint32_t* d_in, size_t n, uint64_t base, uint32_t* d_lem, unsigned long long* bad,
                   hipStream_t st);

// The new file of a contribution to f: the header and sections 1-6 laid out in `out` (2-6 to be filled at
// sec_out[id]), with room reserved for section 7; then section 7 with `rec` appended to f's records
void ptau_layout(const PtauFile& f, std::vector<uint8_t>& out, uint8_t* (&sec_out)[8]);
void ptau_append_section7(const PtauFile& f, std::vector<uint8_t>& out, const std::vector<uint8_t>& rec);

}  // namespace pstream
}  // namespace zkp
