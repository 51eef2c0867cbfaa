// The single-stream chunk loop of points_check, g2_subgroup_check, points_decompress and
// points_from_uncompressed: n > 0 points through a per-point kernel that counts the points it refuses.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "hip_check.hpp"
#include "hip_raii.hpp"
#include "zkey_verify.hpp"

namespace zkp {

// On the current device, in chunks of at most ch points: upload in_pb bytes per point, launch(d_in, m, base,
// d_out, d_bad, st), download out_pb bytes per point into out (null: the kernel only counts, d_out is null).
// *n_bad = the refused points, *first_bad = the smallest index among them (all ones if none).
template <class Launch>
void points_through(size_t ch, size_t in_pb, size_t out_pb, const uint8_t* in, size_t n, uint8_t* out, uint64_t* n_bad,
                    uint64_t* first_bad, Launch launch) {
  const size_t CH = std::min(n, ch);
  DevBuf<> din(CH * in_pb / 4), dout;
  if (out) dout = DevBuf<>(CH * out_pb / 4);
  DevBuf<unsigned long long> dbad(2);
  Stream st(hipStreamNonBlocking);  // last: drained before the buffers go
  points_bad_reset(dbad, st);
  for (size_t at = 0; at < n; at += CH) {
    const size_t m = std::min(CH, n - at);
    HIPX(hipMemcpyAsync(din, in + at * in_pb, m * in_pb, hipMemcpyHostToDevice, st));
    launch(din.get(), m, at, dout.get(), dbad.get(), st);
    if (out) HIPX(hipMemcpyAsync(out + at * out_pb, dout, m * out_pb, hipMemcpyDeviceToHost, st));
    HIPX(hipStreamSynchronize(st));  // the next upload overwrites din
  }
  unsigned long long h[2];
  HIPX(hipMemcpyAsync(h, dbad, 16, hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  *n_bad = h[0], *first_bad = h[1];
}

}  // namespace zkp
