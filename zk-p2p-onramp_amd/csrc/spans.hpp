// Device time of stretches of one stream's work, summed per stage, and the host's wall time beside it: the
// two clocks of every timing vector.
#pragma once
#include <chrono>
#include <vector>

#include "hip_check.hpp"
#include "hip_raii.hpp"

namespace zkp {

// host ms since t0
inline double wall_ms(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// device ms between pairs of events, read once everything is complete
struct Spans {
  std::vector<Event> ev;
  std::vector<double*> into;
  void begin(hipStream_t st) {
    ev.emplace_back(true);
    HIPX(hipEventRecord(ev.back(), st));
  }
  void end(hipStream_t st, double* sum) {
    ev.emplace_back(true);
    HIPX(hipEventRecord(ev.back(), st));
    into.push_back(sum);
  }
  void collect() {
    for (size_t i = 0; i < into.size(); ++i) {
      float ms;
      HIPX(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
      *into[i] += ms;
    }
    ev.clear();
    into.clear();
  }
};

}  // namespace zkp
