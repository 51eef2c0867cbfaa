// Device time of stretches of one stream's work, summed per stage (ptau_prepare.hip, ptau_verify.hip).
#pragma once
#include <vector>

#include "hip_check.hpp"
#include "hip_raii.hpp"

namespace zkp {

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
