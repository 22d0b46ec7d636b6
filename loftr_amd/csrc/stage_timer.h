// Stage timings of a fixed launch schedule (host side): an event at every stage boundary of the caller's stream, read once at the end.
// With stage_ms == nullptr nothing is created, recorded or waited for.  A failed event call is remembered and makes finish() return
// LOFTR_ERR_LAUNCH; the events are destroyed on every path out of the entry point.
#pragma once
#include <vector>
#include "common.h"

class StageTimer {
 public:
  StageTimer(float* stage_ms, int n_stages, hipStream_t stream) : ms_(stage_ms), n_(n_stages), s_(stream) {}
  StageTimer(const StageTimer&) = delete;
  StageTimer& operator=(const StageTimer&) = delete;
  ~StageTimer() { for (hipEvent_t e : ev_) (void)hipEventDestroy(e); }

  // one stage boundary: stage k runs between mark k and mark k + 1
  void mark() {
    if (!ms_ || failed_) return;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) { failed_ = true; return; }
    ev_.push_back(e);
    if (hipEventRecord(e, s_) != hipSuccess) failed_ = true;
  }

  // the end of the entry point: waits for the stream and writes stage_ms [n_stages] (0 for a stage without both of its marks)
  int finish() {
    if (!ms_) return LOFTR_OK;
    for (int k = 0; k < n_; ++k) ms_[k] = 0.f;
    if (hipStreamSynchronize(s_) != hipSuccess) failed_ = true;
    for (size_t k = 0; !failed_ && k + 1 < ev_.size() && k < (size_t)n_; ++k)
      if (hipEventElapsedTime(&ms_[k], ev_[k], ev_[k + 1]) != hipSuccess) failed_ = true;
    return failed_ ? LOFTR_ERR_LAUNCH : LOFTR_OK;
  }

 private:
  float* ms_;
  int n_;
  hipStream_t s_;
  std::vector<hipEvent_t> ev_;
  bool failed_ = false;
};
