// Track refinement, host routine: the fine-window centres, coarse cells and snapped points of M point pairs (the contract
// is in include/loftr_hip.h).  This function DEFINES the result: loftr_refine_centres (refine_gpu.hip) reproduces it bit for bit, which
// is why the per-row step lives in refine_core.h.  This file is the loop.
#include <stdint.h>
#include "../../include/loftr_hip.h"
#include "refine_core.h"

#pragma clang fp contract(off)

using namespace refine;

extern "C" int loftr_refine_centres_host(const float* pts0, const float* pts1, const int64_t* b_ids, long M, const float* scale0,
                                         const float* scale1, int n_pairs, int hf0, int wf0, int hf1, int wf1, int h0c, int w0c, int h1c,
                                         int w1c, int stride, float s, int* c0, int* c1, int64_t* i_ids, int64_t* j_ids, float* pts0_s,
                                         float* pts1_s, uint8_t* ok) {
  const Geometry g{hf0, wf0, hf1, wf1, h0c, w0c, h1c, w1c, stride, s};
  const int st = check_args(pts0, pts1, b_ids, M, n_pairs, g, c0, c1, i_ids, j_ids, pts0_s, pts1_s, ok);
  if (st != LOFTR_OK) return st;
  for (long m = 0; m < M; ++m) row(m, pts0, pts1, b_ids, scale0, scale1, n_pairs, g, c0, c1, i_ids, j_ids, pts0_s, pts1_s, ok);
  return LOFTR_OK;
}
