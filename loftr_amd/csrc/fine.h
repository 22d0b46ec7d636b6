// Host orchestration of FinePreprocess (fine.hip), shared by loftr_fine_preprocess and the feature-bank variant
// loftr_fine_preprocess_gather (bank.hip).  They differ only in where the W x W windows are read from.
#pragma once
#include "linear.h"

// Launches the window gather of the M matches into the two SP window tiles [M, W*W, Cf] on `st`.
struct WindowGather {
  int (*launch)(const void* ctx, sp_t* win0, sp_t* win1, hipStream_t st);
  const void* ctx;
};

// Everything of loftr_fine_preprocess after its argument checks: weight conversion, window gather (`gather`), coarse gather,
// down-projection and merge GEMMs.  M > 0.
int fine_preprocess_run(const WindowGather& gather, const float* feat_c0, const float* feat_c1, int L, int S, int Cc,
                        const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M, int W, int Cf,
                        const float* down_w, const float* down_b, const float* merge_w, const float* merge_b,
                        float* out0, float* out1, void* ws, size_t ws_bytes, hipStream_t st);
