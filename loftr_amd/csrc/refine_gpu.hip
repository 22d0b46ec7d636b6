// Track refinement on the GPU (the contract is in include/loftr_hip.h): the centres of refine_core.h a thread per row, and
// FinePreprocess with its W x W windows placed at centres the caller names instead of at coarse cells.
//   refine_windows_at_kernel is bank_windows_kernel (bank.hip) with the centre of match m read from c0 / c1 [M, 2] (x, y) in fine
//   pixels: the same per-element arithmetic and sp_store call, so at centres stride * cell the output words are that kernel's.
//   Slot offsets are 64-bit, a slot outside the bank gives NaN, a pixel outside the map 0; the window coordinates are formed in 64
//   bits, so no centre, however wrong, reaches memory outside the map.  Everything after the windows is fine_preprocess_run (fine.hip).
//   The kernel names share no base name with a kernel of profiles/pmc_traffic.json (see the note at the top of bank.hip).
#include "common.h"
#include "fine.h"
#include "refine_core.h"

#pragma clang fp contract(off)

namespace {

using namespace refine;

constexpr int kThreads = 256;

// grid ceil(M / 256) x 256
__global__ void __launch_bounds__(kThreads) refine_centres_kernel(const float* __restrict__ pts0, const float* __restrict__ pts1,
                                                                  const int64_t* __restrict__ b_ids, long M,
                                                                  const float* __restrict__ scale0, const float* __restrict__ scale1,
                                                                  int n_pairs, Geometry g, int* __restrict__ c0, int* __restrict__ c1,
                                                                  int64_t* __restrict__ i_ids, int64_t* __restrict__ j_ids,
                                                                  float* __restrict__ pts0_s, float* __restrict__ pts1_s,
                                                                  uint8_t* __restrict__ ok) {
  const long m = (long)blockIdx.x * kThreads + threadIdx.x;
  if (m < M) row(m, pts0, pts1, b_ids, scale0, scale1, n_pairs, g, c0, c1, i_ids, j_ids, pts0_s, pts1_s, ok);
}

__device__ __forceinline__ bool slot_ok(int slot, int n_slots) { return slot >= 0 && slot < n_slots; }

// The windows of match m around (c0[m], c1[m]) of the fine maps bank_f0[slot0[b]] / bank_f1[slot1[b]] (b = b_ids[m], pair-local).
//   grid (M, 2), Cf threads (Cf even, a multiple of 32).  Channels-last banks: the Cf threads of a block read the Cf contiguous
//   floats of one pixel at every step.
__global__ void refine_windows_at_kernel(loftr_fmap f0, loftr_fmap f1, int n_slots0, int n_slots1,
                                         const int32_t* __restrict__ slot0, const int32_t* __restrict__ slot1,
                                         const int64_t* __restrict__ b_ids, const int* __restrict__ c0, const int* __restrict__ c1, int M,
                                         int W, int Cf, sp_t* __restrict__ win0, sp_t* __restrict__ win1) {
  const int m = blockIdx.x, side = blockIdx.y;
  const loftr_fmap f = side ? f1 : f0;
  const int* centre = (side ? c1 : c0) + 2 * (long)m;
  const long b = b_ids[m];
  const int slot = (side ? slot1 : slot0)[b];
  const bool ok = slot_ok(slot, side ? n_slots1 : n_slots0);
  const long cx = centre[0], cy = centre[1];
  const int r = W / 2;
  sp_t* out = (side ? win1 : win0) + (long)m * W * W * Cf;
  for (int c = threadIdx.x; c < Cf; c += blockDim.x) {
    const float* base = f.data + (ok ? (long)slot * f.sn : 0L) + (long)c * f.sc;
    for (int wy = 0; wy < W; ++wy) {
      const long y = cy + wy - r;
      for (int wx = 0; wx < W; ++wx) {
        const long x = cx + wx - r;
        float v = ok ? 0.f : __builtin_nanf("");
        if (ok && y >= 0 && y < f.H && x >= 0 && x < f.W) v = base[y * f.sh + x * f.sw];
        sp_store(out + (wy * W + wx) * Cf, c, v, true);
      }
    }
  }
}

struct WindowsAt {
  loftr_fmap f0, f1; int n_slots0, n_slots1; const int32_t *slot0, *slot1;
  const int64_t* b_ids; const int *c0, *c1; int M, W, Cf;
};
int launch_windows_at(const void* ctx, sp_t* win0, sp_t* win1, hipStream_t st) {
  const WindowsAt& a = *(const WindowsAt*)ctx;
  hipLaunchKernelGGL(refine_windows_at_kernel, dim3(a.M, 2), dim3(a.Cf < 64 ? 64 : a.Cf), 0, st, a.f0, a.f1, a.n_slots0, a.n_slots1,
                     a.slot0, a.slot1, a.b_ids, a.c0, a.c1, a.M, a.W, a.Cf, win0, win1);
  return LOFTR_OK;
}

}  // namespace

extern "C" int loftr_refine_centres(const float* pts0, const float* pts1, const int64_t* b_ids, long M, const float* scale0,
                                    const float* scale1, int n_pairs, int hf0, int wf0, int hf1, int wf1, int h0c, int w0c, int h1c,
                                    int w1c, int stride, float s, int* c0, int* c1, int64_t* i_ids, int64_t* j_ids, float* pts0_s,
                                    float* pts1_s, uint8_t* ok, void* stream) {
  const Geometry g{hf0, wf0, hf1, wf1, h0c, w0c, h1c, w1c, stride, s};
  const int st = check_args(pts0, pts1, b_ids, M, n_pairs, g, c0, c1, i_ids, j_ids, pts0_s, pts1_s, ok);
  if (st != LOFTR_OK) return st;
  if (M == 0) return LOFTR_OK;
  if ((M + kThreads - 1) / kThreads >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(refine_centres_kernel, dim3((unsigned)((M + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, pts0,
                     pts1, b_ids, M, scale0, scale1, n_pairs, g, c0, c1, i_ids, j_ids, pts0_s, pts1_s, ok);
  LOFTR_CHECK_LAUNCH();
  return LOFTR_OK;
}

extern "C" int loftr_fine_preprocess_gather_at(const loftr_fmap* bank_f0, int n_slots0, const int32_t* slot0,
                                               const loftr_fmap* bank_f1, int n_slots1, const int32_t* slot1,
                                               const float* feat_c0, const float* feat_c1, int L, int S, int Cc,
                                               const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids,
                                               int M, int w0c, int w1c, int stride, int W, int Cf,
                                               const float* down_w, const float* down_b, const float* merge_w,
                                               const float* merge_b, float* out0, float* out1, void* ws,
                                               size_t ws_bytes, const int* c0, const int* c1, void* stream) {
  LOFTR_CHECK_ARG(M >= 0);
  if (M == 0) return LOFTR_OK;
  LOFTR_CHECK_ARG(bank_f0 && bank_f1 && bank_f0->data && bank_f1->data && slot0 && slot1 && n_slots0 > 0 && n_slots1 > 0);
  LOFTR_CHECK_ARG(b_ids && i_ids && j_ids && c0 && c1 && out0 && out1);
  LOFTR_CHECK_ARG(w0c > 0 && w1c > 0 && stride > 0 && W > 0 && (W & 1) && Cf > 0 && Cf <= 1024);
  const WindowsAt wa{*bank_f0, *bank_f1, n_slots0, n_slots1, slot0, slot1, b_ids, c0, c1, M, W, Cf};
  return fine_preprocess_run(WindowGather{launch_windows_at, &wa}, feat_c0, feat_c1, L, S, Cc, b_ids, i_ids, j_ids, M, W, Cf,
                             down_w, down_b, merge_w, merge_b, out0, out1, ws, ws_bytes, (hipStream_t)stream);
}
