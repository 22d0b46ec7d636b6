// Triangulation of tracks from known camera poses on the GPU: loftr_triangulate_tracks_host (triangulate.hip) for every track, with the
// same result bit for bit.  Two kernels, nothing read back between them, no data-dependent grid:
//   1. tri_camera_kernel    (thread per image)   the camera table: P = K [R | t], centre, M = R^T K^-1; an invalid camera is all NaN;
//   2. tri_solve_kernel<G>  (G lanes per track, 256 threads per block)  lane g scores hypotheses g, g + G, ... over the track's
//                           observations; the packed word (count << 32 | 0xFFFFFFFF - h) is maxed over the group with cross-lane
//                           shuffles; lane 0 recomputes the winner's point with the function that scored it and runs the refit (sums in
//                           ascending observation order, as the host); the point goes back to the group through exact 64-bit shuffles;
//                           the minimum cosine over the enumerated inlier pairs is reduced over the lanes (a minimum is order-free).
//      Launched over all tracks with G = 8 for tracks of at most kShortMax = 64 observations (8 tracks per wave) and with G = 64 for
//      longer ones; each launch skips the tracks of the other class.  The boundary is measured: the refit runs in one lane
//      per track, so a 64-lane group idles through it, and 8 lanes win up to the longest tracks of the benchmark load (62).
//      -DTRI_SHORT_MAX=n builds another boundary (how the sweep was made); no result depends on it.
// Identical decisions need identical arithmetic: every formula is triangulate_core.h's, compiled from the same text as the host
// routine's, fp64 without FMA contraction.  The only values that cross lanes are integers, the packed word, a minimum and copies of
// doubles.  Bad offsets / image ids raise a bit in counts[5] (no synchronisation here; the caller reads counts once).
// Plain C++ throughout; all stores are ordinary vector stores.
#include "common.h"
#include "triangulate_core.h"
#include "stage_timer.h"

#pragma clang fp contract(off)

namespace {

using namespace tri;

constexpr int kThreads = 256;
#ifndef TRI_SHORT_MAX
#define TRI_SHORT_MAX 64
#endif
constexpr long kShortMax = TRI_SHORT_MAX;     // longest track of the 8-lane class (a tuning constant: no result depends on it)

// grid ceil(n_images / 64) x 64
__global__ void tri_camera_kernel(const double* __restrict__ K, const double* __restrict__ T, int n_images, double* __restrict__ tab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_images) return;
  double t[kCam];
  cam_table(K + 9 * (long)i, T + 16 * (long)i, t);
  for (int k = 0; k < kCam; ++k) tab[(long)kCam * i + k] = t[k];
}

struct Args {
  const long* offsets; long T;
  const int* image; const float* xy; long N;
  int n_images; const double* tab;
  double thr2, cos_min;
  Out out; uint8_t* bits; unsigned long long* counts;
};

template <int G> __device__ __forceinline__ int group_or(int v) {
  for (int m = G / 2; m >= 1; m >>= 1) v |= __shfl_xor(v, m, G);
  return v;
}
template <int G> __device__ __forceinline__ unsigned long long group_max(unsigned long long v) {
  for (int m = G / 2; m >= 1; m >>= 1) { const unsigned long long w = __shfl_xor(v, m, G); v = w > v ? w : v; }
  return v;
}
template <int G> __device__ __forceinline__ double group_min(double v) {
  for (int m = G / 2; m >= 1; m >>= 1) { const double w = __shfl_xor(v, m, G); v = w < v ? w : v; }
  return v;
}

// grid ceil(T / (256 / G)) x 256.  cls: 0 every track, 1 only tracks of at most kShortMax observations, 2 only longer ones.
// Every thread runs every phase (a group that has nothing to do carries neutral values), so that the shuffles sit in uniform code.
template <int G>
__global__ void __launch_bounds__(kThreads) tri_solve_kernel(Args a, int cls) {
  __shared__ unsigned s_cnt[kCounts];
  const int tid = threadIdx.x, g = tid % G;
  if (tid < kCounts) s_cnt[tid] = 0;
  __syncthreads();
  const long t = (long)blockIdx.x * (kThreads / G) + tid / G;
  bool live = t < a.T;
  long o0 = 0, L = 0;
  int err = 0;
  if (live) {                                                          // offsets: 0 first, N last, ascending, inside [0, N]
    long b, e;
    if (!tracks::span(a.offsets, a.T, a.N, t, &b, &e)) { err = kBadOffsets; live = false; }
    else { o0 = b; L = e - b; }
  }
  if (live && cls) live = (cls == 1) == (L <= kShortMax);
  int flag = 0;                                                        // 1: an image id out of range, 2: an invalid camera
  if (live)
    for (long k = g; k < L; k += G) {
      const int im = a.image[o0 + k];
      if (im < 0 || im >= a.n_images) flag |= 1;
      else if (!cam_valid(a.tab + (long)kCam * im)) flag |= 2;
    }
  flag = group_or<G>(flag);
  if (live && (flag & 1)) { err |= kBadImage; live = false; }
  int st = -1;
  if (live && L < 2) st = kTooShort;
  else if (live && (flag & 2)) st = kBadCamera;
  const bool solve = live && st < 0;
  const Obs o{a.tab, a.image, a.xy, a.thr2, a.cos_min};
  const int nh = solve ? n_pairs(L) : 0;
  unsigned long long best = 0;
  for (int h = g; h < nh; h += G) {
    const unsigned long long word = hyp_word(o, o0, L, h);
    if (word > best) best = word;
  }
  best = group_max<G>(best);
  if (solve && best == 0) st = kNoHypothesis;
  const bool fit = solve && best != 0;
  uint8_t* bits = a.bits + o0;
  double X[3] = {0.0, 0.0, 0.0}, rms = 0.0;
  long cnt = 0;
  if (fit && g == 0) {
    hyp_point(o, o0, L, (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)), X);
    cnt = refit_track(o, o0, L, X, bits, &rms);
  }
  __threadfence_block();                                               // lane 0's mask is read by the lanes of its group below
  for (int c = 0; c < 3; ++c) X[c] = __shfl(X[c], 0, G);
  double min_cos = 2.0;
  if (fit)
    for (int h = g; h < nh; h += G) {
      double cs;
      if (pair_cos(o, o0, L, h, X, bits, &cs) && cs < min_cos) min_cos = cs;
    }
  min_cos = group_min<G>(min_cos);
  if (fit) st = min_cos > a.cos_min ? kSmallAngle : kOk;
  if (live) {
    if (st != kOk) for (long k = g; k < L; k += G) bits[k] = 0;
    if (g == 0) {
      write_track(a.out, t, st, X, cnt, rms, min_cos, min_cos != 2.0);
      atomicAdd(&s_cnt[st], 1u);
      if (st == kOk) atomicAdd(&s_cnt[6], (unsigned)cnt);
    }
  }
  if (err) atomicOr(&s_cnt[5], (unsigned)err);
  __syncthreads();
  if (tid < kCounts && s_cnt[tid]) {
    if (tid == 5) atomicOr(a.counts + 5, (unsigned long long)s_cnt[5]);
    else atomicAdd(a.counts + tid, (unsigned long long)s_cnt[tid]);
  }
}

size_t table_bytes(int n_images) { return align_up(sizeof(double) * kCam * (size_t)(n_images > 0 ? n_images : 1), 256); }

}  // namespace

extern "C" size_t loftr_triangulate_tracks_workspace_bytes(long T, long N, int n_images) {
  if (T < 0 || N < 0 || n_images < 0 || T >= (1L << 31) || N >= (1L << 31)) return 0;
  return table_bytes(n_images);
}

extern "C" int loftr_triangulate_tracks(const long* offsets, long T, const int* obs_image, const float* obs_xy, long N, const double* K,
                                        const double* T_cam_from_world, int n_images, double thresh_px, double cos_min_angle, float* xyz,
                                        int* n_inliers, float* rms_px, float* tri_cos, uint8_t* status, uint8_t* obs_inlier, long* counts,
                                        int group, void* ws, size_t ws_bytes, float* stage_ms, void* stream) {
  LOFTR_CHECK_ARG(offsets && counts && ws && T >= 0 && N >= 0 && n_images >= 0);
  LOFTR_CHECK_ARG(group == 0 || group == 8 || group == 64);
  LOFTR_CHECK_ARG(thresh_px >= 0.0 && cos_min_angle >= -1.0 && cos_min_angle <= 1.0);
  LOFTR_CHECK_ARG(T == 0 || (xyz && n_inliers && rms_px && tri_cos && status));
  LOFTR_CHECK_ARG(N == 0 || (obs_image && obs_xy && obs_inlier));
  LOFTR_CHECK_ARG(n_images == 0 || (K && T_cam_from_world));
  LOFTR_CHECK_ARG(T > 0 || N == 0);                                     // observations outside every track: offsets[T] != N
  if (T >= (1L << 31) || N >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  if (ws_bytes < table_bytes(n_images)) return LOFTR_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  double* tab = (double*)ws;
  StageTimer timer(stage_ms, LOFTR_TRIANGULATE_STAGES, s);
  if (hipMemsetAsync(counts, 0, sizeof(long) * kCounts, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  timer.mark();
  if (n_images > 0) {
    hipLaunchKernelGGL(tri_camera_kernel, dim3((unsigned)((n_images + 63) / 64)), dim3(64), 0, s, K, T_cam_from_world, n_images, tab);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  const Args a{offsets, T, obs_image, obs_xy, N, n_images, tab, thresh_px * thresh_px, cos_min_angle,
               Out{xyz, n_inliers, rms_px, tri_cos, status}, obs_inlier, (unsigned long long*)counts};
  if (T > 0 && group != 64) {
    hipLaunchKernelGGL(tri_solve_kernel<8>, dim3((unsigned)((T + 31) / 32)), dim3(kThreads), 0, s, a, group == 0 ? 1 : 0);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  if (T > 0 && group != 8) {
    hipLaunchKernelGGL(tri_solve_kernel<64>, dim3((unsigned)((T + 3) / 4)), dim3(kThreads), 0, s, a, group == 0 ? 2 : 0);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  return timer.finish();
}
