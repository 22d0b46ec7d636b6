// Removing the radial coefficient of a camera on pixels on the GPU: loftr_undistort_points_host's result bit for bit.
// A thread per point, the arithmetic radial_core.h's from the same text, fp64 without FMA contraction.  Two launches on the caller's
// stream: the first zeroes the counts (thread 0 of a launch of its own) and checks every image id, the second reads the error bit the
// first may have raised -- a kernel boundary is the only ordering -- and writes nothing when it is up.  Integer atomics only, no
// readback.  Plain C++, ordinary vector stores.
#include "common.h"
#include "radial_core.h"

#pragma clang fp contract(off)

namespace {

using namespace radial;

constexpr int kThreads = 256;

__global__ void undistort_init_kernel(long* counts) {
  for (int i = 0; i < kCounts; ++i) counts[i] = 0;
}

// grid ceil(M / 256) x 256
__global__ void __launch_bounds__(kThreads) undistort_check_kernel(const int* __restrict__ image, long M, int n, long* counts) {
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;
  const bool bad = p < M && (image[p] < 0 || image[p] >= n);
  if (__any(bad) && threadIdx.x % 64 == 0) atomicOr((unsigned long long*)&counts[1], (unsigned long long)kBadImage);
}

// grid ceil(M / 256) x 256 (at least 1)
__global__ void __launch_bounds__(kThreads) undistort_kernel(const float* __restrict__ xy, const int* __restrict__ image, long M,
                                                             const double* __restrict__ K, const double* __restrict__ k, float* xy_out,
                                                             uint8_t* ok, long* counts) {
  __shared__ unsigned s_ok;
  if (threadIdx.x == 0) s_ok = 0;
  __syncthreads();
  if (counts[1]) return;                                                 // (uniform over the launch: written by the launch before)
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;
  if (p < M) {
    const int i = image[p];
    float out[2];
    const bool good = undistort_point(K + 9 * (long)i, k[i], xy[2 * p], xy[2 * p + 1], out);
    xy_out[2 * p] = out[0]; xy_out[2 * p + 1] = out[1];
    ok[p] = (uint8_t)good;
    if (good) atomicAdd(&s_ok, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const long here = M - (long)blockIdx.x * kThreads < kThreads ? M - (long)blockIdx.x * kThreads : kThreads;
    if (s_ok) atomicAdd((unsigned long long*)&counts[0], (unsigned long long)s_ok);
    if (here > (long)s_ok) atomicAdd((unsigned long long*)&counts[2], (unsigned long long)(here - (long)s_ok));
  }
}

}  // namespace

extern "C" int loftr_undistort_points(const float* xy, const int* image, long M, const double* K, const double* radial, int n_images,
                                      float* xy_out, uint8_t* ok, long* counts, void* stream) {
  const int st = check_args(xy, image, M, K, radial, n_images, xy_out, ok, counts);
  if (st != LOFTR_OK) return st;
  if ((M + kThreads - 1) / kThreads >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(undistort_init_kernel, dim3(1), dim3(1), 0, s, counts);
  LOFTR_CHECK_LAUNCH();
  if (M == 0) return LOFTR_OK;
  const dim3 grid((unsigned)((M + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(undistort_check_kernel, grid, dim3(kThreads), 0, s, image, M, n_images, counts);
  LOFTR_CHECK_LAUNCH();
  hipLaunchKernelGGL(undistort_kernel, grid, dim3(kThreads), 0, s, xy, image, M, K, radial, xy_out, ok, counts);
  LOFTR_CHECK_LAUNCH();
  return LOFTR_OK;
}
