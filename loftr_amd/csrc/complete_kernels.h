// The two table kernels that track completion (complete_gpu.hip) and track merging (merge_gpu.hip) both launch
// first: the camera table and the check of the tables.  One text, included by both translation units (each gets its own copy in its
// anonymous namespace); every per-item step is complete_core.h's.
#pragma once
#include "common.h"
#include "complete_core.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
typedef unsigned long long u64;

// grid ceil(n_images / 64) x 64
__global__ void complete_camera_kernel(const double* __restrict__ K, const double* __restrict__ T, int n_images, double* __restrict__ tab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_images) return;
  double t[tri::kCam];
  tri::cam_table(K + 9 * (long)i, T + 16 * (long)i, t);
  for (int k = 0; k < tri::kCam; ++k) tab[(long)tri::kCam * i + k] = t[k];
}

// grid ceil(max(T, K, n) / 256) x 256
__global__ void __launch_bounds__(kThreads) complete_check_kernel(complete::In a, u64* counts) {
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  int err = 0;
  if (t < a.T) err |= complete::check_row(a, t);
  if (t < a.K) err |= complete::check_keypoint(a, t);
  if (t < a.n) err |= complete::check_image(a, (int)t);
  if (err) atomicOr(counts + complete::kErrors, (u64)err);
}

__device__ __forceinline__ unsigned votes(bool p) { return (unsigned)__popcll(__ballot(p)); }

}  // namespace
