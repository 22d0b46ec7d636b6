// Removing (and applying) the radial coefficient of a camera on pixels, host code: these routines DEFINE the result, the kernel of
// undistort_gpu.hip reproduces it bit for bit.  All the arithmetic is radial_core.h's; this file is the loop and the check of the image
// ids (the contract is in include/loftr_hip.h).
#include <stdint.h>
#include "../../include/loftr_hip.h"
#include "radial_core.h"

#pragma clang fp contract(off)

using namespace radial;

namespace {

template <class F> int run(const float* xy, const int* image, long M, const double* K, const double* k, int n, float* xy_out, uint8_t* ok,
                           long* counts, F point) {
  const int st = check_args(xy, image, M, K, k, n, xy_out, ok, counts);
  if (st != LOFTR_OK) return st;
  for (int i = 0; i < kCounts; ++i) counts[i] = 0;
  for (long p = 0; p < M; ++p)
    if (image[p] < 0 || image[p] >= n) { counts[1] = kBadImage; return LOFTR_ERR_BAD_ARG; }     // nothing is written
  for (long p = 0; p < M; ++p) {
    const int i = image[p];
    ok[p] = (uint8_t)point(K + 9 * i, k[i], xy[2 * p], xy[2 * p + 1], xy_out + 2 * p);
    counts[0] += ok[p];
  }
  counts[2] = M - counts[0];
  return LOFTR_OK;
}

}  // namespace

extern "C" int loftr_undistort_points_host(const float* xy, const int* image, long M, const double* K, const double* radial, int n_images,
                                           float* xy_out, uint8_t* ok, long* counts) {
  return run(xy, image, M, K, radial, n_images, xy_out, ok, counts, undistort_point);
}

extern "C" int loftr_distort_points_host(const float* xy, const int* image, long M, const double* K, const double* radial, int n_images,
                                         float* xy_out, uint8_t* ok, long* counts) {
  return run(xy, image, M, K, radial, n_images, xy_out, ok, counts, distort_point);
}
