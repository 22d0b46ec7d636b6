// One radial coefficient on normalised coordinates, x_d = x (1 + k r^2): removing it from pixels (loftr_undistort_points_host /
// loftr_undistort_points) and applying it (loftr_distort_points_host, for the tests and the tools).  As in bundle_core.h every function
// here is compiled for the host routine (undistort.hip) and for the kernel (undistort_gpu.hip) from this one text, fp64, without FMA
// contraction, + - * / and sqrt only, so that both sides produce identical bits; a point depends on nothing but its own inputs, so the
// identity is per point.  The rule is stated in include/loftr_hip.h and DESIGN §18.4.  This is the camera model the Radial mode of the
// bundle adjustment fits (bundle_core.h: residual_radial); every other stage of the chain reads pinhole pixels and gets them from here.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/loftr_hip.h"

#pragma clang fp contract(off)

#define RD_HD __host__ __device__ inline

namespace radial {

constexpr int kCounts = 8;                 // counts[]: see include/loftr_hip.h
constexpr int kNewton = 12;                // Newton iterations, fixed: no data-dependent exit
constexpr double kTol = 1e-9;              // |r (1 + k r^2) - r_d| <= kTol (1 + r_d)
enum : int { kBadImage = 1 };              // error bit (counts[1])

RD_HD bool fin(double x) { return fabs(x) <= 1.7976931348623157e308; }        // false for NaN and the infinities

// the intrinsics of image i are usable: fx, skew, cx, fy, cy and k finite, fx and fy not zero
RD_HD bool camera_ok(const double* K, double k) {
  return fin(K[0]) && fin(K[1]) && fin(K[2]) && fin(K[4]) && fin(K[5]) && fin(k) && K[0] != 0.0 && K[4] != 0.0;
}
// pixel -> normalised: y = (v - cy) / fy, x = ((u - cx) - skew y) / fx
RD_HD void normalise(const double* K, double u, double v, double* x, double* y) {
  *y = (v - K[5]) / K[4];
  *x = ((u - K[2]) - K[1] * *y) / K[0];
}
// normalised -> pixel, rounded to f32: ((fx x + skew y) + cx, fy y + cy) -> both finite
RD_HD bool to_pixel(const double* K, double x, double y, float* out) {
  out[0] = (float)((K[0] * x + K[1] * y) + K[2]);
  out[1] = (float)(K[4] * y + K[5]);
  return fin((double)out[0]) && fin((double)out[1]);
}
RD_HD void fail(float* out) {                                           // the quiet NaN 0x7fc00000 on both sides
  union { uint32_t u; float f; } q;
  q.u = 0x7fc00000u;
  out[0] = out[1] = q.f;
}

// The distorted pixel -> the pinhole pixel of the same ray.  r_d = sqrt(x_d^2 + y_d^2); r starts at r_d and takes kNewton steps
// r = r - (r (1 + k (r r)) - r_d) / (1 + 3 k (r r)); m = 1 + k (r r), x = x_d / m, y = y_d / m (so r_d = 0 gives the principal point).
// ok iff the camera is usable, u and v and every value on the way are finite, 1 + 3 k (r r) > 0 at the result (the result lies on the
// monotone branch) and the residual of the equation is within kTol (1 + r_d).  A point that is not ok is (NaN, NaN).  k = 0 is ok and
// the point is recomputed through K: NOT promised to be the input's bits.
RD_HD bool undistort_point(const double* K, double k, float u, float v, float* out) {
  bool ok = camera_ok(K, k) && fin((double)u) && fin((double)v);
  double xd, yd;
  normalise(K, (double)u, (double)v, &xd, &yd);
  const double rd = sqrt(xd * xd + yd * yd);
  double r = rd;
  for (int it = 0; it < kNewton; ++it) r = r - (r * (1.0 + k * (r * r)) - rd) / (1.0 + (3.0 * k) * (r * r));
  const double m = 1.0 + k * (r * r), res = r * m - rd;
  ok = ok && fin(rd) && fin(r) && 1.0 + (3.0 * k) * (r * r) > 0.0 && fabs(res) <= kTol * (1.0 + rd);
  ok = ok && to_pixel(K, xd / m, yd / m, out);
  if (!ok) fail(out);
  return ok;
}
// The pinhole pixel -> the distorted pixel: r2 = x x + y y, m = 1 + k r2, (x m, y m) through K.  ok iff the camera is usable and
// everything is finite.
RD_HD bool distort_point(const double* K, double k, float u, float v, float* out) {
  bool ok = camera_ok(K, k) && fin((double)u) && fin((double)v);
  double x, y;
  normalise(K, (double)u, (double)v, &x, &y);
  const double m = 1.0 + k * (x * x + y * y);
  ok = ok && to_pixel(K, x * m, y * m, out);
  if (!ok) fail(out);
  return ok;
}

// the argument checks of the entry points -> LOFTR_OK when the run may start
inline int check_args(const float* xy, const int* image, long M, const double* K, const double* radial, int n, const float* xy_out,
                      const uint8_t* ok, const long* counts) {
  if (M < 0 || n < 0 || !counts) return LOFTR_ERR_BAD_ARG;
  if (M > 0 && (!xy || !image || !xy_out || !ok)) return LOFTR_ERR_BAD_ARG;
  if (n > 0 && (!K || !radial)) return LOFTR_ERR_BAD_ARG;
  return LOFTR_OK;
}

}  // namespace radial
