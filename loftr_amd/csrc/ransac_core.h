// What the three RANSAC estimators (relative pose, homography / fundamental matrix, absolute pose) share, written once for the host
// estimators (pose.hip, geometry.hip, absolute_pose.hip) and their batched GPU forms (*_gpu.hip): the caps, the xorshift64* sampler with
// its duplicate rejection, the adaptive stopping rule, the fixed summation tree of the refits, the complex arithmetic of the Aberth
// root finders and the small dense linear algebra.  Every __host__ __device__ function here is compiled for both sides from this one
// text, fp64, without FMA contraction, so that the two sides take identical decisions: IEEE + - * / and sqrt are correctly rounded on
// both, frexp / ldexp are exact, and the only libm values (cos / sin of the Aberth start angles) are tabulated on the host and handed
// to the device.  pose_core.h, geometry_core.h and absolute_pose_core.h build on it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#pragma clang fp contract(off)

#define RANSAC_HD __host__ __device__ inline

namespace ransac {

constexpr int kIters = 1000;               // RANSAC iteration cap (cv2.findEssentialMat's documented default)
// A least-squares refit is repeated on the adopted model's inliers while it strictly gains inliers, at most this many fits.
constexpr int kRefitRounds = 4;
constexpr int kLanes = 256;                // strided partial sums of a refit: partial k takes matches i = k (mod 256), ascending
constexpr int kMaxSample = 7;              // largest minimal sample (fundamental matrix)

struct Rng {                                                     // xorshift64*
  uint64_t s;
  RANSAC_HD explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) { if (!s) s = 1; }
  RANSAC_HD uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
  RANSAC_HD long below(long n) { return (long)(next() % (uint64_t)n); }
};
// the s distinct indices below n of one minimal sample: a draw that repeats an earlier index of the sample is drawn again
RANSAC_HD void draw_sample(Rng& rng, long n, int s, int* d) {
  for (int k = 0; k < s;) {
    const int c = (int)rng.below(n);
    bool dup = false;
    for (int j = 0; j < k; ++j) dup = dup || d[j] == c;
    if (!dup) d[k++] = c;
  }
}

// The adaptive iteration count from the confidence: iteration `it` found a new best hypothesis with cnt of M inliers; the loop's new
// bound.  Host only (the GPU estimators replay their loops on the host): the bound depends on the host libm's pow / log.
inline int adaptive_iters(long cnt, long M, int s, float conf, int it, int iters) {
  const double w = (double)cnt / (double)M;
  const double p_all = pow(w, (double)s);
  if (p_all > 1 - 1e-12) return it + 1;
  if (p_all > 1e-12) {
    const double need = log(1.0 - (double)conf) / log(1.0 - p_all);
    if (need < iters) return need < it + 1 ? it + 1 : (int)ceil(need);
  }
  return iters;
}

// the fixed pairwise tree over the kLanes strided partials (host; ransac_gpu.h's block_tree is the same tree in LDS)
inline double tree(double* p) {
  for (int st = kLanes / 2; st >= 1; st >>= 1) for (int k = 0; k < st; ++k) p[k] = p[k] + p[k + st];
  return p[0];
}

// ---- small dense linear algebra -----------------------------------------------------------------------------------------------------
// symmetric eigen-decomposition by cyclic Jacobi: a (n x n, destroyed) -> eigenvalues w, eigenvectors in the columns of v
template <int n>
RANSAC_HD void jacobi_eig(double* a, double* w, double* v) {
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) v[i * n + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
    for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) off += a[i * n + j] * a[i * n + j];
    if (off < 1e-300) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[p * n + q];
        if (fabs(apq) < 1e-300) continue;
        const double theta = (a[q * n + q] - a[p * n + p]) / (2 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
        const double c = 1 / sqrt(t * t + 1), s = t * c;
        for (int k = 0; k < n; ++k) {
          const double akp = a[k * n + p], akq = a[k * n + q];
          a[k * n + p] = c * akp - s * akq; a[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = a[p * n + k], aqk = a[q * n + k];
          a[p * n + k] = c * apk - s * aqk; a[q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = v[k * n + p], vkq = v[k * n + q];
          v[k * n + p] = c * vkp - s * vkq; v[k * n + q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < n; ++i) w[i] = a[i * n + i];
}

RANSAC_HD void mat3_mul(const double* a, const double* b, double* c) {
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}
RANSAC_HD void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
// determinant of the matrix with rows r0, r1, r2 (cofactors along r0)
RANSAC_HD double det3_rows(const double* r0, const double* r1, const double* r2) {
  return r0[0] * (r1[1] * r2[2] - r1[2] * r2[1]) - r0[1] * (r1[0] * r2[2] - r1[2] * r2[0]) + r0[2] * (r1[0] * r2[1] - r1[1] * r2[0]);
}

// E = U diag(s) V^T with U, V proper or improper orthogonal (columns), s descending, via the eigen-decomposition of E^T E
RANSAC_HD void svd3(const double* E, double* U, double* s, double* V) {
  double ete[9], w[3], v[9];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) ete[i * 3 + j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
  jacobi_eig<3>(ete, w, v);
  int o[3] = {0, 1, 2};
  for (int i = 0; i < 3; ++i) for (int j = i + 1; j < 3; ++j) if (w[o[j]] > w[o[i]]) { int t = o[i]; o[i] = o[j]; o[j] = t; }
  for (int k = 0; k < 3; ++k) {
    s[k] = sqrt(w[o[k]] > 0 ? w[o[k]] : 0);
    for (int i = 0; i < 3; ++i) V[i * 3 + k] = v[i * 3 + o[k]];
  }
  double u[3][3];
  for (int k = 0; k < 2; ++k) {
    for (int i = 0; i < 3; ++i) u[k][i] = E[i * 3] * V[k] + E[i * 3 + 1] * V[3 + k] + E[i * 3 + 2] * V[6 + k];
    double nrm = sqrt(u[k][0] * u[k][0] + u[k][1] * u[k][1] + u[k][2] * u[k][2]);
    if (nrm < 1e-300) nrm = 1;
    for (int i = 0; i < 3; ++i) u[k][i] /= nrm;
  }
  // re-orthogonalise the second against the first, third = cross product
  double d = u[0][0] * u[1][0] + u[0][1] * u[1][1] + u[0][2] * u[1][2];
  for (int i = 0; i < 3; ++i) u[1][i] -= d * u[0][i];
  double nrm = sqrt(u[1][0] * u[1][0] + u[1][1] * u[1][1] + u[1][2] * u[1][2]);
  if (nrm < 1e-300) nrm = 1;
  for (int i = 0; i < 3; ++i) u[1][i] /= nrm;
  cross3(u[0], u[1], u[2]);
  for (int k = 0; k < 3; ++k) for (int i = 0; i < 3; ++i) U[i * 3 + k] = u[k][i];
}

// ---- complex arithmetic as the host's C++ library computes it -------------------------------------------------------------------------
// The Aberth root finders were first written with std::complex; these are the operations it performs, bit for bit: the inline
// (ac - bd, ad + bc) product clang emits (its __muldc3 fallback only runs when both parts are NaN), libstdc++'s scaled |z|, and
// compiler-rt's __divdc3 with its logb.
struct cd { double re, im; };
RANSAC_HD cd c_add(cd a, cd b) { return {a.re + b.re, a.im + b.im}; }
RANSAC_HD cd c_sub(cd a, cd b) { return {a.re - b.re, a.im - b.im}; }
RANSAC_HD cd c_mul(cd a, cd b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
RANSAC_HD double c_abs(cd z) {                                   // libstdc++ __complex_abs
  double x = z.re, y = z.im;
  const double ax = fabs(x), ay = fabs(y);
  const double s = ax < ay ? ay : ax;
  if (s == 0.0) return s;
  x /= s;
  y /= s;
  return s * sqrt(x * x + y * y);
}
RANSAC_HD double crt_logb(double x) {                            // compiler-rt logb: exponent of a finite non-zero x
  if (isnan(x)) return x;
  if (isinf(x)) return INFINITY;
  if (x == 0.0) return -INFINITY;
  int e;
  frexp(x, &e);
  return (double)(e - 1);
}
// x * 2^k correctly rounded, which is ldexp.  On the host the product with the exactly representable 2^k (|k| <= 1022) is that same
// IEEE operation without the call into libm, which otherwise is a third of the five-point estimator's time; the device's ldexp is one
// instruction.
RANSAC_HD double scale2(double x, int k) {
#ifndef __HIP_DEVICE_COMPILE__
  if (k >= -1022 && k <= 1022) {
    const uint64_t bits = (uint64_t)(k + 1023) << 52;
    double p;
    memcpy(&p, &bits, sizeof(p));
    return x * p;
  }
#endif
  return ldexp(x, k);
}
RANSAC_HD cd c_div(cd num, cd den) {                             // compiler-rt __divdc3
  double a = num.re, b = num.im, c = den.re, d = den.im;
  int ilogbw = 0;
  const double ac = fabs(c), ad = fabs(d);
  const double mx = isnan(c) ? ad : (isnan(d) ? ac : (ac > ad ? ac : ad));
  const double logbw = crt_logb(mx);
  if (isfinite(logbw)) {
    ilogbw = (int)logbw;
    c = scale2(c, -ilogbw);
    d = scale2(d, -ilogbw);
  }
  const double denom = c * c + d * d;
  cd z{scale2((a * c + b * d) / denom, -ilogbw), scale2((b * c - a * d) / denom, -ilogbw)};
  if (isnan(z.re) && isnan(z.im)) {
    if (denom == 0.0 && (!isnan(a) || !isnan(b))) {
      z.re = copysign(INFINITY, c) * a;
      z.im = copysign(INFINITY, c) * b;
    } else if ((isinf(a) || isinf(b)) && isfinite(c) && isfinite(d)) {
      a = copysign(isinf(a) ? 1.0 : 0.0, a);
      b = copysign(isinf(b) ? 1.0 : 0.0, b);
      z.re = INFINITY * (a * c + b * d);
      z.im = INFINITY * (b * c - a * d);
    } else if (isinf(logbw) && logbw > 0.0 && isfinite(a) && isfinite(b)) {
      c = copysign(isinf(c) ? 1.0 : 0.0, c);
      d = copysign(isinf(d) ? 1.0 : 0.0, d);
      z.re = 0.0 * (a * c + b * d);
      z.im = 0.0 * (b * c - a * d);
    }
  }
  return z;
}

// cos / sin of the Aberth start angles 2 pi i / n + 0.4 (std::polar(rho, theta)), n = 1..N, from the host's libm
template <int N> struct PolarAngles { double c[N][N], s[N][N]; };
template <int N>
inline PolarAngles<N> polar_table() {                             // host only
  PolarAngles<N> t{};
  for (int n = 1; n <= N; ++n)
    for (int i = 0; i < n; ++i) {
      const double theta = 2 * M_PI * i / n + 0.4;
      t.c[n - 1][i] = cos(theta);
      t.s[n - 1][i] = sin(theta);
    }
  return t;
}

}  // namespace ransac
