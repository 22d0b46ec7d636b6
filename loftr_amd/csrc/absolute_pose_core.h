// Absolute pose (camera resection) from 2D-3D correspondences: the arithmetic shared by the host estimator (absolute_pose.hip) and the
// batched GPU estimator (absolute_pose_gpu.hip).  As in geometry_core.h, every function here is compiled for both sides from this one
// text, fp64, without FMA contraction, so that the two sides take identical decisions: IEEE + - * / and sqrt are correctly rounded on
// both, frexp / ldexp are exact, and the only libm values (cos / sin of the Aberth start angles) are tabulated on the host and handed
// to the device.  No acos, cbrt or trigonometric function is evaluated on the shared path.
//
// The sampler, the complex arithmetic of the root finder (here up to degree 4) and the small vector helpers are ransac_core.h's.
//
// Minimal solver: Grunert's P3P in the form of Haralick, Lee, Ottenberg, Noelle, "Review and analysis of solutions of the three point
// perspective pose estimation problem" (IJCV 1994).  With the camera-to-point distances s1, s2 = u s1, s3 = v s1, the law of cosines
// on the three sides a = |P2 P3|, b = |P1 P3|, c = |P1 P2| gives u = N(v) / D(v) (N quadratic, D linear) and the quartic
//     N^2 + D^2 (1 - (c^2 / b^2) (1 + v^2 - 2 v cos beta)) - 2 cos gamma N D = 0
// in the depth ratio v, whose coefficients are formed here by polynomial multiplication.  Its real positive roots come from the
// Aberth + Newton routine, the distances are polished by Newton steps on the three cosine-law equations, and the rigid motion follows
// from the orthonormal frames of the two point triples (no SVD).
#pragma once
#include "ransac_core.h"

#pragma clang fp contract(off)

#define ABS_HD __host__ __device__ inline

namespace absp {

using namespace ransac;

constexpr int kSample = 3;
constexpr int kSol = 4;                    // hypothesis slots per minimal sample
constexpr int kGnIters = 5;                // Gauss-Newton steps of one fit (fixed: every bit is equal on both sides)
constexpr int kSums = 27;                  // 21 upper-triangle entries of J^T J + 6 of J^T r
// Degenerate samples (relative, scale-free; shared by host and device):
//   world points:  |(P2 - P1) x (P3 - P1)|^2 <= kCollinear^2 * (longest squared side)^2 -- the triangle's sine-scaled area;
//   bearings:      |f_i x f_j|^2 <= kCoincident^2 for a pair of the three unit bearings -- the sine of the angle between them.
constexpr double kCollinear = 1e-6;
constexpr double kCoincident = 1e-7;
// A polished solution is kept when each cosine-law equation holds to kResidual * (longest squared side).
constexpr double kResidual = 1e-10;

using PolarTable = ransac::PolarAngles<4>;    // Aberth start angles up to degree 4

// Small arrays indexed by a run-time value: a select chain over constant indices instead of an address computation, so that the
// device compiler keeps them in registers (same values, no arithmetic).
template <int N, int K = N - 1> struct Pick {
  static ABS_HD double get(const double (&a)[N], int i) { const double v = Pick<N, K - 1>::get(a, i); return K == i ? a[K] : v; }
  static ABS_HD void put(double (&a)[N], int i, double v) { Pick<N, K - 1>::put(a, i, v); a[K] = K == i ? v : a[K]; }
};
template <int N> struct Pick<N, 0> {
  static ABS_HD double get(const double (&a)[N], int) { return a[0]; }
  static ABS_HD void put(double (&a)[N], int i, double v) { a[0] = 0 == i ? v : a[0]; }
};
template <int N> ABS_HD double get(const double (&a)[N], int i) { return Pick<N>::get(a, i); }
template <int N> ABS_HD void put(double (&a)[N], int i, double v) { Pick<N>::put(a, i, v); }

// pose_core.h's real_roots for a polynomial of degree <= 4 (ascending coefficients pin[0..5)), kept apart for its select-chain arrays,
// which stay in registers: Aberth-Ehrlich + Newton polishing on the real axis; the distinct real roots go to r[0..*nr)
ABS_HD void real_roots4(const double (&pin)[5], double (&r)[4], int* nr, const PolarTable& tab) {
  double p[5] = {pin[0], pin[1], pin[2], pin[3], pin[4]};
  int pn = 5;
  while (pn > 1 && fabs(get(p, pn - 1)) < 1e-14 * fabs(p[0] + 1e-300) && fabs(get(p, pn - 1)) < 1e-300) --pn;
  double scale = 0;
  for (int i = 0; i < pn; ++i) { const double a = fabs(get(p, i)); scale = a > scale ? a : scale; }
  if (scale == 0) return;
  while (pn > 1 && fabs(get(p, pn - 1)) < 1e-13 * scale) --pn;
  const int n = pn - 1;
  if (n < 1) return;
  const double lead = get(p, n);
  double radius = 0;
  for (int i = 0; i < n; ++i) { const double q = fabs(get(p, i) / lead); radius = q > radius ? q : radius; }
  radius = 1 + radius;
  double tc[16], ts[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) { tc[k] = tab.c[k / 4][k % 4]; ts[k] = tab.s[k / 4][k % 4]; }
  double zre[4] = {0, 0, 0, 0}, zim[4] = {0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const double rho = radius * (0.3 + 0.7 * (i + 1) / n);
    put(zre, i, rho * get(tc, (n - 1) * 4 + i));
    put(zim, i, rho * get(ts, (n - 1) * 4 + i));
  }
  const cd tiny{1e-300, 0}, one{1.0, 0.0};
  for (int it = 0; it < 200; ++it) {
    double change = 0;
    for (int i = 0; i < n; ++i) {
      const cd zi{get(zre, i), get(zim, i)};
      cd f{lead, 0.0}, df{0.0, 0.0};
      for (int k = n - 1; k >= 0; --k) { df = c_add(c_mul(df, zi), f); f = c_mul(f, zi); f.re = f.re + get(p, k); }
      if (c_abs(f) < 1e-300) continue;
      const cd ratio = c_div(f, c_abs(df) > 1e-300 ? df : tiny);
      cd sum{0.0, 0.0};
      for (int j = 0; j < n; ++j) if (j != i) { const cd d = c_sub(zi, cd{get(zre, j), get(zim, j)}); sum = c_add(sum, c_div(one, c_abs(d) > 1e-300 ? d : tiny)); }
      const cd rs = c_mul(ratio, sum);
      const cd step = c_div(ratio, cd{-rs.re + 1.0, -rs.im});
      const cd zn = c_sub(zi, step);
      put(zre, i, zn.re);
      put(zim, i, zn.im);
      const double as = c_abs(step);
      change = as > change ? as : change;
    }
    if (change < 1e-14 * radius) break;
  }
  for (int i = 0; i < n; ++i) {
    const double re = get(zre, i);
    if (fabs(get(zim, i)) > 1e-6 * (1 + fabs(re))) continue;
    double x = re;
    for (int it = 0; it < 8; ++it) {
      double f = lead, df = 0;
      for (int k = n - 1; k >= 0; --k) { df = df * x + f; f = f * x + get(p, k); }
      if (fabs(df) < 1e-300) break;
      x -= f / df;
    }
    bool dup = false;
    for (int k = 0; k < *nr; ++k) if (fabs(get(r, k) - x) < 1e-9 * (1 + fabs(x))) dup = true;
    if (!dup) { put(r, *nr, x); ++*nr; }
  }
}

// ---- small vectors ----------------------------------------------------------------------------------------------------------------
ABS_HD double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
ABS_HD void sub3(const double* a, const double* b, double* c) { c[0] = a[0] - b[0]; c[1] = a[1] - b[1]; c[2] = a[2] - b[2]; }
// right-handed orthonormal frame (e1, e2, e3 in rows) of the triangle A B C: e1 along AB, e3 along AB x AC
ABS_HD bool triangle_frame(const double* A, const double* B, const double* C, double* e) {
  double ab[3], ac[3], n[3];
  sub3(B, A, ab); sub3(C, A, ac);
  cross3(ab, ac, n);
  const double l1 = sqrt(dot3(ab, ab)), l3 = sqrt(dot3(n, n));
  if (!(l1 > 0) || !(l3 > 0) || !isfinite(l1) || !isfinite(l3)) return false;
  for (int i = 0; i < 3; ++i) { e[i] = ab[i] / l1; e[6 + i] = n[i] / l3; }
  cross3(e + 6, e, e + 3);
  return true;
}

// ---- camera -----------------------------------------------------------------------------------------------------------------------
// K upper triangular with K[2] = (0, 0, 1): u = (fx x + sk y) / z + cx, v = fy y / z + cy
struct Cam { double fx, sk, cx, fy, cy; };
ABS_HD Cam cam_from_K(const float* K) { return {(double)K[0], (double)K[1], (double)K[2], (double)K[4], (double)K[5]}; }
// unit bearing f = K^-1 (u, v, 1) / |.| by the closed-form inverse
ABS_HD void bearing(const Cam& c, double u, double v, double* f) {
  const double y = (v - c.cy) / c.fy;
  const double x = (u - c.cx - c.sk * y) / c.fx;
  const double n = sqrt(x * x + y * y + 1.0);
  f[0] = x / n; f[1] = y / n; f[2] = 1.0 / n;
}

// ---- P3P: world points X [3,3], unit bearings f [3,3] -> up to kSol poses [., 12] (R [9] row-major, then t [3]) with x_cam = R X + t --
// The poses are written as they are found (on the device straight to global memory: the solver keeps no array of them).
constexpr int kPose = 12;
ABS_HD int p3p(const double* X, const double* f, double* poses, const PolarTable& tab) {
  const double *P1 = X, *P2 = X + 3, *P3 = X + 6, *f1 = f, *f2 = f + 3, *f3 = f + 6;
  double d12[3], d13[3], d23[3], nrm[3];
  sub3(P2, P1, d12); sub3(P3, P1, d13); sub3(P3, P2, d23);
  const double a2 = dot3(d23, d23), b2 = dot3(d13, d13), c2 = dot3(d12, d12);
  cross3(d12, d13, nrm);
  double m = a2 > b2 ? a2 : b2;
  m = c2 > m ? c2 : m;
  if (!(dot3(nrm, nrm) > kCollinear * kCollinear * m * m) || !isfinite(m)) return 0;          // (near-)collinear world points
  for (int i = 0; i < 3; ++i) {
    double x[3];
    cross3(f + 3 * i, f + 3 * ((i + 1) % 3), x);
    if (!(dot3(x, x) > kCoincident * kCoincident)) return 0;                                 // coincident bearings
  }
  const double ca = dot3(f2, f3), cb = dot3(f1, f3), cg = dot3(f1, f2);
  const double q = (a2 - c2) / b2, k = c2 / b2;
  const double n0 = 1.0 + q, n1 = -2.0 * q * cb, n2 = q - 1.0;                               // N(v)
  const double d0 = 2.0 * cg, d1 = -2.0 * ca;                                                // D(v)
  const double w0 = 1.0 - k, w1 = 2.0 * k * cb, w2 = -k;                                     // 1 - k (1 + v^2 - 2 v cos beta)
  const double dd0 = d0 * d0, dd1 = 2.0 * d0 * d1, dd2 = d1 * d1;
  double p[5];
  p[0] = n0 * n0 + dd0 * w0 - d0 * (n0 * d0);
  p[1] = 2.0 * n0 * n1 + (dd0 * w1 + dd1 * w0) - d0 * (n0 * d1 + n1 * d0);
  p[2] = (n1 * n1 + 2.0 * n0 * n2) + (dd0 * w2 + dd1 * w1 + dd2 * w0) - d0 * (n1 * d1 + n2 * d0);
  p[3] = 2.0 * n1 * n2 + (dd1 * w2 + dd2 * w1) - d0 * (n2 * d1);
  p[4] = n2 * n2 + dd2 * w2;
  double roots[4] = {0, 0, 0, 0};
  int nr = 0;
  real_roots4(p, roots, &nr, tab);
  double ew[9];
  if (!triangle_frame(P1, P2, P3, ew)) return 0;
  const double cw[3] = {(P1[0] + P2[0] + P3[0]) / 3.0, (P1[1] + P2[1] + P3[1]) / 3.0, (P1[2] + P2[2] + P3[2]) / 3.0};
  int ns = 0;
  for (int r = 0; r < nr && ns < kSol; ++r) {
    const double v = get(roots, r);
    if (!(v > 0)) continue;
    const double Dv = d0 + d1 * v;
    if (!(fabs(Dv) > 1e-9 * (fabs(d0) + fabs(d1 * v)))) continue;                            // u is indeterminate at this root
    const double u = (n0 + v * (n1 + v * n2)) / Dv;
    if (!(u > 0)) continue;
    double s1 = sqrt(b2 / (1.0 + v * (v - 2.0 * cb))), s2 = u * s1, s3 = v * s1;
    bool ok = true;
    for (int it = 0; it < 4 && ok; ++it) {                                                   // Newton on the three cosine-law equations
      const double F0 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * ca - a2, F1 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * cb - b2,
                   F2 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * cg - c2;
      const double j01 = 2.0 * (s2 - s3 * ca), j02 = 2.0 * (s3 - s2 * ca), j10 = 2.0 * (s1 - s3 * cb), j12 = 2.0 * (s3 - s1 * cb),
                   j20 = 2.0 * (s1 - s2 * cg), j21 = 2.0 * (s2 - s1 * cg);
      // J = [0 j01 j02; j10 0 j12; j20 j21 0], solved by Cramer's rule
      const double det = j01 * j12 * j20 + j02 * j10 * j21;
      if (!(fabs(det) > 1e-300) || !isfinite(det)) { ok = false; break; }
      const double e0 = (F0 * (-(j12 * j21)) - j01 * (-(j12 * F2)) + j02 * (F1 * j21)) / det;
      const double e1 = (-(F0 * (-(j12 * j20))) + j02 * (j10 * F2 - F1 * j20)) / det;
      const double e2 = (-(j01 * (j10 * F2 - F1 * j20)) + F0 * (j10 * j21)) / det;
      s1 -= e0; s2 -= e1; s3 -= e2;
    }
    if (!ok || !(s1 > 0) || !(s2 > 0) || !(s3 > 0)) continue;
    const double F0 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * ca - a2, F1 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * cb - b2,
                 F2 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * cg - c2;
    if (!(fabs(F0) <= kResidual * m) || !(fabs(F1) <= kResidual * m) || !(fabs(F2) <= kResidual * m)) continue;
    double Y[9], ec[9];
    for (int i = 0; i < 3; ++i) { Y[i] = s1 * f1[i]; Y[3 + i] = s2 * f2[i]; Y[6 + i] = s3 * f3[i]; }
    if (!triangle_frame(Y, Y + 3, Y + 6, ec)) continue;
    double* Ro = poses + kPose * ns;
    double* to = Ro + 9;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Ro[i * 3 + j] = ec[i] * ew[j] + ec[3 + i] * ew[3 + j] + ec[6 + i] * ew[6 + j];
    for (int i = 0; i < 3; ++i) to[i] = (Y[i] + Y[3 + i] + Y[6 + i]) / 3.0 - dot3(Ro + 3 * i, cw);
    bool dup = false;                                                                        // two roots polished to one solution
    for (int j = 0; j < ns; ++j) {
      double d = 0;
      for (int i = 0; i < 3; ++i) d += fabs(poses[kPose * j + 9 + i] - to[i]);
      double dr = 0;
      for (int i = 0; i < 9; ++i) dr += fabs(poses[kPose * j + i] - Ro[i]);
      if (d <= 1e-9 * (1.0 + fabs(to[0]) + fabs(to[1]) + fabs(to[2])) && dr <= 1e-9) dup = true;
    }
    if (!dup) ++ns;
  }
  return ns;
}

// ---- scorer: p = K (R X + t); inlier iff p_z > 0 and |(p_x / p_z, p_y / p_z) - (u, v)|^2 <= thr2 --------------------------------------
ABS_HD bool is_inlier(const Cam& c, const double* R, const double* t, const double* X, double u, double v, double thr2) {
  const double x = dot3(R, X) + t[0], y = dot3(R + 3, X) + t[1], z = dot3(R + 6, X) + t[2];
  if (!(z > 0)) return false;
  const double du = (c.fx * x + c.sk * y + c.cx * z) / z - u, dv = (c.fy * y + c.cy * z) / z - v;
  return du * du + dv * dv <= thr2;
}

// ---- Gauss-Newton refit on the pixel reprojection error ---------------------------------------------------------------------------
// Parameters: a left rotation increment w (x_cam = Rot(w) R X + t + dt) and an additive translation increment dt.  With Y = R X and
// g the gradient of a pixel coordinate with respect to x_cam, the Jacobian row is (Y x g, g).  One match adds its 21 + 6 terms of
// J^T J (upper triangle, row-major) and J^T r to acc; a match with p_z <= 0 adds nothing.
ABS_HD void accum27(const Cam& c, const double* R, const double* t, const double* X, double u, double v, double* acc) {
  const double Y[3] = {dot3(R, X), dot3(R + 3, X), dot3(R + 6, X)};
  const double x = Y[0] + t[0], y = Y[1] + t[1], z = Y[2] + t[2];
  if (!(z > 0)) return;
  const double a = c.fx * x + c.sk * y, b = c.fy * y;
  const double ru = (a + c.cx * z) / z - u, rv = (b + c.cy * z) / z - v;
  const double gu[3] = {c.fx / z, c.sk / z, -(a / (z * z))}, gv[3] = {0.0, c.fy / z, -(b / (z * z))};
  double ju[6], jv[6];
  cross3(Y, gu, ju); cross3(Y, gv, jv);
  for (int i = 0; i < 3; ++i) { ju[3 + i] = gu[i]; jv[3 + i] = gv[i]; }
  int k = 0;
  for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) acc[k++] += ju[i] * ju[j] + jv[i] * jv[j];
  for (int i = 0; i < 6; ++i) acc[k++] += ju[i] * ru + jv[i] * rv;
}
// One step from the reduced sums: (J^T J) d = -J^T r by a fixed-order elimination without pivoting; a non-positive pivot or a
// non-finite step fails.  The rotation increment is applied through the normalised quaternion (1, w / 2).
ABS_HD bool gn_step(const double* sums, double* R, double* t) {
  double A[6][6], b[6], d[6];
  int k = 0;
  for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) { A[i][j] = sums[k]; A[j][i] = sums[k]; ++k; }
  for (int i = 0; i < 6; ++i) b[i] = -sums[k++];
  for (int c = 0; c < 6; ++c) {
    const double piv = A[c][c];
    if (!(piv > 0) || !isfinite(piv)) return false;
    for (int i = c + 1; i < 6; ++i) {
      const double f = A[i][c] / piv;
      for (int j = c; j < 6; ++j) A[i][j] -= f * A[c][j];
      b[i] -= f * b[c];
    }
  }
  for (int i = 5; i >= 0; --i) {
    double s = b[i];
    for (int j = i + 1; j < 6; ++j) s -= A[i][j] * d[j];
    d[i] = s / A[i][i];
    if (!isfinite(d[i])) return false;
  }
  const double hx = 0.5 * d[0], hy = 0.5 * d[1], hz = 0.5 * d[2];
  const double qn = sqrt(1.0 + hx * hx + hy * hy + hz * hz);
  const double qw = 1.0 / qn, qx = hx / qn, qy = hy / qn, qz = hz / qn;
  const double Q[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                       2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                       2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
  double Rn[9];
  mat3_mul(Q, R, Rn);
  for (int i = 0; i < 9; ++i) R[i] = Rn[i];
  for (int i = 0; i < 3; ++i) t[i] += d[3 + i];
  return true;
}

}  // namespace absp
