// Homography / fundamental-matrix estimation: the arithmetic shared by the host estimator (geometry.hip) and the batched GPU
// estimator (geometry_gpu.hip).  Every function here is compiled for both sides from this one text, fp64, without FMA
// contraction, so that the two sides take identical decisions: IEEE + - * / and sqrt are correctly rounded on both, frexp / ldexp
// are exact, and the only libm values (cos / sin of the Aberth start angles) are tabulated on the host and handed to the device.
//
// The sampler, the small dense linear algebra (cyclic Jacobi, svd3) and the complex arithmetic of the root finder are ransac_core.h's.
#pragma once
#include "ransac_core.h"

#pragma clang fp contract(off)

#define GEO_HD __host__ __device__ inline

namespace geo {

using namespace ransac;

// A homography sample is rejected when a triple of its four points has |signed area| (twice the triangle's area, in the
// Hartley-normalised frame of the four points: centroid 0, mean distance sqrt 2) below this, in either image.
constexpr double kCollinearArea = 1e-3;

GEO_HD int sample_size(int model) { return model == 0 ? 4 : 7; }
GEO_HD int max_solutions(int model) { return model == 0 ? 1 : 3; }

using PolarTable = ransac::PolarAngles<3>;   // Aberth start angles up to degree 3

// pose_core.h's real_roots for a polynomial of degree <= 3 (ascending coefficients pin[0..4)), kept apart for its arrays of that size,
// which stay in registers: Aberth-Ehrlich + Newton polishing on the real axis; the distinct real roots go to r[0..*nr)
GEO_HD void real_roots3(const double* pin, double* r, int* nr, const PolarTable& tab) {
  double p[4] = {pin[0], pin[1], pin[2], pin[3]};
  int pn = 4;
  while (pn > 1 && fabs(p[pn - 1]) < 1e-14 * fabs(p[0] + 1e-300) && fabs(p[pn - 1]) < 1e-300) --pn;
  double scale = 0;
  for (int i = 0; i < pn; ++i) scale = fabs(p[i]) > scale ? fabs(p[i]) : scale;
  if (scale == 0) return;
  while (pn > 1 && fabs(p[pn - 1]) < 1e-13 * scale) --pn;
  const int n = pn - 1;
  if (n < 1) return;
  double radius = 0;
  for (int i = 0; i < n; ++i) { const double q = fabs(p[i] / p[n]); radius = q > radius ? q : radius; }
  radius = 1 + radius;
  cd z[3];
  for (int i = 0; i < n; ++i) {
    const double rho = radius * (0.3 + 0.7 * (i + 1) / n);
    z[i] = {rho * tab.c[n - 1][i], rho * tab.s[n - 1][i]};
  }
  const cd tiny{1e-300, 0}, one{1.0, 0.0};
  for (int it = 0; it < 200; ++it) {
    double change = 0;
    for (int i = 0; i < n; ++i) {
      cd f{p[n], 0.0}, df{0.0, 0.0};
      for (int k = n - 1; k >= 0; --k) { df = c_add(c_mul(df, z[i]), f); f = c_mul(f, z[i]); f.re = f.re + p[k]; }
      if (c_abs(f) < 1e-300) continue;
      const cd ratio = c_div(f, c_abs(df) > 1e-300 ? df : tiny);
      cd sum{0.0, 0.0};
      for (int j = 0; j < n; ++j) if (j != i) { const cd d = c_sub(z[i], z[j]); sum = c_add(sum, c_div(one, c_abs(d) > 1e-300 ? d : tiny)); }
      const cd rs = c_mul(ratio, sum);
      const cd step = c_div(ratio, cd{-rs.re + 1.0, -rs.im});
      z[i] = c_sub(z[i], step);
      const double as = c_abs(step);
      change = as > change ? as : change;
    }
    if (change < 1e-14 * radius) break;
  }
  for (int i = 0; i < n; ++i) {
    if (fabs(z[i].im) > 1e-6 * (1 + fabs(z[i].re))) continue;
    double x = z[i].re;
    for (int it = 0; it < 8; ++it) {
      double f = p[n], df = 0;
      for (int k = n - 1; k >= 0; --k) { df = df * x + f; f = f * x + p[k]; }
      if (fabs(df) < 1e-300) break;
      x -= f / df;
    }
    bool dup = false;
    for (int k = 0; k < *nr; ++k) if (fabs(r[k] - x) < 1e-9 * (1 + fabs(x))) dup = true;
    if (!dup) r[(*nr)++] = x;
  }
}

// ---- normalisation ---------------------------------------------------------------------------------------------------------------
// Hartley: x' = (x - c) * s with s = sqrt 2 / (mean distance to the centroid c)
struct Norm { double cx, cy, s; };
GEO_HD bool make_norm(double cx, double cy, double sd, double cnt, Norm* N) {     // centroid, sum of distances to it, count
  const double md = sd / cnt;
  if (!(md > 1e-300) || !isfinite(md)) return false;
  N->cx = cx; N->cy = cy; N->s = 1.4142135623730951 / md;
  return true;
}
GEO_HD bool sample_norm(const double* x, const double* y, int n, Norm* N) {                            // sequential over the sample
  double sx = 0, sy = 0;
  for (int i = 0; i < n; ++i) { sx += x[i]; sy += y[i]; }
  const double cx = sx / n, cy = sy / n;
  double sd = 0;
  for (int i = 0; i < n; ++i) { const double dx = x[i] - cx, dy = y[i] - cy; sd += sqrt(dx * dx + dy * dy); }
  return make_norm(cx, cy, sd, (double)n, N);
}
GEO_HD void norm_matrix(const Norm& N, double* T) {              // T x = x'
  T[0] = N.s; T[1] = 0; T[2] = -(N.s * N.cx); T[3] = 0; T[4] = N.s; T[5] = -(N.s * N.cy); T[6] = 0; T[7] = 0; T[8] = 1;
}
GEO_HD void norm_matrix_inv(const Norm& N, double* T) {          // T x' = x
  T[0] = 1 / N.s; T[1] = 0; T[2] = N.cx; T[3] = 0; T[4] = 1 / N.s; T[5] = N.cy; T[6] = 0; T[7] = 0; T[8] = 1;
}
GEO_HD bool unit_norm(double* m) {
  double nrm = 0;
  for (int i = 0; i < 9; ++i) nrm += m[i] * m[i];
  nrm = sqrt(nrm);
  if (!(nrm > 1e-300) || !isfinite(nrm)) return false;
  for (int i = 0; i < 9; ++i) m[i] /= nrm;
  return true;
}
// model in the normalised frames -> pixels:  H = T1^-1 H' T0,  F = T1^T F' T0;  unit Frobenius norm
GEO_HD bool denormalise(int model, const double* mn, const Norm& n0, const Norm& n1, double* out) {
  double T0[9], T1[9], L[9], tmp[9];
  norm_matrix(n0, T0);
  if (model == 0) norm_matrix_inv(n1, L);
  else { norm_matrix(n1, T1); for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) L[i * 3 + j] = T1[j * 3 + i]; }
  mat3_mul(L, mn, tmp);
  mat3_mul(tmp, T0, out);
  return unit_norm(out);
}

// design-matrix rows of one correspondence (x0, y0) -> (x1, y1):  homography two rows (r, r2), fundamental one (r)
GEO_HD void design_rows(int model, double x0, double y0, double x1, double y1, double* r, double* r2) {
  if (model == 0) {
    r[0] = -x0; r[1] = -y0; r[2] = -1.0; r[3] = 0.0; r[4] = 0.0; r[5] = 0.0; r[6] = x1 * x0; r[7] = x1 * y0; r[8] = x1;
    r2[0] = 0.0; r2[1] = 0.0; r2[2] = 0.0; r2[3] = -x0; r2[4] = -y0; r2[5] = -1.0; r2[6] = y1 * x0; r2[7] = y1 * y0; r2[8] = y1;
  } else {
    r[0] = x1 * x0; r[1] = x1 * y0; r[2] = x1; r[3] = y1 * x0; r[4] = y1 * y0; r[5] = y1; r[6] = x0; r[7] = y0; r[8] = 1.0;
  }
}
// the 45 upper-triangle entries (row-major: (0,0) (0,1) .. (0,8) (1,1) ..) of A^T A, one correspondence added
GEO_HD void accum45(int model, double x0, double y0, double x1, double y1, double* acc) {
  double r[9], r2[9];
  design_rows(model, x0, y0, x1, y1, r, r2);
  int k = 0;
  if (model == 0) { for (int a = 0; a < 9; ++a) for (int b = a; b < 9; ++b) acc[k++] += r[a] * r[b] + r2[a] * r2[b]; }
  else { for (int a = 0; a < 9; ++a) for (int b = a; b < 9; ++b) acc[k++] += r[a] * r[b]; }
}
// eigenvectors of the two smallest eigenvalues of the symmetric matrix with upper triangle acc45 (first index wins ties)
GEO_HD void null_vectors(const double* acc45, double* v0, double* v1) {
  double a[81], w[9], v[81];
  int k = 0;
  for (int i = 0; i < 9; ++i) for (int j = i; j < 9; ++j) { a[i * 9 + j] = acc45[k]; a[j * 9 + i] = acc45[k]; ++k; }
  jacobi_eig<9>(a, w, v);
  int m0 = 0;
  for (int i = 1; i < 9; ++i) if (w[i] < w[m0]) m0 = i;
  int m1 = m0 == 0 ? 1 : 0;
  for (int i = 0; i < 9; ++i) if (i != m0 && w[i] < w[m1]) m1 = i;
  for (int i = 0; i < 9; ++i) { v0[i] = v[i * 9 + m0]; if (v1) v1[i] = v[i * 9 + m1]; }
}

// ---- minimal solvers: s pixel correspondences -> up to max_solutions(model) unit-norm matrices (row-major) in mats ---------------
// Homography: H x0 has a positive third coordinate at the four sample points (the sign convention the scorer relies on).
GEO_HD int solve_minimal(int model, const double* x0, const double* y0, const double* x1, const double* y1, double* mats,
                         const PolarTable& tab) {
  const int s = sample_size(model);
  Norm n0, n1;
  if (!sample_norm(x0, y0, s, &n0) || !sample_norm(x1, y1, s, &n1)) return 0;
  double a0[7], b0[7], a1[7], b1[7];
  for (int i = 0; i < s; ++i) {
    a0[i] = (x0[i] - n0.cx) * n0.s; b0[i] = (y0[i] - n0.cy) * n0.s;
    a1[i] = (x1[i] - n1.cx) * n1.s; b1[i] = (y1[i] - n1.cy) * n1.s;
  }
  if (model == 0) {
    for (int i = 0; i < 4; ++i) for (int j = i + 1; j < 4; ++j) for (int k = j + 1; k < 4; ++k) {
      const double s0 = (a0[j] - a0[i]) * (b0[k] - b0[i]) - (b0[j] - b0[i]) * (a0[k] - a0[i]);
      const double s1 = (a1[j] - a1[i]) * (b1[k] - b1[i]) - (b1[j] - b1[i]) * (a1[k] - a1[i]);
      if (!(fabs(s0) >= kCollinearArea) || !(fabs(s1) >= kCollinearArea)) return 0;     // three collinear points
      if ((s0 > 0) != (s1 > 0)) return 0;                                               // orientation flipped
    }
  }
  double acc[45];
  for (int i = 0; i < 45; ++i) acc[i] = 0.0;
  for (int i = 0; i < s; ++i) accum45(model, a0[i], b0[i], a1[i], b1[i], acc);
  double f1[9], f2[9];
  null_vectors(acc, f1, model == 0 ? nullptr : f2);
  if (model == 0) {
    if (!denormalise(0, f1, n0, n1, mats)) return 0;
    const double w0 = mats[6] * x0[0] + mats[7] * y0[0] + mats[8];
    if (w0 < 0) for (int i = 0; i < 9; ++i) mats[i] = -mats[i];
    for (int i = 0; i < 4; ++i) if (!(mats[6] * x0[i] + mats[7] * y0[i] + mats[8] > 0)) return 0;
    return 1;
  }
  // det(a f1 + (1 - a) f2) = det(G + a D), G = f2, D = f1 - f2: a cubic in a
  double D[9];
  for (int i = 0; i < 9; ++i) D[i] = f1[i] - f2[i];
  const double* G = f2;
  double c[4];
  c[0] = det3_rows(G, G + 3, G + 6);
  c[1] = det3_rows(D, G + 3, G + 6) + det3_rows(G, D + 3, G + 6) + det3_rows(G, G + 3, D + 6);
  c[2] = det3_rows(G, D + 3, D + 6) + det3_rows(D, G + 3, D + 6) + det3_rows(D, D + 3, G + 6);
  c[3] = det3_rows(D, D + 3, D + 6);
  double roots[3];
  int nr = 0;
  real_roots3(c, roots, &nr, tab);
  int ns = 0;
  for (int k = 0; k < nr; ++k) {
    double fn[9];
    for (int i = 0; i < 9; ++i) fn[i] = G[i] + roots[k] * D[i];
    if (denormalise(1, fn, n0, n1, mats + 9 * ns)) ++ns;
  }
  return ns;
}

// ---- residual test: is the correspondence within thr2 (squared pixels) of the model? --------------------------------------------
// Homography: squared forward transfer error |x1 - pi(H x0)|^2; a non-positive third coordinate of H x0 is an outlier.
// Fundamental: squared Sampson distance (on pixels; `<=`, where the five-point estimator on normalised points has `<`).
GEO_HD bool is_inlier(int model, const double* m, double x0, double y0, double x1, double y1, double thr2) {
  if (model == 0) {
    const double w = m[6] * x0 + m[7] * y0 + m[8];
    if (!(w > 0)) return false;
    const double du = x1 - (m[0] * x0 + m[1] * y0 + m[2]) / w, dv = y1 - (m[3] * x0 + m[4] * y0 + m[5]) / w;
    return du * du + dv * dv <= thr2;
  }
  const double l0 = m[0] * x0 + m[1] * y0 + m[2], l1 = m[3] * x0 + m[4] * y0 + m[5], l2 = m[6] * x0 + m[7] * y0 + m[8];
  const double m0 = m[0] * x1 + m[3] * y1 + m[6], m1 = m[1] * x1 + m[4] * y1 + m[7];
  const double r = x1 * l0 + y1 * l1 + l2;
  const double den = l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1;
  return den > 0 && r * r <= thr2 * den;
}

// ---- least-squares refit from the reduced sums ----------------------------------------------------------------------------------
// acc45: normal matrix of the inliers in their Hartley frames n0 / n1.  Homography: sign with a positive third coordinate at the
// inliers' centroid in image 0.  Fundamental: rank 2 enforced in the normalised frame (smallest singular value zeroed).
GEO_HD bool refit_solve(int model, const double* acc45, const Norm& n0, const Norm& n1, double* out) {
  double f[9];
  null_vectors(acc45, f, nullptr);
  if (model == 1) {
    double U[9], s[3], V[9], us[9];
    svd3(f, U, s, V);
    s[2] = 0.0;
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) us[i * 3 + k] = U[i * 3 + k] * s[k];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) f[i * 3 + j] = us[i * 3] * V[j * 3] + us[i * 3 + 1] * V[j * 3 + 1] + us[i * 3 + 2] * V[j * 3 + 2];
  }
  if (!denormalise(model, f, n0, n1, out)) return false;
  if (model == 0 && out[6] * n0.cx + out[7] * n0.cy + out[8] < 0) for (int i = 0; i < 9; ++i) out[i] = -out[i];
  return true;
}

// the matrix as it is returned: the fundamental matrix with its entry of largest magnitude (first in row-major order) positive;
// the homography keeps the sign of its solver (positive third coordinate at the data)
GEO_HD void output_sign(int model, double* m) {
  if (model == 0) return;
  int k = 0;
  for (int i = 1; i < 9; ++i) if (fabs(m[i]) > fabs(m[k])) k = i;
  if (m[k] < 0) for (int i = 0; i < 9; ++i) m[i] = -m[i];
}

}  // namespace geo
