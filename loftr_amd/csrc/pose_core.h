// Five-point relative pose: the arithmetic shared by the host estimator (pose.hip) and the batched GPU estimator (pose_gpu.hip).  As in
// geometry_core.h, every function here is compiled for both sides from this one text, fp64, without FMA contraction, so that the two
// sides take identical decisions (ransac_core.h says what that rests on).
//   * D. Nister, "An efficient solution to the five-point relative pose problem", PAMI 2004: the 4-dimensional null space of the
//     epipolar constraints, the ten cubic constraints (det E = 0, 2 E E^T E - tr(E E^T) E = 0) eliminated by Gauss-Jordan to a 3x3
//     polynomial matrix in z whose determinant is a tenth-degree polynomial; its real roots by Aberth-Ehrlich + Newton polishing;
//   * the squared Sampson distance against the squared threshold;
//   * the four (R, t) decompositions of E and the triangulation (4x4 Jacobi) that tells which one has a point in front of both cameras.
#pragma once
#include "ransac_core.h"

#pragma clang fp contract(off)

#define POSE_HD __host__ __device__ inline

namespace pose {

using namespace ransac;

constexpr int kSample = 5;
constexpr int kSol = 10;                     // solutions per minimal sample, at most
using PolarTable = ransac::PolarAngles<10>;

// ---- polynomials in (x, y, z) up to degree 3, in the column order of the elimination ---------------------------------------------
// x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
constexpr int kMono[20][3] = {{3,0,0},{0,3,0},{2,1,0},{1,2,0},{2,0,1},{2,0,0},{0,2,1},{0,2,0},{1,1,1},{1,1,0},
                              {1,0,2},{1,0,1},{1,0,0},{0,1,2},{0,1,1},{0,1,0},{0,0,3},{0,0,2},{0,0,1},{0,0,0}};
struct MulTable { signed char t[20][20]; };  // index of the product of two monomials, -1 above degree 3
constexpr MulTable make_mul_table() {
  MulTable m{};
  for (int i = 0; i < 20; ++i) for (int j = 0; j < 20; ++j) {
    const int x = kMono[i][0] + kMono[j][0], y = kMono[i][1] + kMono[j][1], z = kMono[i][2] + kMono[j][2];
    int k = -1;
    if (x + y + z <= 3) for (int c = 0; c < 20; ++c) if (kMono[c][0] == x && kMono[c][1] == y && kMono[c][2] == z) k = c;
    m.t[i][j] = (signed char)k;
  }
  return m;
}
constexpr MulTable kMul = make_mul_table();                 // (at namespace scope: constant memory on the device, folded where the loops unroll)
constexpr int kIx = 12, kIy = 15, kIz = 18, kI1 = 19;       // x, y, z, 1 in kMono

struct Poly { double c[20]; };
POSE_HD Poly pzero() { Poly r; for (int i = 0; i < 20; ++i) r.c[i] = 0.0; return r; }
POSE_HD Poly operator+(const Poly& a, const Poly& b) { Poly r; for (int i = 0; i < 20; ++i) r.c[i] = a.c[i] + b.c[i]; return r; }
POSE_HD Poly operator-(const Poly& a, const Poly& b) { Poly r; for (int i = 0; i < 20; ++i) r.c[i] = a.c[i] - b.c[i]; return r; }
POSE_HD Poly operator*(const Poly& a, double s) { Poly r; for (int i = 0; i < 20; ++i) r.c[i] = a.c[i] * s; return r; }
POSE_HD Poly operator*(const Poly& a, const Poly& b) {      // the product must stay within degree 3 (callers guarantee it)
  Poly r = pzero();
  for (int i = 0; i < 20; ++i) if (a.c[i] != 0)
    for (int j = 0; j < 20; ++j) { const int k = kMul.t[i][j]; if (b.c[j] != 0 && k >= 0) r.c[k] += a.c[i] * b.c[j]; }
  return r;
}

// polynomials in z: n ascending coefficients, at most degree 10
struct P1 { double c[11]; int n; };
POSE_HD P1 p1_make(int n) { P1 r; r.n = n; for (int i = 0; i < 11; ++i) r.c[i] = 0.0; return r; }
POSE_HD P1 p1_mul(const P1& a, const P1& b) {
  P1 r = p1_make(a.n + b.n - 1);
  for (int i = 0; i < a.n; ++i) for (int j = 0; j < b.n; ++j) r.c[i + j] += a.c[i] * b.c[j];
  return r;
}
POSE_HD P1 p1_sub(const P1& a, const P1& b) {
  P1 r = p1_make(a.n > b.n ? a.n : b.n);
  for (int i = 0; i < a.n; ++i) r.c[i] += a.c[i];
  for (int i = 0; i < b.n; ++i) r.c[i] -= b.c[i];
  return r;
}
POSE_HD P1 p1_add(const P1& a, const P1& b) {
  P1 r = p1_make(a.n > b.n ? a.n : b.n);
  for (int i = 0; i < a.n; ++i) r.c[i] += a.c[i];
  for (int i = 0; i < b.n; ++i) r.c[i] += b.c[i];
  return r;
}
POSE_HD double p1_eval(const P1& a, double z) { double r = 0; for (int i = a.n; i-- > 0;) r = r * z + a.c[i]; return r; }

// real roots of a polynomial of degree <= 10 by Aberth-Ehrlich iteration + Newton polishing on the real axis; the distinct ones are
// appended to r[0..*nr).  (geometry_core.h's real_roots3 and absolute_pose_core.h's real_roots4 are this routine at a fixed degree,
// kept apart for their register-resident arrays.)
POSE_HD void real_roots(const P1& pin, double* r, int* nr, const PolarTable& tab) {
  P1 p = pin;
  while (p.n > 1 && fabs(p.c[p.n - 1]) < 1e-14 * fabs(p.c[0] + 1e-300) && fabs(p.c[p.n - 1]) < 1e-300) --p.n;
  double scale = 0;
  for (int i = 0; i < p.n; ++i) scale = fabs(p.c[i]) > scale ? fabs(p.c[i]) : scale;
  if (scale == 0) return;
  while (p.n > 1 && fabs(p.c[p.n - 1]) < 1e-13 * scale) --p.n;                 // numerically lower degree
  const int n = p.n - 1;
  if (n < 1) return;
  double radius = 0;
  for (int i = 0; i < n; ++i) { const double q = fabs(p.c[i] / p.c[n]); radius = q > radius ? q : radius; }
  radius = 1 + radius;                                                         // Cauchy bound
  cd z[10];
  for (int i = 0; i < n; ++i) {
    const double rho = radius * (0.3 + 0.7 * (i + 1) / n);
    z[i] = {rho * tab.c[n - 1][i], rho * tab.s[n - 1][i]};
  }
  const cd tiny{1e-300, 0}, one{1.0, 0.0};
  for (int it = 0; it < 200; ++it) {
    double change = 0;
    for (int i = 0; i < n; ++i) {
      cd f{p.c[n], 0.0}, df{0.0, 0.0};
      for (int k = n - 1; k >= 0; --k) { df = c_add(c_mul(df, z[i]), f); f = c_mul(f, z[i]); f.re = f.re + p.c[k]; }
      if (c_abs(f) < 1e-300) continue;
      const cd ratio = c_div(f, c_abs(df) > 1e-300 ? df : tiny);
      cd sum{0.0, 0.0};
      for (int j = 0; j < n; ++j) if (j != i) { const cd d = c_sub(z[i], z[j]); sum = c_add(sum, c_div(one, c_abs(d) > 1e-300 ? d : tiny)); }
      const cd rs = c_mul(ratio, sum);
      const cd step = c_div(ratio, cd{-rs.re + 1.0, -rs.im});     // 1.0 - ratio * sum as std::complex forms it: (-(ratio * sum)) += 1.0
      z[i] = c_sub(z[i], step);
      const double as = c_abs(step);
      change = as > change ? as : change;
    }
    if (change < 1e-14 * radius) break;
  }
  for (int i = 0; i < n; ++i) {
    if (fabs(z[i].im) > 1e-6 * (1 + fabs(z[i].re))) continue;
    double x = z[i].re;
    for (int it = 0; it < 8; ++it) {                                            // polish
      double f = p.c[n], df = 0;
      for (int k = n - 1; k >= 0; --k) { df = df * x + f; f = f * x + p.c[k]; }
      if (fabs(df) < 1e-300) break;
      x -= f / df;
    }
    bool dup = false;
    for (int k = 0; k < *nr; ++k) if (fabs(r[k] - x) < 1e-9 * (1 + fabs(x))) dup = true;
    if (!dup) r[(*nr)++] = x;
  }
}

// ---- five-point solver: n >= 5 normalised correspondences -> up to 10 unit-norm essential matrices (row-major) in Es [10, 9] ------
// Correspondence k is point idx[k] (k itself without idx) of q0 / q1, whose points are `stride` doubles apart.
POSE_HD int five_point(const double* q0, const double* q1, int stride, const int* idx, int n, double* Es, const PolarTable& tab) {
  // epipolar constraints q1^T E q0 = 0  ->  A e = 0,  e = row-major E
  double ata[81];
  for (int i = 0; i < 81; ++i) ata[i] = 0.0;
  for (int k = 0; k < n; ++k) {
    const long i = (long)stride * (idx ? idx[k] : k);
    const double x0 = q0[i], y0 = q0[i + 1], x1 = q1[i], y1 = q1[i + 1];
    const double r[9] = {x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, 1.0};
    for (int a = 0; a < 9; ++a) for (int b = 0; b < 9; ++b) ata[a * 9 + b] += r[a] * r[b];
  }
  double w[9], v[81];
  jacobi_eig<9>(ata, w, v);
  int order[9];
  for (int i = 0; i < 9; ++i) order[i] = i;
  for (int i = 0; i < 9; ++i) for (int j = i + 1; j < 9; ++j) if (w[order[j]] < w[order[i]]) { int t = order[i]; order[i] = order[j]; order[j] = t; }
  double N[4][9];                                           // null-space basis X, Y, Z, W
  for (int b = 0; b < 4; ++b) for (int i = 0; i < 9; ++i) N[b][i] = v[i * 9 + order[b]];
  // E(x, y, z) = x X + y Y + z Z + W as polynomials
  Poly E[9];
  for (int i = 0; i < 9; ++i) { E[i] = pzero(); E[i].c[kIx] = N[0][i]; E[i].c[kIy] = N[1][i]; E[i].c[kIz] = N[2][i]; E[i].c[kI1] = N[3][i]; }
  double M[10][20];
  {                                                         // det E = 0
    const Poly e0 = E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6]) + E[2] * (E[3] * E[7] - E[4] * E[6]);
    for (int c = 0; c < 20; ++c) M[0][c] = e0.c[c];
  }
  // 2 E E^T E - tr(E E^T) E = 0
  Poly EEt[9];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j)
    EEt[i * 3 + j] = E[i * 3] * E[j * 3] + E[i * 3 + 1] * E[j * 3 + 1] + E[i * 3 + 2] * E[j * 3 + 2];
  const Poly tr = EEt[0] + EEt[4] + EEt[8];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
    const Poly t = EEt[i * 3] * E[j] + EEt[i * 3 + 1] * E[3 + j] + EEt[i * 3 + 2] * E[6 + j];
    const Poly e = t * 2.0 - tr * E[i * 3 + j];
    for (int c = 0; c < 20; ++c) M[1 + i * 3 + j][c] = e.c[c];
  }
  // Gauss-Jordan on the first ten columns (partial pivoting)
  for (int c = 0; c < 10; ++c) {
    int piv = c;
    for (int r = c + 1; r < 10; ++r) if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
    if (fabs(M[piv][c]) < 1e-14) return 0;                   // degenerate sample
    if (piv != c) for (int k = 0; k < 20; ++k) { const double t = M[c][k]; M[c][k] = M[piv][k]; M[piv][k] = t; }
    const double inv = 1.0 / M[c][c];
    for (int k = 0; k < 20; ++k) M[c][k] *= inv;
    for (int r = 0; r < 10; ++r) if (r != c) {
      const double f = M[r][c];
      if (f != 0) for (int k = 0; k < 20; ++k) M[r][k] -= f * M[c][k];
    }
  }
  // rows e..j (4..9): <x^2z>, <x^2>, <y^2z>, <y^2>, <xyz>, <xy>;  k = e - z f, l = g - z h, m = i - z j are
  // x * p3(z) + y * q3(z) + r4(z): the 3x3 polynomial matrix B(z)
  P1 B[3][3];
  for (int t = 0; t < 3; ++t) {
    const double* a = M[4 + 2 * t];                         // the row that carries the extra z
    const double* b = M[5 + 2 * t];
    B[t][0] = p1_make(4); B[t][0].c[0] = a[12]; B[t][0].c[1] = a[11] - b[12]; B[t][0].c[2] = a[10] - b[11]; B[t][0].c[3] = -b[10];   // x: 1, z, z^2, z^3
    B[t][1] = p1_make(4); B[t][1].c[0] = a[15]; B[t][1].c[1] = a[14] - b[15]; B[t][1].c[2] = a[13] - b[14]; B[t][1].c[3] = -b[13];   // y
    B[t][2] = p1_make(5); B[t][2].c[0] = a[19]; B[t][2].c[1] = a[18] - b[19]; B[t][2].c[2] = a[17] - b[18]; B[t][2].c[3] = a[16] - b[17];
    B[t][2].c[4] = -b[16];                                                                                                         // 1: up to z^4
  }
  const P1 det = p1_add(p1_sub(p1_mul(B[0][0], p1_sub(p1_mul(B[1][1], B[2][2]), p1_mul(B[1][2], B[2][1]))),
                               p1_mul(B[0][1], p1_sub(p1_mul(B[1][0], B[2][2]), p1_mul(B[1][2], B[2][0])))),
                        p1_mul(B[0][2], p1_sub(p1_mul(B[1][0], B[2][1]), p1_mul(B[1][1], B[2][0]))));
  double zs[10];
  int nz = 0;
  real_roots(det, zs, &nz, tab);
  int ns = 0;
  for (int iz = 0; iz < nz; ++iz) {
    const double z = zs[iz];
    if (ns >= kSol) break;
    double b[3][3];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) b[r][c] = p1_eval(B[r][c], z);
    // (x, y, 1) spans the null space of B(z): cross product of the two best-conditioned rows
    double best[3] = {0, 0, 0}, bestn = -1;
    for (int r0 = 0; r0 < 3; ++r0) for (int r1 = r0 + 1; r1 < 3; ++r1) {
      double c[3];
      cross3(b[r0], b[r1], c);
      const double nn = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
      if (nn > bestn && fabs(c[2]) > 1e-12 * sqrt(nn + 1e-300)) { bestn = nn; best[0] = c[0]; best[1] = c[1]; best[2] = c[2]; }
    }
    if (bestn <= 0) continue;
    const double x = best[0] / best[2], y = best[1] / best[2];
    double* e = Es + ns * 9;
    double nrm = 0;
    for (int i = 0; i < 9; ++i) { e[i] = x * N[0][i] + y * N[1][i] + z * N[2][i] + N[3][i]; nrm += e[i] * e[i]; }
    nrm = sqrt(nrm);
    if (!(nrm > 1e-300)) continue;
    for (int i = 0; i < 9; ++i) e[i] /= nrm;
    ++ns;
  }
  return ns;
}

// ransac_thr = thresh / mean([K0[0,0], K1[1,1], K0[0,0], K1[1,1]]) of the reference's estimate_pose, squared
POSE_HD double sampson_thr2(float thresh_px, const float* K0, const float* K1) {
  const double thr = (double)thresh_px / (((double)K0[0] + K1[4] + K0[0] + K1[4]) / 4.0);
  return thr * thr;
}
// is the squared Sampson distance of the correspondence below thr2?
POSE_HD bool sampson_in(const double* E, double x0, double y0, double x1, double y1, double thr2) {
  const double l0 = E[0] * x0 + E[1] * y0 + E[2], l1 = E[3] * x0 + E[4] * y0 + E[5], l2 = E[6] * x0 + E[7] * y0 + E[8];   // E q0
  const double m0 = E[0] * x1 + E[3] * y1 + E[6], m1 = E[1] * x1 + E[4] * y1 + E[7];                                     // E^T q1
  const double r = x1 * l0 + y1 * l1 + l2;
  const double den = l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1;
  return den > 0 && r * r < thr2 * den;
}

// E = U diag(1,1,0) V^T -> the four candidates R in {U W V^T, U W^T V^T}, t = +-u3, in the order (R1, +), (R2, +), (R1, -), (R2, -)
POSE_HD void pose_candidates(const double* E, double (*R)[9], double (*t)[3]) {
  double U[9], s[3], V[9];
  svd3(E, U, s, V);
  if (det3_rows(U, U + 3, U + 6) < 0) for (int i = 0; i < 9; ++i) U[i] = -U[i];
  if (det3_rows(V, V + 3, V + 6) < 0) for (int i = 0; i < 9; ++i) V[i] = -V[i];
  const double Wm[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, Wt[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
  double Vt[9];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Vt[i * 3 + j] = V[j * 3 + i];
  double R1[9], R2[9], tmp[9];
  mat3_mul(U, Wm, tmp); mat3_mul(tmp, Vt, R1);
  mat3_mul(U, Wt, tmp); mat3_mul(tmp, Vt, R2);
  for (int i = 0; i < 9; ++i) { R[0][i] = R1[i]; R[1][i] = R2[i]; R[2][i] = R1[i]; R[3][i] = R2[i]; }
  for (int i = 0; i < 3; ++i) { t[0][i] = t[1][i] = U[2 + 3 * i]; t[2][i] = t[3][i] = -U[2 + 3 * i]; }
}

// cheirality of one correspondence: P0 = [I | 0], P1 = [R | t]; linear triangulation A X = 0 with the four rows below, X the eigenvector
// of the smallest eigenvalue of A^T A; in front of both cameras and nearer than dist?
POSE_HD bool in_front(const double* R, const double* t, double x0, double y0, double x1, double y1, double dist) {
  double A[4][4] = {{-1, 0, x0, 0}, {0, -1, y0, 0},
                    {x1 * R[6] - R[0], x1 * R[7] - R[1], x1 * R[8] - R[2], x1 * t[2] - t[0]},
                    {y1 * R[6] - R[3], y1 * R[7] - R[4], y1 * R[8] - R[5], y1 * t[2] - t[1]}};
  double ata[16], w[4], v[16];
  for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) { double s = 0; for (int k = 0; k < 4; ++k) s += A[k][a] * A[k][b]; ata[a * 4 + b] = s; }
  jacobi_eig<4>(ata, w, v);
  int m = 0;
  for (int k = 1; k < 4; ++k) if (w[k] < w[m]) m = k;
  double X[4] = {v[m], v[4 + m], v[8 + m], v[12 + m]};
  if (fabs(X[3]) < 1e-300) return false;
  for (int k = 0; k < 3; ++k) X[k] /= X[3];
  const double z0 = X[2];
  const double z1 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
  return z0 > 0 && z0 < dist && z1 > 0 && z1 < dist;
}

}  // namespace pose
