// Batched relative pose on the GPU: loftr_estimate_pose (pose.hip, host code) for every pair of a batch, with the same
// result -- same inlier count, same inlier mask, R and t equal after the float32 rounding -- for the same seed.
//
// The host loop's random stream does not depend on the scores: iteration `it` always draws its five distinct indices from
// the same xorshift64* state sequence, and the adaptive iteration count only truncates that sequence.  So all max_iters
// minimal samples of a pair are drawn up front, solved and scored in parallel, and the sequential decision is replayed
// afterwards over the counts:
//   1. pose_prep_kernel    (thread per match)   pixels -> normalised points (fp64), m_bids checked (range, grouping);
//   2. pose_sample_kernel  (thread per pair)    pair offsets, threshold, the 1000 samples of Rng(seed) with the host's
//                                               duplicate rejection (integer arithmetic only: exact by construction);
//   3. pose_solve_kernel   (thread per sample)  Nister's five-point solver restated from pose.hip, same operations in the
//                                               same order -> up to 10 unit-norm E per sample, appended to a per-pair
//                                               work list of hypotheses;
//   4. pose_score_kernel   (thread per hypothesis, 512-match tiles of the pair in LDS) Sampson inlier counts with the
//                                               host's expression;
//   5. host replay of the RANSAC loop over the copied counts (strict `>`, the adaptive count with the host's own pow /
//      log, `best < 5` -> none): one device->host copy and one host->device copy per batch;
//   6. pose_recover_kernel (block per pair)     RANSAC mask of the best E, svd3 + sign fixes + four (R, t) candidates,
//                                               cheirality (4x4 Jacobi triangulation per inlier), first maximum wins.
// Identical decisions need identical arithmetic: fp64 everywhere, no FMA contraction (the pragma below; the x86 host path
// has no FMA), the host's operation order, IEEE division / sqrt (correctly rounded on both sides).  The host's library
// calls are reproduced: std::polar's cos / sin only depend on (degree, root index) and are tabulated on the host with the
// host's libm; complex division is compiler-rt's __divdc3 (the one the library links), restated below; std::abs of a
// complex is libstdc++'s scaled formula (HIP compilation turns off its C99 cabs path); complex multiplication is the
// inline (ac - bd, ad + bc) clang emits (its __muldc3 fallback only runs when both parts are NaN).
#include <math.h>
#include <string.h>
#include <vector>
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kIters = 1000;                 // loftr_estimate_pose: max_iters
constexpr int kSol = 10;                     // solutions per minimal sample, at most
constexpr int kHyp = kIters * kSol;          // hypothesis slots per pair
constexpr int kScoreThreads = 256;
constexpr int kScoreTile = 512;              // matches per LDS tile of the scorer (16 KiB)
constexpr int kRecoverThreads = 256;

enum : int { kBadBid = 1, kUngrouped = 2 };  // status word bits (device-side findings)

// ---- small dense linear algebra (pose.hip: jacobi_eig, mat3_mul, det3, cross3, svd3) ---------------------------------
template <int n>
__device__ void jacobi_eig(double* a, double* w, double* v) {
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

__device__ void mat3_mul(const double* a, const double* b, double* c) {
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}
__device__ double det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
__device__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ void svd3(const double* E, double* U, double* s, double* V) {
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
  double d = u[0][0] * u[1][0] + u[0][1] * u[1][1] + u[0][2] * u[1][2];
  for (int i = 0; i < 3; ++i) u[1][i] -= d * u[0][i];
  double nrm = sqrt(u[1][0] * u[1][0] + u[1][1] * u[1][1] + u[1][2] * u[1][2]);
  if (nrm < 1e-300) nrm = 1;
  for (int i = 0; i < 3; ++i) u[1][i] /= nrm;
  cross3(u[0], u[1], u[2]);
  for (int k = 0; k < 3; ++k) for (int i = 0; i < 3; ++i) U[i * 3 + k] = u[k][i];
}

// ---- polynomials in (x, y, z) up to degree 3, pose.hip's monomial order ------------------------------------------------
constexpr int kMono[20][3] = {{3,0,0},{0,3,0},{2,1,0},{1,2,0},{2,0,1},{2,0,0},{0,2,1},{0,2,0},{1,1,1},{1,1,0},
                              {1,0,2},{1,0,1},{1,0,0},{0,1,2},{0,1,1},{0,1,0},{0,0,3},{0,0,2},{0,0,1},{0,0,0}};
struct MulTable { signed char t[20][20]; };
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
__constant__ MulTable kMul = make_mul_table();
constexpr int kIx = 12, kIy = 15, kIz = 18, kI1 = 19;       // x, y, z, 1 in kMono

struct Poly { double c[20]; };
__device__ Poly pzero() { Poly r; for (int i = 0; i < 20; ++i) r.c[i] = 0.0; return r; }
__device__ Poly operator+(const Poly& a, const Poly& b) { Poly r; for (int i = 0; i < 20; ++i) r.c[i] = a.c[i] + b.c[i]; return r; }
__device__ Poly operator-(const Poly& a, const Poly& b) { Poly r; for (int i = 0; i < 20; ++i) r.c[i] = a.c[i] - b.c[i]; return r; }
__device__ Poly operator*(const Poly& a, double s) { Poly r; for (int i = 0; i < 20; ++i) r.c[i] = a.c[i] * s; return r; }
__device__ Poly operator*(const Poly& a, const Poly& b) {
  Poly r = pzero();
  for (int i = 0; i < 20; ++i) if (a.c[i] != 0)
    for (int j = 0; j < 20; ++j) { const int k = kMul.t[i][j]; if (b.c[j] != 0 && k >= 0) r.c[k] += a.c[i] * b.c[j]; }
  return r;
}

// polynomials in z (pose.hip's std::vector P1 with its sizes): ascending coefficients, at most degree 10
struct P1 { double c[11]; int n; };
__device__ P1 p1_make(int n) { P1 r; r.n = n; for (int i = 0; i < 11; ++i) r.c[i] = 0.0; return r; }
__device__ P1 p1_mul(const P1& a, const P1& b) {
  P1 r = p1_make(a.n + b.n - 1);
  for (int i = 0; i < a.n; ++i) for (int j = 0; j < b.n; ++j) r.c[i + j] += a.c[i] * b.c[j];
  return r;
}
__device__ P1 p1_sub(const P1& a, const P1& b) {
  P1 r = p1_make(a.n > b.n ? a.n : b.n);
  for (int i = 0; i < a.n; ++i) r.c[i] += a.c[i];
  for (int i = 0; i < b.n; ++i) r.c[i] -= b.c[i];
  return r;
}
__device__ P1 p1_add(const P1& a, const P1& b) {
  P1 r = p1_make(a.n > b.n ? a.n : b.n);
  for (int i = 0; i < a.n; ++i) r.c[i] += a.c[i];
  for (int i = 0; i < b.n; ++i) r.c[i] += b.c[i];
  return r;
}
__device__ double p1_eval(const P1& a, double z) { double r = 0; for (int i = a.n; i-- > 0;) r = r * z + a.c[i]; return r; }

// ---- complex arithmetic as the host library computes it -----------------------------------------------------------------
struct cd { double re, im; };
__device__ cd c_add(cd a, cd b) { return {a.re + b.re, a.im + b.im}; }
__device__ cd c_sub(cd a, cd b) { return {a.re - b.re, a.im - b.im}; }
__device__ cd c_mul(cd a, cd b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ double c_abs(cd z) {                                  // libstdc++ __complex_abs
  double x = z.re, y = z.im;
  const double ax = fabs(x), ay = fabs(y);
  const double s = ax < ay ? ay : ax;
  if (s == 0.0) return s;
  x /= s;
  y /= s;
  return s * sqrt(x * x + y * y);
}
__device__ double crt_logb(double x) {                           // compiler-rt logb: exponent of a finite non-zero x
  if (isnan(x)) return x;
  if (isinf(x)) return INFINITY;
  if (x == 0.0) return -INFINITY;
  int e;
  frexp(x, &e);
  return (double)(e - 1);
}
__device__ cd c_div(cd num, cd den) {                            // compiler-rt __divdc3
  double a = num.re, b = num.im, c = den.re, d = den.im;
  int ilogbw = 0;
  const double ac = fabs(c), ad = fabs(d);
  const double mx = isnan(c) ? ad : (isnan(d) ? ac : (ac > ad ? ac : ad));
  const double logbw = crt_logb(mx);
  if (isfinite(logbw)) {
    ilogbw = (int)logbw;
    c = ldexp(c, -ilogbw);
    d = ldexp(d, -ilogbw);
  }
  const double denom = c * c + d * d;
  cd z{ldexp((a * c + b * d) / denom, -ilogbw), ldexp((b * c - a * d) / denom, -ilogbw)};
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

// cos / sin of the Aberth start angles 2 pi i / n + 0.4, n = 1..10, computed on the host (the host estimator's libm)
struct PolarTable { double c[10][10], s[10][10]; };

// pose.hip real_roots: Aberth-Ehrlich + Newton polishing; roots appended to r[0..*nr)
__device__ void real_roots(const P1& pin, double* r, int* nr, const PolarTable& tab) {
  P1 p = pin;
  while (p.n > 1 && fabs(p.c[p.n - 1]) < 1e-14 * fabs(p.c[0] + 1e-300) && fabs(p.c[p.n - 1]) < 1e-300) --p.n;
  double scale = 0;
  for (int i = 0; i < p.n; ++i) scale = fabs(p.c[i]) > scale ? fabs(p.c[i]) : scale;
  if (scale == 0) return;
  while (p.n > 1 && fabs(p.c[p.n - 1]) < 1e-13 * scale) --p.n;
  const int n = p.n - 1;
  if (n < 1) return;
  double radius = 0;
  for (int i = 0; i < n; ++i) { const double q = fabs(p.c[i] / p.c[n]); radius = q > radius ? q : radius; }
  radius = 1 + radius;
  cd z[10];
  for (int i = 0; i < n; ++i) {
    const double rho = radius * (0.3 + 0.7 * (i + 1) / n);
    z[i] = {rho * tab.c[n - 1][i], rho * tab.s[n - 1][i]};
  }
  const cd tiny{1e-300, 0};
  for (int it = 0; it < 200; ++it) {
    double change = 0;
    for (int i = 0; i < n; ++i) {
      cd f{p.c[n], 0.0}, df{0.0, 0.0};
      for (int k = n - 1; k >= 0; --k) { df = c_add(c_mul(df, z[i]), f); f = c_mul(f, z[i]); f.re = f.re + p.c[k]; }
      if (c_abs(f) < 1e-300) continue;
      const cd ratio = c_div(f, c_abs(df) > 1e-300 ? df : tiny);
      cd sum{0.0, 0.0};
      for (int j = 0; j < n; ++j) if (j != i) { const cd d = c_sub(z[i], z[j]); sum = c_add(sum, c_div(cd{1.0, 0.0}, c_abs(d) > 1e-300 ? d : tiny)); }
      const cd rs = c_mul(ratio, sum);
      const cd step = c_div(ratio, cd{-rs.re + 1.0, -rs.im});     // 1.0 - ratio * sum: (-(ratio * sum)) += 1.0
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

// pose.hip five_point on the five correspondences idx[0..5) of q0 / q1 -> up to 10 unit-norm E (row-major) in Es
__device__ int five_point(const double* q0, const double* q1, const int* idx, double* Es, const PolarTable& tab) {
  double ata[81];
  for (int i = 0; i < 81; ++i) ata[i] = 0.0;
  for (int k = 0; k < 5; ++k) {
    const int i = idx[k];
    const double x0 = q0[2 * i], y0 = q0[2 * i + 1], x1 = q1[2 * i], y1 = q1[2 * i + 1];
    const double r[9] = {x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, 1.0};
    for (int a = 0; a < 9; ++a) for (int b = 0; b < 9; ++b) ata[a * 9 + b] += r[a] * r[b];
  }
  double w[9], v[81];
  jacobi_eig<9>(ata, w, v);
  int order[9];
  for (int i = 0; i < 9; ++i) order[i] = i;
  for (int i = 0; i < 9; ++i) for (int j = i + 1; j < 9; ++j) if (w[order[j]] < w[order[i]]) { int t = order[i]; order[i] = order[j]; order[j] = t; }
  double N[4][9];
  for (int b = 0; b < 4; ++b) for (int i = 0; i < 9; ++i) N[b][i] = v[i * 9 + order[b]];
  Poly E[9];
  for (int i = 0; i < 9; ++i) { E[i] = pzero(); E[i].c[kIx] = N[0][i]; E[i].c[kIy] = N[1][i]; E[i].c[kIz] = N[2][i]; E[i].c[kI1] = N[3][i]; }
  double M[10][20];
  {
    const Poly e0 = E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6]) + E[2] * (E[3] * E[7] - E[4] * E[6]);
    for (int c = 0; c < 20; ++c) M[0][c] = e0.c[c];
  }
  Poly EEt[9];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j)
    EEt[i * 3 + j] = E[i * 3] * E[j * 3] + E[i * 3 + 1] * E[j * 3 + 1] + E[i * 3 + 2] * E[j * 3 + 2];
  const Poly tr = EEt[0] + EEt[4] + EEt[8];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
    const Poly t = EEt[i * 3] * E[j] + EEt[i * 3 + 1] * E[3 + j] + EEt[i * 3 + 2] * E[6 + j];
    const Poly e = t * 2.0 - tr * E[i * 3 + j];
    for (int c = 0; c < 20; ++c) M[1 + i * 3 + j][c] = e.c[c];
  }
  for (int c = 0; c < 10; ++c) {
    int piv = c;
    for (int r = c + 1; r < 10; ++r) if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
    if (fabs(M[piv][c]) < 1e-14) return 0;
    if (piv != c) for (int k = 0; k < 20; ++k) { const double t = M[c][k]; M[c][k] = M[piv][k]; M[piv][k] = t; }
    const double inv = 1.0 / M[c][c];
    for (int k = 0; k < 20; ++k) M[c][k] *= inv;
    for (int r = 0; r < 10; ++r) if (r != c) {
      const double f = M[r][c];
      if (f != 0) for (int k = 0; k < 20; ++k) M[r][k] -= f * M[c][k];
    }
  }
  P1 B[3][3];
  for (int t = 0; t < 3; ++t) {
    const double* a = M[4 + 2 * t];
    const double* b = M[5 + 2 * t];
    B[t][0] = p1_make(4); B[t][0].c[0] = a[12]; B[t][0].c[1] = a[11] - b[12]; B[t][0].c[2] = a[10] - b[11]; B[t][0].c[3] = -b[10];
    B[t][1] = p1_make(4); B[t][1].c[0] = a[15]; B[t][1].c[1] = a[14] - b[15]; B[t][1].c[2] = a[13] - b[14]; B[t][1].c[3] = -b[13];
    B[t][2] = p1_make(5); B[t][2].c[0] = a[19]; B[t][2].c[1] = a[18] - b[19]; B[t][2].c[2] = a[17] - b[18]; B[t][2].c[3] = a[16] - b[17];
    B[t][2].c[4] = -b[16];
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

// pose.hip score, one correspondence
__device__ __forceinline__ bool sampson_in(const double* E, double x0, double y0, double x1, double y1, double thr2) {
  const double l0 = E[0] * x0 + E[1] * y0 + E[2], l1 = E[3] * x0 + E[4] * y0 + E[5], l2 = E[6] * x0 + E[7] * y0 + E[8];
  const double m0 = E[0] * x1 + E[3] * y1 + E[6], m1 = E[1] * x1 + E[4] * y1 + E[7];
  const double r = x1 * l0 + y1 * l1 + l2;
  const double den = l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1;
  return den > 0 && r * r < thr2 * den;
}

// pose.hip cheirality, one inlier correspondence
__device__ bool in_front(const double* R, const double* t, double x0, double y0, double x1, double y1, double dist) {
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

__device__ long lower_bound(const long* a, long n, long key) {
  long lo = 0, hi = n;
  while (lo < hi) { const long mid = lo + (hi - lo) / 2; if (a[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}

// pair p's matches [start[p], start[p] + count) (a negative difference -- only with ungrouped m_bids -- counts as none)
__device__ __forceinline__ long pair_count(const long* start, int p) { const long n = start[p + 1] - start[p]; return n > 0 ? n : 0; }

// ---- kernels ------------------------------------------------------------------------------------------------------------
// grid ceil(M / 256) x 256: normalised points q = (kpts - [cx, cy]) / [fx, fy] in fp64, m_bids checked
__global__ void pose_prep_kernel(const float* __restrict__ k0, const float* __restrict__ k1, const long* __restrict__ m_bids, long M,
                                 const float* __restrict__ K0, const float* __restrict__ K1, int P, double* __restrict__ q0,
                                 double* __restrict__ q1, int* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const long b = m_bids[i];
  if (b < 0 || b >= P) { atomicOr(status, (int)kBadBid); return; }
  if (i > 0 && m_bids[i - 1] > b) atomicOr(status, (int)kUngrouped);
  const float* A = K0 + 9 * b;
  const float* B = K1 + 9 * b;
  q0[2 * i] = ((double)k0[2 * i] - A[2]) / A[0]; q0[2 * i + 1] = ((double)k0[2 * i + 1] - A[5]) / A[4];
  q1[2 * i] = ((double)k1[2 * i] - B[2]) / B[0]; q1[2 * i + 1] = ((double)k1[2 * i + 1] - B[5]) / B[4];
}

// pose.hip Rng (xorshift64*)
struct Rng {
  uint64_t s;
  __device__ explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) { if (!s) s = 1; }
  __device__ uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
  __device__ long below(long n) { return (long)(next() % (uint64_t)n); }
};

// grid ceil((P + 1) / 64) x 64: pair offsets, squared threshold, the kIters minimal samples of every pair with >= 5 matches
__global__ void pose_sample_kernel(const long* __restrict__ m_bids, long M, int P, const float* __restrict__ K0,
                                   const float* __restrict__ K1, float thresh_px, unsigned seed, long* __restrict__ start,
                                   double* __restrict__ thr2, int* __restrict__ idx, int* __restrict__ n_hyp) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > P) return;
  const long s0 = lower_bound(m_bids, M, p);
  start[p] = s0;
  if (p == P) return;
  n_hyp[p] = 0;
  const float* A = K0 + 9 * (long)p;
  const float* B = K1 + 9 * (long)p;
  const double thr = (double)thresh_px / (((double)A[0] + B[4] + A[0] + B[4]) / 4.0);
  thr2[p] = thr * thr;
  const long n = lower_bound(m_bids, M, p + 1) - s0;
  if (n < 5) return;
  Rng rng(seed);
  int* out = idx + (long)p * kIters * 5;
  for (int it = 0; it < kIters; ++it) {
    int d[5];
    for (int k = 0; k < 5;) {
      const int c = (int)rng.below(n);
      bool dup = false;
      for (int j = 0; j < k; ++j) dup = dup || d[j] == c;
      if (!dup) d[k++] = c;
    }
    for (int k = 0; k < 5; ++k) out[it * 5 + k] = d[k];
  }
}

// grid ceil(P * kIters / 64) x 64: one minimal sample per thread -> Es [P, kHyp, 9], counts [P, kHyp] = -1 (filled by the
// scorer for the solutions), hypothesis work list hyp [P, kHyp] of slot ids it * kSol + s (any order), n_hyp [P]
__global__ void __launch_bounds__(64) pose_solve_kernel(const double* __restrict__ q0, const double* __restrict__ q1,
                                                        const long* __restrict__ start, const int* __restrict__ idx, int P,
                                                        PolarTable tab, double* __restrict__ Es, int* __restrict__ counts,
                                                        int* __restrict__ hyp, int* __restrict__ n_hyp, const int* __restrict__ status) {
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long)P * kIters || *status) return;
  const int p = (int)(g / kIters), it = (int)(g % kIters);
  int* cnt = counts + (long)p * kHyp + it * kSol;
  for (int s = 0; s < kSol; ++s) cnt[s] = -1;
  if (pair_count(start, p) < 5) return;
  const long s0 = start[p];
  int d[5];
  for (int k = 0; k < 5; ++k) d[k] = idx[g * 5 + k];
  double* e = Es + ((long)p * kHyp + it * kSol) * 9;
  const int ns = five_point(q0 + 2 * s0, q1 + 2 * s0, d, e, tab);
  if (ns == 0) return;
  const int base = atomicAdd(n_hyp + p, ns);
  for (int s = 0; s < ns; ++s) hyp[(long)p * kHyp + base + s] = it * kSol + s;
}

// grid (P, kHyp / 256 rounded up) x 256: thread = hypothesis of the pair's work list; the pair's matches stream through LDS
__global__ void __launch_bounds__(kScoreThreads) pose_score_kernel(const double* __restrict__ q0, const double* __restrict__ q1,
                                                                  const long* __restrict__ start, const double* __restrict__ thr2,
                                                                  const double* __restrict__ Es, const int* __restrict__ hyp,
                                                                  const int* __restrict__ n_hyp, int* __restrict__ counts,
                                                                  const int* __restrict__ status) {
  __shared__ double pts[kScoreTile][4];
  const int p = blockIdx.x;
  const int nh = n_hyp[p];
  const int h = blockIdx.y * kScoreThreads + threadIdx.x;
  if (*status || (int)blockIdx.y * kScoreThreads >= nh) return;           // (uniform over the block)
  const bool valid = h < nh;
  const int slot = valid ? hyp[(long)p * kHyp + h] : 0;
  double E[9];
  for (int i = 0; i < 9; ++i) E[i] = valid ? Es[((long)p * kHyp + slot) * 9 + i] : 0.0;
  const long s0 = start[p], n = pair_count(start, p);
  const double t2 = thr2[p];
  int cnt = 0;
  for (long b = 0; b < n; b += kScoreTile) {
    const int m = (int)(n - b < kScoreTile ? n - b : kScoreTile);
    __syncthreads();
    for (int j = threadIdx.x; j < m; j += kScoreThreads) {
      const long i = s0 + b + j;
      pts[j][0] = q0[2 * i]; pts[j][1] = q0[2 * i + 1]; pts[j][2] = q1[2 * i]; pts[j][3] = q1[2 * i + 1];
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) cnt += sampson_in(E, pts[j][0], pts[j][1], pts[j][2], pts[j][3], t2);
  }
  if (valid) counts[(long)p * kHyp + slot] = cnt;
}

// grid P x 256: the RANSAC mask of the selected hypothesis, the four (R, t) of its E and the cheirality vote.  Outputs of a
// pair without a pose (best[p] < 0, or no point in front of both cameras): n_inliers = -1, R = t = 0, mask 0.
__global__ void __launch_bounds__(kRecoverThreads) pose_recover_kernel(const double* __restrict__ q0, const double* __restrict__ q1,
                                                                      const long* __restrict__ start, const double* __restrict__ thr2,
                                                                      const double* __restrict__ Es, const int* __restrict__ best,
                                                                      uint8_t* __restrict__ bits, float* __restrict__ R_out,
                                                                      float* __restrict__ t_out, uint8_t* __restrict__ mask,
                                                                      long* __restrict__ n_inliers) {
  __shared__ double sR[4][9], st[4][3], sE[9];
  __shared__ int votes[4], pick[2];
  const int p = blockIdx.x, tid = threadIdx.x;
  const long s0 = start[p], n = pair_count(start, p);
  const int b = best[p];
  if (tid < 4) votes[tid] = 0;
  if (b >= 0 && tid < 9) sE[tid] = Es[((long)p * kHyp + b) * 9 + tid];
  __syncthreads();
  if (b >= 0 && tid == 0) {
    // E = U diag(1,1,0) V^T -> R in {U W V^T, U W^T V^T}, t = +-u3 (pose.hip, same order)
    double U[9], s[3], V[9];
    svd3(sE, U, s, V);
    if (det3(U) < 0) for (int i = 0; i < 9; ++i) U[i] = -U[i];
    if (det3(V) < 0) for (int i = 0; i < 9; ++i) V[i] = -V[i];
    const double Wm[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, Wt[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
    double Vt[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Vt[i * 3 + j] = V[j * 3 + i];
    double R1[9], R2[9], tmp[9];
    mat3_mul(U, Wm, tmp); mat3_mul(tmp, Vt, R1);
    mat3_mul(U, Wt, tmp); mat3_mul(tmp, Vt, R2);
    for (int i = 0; i < 9; ++i) { sR[0][i] = R1[i]; sR[1][i] = R2[i]; sR[2][i] = R1[i]; sR[3][i] = R2[i]; }
    for (int i = 0; i < 3; ++i) { st[0][i] = st[1][i] = U[2 + 3 * i]; st[2][i] = st[3][i] = -U[2 + 3 * i]; }
  }
  __syncthreads();
  if (b >= 0) {
    const double t2 = thr2[p];
    int v[4] = {0, 0, 0, 0};
    for (long j = tid; j < n; j += kRecoverThreads) {
      const long i = s0 + j;
      const double x0 = q0[2 * i], y0 = q0[2 * i + 1], x1 = q1[2 * i], y1 = q1[2 * i + 1];
      unsigned f = 0;
      if (sampson_in(sE, x0, y0, x1, y1, t2))
        for (int c = 0; c < 4; ++c) if (in_front(sR[c], st[c], x0, y0, x1, y1, 1e9)) { f |= 1u << c; ++v[c]; }
      bits[i] = (uint8_t)f;
    }
    for (int c = 0; c < 4; ++c) if (v[c]) atomicAdd(&votes[c], v[c]);
  }
  __syncthreads();
  if (tid == 0) {
    long bestc = -1;
    int bi = 0;
    if (b >= 0) for (int c = 0; c < 4; ++c) if (votes[c] > bestc) { bestc = votes[c]; bi = c; }
    pick[0] = bestc > 0 ? bi : -1;
    n_inliers[p] = bestc > 0 ? bestc : -1;
    for (int i = 0; i < 9; ++i) R_out[9 * (long)p + i] = bestc > 0 ? (float)sR[bi][i] : 0.f;
    for (int i = 0; i < 3; ++i) t_out[3 * (long)p + i] = bestc > 0 ? (float)st[bi][i] : 0.f;
  }
  __syncthreads();
  const int bi = pick[0];
  for (long j = tid; j < n; j += kRecoverThreads) mask[s0 + j] = bi >= 0 ? (bits[s0 + j] >> bi) & 1 : 0;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
PolarTable polar_table() {
  PolarTable t;
  memset(&t, 0, sizeof(t));
  for (int n = 1; n <= 10; ++n)
    for (int i = 0; i < n; ++i) {
      const double theta = 2 * M_PI * i / n + 0.4;                // pose.hip real_roots: std::polar(rho, theta)
      t.c[n - 1][i] = cos(theta);
      t.s[n - 1][i] = sin(theta);
    }
  return t;
}

// workspace layout (byte offsets, 256-aligned)
struct Layout { size_t status, start, counts, q0, q1, thr2, idx, Es, hyp, n_hyp, best, bits, total; };
Layout layout(long M, int P) {
  Layout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
  // status, start and counts are contiguous: the one device -> host copy of the replay
  L.status = take(8);
  L.start = L.status + 8;
  o = align_up(L.start + sizeof(long) * (P + 1), 8);
  L.counts = o;
  o = align_up(o + sizeof(int) * (size_t)P * kHyp, 256);
  L.q0 = take(sizeof(double) * 2 * M);
  L.q1 = take(sizeof(double) * 2 * M);
  L.thr2 = take(sizeof(double) * P);
  L.idx = take(sizeof(int) * 5 * (size_t)P * kIters);
  L.Es = take(sizeof(double) * 9 * (size_t)P * kHyp);
  L.hyp = take(sizeof(int) * (size_t)P * kHyp);
  L.n_hyp = take(sizeof(int) * P);
  L.best = take(sizeof(int) * P);
  L.bits = take(M);
  L.total = o;
  return L;
}

}  // namespace

extern "C" size_t loftr_estimate_pose_batched_workspace_bytes(long M, int P) {
  if (M < 0 || P < 0) return 0;
  return layout(M, P).total;
}

extern "C" int loftr_estimate_pose_batched(const float* mkpts0_f, const float* mkpts1_f, const long* m_bids, long M,
                                           const float* K0, const float* K1, int P, float thresh_px, float conf, unsigned seed,
                                           float* R_out, float* t_out, uint8_t* inliers_out, long* n_inliers, void* ws,
                                           size_t ws_bytes, void* stream) {
  LOFTR_CHECK_ARG(M >= 0 && P >= 0);
  if (P == 0) return M == 0 ? LOFTR_OK : LOFTR_ERR_BAD_ARG;             // every pair id would be out of range
  LOFTR_CHECK_ARG(K0 && K1 && R_out && t_out && n_inliers && ws);
  LOFTR_CHECK_ARG(M == 0 || (mkpts0_f && mkpts1_f && m_bids && inliers_out));
  if ((M + 255) / 256 >= (1L << 31) || M >= (1L << 31) || (long)P * kIters >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  const Layout L = layout(M, P);
  if (ws_bytes < L.total) return LOFTR_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  int* status = (int*)(w + L.status);
  long* start = (long*)(w + L.start);
  int* counts = (int*)(w + L.counts);
  double *q0 = (double*)(w + L.q0), *q1 = (double*)(w + L.q1), *thr2 = (double*)(w + L.thr2), *Es = (double*)(w + L.Es);
  int *idx = (int*)(w + L.idx), *hyp = (int*)(w + L.hyp), *n_hyp = (int*)(w + L.n_hyp), *best = (int*)(w + L.best);
  uint8_t* bits = (uint8_t*)(w + L.bits);
  if (hipMemsetAsync(status, 0, sizeof(int), s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  if (M > 0) {
    hipLaunchKernelGGL(pose_prep_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, mkpts0_f, mkpts1_f, m_bids, M, K0, K1, P,
                       q0, q1, status);
    LOFTR_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(pose_sample_kernel, dim3((unsigned)((P + 1 + 63) / 64)), dim3(64), 0, s, m_bids, M, P, K0, K1, thresh_px, seed,
                     start, thr2, idx, n_hyp);
  LOFTR_CHECK_LAUNCH();
  static const PolarTable tab = polar_table();
  hipLaunchKernelGGL(pose_solve_kernel, dim3((unsigned)(((long)P * kIters + 63) / 64)), dim3(64), 0, s, q0, q1, start, idx, P, tab, Es,
                     counts, hyp, n_hyp, status);
  LOFTR_CHECK_LAUNCH();
  hipLaunchKernelGGL(pose_score_kernel, dim3((unsigned)P, (unsigned)((kHyp + kScoreThreads - 1) / kScoreThreads)), dim3(kScoreThreads), 0,
                     s, q0, q1, start, thr2, Es, hyp, n_hyp, counts, status);
  LOFTR_CHECK_LAUNCH();
  // ---- replay of the host loop (pose.hip loftr_estimate_pose) over the counts: one copy down, one copy up ----
  const size_t down = L.counts + sizeof(int) * (size_t)P * kHyp - L.status;
  std::vector<char> host(down);
  if (hipMemcpyAsync(host.data(), w + L.status, down, hipMemcpyDeviceToHost, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  if (hipStreamSynchronize(s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  int st;
  memcpy(&st, host.data(), sizeof(int));
  if (st) return LOFTR_ERR_BAD_ARG;                                     // m_bids out of [0, P) or not grouped by ascending pair
  const long* h_start = (const long*)(host.data() + (L.start - L.status));
  const int* h_counts = (const int*)(host.data() + (L.counts - L.status));
  std::vector<int> h_best(P);
  for (int p = 0; p < P; ++p) {
    const long Mp = h_start[p + 1] - h_start[p];
    h_best[p] = -1;
    if (Mp < 5) continue;
    const int* c = h_counts + (size_t)p * kHyp;
    long bestn = 0;
    int max_iters = kIters, iters = max_iters;
    for (int it = 0; it < iters; ++it) {
      for (int sol = 0; sol < kSol && c[it * kSol + sol] >= 0; ++sol) {
        const long cnt = c[it * kSol + sol];
        if (cnt > bestn) {
          bestn = cnt;
          h_best[p] = it * kSol + sol;
          const double wr = (double)cnt / (double)Mp;
          const double p_all = pow(wr, 5.0);
          if (p_all > 1 - 1e-12) iters = it + 1;
          else if (p_all > 1e-12) {
            const double need = log(1.0 - (double)conf) / log(1.0 - p_all);
            if (need < iters) iters = need < it + 1 ? it + 1 : (int)ceil(need);
          }
        }
      }
    }
    if (bestn < 5) h_best[p] = -1;
  }
  if (hipMemcpyAsync(best, h_best.data(), sizeof(int) * P, hipMemcpyHostToDevice, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  hipLaunchKernelGGL(pose_recover_kernel, dim3((unsigned)P), dim3(kRecoverThreads), 0, s, q0, q1, start, thr2, Es, best, bits, R_out, t_out,
                     inliers_out, n_inliers);
  LOFTR_CHECK_LAUNCH();
  // h_best is pageable host memory that goes out of scope on return: wait for the stream rather than rely on the copy staging it
  if (hipStreamSynchronize(s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  return LOFTR_OK;
}
