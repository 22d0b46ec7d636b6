// 3D similarity (dst = s R src + t; rigid with s == 1) between two point sets: the arithmetic shared by the host estimator
// (similarity.hip), its batched GPU form (similarity_gpu.hip) and the routine that moves a model (loftr_transform_model*).  As in
// absolute_pose_core.h, every function here is compiled for both sides from this one text, fp64, without FMA contraction, so that
// the two sides take identical decisions and return identical bits: IEEE + - * / and sqrt are correctly rounded on both.  No libm
// function is evaluated on the shared path.  The sampler, the summation tree and svd3 are ransac_core.h's.
//
// One closed form (Kabsch / Umeyama, "Least-squares estimation of transformation parameters between two point patterns", PAMI 1991)
// serves the minimal sample and the refit: with the centroids mu_s, mu_d, the cross-covariance H = sum (dst_i - mu_d)(src_i - mu_s)^T
// and q = sum |src_i - mu_s|^2,
//     H = U diag(sigma) V^T,  R = U diag(1, 1, d) V^T,  s = tr(R^T H) / q,  t = mu_d - s R mu_s.
// ransac::svd3 returns factors that are proper or improper: V comes from a Jacobi eigen-decomposition and may have either
// determinant; the first two columns of U are H v_k normalised and its third column is their cross product.  d = +1 when
// det(U) det(V) > 0 and -1 otherwise turns U diag(1, 1, d) V^T into the proper rotation that maximises tr(R^T H).  Because U's third
// column is a cross product, svd3's sigma_2 carries no sign of its own (H = U diag(sigma_0, sigma_1, +-sigma_2) V^T), and on a
// rank-2 H it is the square root of a rounding error; so the trace sigma_0 + sigma_1 +- sigma_2 of Umeyama's scale is evaluated as
// the sum of the nine products R_ij H_ij, which is that number without the sign question and without the square root.
// Three points are always coplanar, so the H of a minimal sample has rank <= 2: its two leading singular pairs fix how the source
// plane maps onto the destination plane, svd3's cross-product column supplies a unit normal, and the d rule picks, of the two
// orthogonal maps that agree on the plane, the one that is a rotation and not a reflection.  That rotation is unique whenever the
// triple is not collinear (sigma_1 > 0), which the degeneracy rule guarantees.
#pragma once
#include "ransac_core.h"

#pragma clang fp contract(off)

#define SIM_HD __host__ __device__ inline

namespace simt {

using namespace ransac;

constexpr int kSample = 3;
constexpr int kSol = 1;                    // one model per minimal sample
constexpr int kModel = 13;                 // doubles per model: s, R (9, row-major), t (3)
constexpr int kPt = 6;                     // doubles per correspondence: src (3), dst (3)
constexpr int kSums1 = 6;                  // refit pass 1: sum src, sum dst
constexpr int kSums2 = 10;                 // refit pass 2: the 9 entries of H about the centroids, sum |src - mu_s|^2
// Degenerate samples (relative, scale-free; shared by host and device), for the source triple and for the destination triple:
//   |(P2 - P1) x (P3 - P1)|^2 <= kCollinear^2 * (longest squared side)^2 -- absolute_pose_core.h's rule.
constexpr double kCollinear = 1e-6;

SIM_HD double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SIM_HD void sub3(const double* a, const double* b, double* c) { c[0] = a[0] - b[0]; c[1] = a[1] - b[1]; c[2] = a[2] - b[2]; }

// collinear or coincident points P [3,3] (or a point that is not finite)
SIM_HD bool degenerate_triple(const double* P) {
  double d12[3], d13[3], d23[3], nrm[3];
  sub3(P + 3, P, d12); sub3(P + 6, P, d13); sub3(P + 6, P + 3, d23);
  const double a2 = dot3(d23, d23), b2 = dot3(d13, d13), c2 = dot3(d12, d12);
  double m = a2 > b2 ? a2 : b2;
  m = c2 > m ? c2 : m;
  cross3(d12, d13, nrm);
  return !(dot3(nrm, nrm) > kCollinear * kCollinear * m * m) || !isfinite(m);
}

// s R x + t: the rotation's rows left to right, then the scale, then the translation
SIM_HD void apply(const double* m, const double* x, double* y) {
  const double* R = m + 1;
  for (int i = 0; i < 3; ++i) y[i] = m[0] * (R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2]) + m[10 + i];
}

// q: src (3), dst (3)
SIM_HD bool is_inlier(const double* m, const double* q, double thr2) {
  double y[3], e[3];
  apply(m, q, y);
  sub3(y, q + 3, e);
  return dot3(e, e) <= thr2;               // (false for a NaN)
}

// one correspondence's terms of the second refit pass (a [kSums2])
SIM_HD void accum10(const double* mu_s, const double* mu_d, const double* q, double* a) {
  double ds[3], dd[3];
  sub3(q, mu_s, ds); sub3(q + 3, mu_d, dd);
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) a[3 * r + c] = a[3 * r + c] + dd[r] * ds[c];
  a[9] = a[9] + dot3(ds, ds);
}

// the closed form from the moments (H [9] row-major, q = sum |src - mu_s|^2); false without a model (s not finite or not positive)
SIM_HD bool model_from_moments(const double* H, double q, const double* mu_s, const double* mu_d, int with_scale, double* m) {
  double U[9], sg[3], V[9];
  svd3(H, U, sg, V);
  const double du = det3_rows(U, U + 3, U + 6), dv = det3_rows(V, V + 3, V + 6);
  const double d = du * dv > 0 ? 1.0 : -1.0;
  double* R = m + 1;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + d * (U[3 * i + 2] * V[3 * j + 2]);
  double s = 1.0;
  if (with_scale) {
    double tr = 0;
    for (int k = 0; k < 9; ++k) tr = tr + R[k] * H[k];
    s = tr / q;
  }
  if (!isfinite(s) || !(s > 0)) return false;
  for (int k = 0; k < 9; ++k) if (!isfinite(R[k])) return false;
  m[0] = s;
  for (int i = 0; i < 3; ++i) m[10 + i] = mu_d[i] - s * (R[3 * i] * mu_s[0] + R[3 * i + 1] * mu_s[1] + R[3 * i + 2] * mu_s[2]);
  return true;
}

// minimal solver: src [3,3], dst [3,3] -> 0 or 1 models
SIM_HD int minimal(const double* src, const double* dst, int with_scale, double* m) {
  if (degenerate_triple(src) || degenerate_triple(dst)) return 0;
  double mu_s[3], mu_d[3], a[kSums2];
  for (int c = 0; c < 3; ++c) { mu_s[c] = (src[c] + src[3 + c] + src[6 + c]) / 3.0; mu_d[c] = (dst[c] + dst[3 + c] + dst[6 + c]) / 3.0; }
  for (int k = 0; k < kSums2; ++k) a[k] = 0.0;
  for (int i = 0; i < 3; ++i) {
    const double q[6] = {src[3 * i], src[3 * i + 1], src[3 * i + 2], dst[3 * i], dst[3 * i + 1], dst[3 * i + 2]};
    accum10(mu_s, mu_d, q, a);
  }
  return model_from_moments(a, a[9], mu_s, mu_d, with_scale, m) ? 1 : 0;
}

// ---- moving a model (loftr_transform_model_host / loftr_transform_model) -------------------------------------------------------------
// X' = f32(s R X + t), in apply()'s order
SIM_HD void transform_point(const double* m, const float* x, float* y) {
  const double X[3] = {(double)x[0], (double)x[1], (double)x[2]};
  double Y[3];
  apply(m, X, Y);
  y[0] = (float)Y[0]; y[1] = (float)Y[1]; y[2] = (float)Y[2];
}
// T [16] row-major camera-from-world -> R_c' = R_c R^T, t_c' = s t_c - R_c' t, bottom row 0 0 0 1 (To may be T)
SIM_HD void transform_pose(const double* m, const double* T, double* To) {
  const double* R = m + 1;
  double Rc[9], tc[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Rc[3 * i + j] = T[4 * i] * R[3 * j] + T[4 * i + 1] * R[3 * j + 1] + T[4 * i + 2] * R[3 * j + 2];
    tc[i] = T[4 * i + 3];
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) To[4 * i + j] = Rc[3 * i + j];
    To[4 * i + 3] = m[0] * tc[i] - (Rc[3 * i] * m[10] + Rc[3 * i + 1] * m[11] + Rc[3 * i + 2] * m[12]);
  }
  To[12] = 0.0; To[13] = 0.0; To[14] = 0.0; To[15] = 1.0;
}

}  // namespace simt
