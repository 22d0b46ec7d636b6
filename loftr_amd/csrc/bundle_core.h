// Bundle adjustment of the triangulated model: the arithmetic and the per-item steps shared by the host routine (bundle.hip) and the GPU
// kernels (bundle_gpu.hip).  As in triangulate_core.h, every function here is compiled for both sides from this one text, fp64, without
// FMA contraction, and uses + - * / and sqrt only (correctly rounded on both sides), so that host and device take identical decisions and
// produce identical bits.  The rule is stated in include/loftr_hip.h and DESIGN §18; the checks of the track table, its error bits and
// the carving step of the workspace are tracks_core.h's.
//
// The run is a sequence of PHASES; a phase is a loop over tracks, over cameras or one single step, and a phase boundary is the only
// ordering (a kernel boundary on the device, the end of a loop on the host).  Every per-item step below reads only what earlier phases
// wrote, so the result does not depend on how a phase is spread over threads.  Every test is written so that a NaN takes the safe side.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "tracks_core.h"

#pragma clang fp contract(off)

#define BA_HD __host__ __device__ inline

namespace ba {

constexpr int kCounts = 16;                // counts[]: see include/loftr_hip.h
constexpr int kTab = 17;                   // doubles per camera of the state table: R [9], t [3], fx, skew, cx, fy, cy
constexpr int kChunk = 4096;               // osum: osum64 per chunk of 4096, then osum of the chunk sums
constexpr double kLambda0 = 1e-4, kLambdaMin = 1e-10, kLambdaMax = 1e10;

enum : int { kConverged = 0, kMaxIters = 1, kStalled = 2, kNothing = 3 };
using tracks::kBadImage;                   // error bits (counts[1])
using tracks::kBadOffsets;
using tracks::kBadGroups;
using tracks::sizes_ok;
enum : int { kActPsp = 0, kActRz0, kActRz, kActCost0, kActSq0, kActCostT, kActSqT };   // what the last level of an osum feeds

BA_HD bool fin(double x) { return fabs(x) <= 1.7976931348623157e308; }        // false for NaN and the infinities

// what one thread owns: damping, counters, flags and the scalars of the conjugate gradients
struct Ctrl {
  int done, err, bad_f, bad_a, bad_e, pcg_done, fresh, cur, status, n_iters, n_accepted, n_focal;   // bad_*: raised in the factor / apply / evaluate phase
  long long n_pcg;
  unsigned long long n_active_obs, n_active_pts, n_free;
  double lambda, cost, sq, cost_t, sq_t, cost0, sq0, rz, rz0, psp, alpha, beta;
};

struct Ctx {
  // the problem
  const long* offsets; long T;
  const int* image; const float* xy; const uint8_t* mask; long N;
  const float* xyz_in; const double* K; const double* Tin; const uint8_t* fixed; int n;
  const long* cam_offsets; const int* cam_obs;
  double huber, pcg_tol2, ftol;
  // the result
  double* T_out; float* xyz_out; uint8_t* obs_active; uint8_t* cam_free; uint8_t* point_active; long* counts;
  // the workspace (layout(): the same on both sides)
  double *tab, *quat, *X;                   // [2][n][17], [2][n][4], [2][T][3]: the state and the trial, told apart by ctrl->cur
  double *V, *gp, *Vf, *z;                  // [T][6] sum B^T B, [T][3] sum B^T r, [T][6] factor of the damped V, [T][3] track half
  double *U, *gc, *Uf;                      // [n][21] sum A^T A, [n][6] sum A^T r, [n][21] factor of the damped U  (28, 7, 28 when M = 7)
  double *x, *r, *zc, *p, *Sp;              // [n][M] each: conjugate gradients over the cameras
  double *part, *part2, *red;               // [max(T, n)] x 2 terms of an osum, [2][ceil(max / 4096)] its chunk sums
  int* obs_track;                           // [N]
  uint8_t* cam_valid;                       // [n]
  Ctrl* ctrl;
};

// §18.1, focal refinement: the camera block is M = 7 wide (the seventh parameter is the relative focal step) and the problem carries the
// extra inputs and outputs.  Every step that touches the camera block is a template on M; M = 6 is the fixed-intrinsics rule.
struct Ctx7 : Ctx {
  const uint8_t* refine_focal; int min_focal_obs; double focal_lo, focal_hi;
  double* K_out; uint8_t* cam_focal;
};
template <int M> struct CtxOf { using type = Ctx; };
template <> struct CtxOf<7> { using type = Ctx7; };
template <int M> using CtxT = typename CtxOf<M>::type;
template <int M> constexpr int kTri = M * (M + 1) / 2;      // entries of the upper triangle of a camera block: 21 or 28

// carves the workspace; base may be null (then only the size counts) -> bytes
template <int M> inline size_t layout(Ctx& c, char* base) {
  const size_t T = (size_t)c.T, n = (size_t)c.n, N = (size_t)c.N, m = (T > n ? T : n) + 1, ch = (m + kChunk - 1) / kChunk;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = tracks::carve(&off, bytes ? bytes : 1); return base ? base + at : nullptr; };
  c.ctrl = (Ctrl*)take(sizeof(Ctrl));
  c.tab = (double*)take(8 * 2 * n * kTab); c.quat = (double*)take(8 * 2 * n * 4); c.X = (double*)take(8 * 2 * T * 3);
  c.V = (double*)take(8 * T * 6); c.gp = (double*)take(8 * T * 3); c.Vf = (double*)take(8 * T * 6); c.z = (double*)take(8 * T * 3);
  c.U = (double*)take(8 * n * kTri<M>); c.gc = (double*)take(8 * n * M); c.Uf = (double*)take(8 * n * kTri<M>);
  c.x = (double*)take(8 * n * M); c.r = (double*)take(8 * n * M); c.zc = (double*)take(8 * n * M); c.p = (double*)take(8 * n * M);
  c.Sp = (double*)take(8 * n * M);
  c.part = (double*)take(8 * m); c.part2 = (double*)take(8 * m); c.red = (double*)take(8 * 2 * ch);
  c.obs_track = (int*)take(4 * N); c.cam_valid = (uint8_t*)take(n);
  return off;
}

// ---- rule 1: the state ---------------------------------------------------------------------------------------------------------------
// unit quaternion (w, x, y, z) of the rotation in T [4,4]: Shepperd's branch on the largest of trace, R00, R11, R22 (the first on ties)
BA_HD void quat_from_matrix(const double* T, double* q) {
  const double r00 = T[0], r01 = T[1], r02 = T[2], r10 = T[4], r11 = T[5], r12 = T[6], r20 = T[8], r21 = T[9], r22 = T[10];
  const double tr = (r00 + r11) + r22;
  double w, x, y, z;
  if (tr >= r00 && tr >= r11 && tr >= r22) {
    const double s = 2.0 * sqrt(1.0 + tr);
    w = 0.25 * s; x = (r21 - r12) / s; y = (r02 - r20) / s; z = (r10 - r01) / s;
  } else if (r00 >= r11 && r00 >= r22) {
    const double s = 2.0 * sqrt(((1.0 + r00) - r11) - r22);
    w = (r21 - r12) / s; x = 0.25 * s; y = (r01 + r10) / s; z = (r02 + r20) / s;
  } else if (r11 >= r22) {
    const double s = 2.0 * sqrt(((1.0 + r11) - r00) - r22);
    w = (r02 - r20) / s; x = (r01 + r10) / s; y = 0.25 * s; z = (r12 + r21) / s;
  } else {
    const double s = 2.0 * sqrt(((1.0 + r22) - r00) - r11);
    w = (r10 - r01) / s; x = (r02 + r20) / s; y = (r12 + r21) / s; z = 0.25 * s;
  }
  const double nq = sqrt(((w * w + x * x) + y * y) + z * z);
  q[0] = w / nq; q[1] = x / nq; q[2] = y / nq; q[3] = z / nq;
}
BA_HD void matrix_from_quat(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}
BA_HD double* tab_of(const Ctx& c, int buf, long i) { return c.tab + ((long)buf * c.n + i) * kTab; }
BA_HD double* quat_of(const Ctx& c, int buf, long i) { return c.quat + ((long)buf * c.n + i) * 4; }
BA_HD double* X_of(const Ctx& c, int buf, long t) { return c.X + ((long)buf * c.T + t) * 3; }

// phase "camera setup", per camera: validity, quaternion, both copies of the table; the output matrix starts as the input's bits.
// The table holds R(q) for a valid camera that is not fixed and the input's R otherwise.
BA_HD void cam_setup(const Ctx& c, long i) {
  const double *K = c.K + 9 * i, *T = c.Tin + 16 * i;
  const double fx = K[0], sk = K[1], cx = K[2], fy = K[4], cy = K[5];
  bool ok = fin(fx) && fin(sk) && fin(cx) && fin(fy) && fin(cy) && fx != 0.0 && fy != 0.0;
  for (int k = 0; k < 12; ++k) ok = ok && fin(T[k]);
  double q[4], R[9];
  quat_from_matrix(T, q);
  ok = ok && fin(q[0]) && fin(q[1]) && fin(q[2]) && fin(q[3]);
  if (ok && !c.fixed[i]) matrix_from_quat(q, R);
  else for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) R[3 * r + k] = T[4 * r + k];
  for (int buf = 0; buf < 2; ++buf) {
    double *tab = tab_of(c, buf, i), *qq = quat_of(c, buf, i);
    for (int k = 0; k < 9; ++k) tab[k] = R[k];
    for (int k = 0; k < 3; ++k) tab[9 + k] = T[4 * k + 3];
    tab[12] = fx; tab[13] = sk; tab[14] = cx; tab[15] = fy; tab[16] = cy;
    for (int k = 0; k < 4; ++k) qq[k] = q[k];
  }
  c.cam_valid[i] = (uint8_t)ok;
  const uint64_t* src = (const uint64_t*)T;
  uint64_t* dst = (uint64_t*)(c.T_out + 16 * i);
  for (int k = 0; k < 16; ++k) dst[k] = src[k];
}

// ... and with focal refinement: the output intrinsics start as the input's bits
BA_HD void cam_setup_focal(const Ctx7& c, long i) {
  const uint64_t* src = (const uint64_t*)(c.K + 9 * i);
  uint64_t* dst = (uint64_t*)(c.K_out + 9 * i);
  for (int k = 0; k < 9; ++k) dst[k] = src[k];
}
// phase "camera groups", the last step of a camera with cnt active observations: does it refine its focal?
BA_HD bool cam_focal_rule(const Ctx7& c, long i, bool is_free, long cnt) {
  return is_free && c.refine_focal[i] != 0 && cnt >= (long)c.min_focal_obs;
}

// ---- rule 3: residual and Jacobians ----------------------------------------------------------------------------------------------------
// P = R X, Y = P + t -> Y_z > 0
BA_HD bool transform(const double* cam, const double* X, double* P, double* Y) {
  for (int r = 0; r < 3; ++r) {
    P[r] = (cam[3 * r] * X[0] + cam[3 * r + 1] * X[1]) + cam[3 * r + 2] * X[2];
    Y[r] = P[r] + cam[9 + r];
  }
  return Y[2] > 0.0;
}
BA_HD void residual(const double* cam, const double* Y, double u, double v, double* r) {
  const double a = Y[0] / Y[2], b = Y[1] / Y[2];
  r[0] = ((cam[12] * a + cam[13] * b) + cam[14]) - u;
  r[1] = (cam[15] * b + cam[16]) - v;
}
// rule 4: sw = sqrt(weight), rho, sq = |r|^2
BA_HD void loss(const double* r, double huber, double* sw, double* rho, double* sq) {
  const double s = r[0] * r[0] + r[1] * r[1];
  *sq = s;
  if (huber > 0.0) {
    const double nr = sqrt(s);
    if (!(nr <= huber)) { *sw = sqrt(huber / nr); *rho = (2.0 * huber) * nr - huber * huber; return; }
  }
  *sw = 1.0; *rho = s;
}
// A [2,M] = sw dr/d(omega, dt[, delta]), B [2,3] = sw dr/dX.  M = 7: the last column is sw (fx a + skew b, fy b) for a camera that
// refines its focal (`focal`) and zero for any other.
template <int M> BA_HD void jacobians(const double* cam, const double* P, const double* Y, double sw, bool focal, double* A, double* B) {
  const double fx = cam[12], sk = cam[13], fy = cam[15];
  const double du[3] = {sw * (fx / Y[2]), sw * (sk / Y[2]), sw * -(((fx * Y[0] + sk * Y[1]) / Y[2]) / Y[2])};
  const double dv[3] = {0.0, sw * (fy / Y[2]), sw * -(((fy * Y[1]) / Y[2]) / Y[2])};
  A[0] = du[2] * P[1] - du[1] * P[2]; A[1] = du[0] * P[2] - du[2] * P[0]; A[2] = du[1] * P[0] - du[0] * P[1];
  A[3] = du[0]; A[4] = du[1]; A[5] = du[2];
  A[M] = dv[2] * P[1] - dv[1] * P[2]; A[M + 1] = -(dv[2] * P[0]); A[M + 2] = dv[1] * P[0];
  A[M + 3] = 0.0; A[M + 4] = dv[1]; A[M + 5] = dv[2];
  if constexpr (M == 7) {
    if (focal) {
      const double a = Y[0] / Y[2], b = Y[1] / Y[2];
      A[6] = sw * (fx * a + sk * b); A[M + 6] = sw * (fy * b);
    } else {
      A[6] = 0.0; A[M + 6] = 0.0;
    }
  }
  for (int k = 0; k < 3; ++k) {
    B[k] = (du[0] * cam[k] + du[1] * cam[3 + k]) + du[2] * cam[6 + k];
    B[3 + k] = dv[1] * cam[3 + k] + dv[2] * cam[6 + k];
  }
}
// the weighted A, B and residual rs of observation o of track t at state `buf`
template <int M> BA_HD void obs_terms(const CtxT<M>& c, int buf, long o, long t, double* A, double* B, double* rs) {
  const double *cam = tab_of(c, buf, c.image[o]), *X = X_of(c, buf, t);
  bool focal = false;
  if constexpr (M == 7) focal = c.cam_focal[c.image[o]] != 0;
  double P[3], Y[3], r[2], sw, rho, sq;
  transform(cam, X, P, Y);
  residual(cam, Y, (double)c.xy[2 * o], (double)c.xy[2 * o + 1], r);
  loss(r, c.huber, &sw, &rho, &sq);
  jacobians<M>(cam, P, Y, sw, focal, A, B);
  rs[0] = sw * r[0]; rs[1] = sw * r[1];
}

// ---- rule 2: the active set ----------------------------------------------------------------------------------------------------------
// phase "track setup", per track: checks the offsets and the image ids it reads, marks the active observations, copies the point into
// both states and its input bits to the output -> error bits; *n_act = active observations of the track
BA_HD int track_setup(const Ctx& c, long t, long* n_act) {
  *n_act = 0;
  long b, e;
  if (!tracks::span(c.offsets, c.T, c.N, t, &b, &e)) return kBadOffsets;
  const uint32_t* src = (const uint32_t*)(c.xyz_in + 3 * t);
  uint32_t* dst = (uint32_t*)(c.xyz_out + 3 * t);
  double X[3];
  for (int k = 0; k < 3; ++k) {
    dst[k] = src[k];
    X[k] = (double)c.xyz_in[3 * t + k];
    X_of(c, 0, t)[k] = X[k];
    X_of(c, 1, t)[k] = X[k];
  }
  const bool pt = fin(X[0]) && fin(X[1]) && fin(X[2]);
  if (!tracks::images_ok(c.image, b, e, c.n)) return kBadImage;
  long cnt = 0;
  for (long o = b; o < e; ++o) {
    const int im = c.image[o];
    bool a = pt && c.mask[o] != 0 && c.cam_valid[im] != 0 && fin((double)c.xy[2 * o]) && fin((double)c.xy[2 * o + 1]);
    if (a) {
      double P[3], Y[3];
      a = transform(tab_of(c, 0, im), X, P, Y);
    }
    c.obs_active[o] = (uint8_t)a;
    c.obs_track[o] = (int)t;
    cnt += a;
  }
  if (cnt < 2) {
    for (long o = b; o < e; ++o) c.obs_active[o] = 0;
    cnt = 0;
  }
  c.point_active[t] = (uint8_t)(cnt > 0);
  *n_act = cnt;
  return 0;
}
// phase "camera groups": slot k of camera i's list; -> error bits, *active = the observation is active.  Reads nothing through a bad value.
BA_HD int group_check(const Ctx& c, long i, long b, long k, bool* active) {
  *active = false;
  int o;
  if (tracks::group_slot(c.cam_obs, c.image, c.N, i, b, k, &o)) return kBadGroups;
  *active = c.obs_active[o] != 0;
  return 0;
}
BA_HD bool group_range(const Ctx& c, long i, long* b, long* e) { return tracks::span(c.cam_offsets, c.n, c.N, i, b, e); }

// ---- rule 6: fixed-order elimination, M x M, no pivoting --------------------------------------------------------------------------------
// a: upper triangle row-major (M (M + 1) / 2); f: d [M] then the strict lower triangle of L row-major; false on a non-positive pivot.
// The diagonal is damped here: a_ii (1 + lambda), or lambda when a_ii is zero.
BA_HD double damped(double d, double lambda) { return d == 0.0 ? lambda : d * (1.0 + lambda); }
template <int M> BA_HD bool factor(const double* a, double lambda, double* f) {
  double L[M][M], d[M];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double s = damped(a[j * M - j * (j - 1) / 2], lambda);
#pragma unroll
    for (int k = 0; k < j; ++k) s = s - (L[j][k] * L[j][k]) * d[k];
    d[j] = s;
    ok = ok && s > 0.0;
#pragma unroll
    for (int i = j + 1; i < M; ++i) {
      double v = a[j * M - j * (j - 1) / 2 + (i - j)];
#pragma unroll
      for (int k = 0; k < j; ++k) v = v - (L[i][k] * L[j][k]) * d[k];
      L[i][j] = v / s;
    }
  }
#pragma unroll
  for (int j = 0; j < M; ++j) f[j] = d[j];
#pragma unroll
  for (int i = 1; i < M; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) f[M + i * (i - 1) / 2 + j] = L[i][j];
  return ok;
}
template <int M> BA_HD void solve(const double* f, const double* b, double* x) {
  double y[M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = s - f[M + i * (i - 1) / 2 + k] * y[k];
    y[i] = s;
  }
#pragma unroll
  for (int i = M - 1; i >= 0; --i) {
    double s = y[i] / f[i];
#pragma unroll
    for (int k = i + 1; k < M; ++k) s = s - f[M + k * (k - 1) / 2 + i] * y[k];
    y[i] = s;
  }
#pragma unroll
  for (int i = 0; i < M; ++i) x[i] = y[i];
}
template <int M> BA_HD double dotm(const double* a, const double* b) {
  double s = a[0] * b[0];
#pragma unroll
  for (int k = 1; k < M; ++k) s = s + a[k] * b[k];
  return s;
}

// ---- rule 5: the sums ----------------------------------------------------------------------------------------------------------------
// phase "linearise tracks", per track: V = sum B^T B (upper triangle), gp = sum B^T rs, sequentially over the active observations
template <int M> BA_HD void track_lin(const CtxT<M>& c, int buf, long t) {
  double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
  if (c.point_active[t])
    for (long o = c.offsets[t]; o < c.offsets[t + 1]; ++o) {
      if (!c.obs_active[o]) continue;
      double A[2 * M], B[6], rs[2];
      obs_terms<M>(c, buf, o, t, A, B, rs);
      V[0] = V[0] + (B[0] * B[0] + B[3] * B[3]); V[1] = V[1] + (B[0] * B[1] + B[3] * B[4]); V[2] = V[2] + (B[0] * B[2] + B[3] * B[5]);
      V[3] = V[3] + (B[1] * B[1] + B[4] * B[4]); V[4] = V[4] + (B[1] * B[2] + B[4] * B[5]); V[5] = V[5] + (B[2] * B[2] + B[5] * B[5]);
      for (int k = 0; k < 3; ++k) g[k] = g[k] + (B[k] * rs[0] + B[3 + k] * rs[1]);
    }
  for (int k = 0; k < 6; ++k) c.V[6 * t + k] = V[k];
  for (int k = 0; k < 3; ++k) c.gp[3 * t + k] = g[k];
}
// phase "linearise cameras", one element of a camera's osum64: a [27] += (A^T A upper triangle [21], A^T rs [6]) of observation o
// (a [35], 28 and 7 when M = 7)
template <int M> BA_HD void cam_lin_term(const CtxT<M>& c, int buf, long o, double* a) {
  double A[2 * M], B[6], rs[2];
  obs_terms<M>(c, buf, o, c.obs_track[o], A, B, rs);
  int m = 0;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = i; j < M; ++j) { a[m] = a[m] + (A[i] * A[j] + A[M + i] * A[M + j]); ++m; }
#pragma unroll
  for (int i = 0; i < M; ++i) a[kTri<M> + i] = a[kTri<M> + i] + (A[i] * rs[0] + A[M + i] * rs[1]);
}

// ---- rule 6: the step ------------------------------------------------------------------------------------------------------------------
// phase "factor", per track / per free camera -> false on a non-positive pivot
BA_HD bool track_factor(const Ctx& c, long t, double lambda) {
  if (!c.point_active[t]) return true;
  double f[6];
  const bool ok = factor<3>(c.V + 6 * t, lambda, f);
  for (int k = 0; k < 6; ++k) c.Vf[6 * t + k] = f[k];
  return ok;
}
template <int M> BA_HD bool cam_factor(const Ctx& c, long i, double lambda) {
  if (!c.cam_free[i]) return true;
  double f[kTri<M>];
  const bool ok = factor<M>(c.U + kTri<M> * i, lambda, f);
#pragma unroll
  for (int k = 0; k < kTri<M>; ++k) c.Uf[kTri<M> * i + k] = f[k];
  return ok;
}
// phase "track half", per track.  mode 0: z = Vd^-1 gp.  mode 1: z = Vd^-1 sum B^T (A vec_c) over the active observations of free
// cameras, sequentially.  mode 2 (back substitution): dX = Vd^-1 (-(gp + sum B^T (A vec_c))), trial X' = X + dX -> false when not finite.
template <int M> BA_HD bool track_half(const CtxT<M>& c, int buf, long t, int mode, const double* vec) {
  if (!c.point_active[t]) return true;
  double s[3] = {0.0, 0.0, 0.0}, z[3];
  if (mode != 0)
    for (long o = c.offsets[t]; o < c.offsets[t + 1]; ++o) {
      const int im = c.image[o];
      if (!c.obs_active[o] || !c.cam_free[im]) continue;
      double A[2 * M], B[6], rs[2];
      obs_terms<M>(c, buf, o, t, A, B, rs);
      const double* v = vec + M * (long)im;
      const double eu = dotm<M>(A, v), ev = dotm<M>(A + M, v);
      for (int k = 0; k < 3; ++k) s[k] = s[k] + (B[k] * eu + B[3 + k] * ev);
    }
  if (mode == 0) for (int k = 0; k < 3; ++k) s[k] = c.gp[3 * t + k];
  if (mode == 2) for (int k = 0; k < 3; ++k) s[k] = -(c.gp[3 * t + k] + s[k]);
  solve<3>(c.Vf + 6 * t, s, z);
  if (mode != 2) {
    for (int k = 0; k < 3; ++k) c.z[3 * t + k] = z[k];
    return true;
  }
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const double x = X_of(c, buf, t)[k] + z[k];
    X_of(c, 1 - buf, t)[k] = x;
    ok = ok && fin(x);
  }
  return ok;
}
// phase "camera half", one element of a camera's osum64: a [6] += A^T (B z_j) of observation o
template <int M> BA_HD void cam_half_term(const CtxT<M>& c, int buf, long o, double* a) {
  double A[2 * M], B[6], rs[2];
  const long t = c.obs_track[o];
  obs_terms<M>(c, buf, o, t, A, B, rs);
  const double* z = c.z + 3 * t;
  const double eu = (B[0] * z[0] + B[1] * z[1]) + B[2] * z[2], ev = (B[3] * z[0] + B[4] * z[1]) + B[5] * z[2];
#pragma unroll
  for (int k = 0; k < M; ++k) a[k] = a[k] + (A[k] * eu + A[M + k] * ev);
}
// ... and what follows the sum a [6] of free camera i.  mode 0 (right-hand side): b = -(gc - a); x = 0, r = b, zc = M^-1 r, p = zc,
// part = r . zc.  mode 1: Sp = Ud p - a, part = p . Sp.  A camera that is not free has part = +0.
template <int M> BA_HD void cam_half_finish(const Ctx& c, long i, int mode, double lambda, const double* a) {
  if (!c.cam_free[i]) { c.part[i] = 0.0; return; }
  double *x = c.x + M * i, *r = c.r + M * i, *zc = c.zc + M * i, *p = c.p + M * i, *Sp = c.Sp + M * i;
  if (mode == 0) {
    double b[M], zz[M];
#pragma unroll
    for (int k = 0; k < M; ++k) { b[k] = -(c.gc[M * i + k] - a[k]); x[k] = 0.0; r[k] = b[k]; }
    solve<M>(c.Uf + kTri<M> * i, b, zz);
#pragma unroll
    for (int k = 0; k < M; ++k) { zc[k] = zz[k]; p[k] = zz[k]; }
    c.part[i] = dotm<M>(b, zz);
    return;
  }
  const double* U = c.U + kTri<M> * i;
  double pv[M], sp[M];
#pragma unroll
  for (int k = 0; k < M; ++k) pv[k] = p[k];
#pragma unroll
  for (int row = 0; row < M; ++row) {
    double s = 0.0;
#pragma unroll
    for (int col = 0; col < M; ++col) {
      const int lo = row < col ? row : col, hi = row < col ? col : row;
      const double u = U[lo * M - lo * (lo - 1) / 2 + (hi - lo)];
      s = s + (row == col ? damped(u, lambda) : u) * pv[col];
    }
    sp[row] = s - a[row];
    Sp[row] = sp[row];
  }
  c.part[i] = dotm<M>(pv, sp);
}
// phase "update 1", per free camera: x += alpha p, r -= alpha Sp, zc = M^-1 r, part = r . zc
template <int M> BA_HD void cam_update1(const Ctx& c, long i, double alpha) {
  if (!c.cam_free[i]) { c.part[i] = 0.0; return; }
  double r[M], zz[M];
#pragma unroll
  for (int k = 0; k < M; ++k) {
    c.x[M * i + k] = c.x[M * i + k] + alpha * c.p[M * i + k];
    r[k] = c.r[M * i + k] - alpha * c.Sp[M * i + k];
    c.r[M * i + k] = r[k];
  }
  solve<M>(c.Uf + kTri<M> * i, r, zz);
#pragma unroll
  for (int k = 0; k < M; ++k) c.zc[M * i + k] = zz[k];
  c.part[i] = dotm<M>(r, zz);
}
// phase "update 2", per free camera: p = zc + beta p
template <int M> BA_HD void cam_update2(const Ctx& c, long i, double beta) {
  if (!c.cam_free[i]) return;
  for (int k = 0; k < M; ++k) c.p[M * i + k] = c.zc[M * i + k] + beta * c.p[M * i + k];
}

// ---- rule 7: the trial -----------------------------------------------------------------------------------------------------------------
// phase "apply", per free camera: q' = normalise((1, omega / 2) (x) q), t' = t + dt into the other state -> false when not finite
// M = 7, a camera that refines its focal: fx' = fx (1 + delta), skew' = skew (1 + delta), fy' = fy (1 + delta) -> false as well when
// fx' or fy' is not finite or fx' / fx_in or fy' / fy_in is not strictly inside (focal_lo, focal_hi); a NaN fails every test
template <int M> BA_HD bool cam_apply(const CtxT<M>& c, int buf, long i) {
  if (!c.cam_free[i]) return true;
  const double *d = c.x + M * i,*q = quat_of(c, buf, i), *tab = tab_of(c, buf, i);
  double *q2 = quat_of(c, 1 - buf, i), *tab2 = tab_of(c, 1 - buf, i);
  const double a = 0.5 * d[0], b = 0.5 * d[1], e = 0.5 * d[2];
  double w = ((q[0] - a * q[1]) - b * q[2]) - e * q[3];
  double x = ((q[1] + a * q[0]) + b * q[3]) - e * q[2];
  double y = ((q[2] - a * q[3]) + b * q[0]) + e * q[1];
  double z = ((q[3] + a * q[2]) - b * q[1]) + e * q[0];
  const double nq = sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / nq; x = x / nq; y = y / nq; z = z / nq;
  q2[0] = w; q2[1] = x; q2[2] = y; q2[3] = z;
  double R[9];
  matrix_from_quat(q2, R);
  bool ok = fin(w) && fin(x) && fin(y) && fin(z);
  for (int k = 0; k < 9; ++k) tab2[k] = R[k];
  for (int k = 0; k < 3; ++k) {
    tab2[9 + k] = tab[9 + k] + d[3 + k];
    ok = ok && fin(tab2[9 + k]);
  }
  if constexpr (M == 7) {
    if (c.cam_focal[i]) {
      const double s = 1.0 + d[6];
      const double fx = tab[12] * s, sk = tab[13] * s, fy = tab[15] * s;
      tab2[12] = fx; tab2[13] = sk; tab2[15] = fy;
      const double rx = fx / c.K[9 * i], ry = fy / c.K[9 * i + 4];
      ok = ok && fin(fx) && fin(fy) && rx > c.focal_lo && rx < c.focal_hi && ry > c.focal_lo && ry < c.focal_hi;
    }
  }
  return ok;
}
// phase "evaluate", per track at state `buf`: part = sum rho, part2 = sum |r|^2 sequentially over the active observations
// -> false when an active observation is not in front of its camera
BA_HD bool track_eval(const Ctx& c, int buf, long t) {
  double cost = 0.0, sq = 0.0;
  bool ok = true;
  if (c.point_active[t])
    for (long o = c.offsets[t]; o < c.offsets[t + 1]; ++o) {
      if (!c.obs_active[o]) continue;
      const double* cam = tab_of(c, buf, c.image[o]);
      double P[3], Y[3], r[2], sw, rho, s;
      ok = transform(cam, X_of(c, buf, t), P, Y) && ok;
      residual(cam, Y, (double)c.xy[2 * o], (double)c.xy[2 * o + 1], r);
      loss(r, c.huber, &sw, &rho, &s);
      cost = cost + rho;
      sq = sq + s;
    }
  c.part[t] = cost;
  c.part2[t] = sq;
  return ok;
}

// ---- the single steps (one thread) -----------------------------------------------------------------------------------------------------
BA_HD void ctrl_init(const Ctx& c) {
  Ctrl& s = *c.ctrl;
  s.done = s.err = s.bad_f = s.bad_a = s.bad_e = s.pcg_done = s.cur = s.n_iters = s.n_accepted = s.n_focal = 0;
  s.fresh = 1;
  s.status = kMaxIters;
  s.n_pcg = 0;
  s.n_active_obs = s.n_active_pts = s.n_free = 0;
  s.lambda = kLambda0;
  s.cost = s.sq = s.cost_t = s.sq_t = s.cost0 = s.sq0 = s.rz = s.rz0 = s.psp = s.alpha = s.beta = 0.0;
}
// the last level of an osum hands its result to the owner of the scalars
BA_HD void ctrl_feed(const Ctx& c, int action, double v) {
  Ctrl& s = *c.ctrl;
  switch (action) {
    case kActPsp: s.psp = v; s.alpha = s.rz / v; if (!(v > 0.0)) s.pcg_done = 1; break;
    case kActRz0: s.rz = s.rz0 = v; if (v <= c.pcg_tol2 * v) s.pcg_done = 1; break;
    case kActRz: s.beta = v / s.rz; s.rz = v; s.n_pcg += 1; if (v <= c.pcg_tol2 * s.rz0) s.pcg_done = 1; break;
    case kActCost0:
      s.cost = s.cost0 = v;
      if (s.n_active_obs == 0) { s.done = 1; s.status = kNothing; }
      else if (v == 0.0) { s.done = 1; s.status = kConverged; }           // nothing can lower a cost of exactly 0
      break;
    case kActSq0: s.sq = s.sq0 = v; break;
    case kActCostT: s.cost_t = v; break;
    case kActSqT: s.sq_t = v; break;
  }
}
// phase "accept": the end of a trial
BA_HD void ctrl_accept(const Ctx& c) {
  Ctrl& s = *c.ctrl;
  if (s.done || s.err) return;
  s.n_iters += 1;
  if (!(s.bad_f | s.bad_a | s.bad_e) && s.cost_t < s.cost) {
    const double gain = s.cost - s.cost_t;
    s.cost = s.cost_t; s.sq = s.sq_t;
    s.cur = 1 - s.cur;
    s.n_accepted += 1;
    s.fresh = 1;
    s.lambda = s.lambda / 10.0 > kLambdaMin ? s.lambda / 10.0 : kLambdaMin;
    if (gain <= c.ftol * s.cost) { s.done = 1; s.status = kConverged; }
  } else {
    s.fresh = 0;
    s.lambda = 10.0 * s.lambda;
    if (s.lambda > kLambdaMax) { s.done = 1; s.status = kStalled; }
  }
  s.bad_f = s.bad_a = s.bad_e = 0;
  s.pcg_done = 0;
}
// phase "write": the outputs of a free camera / an active point from the final state
template <int M> BA_HD void cam_write(const CtxT<M>& c, int buf, long i) {
  if (!c.cam_free[i]) return;
  const double* tab = tab_of(c, buf, i);
  double* T = c.T_out + 16 * i;
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) T[4 * r + k] = tab[3 * r + k];
    T[4 * r + 3] = tab[9 + r];
  }
  T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
  if constexpr (M == 7) {
    if (c.cam_focal[i]) {                    // the other four entries keep the input's bits (cam_setup_focal)
      double* K = c.K_out + 9 * i;
      K[0] = tab[12]; K[1] = tab[13]; K[2] = tab[14]; K[4] = tab[15]; K[5] = tab[16];
    }
  }
}
BA_HD void track_write(const Ctx& c, int buf, long t) {
  if (!c.point_active[t]) return;
  for (int k = 0; k < 3; ++k) c.xyz_out[3 * t + k] = (float)X_of(c, buf, t)[k];
}
BA_HD long bits_of(double v) { union { double d; long l; } u; u.d = v; return u.l; }
template <int M> BA_HD void ctrl_write(const Ctx& c) {
  const Ctrl& s = *c.ctrl;
  long* k = c.counts;
  const double na = (double)s.n_active_obs;
  k[0] = s.status; k[1] = s.err; k[2] = s.n_iters; k[3] = s.n_accepted; k[4] = (long)s.n_pcg;
  k[5] = (long)s.n_active_obs; k[6] = (long)s.n_active_pts; k[7] = (long)s.n_free;
  k[8] = bits_of(s.cost0); k[9] = bits_of(s.cost);
  k[10] = bits_of(s.n_active_obs ? sqrt(s.sq0 / na) : 0.0); k[11] = bits_of(s.n_active_obs ? sqrt(s.sq / na) : 0.0);
  k[12] = bits_of(s.lambda); k[13] = 0; k[14] = 0; k[15] = 0;
  if constexpr (M == 7) k[13] = s.n_focal;   // cameras that refine their focal
}

// ---- §18.2: one relative focal step per GROUP of cameras ----------------------------------------------------------------------------------
// The unknowns are 6 per free camera and 1 per refining group; the system is E^T S7 E x = E^T b7, E copying a group's value into the seventh
// slot of its members with cam_focal.  The camera vectors keep §18.1's stride of 7: entries 0..5 are the pose part (read and written for a
// free camera only; +0 is used for any other), entry 6 of Sp is the camera's seventh entry BEFORE E^T (written for a member with cam_focal
// only), entry 6 of the others is unused.  The group vectors are [G].  A camera takes part when it is free or has cam_focal ("live"); the
// pose columns of A are +0 for a camera that is not free, the seventh is +0 for one without cam_focal.
enum : int { kBadCamGroups = 8 };          // error bit: cam_group / group_offsets / group_cams are not the stable grouping
enum : int { kActStore = -2 };             // an osum whose result waits in CtrlS::acc for the group sum that follows it
struct CtrlS { double acc; int n_groups; };
struct CtxS : Ctx7 {
  const int* cam_group; const long* group_offsets; const int* group_cams; int G;
  uint8_t* group_focal;
  double *dg, *xg, *rg, *zg, *pg, *Spg, *partg;   // [G] each: sum of U77 over the members, the conjugate gradients over the groups, terms of an osum
  double* sg;                                     // [2][n]: the factor a group has taken so far, in the state and in the trial (ctrl->cur)
  int* cam_cnt;                                   // [n] active observations of a camera that carries, else 0
  CtrlS* cs;
};
constexpr int idx7(int r, int k) { return r * 7 - r * (r - 1) / 2 + (k - r); }   // entry (r, k), r <= k, of a 7 x 7 upper triangle

// layout<7> and what the groups add, sized by n (G <= n), so that the size does not depend on the grouping
inline size_t layout_shared(CtxS& c, char* base) {
  size_t off = layout<7>(c, base);
  const size_t n = (size_t)c.n;
  auto take = [&](size_t bytes) { const size_t at = tracks::carve(&off, bytes ? bytes : 1); return base ? base + at : nullptr; };
  c.cs = (CtrlS*)take(sizeof(CtrlS));
  c.dg = (double*)take(8 * n); c.xg = (double*)take(8 * n); c.rg = (double*)take(8 * n); c.zg = (double*)take(8 * n);
  c.pg = (double*)take(8 * n); c.Spg = (double*)take(8 * n); c.partg = (double*)take(8 * n); c.sg = (double*)take(8 * 2 * n);
  c.cam_cnt = (int*)take(4 * n);
  return off;
}
BA_HD void shared_init(const CtxS& c) { ctrl_init(c); c.cs->acc = 0.0; c.cs->n_groups = 0; }
BA_HD bool live(const CtxS& c, long i) { return c.cam_free[i] != 0 || c.cam_focal[i] != 0; }

// phase "camera groups", the last step of a camera with cnt active observations: does it carry its group's focal (its pose may be fixed)?
// -> error bits
BA_HD int cam_carry(const CtxS& c, long i, long cnt) {
  c.cam_cnt[i] = (c.cam_valid[i] != 0 && c.refine_focal[i] != 0 && cnt >= 1) ? (int)cnt : 0;
  c.cam_focal[i] = 0;
  const int g = c.cam_group[i];
  return g < 0 || g >= c.G ? kBadCamGroups : 0;
}
// phase "focal groups": the span of group g (not empty) and slot k of its list -> error bits, *cnt = what the member carries.  Ascending
// within a group, and groups in the order of their first members.  Reads nothing through a bad value.
BA_HD bool cgroup_range(const CtxS& c, long g, long* b, long* e) { return tracks::span(c.group_offsets, c.G, c.n, g, b, e) && *e > *b; }
BA_HD int cgroup_slot(const CtxS& c, long g, long b, long k, long* cnt) {
  *cnt = 0;
  const int i = c.group_cams[k];
  if (i < 0 || i >= c.n) return kBadCamGroups;
  if (c.cam_group[i] != g) return kBadCamGroups;
  if (k > b && !(c.group_cams[k - 1] < i)) return kBadCamGroups;
  if (k == b && g > 0) {
    const long pb = c.group_offsets[g - 1];
    if (pb < 0 || pb >= c.n || !(c.group_cams[pb] < i)) return kBadCamGroups;
  }
  *cnt = c.cam_cnt[i];
  return 0;
}
BA_HD double* sg_of(const CtxS& c, int buf, long g) { return c.sg + ((long)buf * c.n + g); }
// ... and the end of group g's check: does it refine?  Its factor starts at 1 in both states.
BA_HD bool cgroup_rule(const CtxS& c, long g, long total) {
  *sg_of(c, 0, g) = 1.0; *sg_of(c, 1, g) = 1.0;
  return total >= (long)c.min_focal_obs;
}

// A, B, rs of §18.1 with the columns of a camera that is not free set to +0
BA_HD void obs_terms_s(const CtxS& c, int buf, long o, long t, double* A, double* B, double* rs) {
  obs_terms<7>(c, buf, o, t, A, B, rs);
  if (!c.cam_free[c.image[o]])
    for (int k = 0; k < 6; ++k) { A[k] = 0.0; A[7 + k] = 0.0; }
}
// one element of a live camera's osum64 of the linearisation: a [35]
BA_HD void cam_lin_term_s(const CtxS& c, int buf, long o, double* a) {
  double A[14], B[6], rs[2];
  obs_terms_s(c, buf, o, c.obs_track[o], A, B, rs);
  int m = 0;
#pragma unroll
  for (int i = 0; i < 7; ++i)
#pragma unroll
    for (int j = i; j < 7; ++j) { a[m] = a[m] + (A[i] * A[j] + A[7 + i] * A[7 + j]); ++m; }
#pragma unroll
  for (int i = 0; i < 7; ++i) a[28 + i] = a[28 + i] + (A[i] * rs[0] + A[7 + i] * rs[1]);
}
// phase "factor", per free camera: the 6 x 6 pose block of U (damped) -> Uf [21 of 28]; per refining group: the damped d_g must be positive
BA_HD bool cam_factor_s(const CtxS& c, long i, double lambda) {
  if (!c.cam_free[i]) return true;
  double a[21], f[21];
  int m = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int k = r; k < 6; ++k) a[m++] = c.U[28 * i + idx7(r, k)];
  const bool ok = factor<6>(a, lambda, f);
#pragma unroll
  for (int k = 0; k < 21; ++k) c.Uf[28 * i + k] = f[k];
  return ok;
}
BA_HD bool group_factor(const CtxS& c, long g, double lambda) { return !c.group_focal[g] || damped(c.dg[g], lambda) > 0.0; }
// the vector of a live camera as the operator sees it: the pose part of a free camera, its group's value when it has cam_focal, else +0
BA_HD void cam_vec_s(const CtxS& c, long i, const double* vec, const double* vecg, double* v) {
  const bool fr = c.cam_free[i] != 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = fr ? vec[7 * i + k] : 0.0;
  v[6] = c.cam_focal[i] ? vecg[c.cam_group[i]] : 0.0;
}
// phase "track half", per track: track_half of the live cameras, with (vec, vecg) the camera and group halves of the vector
BA_HD bool track_half_s(const CtxS& c, int buf, long t, int mode, const double* vec, const double* vecg) {
  if (!c.point_active[t]) return true;
  double s[3] = {0.0, 0.0, 0.0}, z[3];
  if (mode != 0)
    for (long o = c.offsets[t]; o < c.offsets[t + 1]; ++o) {
      const int im = c.image[o];
      if (!c.obs_active[o] || !live(c, im)) continue;
      double A[14], B[6], rs[2], v[7];
      obs_terms_s(c, buf, o, t, A, B, rs);
      cam_vec_s(c, im, vec, vecg, v);
      const double eu = dotm<7>(A, v), ev = dotm<7>(A + 7, v);
      for (int k = 0; k < 3; ++k) s[k] = s[k] + (B[k] * eu + B[3 + k] * ev);
    }
  if (mode == 0) for (int k = 0; k < 3; ++k) s[k] = c.gp[3 * t + k];
  if (mode == 2) for (int k = 0; k < 3; ++k) s[k] = -(c.gp[3 * t + k] + s[k]);
  solve<3>(c.Vf + 6 * t, s, z);
  if (mode != 2) {
    for (int k = 0; k < 3; ++k) c.z[3 * t + k] = z[k];
    return true;
  }
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const double x = X_of(c, buf, t)[k] + z[k];
    X_of(c, 1 - buf, t)[k] = x;
    ok = ok && fin(x);
  }
  return ok;
}
// phase "camera half", one element of a live camera's osum64: a [7] += A^T (B z_j)
BA_HD void cam_half_term_s(const CtxS& c, int buf, long o, double* a) {
  double A[14], B[6], rs[2];
  const long t = c.obs_track[o];
  obs_terms_s(c, buf, o, t, A, B, rs);
  const double* z = c.z + 3 * t;
  const double eu = (B[0] * z[0] + B[1] * z[1]) + B[2] * z[2], ev = (B[3] * z[0] + B[4] * z[1]) + B[5] * z[2];
#pragma unroll
  for (int k = 0; k < 7; ++k) a[k] = a[k] + (A[k] * eu + A[7 + k] * ev);
}
// ... and what follows the sum a [7] of camera i.  mode 0: b = -(gc - a); a free camera starts its pose part (x = 0, r = b, zc = M^-1 r,
// p = zc, part = r . zc over 6 terms), a member with cam_focal leaves b_7 in Sp[6] for its group.  mode 1: rows 0..5 of U7d p - a for a
// free camera (part = p . Sp over 6 terms); for a member with cam_focal Sp[6] = sum_{k<6} U_k7 p_k - a_7: the group's own diagonal term
// is added once, at the group.  A camera that is not free has part = +0.
BA_HD void cam_half_finish_s(const CtxS& c, long i, int mode, double lambda, const double* a) {
  const bool fr = c.cam_free[i] != 0, fo = c.cam_focal[i] != 0;
  if (!fr) c.part[i] = 0.0;
  if (!fr && !fo) return;
  double *x = c.x + 7 * i, *r = c.r + 7 * i, *zc = c.zc + 7 * i, *p = c.p + 7 * i, *Sp = c.Sp + 7 * i;
  if (mode == 0) {
    double b[7], zz[6];
#pragma unroll
    for (int k = 0; k < 7; ++k) b[k] = -(c.gc[7 * i + k] - a[k]);
    if (fr) {
#pragma unroll
      for (int k = 0; k < 6; ++k) { x[k] = 0.0; r[k] = b[k]; }
      solve<6>(c.Uf + 28 * i, b, zz);
#pragma unroll
      for (int k = 0; k < 6; ++k) { zc[k] = zz[k]; p[k] = zz[k]; }
      c.part[i] = dotm<6>(b, zz);
    }
    if (fo) Sp[6] = b[6];
    return;
  }
  const double* U = c.U + 28 * i;
  double pv[7], sp[6];
  cam_vec_s(c, i, c.p, c.pg, pv);
  if (fr) {
#pragma unroll
    for (int row = 0; row < 6; ++row) {
      double s = 0.0;
#pragma unroll
      for (int col = 0; col < 7; ++col) {
        const int lo = row < col ? row : col, hi = row < col ? col : row;
        const double u = U[idx7(lo, hi)];
        s = s + (row == col ? damped(u, lambda) : u) * pv[col];
      }
      sp[row] = s - a[row];
      Sp[row] = sp[row];
    }
    c.part[i] = dotm<6>(pv, sp);
  }
  if (fo) {
    double s = 0.0;
#pragma unroll
    for (int col = 0; col < 6; ++col) s = s + U[idx7(col, 6)] * pv[col];
    Sp[6] = s - a[6];
  }
}
// one element of a group's osum64: member i adds v[i] when it has cam_focal (U77 for d_g, Sp[6] for E^T)
BA_HD void group_term(const CtxS& c, long i, const double* v, long stride, double* a) {
  if (c.cam_focal[i]) a[0] = a[0] + v[stride * i];
}
// ... and what follows the sum s of group g.  mode 0: b_g = s; x = 0, r = b, z = r / d, p = z, partg = r z.  mode 1: Sp = d p + s,
// partg = p Sp (d: the damped d_g).  A group that does not refine has partg = +0.
BA_HD void group_half_finish(const CtxS& c, long g, int mode, double lambda, double s) {
  if (!c.group_focal[g]) { c.partg[g] = 0.0; return; }
  const double d = damped(c.dg[g], lambda);
  if (mode == 0) {
    const double z = s / d;
    c.xg[g] = 0.0; c.rg[g] = s; c.zg[g] = z; c.pg[g] = z;
    c.partg[g] = s * z;
    return;
  }
  const double sp = d * c.pg[g] + s;
  c.Spg[g] = sp;
  c.partg[g] = c.pg[g] * sp;
}
// phase "update 1" / "update 2" of the pose part of a free camera and of a refining group
BA_HD void cam_update1_s(const CtxS& c, long i, double alpha) {
  if (!c.cam_free[i]) { c.part[i] = 0.0; return; }
  double r[6], zz[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    c.x[7 * i + k] = c.x[7 * i + k] + alpha * c.p[7 * i + k];
    r[k] = c.r[7 * i + k] - alpha * c.Sp[7 * i + k];
    c.r[7 * i + k] = r[k];
  }
  solve<6>(c.Uf + 28 * i, r, zz);
#pragma unroll
  for (int k = 0; k < 6; ++k) c.zc[7 * i + k] = zz[k];
  c.part[i] = dotm<6>(r, zz);
}
BA_HD void cam_update2_s(const CtxS& c, long i, double beta) {
  if (!c.cam_free[i]) return;
  for (int k = 0; k < 6; ++k) c.p[7 * i + k] = c.zc[7 * i + k] + beta * c.p[7 * i + k];
}
BA_HD void group_update1(const CtxS& c, long g, double alpha, double lambda) {
  if (!c.group_focal[g]) { c.partg[g] = 0.0; return; }
  c.xg[g] = c.xg[g] + alpha * c.pg[g];
  const double r = c.rg[g] - alpha * c.Spg[g], z = r / damped(c.dg[g], lambda);
  c.rg[g] = r; c.zg[g] = z;
  c.partg[g] = r * z;
}
BA_HD void group_update2(const CtxS& c, long g, double beta) {
  if (c.group_focal[g]) c.pg[g] = c.zg[g] + beta * c.pg[g];
}
// phase "apply", per refining group: the factor of the trial s' = s (1 + delta_g).  Per live camera: cam_apply's pose step for a free
// camera; for one with cam_focal fx' = fx_in s', skew' = skew_in s', fy' = fy_in s' (the camera forms s' itself, from the same two
// operands), so that the members of a group leave with ONE factor on their input values however many trials were accepted.
BA_HD void group_apply(const CtxS& c, int buf, long g) {
  if (c.group_focal[g]) *sg_of(c, 1 - buf, g) = *sg_of(c, buf, g) * (1.0 + c.xg[g]);
}
BA_HD bool cam_apply_s(const CtxS& c, int buf, long i) {
  bool ok = true;
  const double* tab = tab_of(c, buf, i);
  double* tab2 = tab_of(c, 1 - buf, i);
  if (c.cam_free[i]) {
    const double *d = c.x + 7 * i, *q = quat_of(c, buf, i);
    double* q2 = quat_of(c, 1 - buf, i);
    const double a = 0.5 * d[0], b = 0.5 * d[1], e = 0.5 * d[2];
    double w = ((q[0] - a * q[1]) - b * q[2]) - e * q[3];
    double x = ((q[1] + a * q[0]) + b * q[3]) - e * q[2];
    double y = ((q[2] - a * q[3]) + b * q[0]) + e * q[1];
    double z = ((q[3] + a * q[2]) - b * q[1]) + e * q[0];
    const double nq = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / nq; x = x / nq; y = y / nq; z = z / nq;
    q2[0] = w; q2[1] = x; q2[2] = y; q2[3] = z;
    double R[9];
    matrix_from_quat(q2, R);
    ok = fin(w) && fin(x) && fin(y) && fin(z);
    for (int k = 0; k < 9; ++k) tab2[k] = R[k];
    for (int k = 0; k < 3; ++k) {
      tab2[9 + k] = tab[9 + k] + d[3 + k];
      ok = ok && fin(tab2[9 + k]);
    }
  }
  if (c.cam_focal[i]) {
    const long g = c.cam_group[i];
    const double s = *sg_of(c, buf, g) * (1.0 + c.xg[g]);
    const double fx = c.K[9 * i] * s, sk = c.K[9 * i + 1] * s, fy = c.K[9 * i + 4] * s;
    tab2[12] = fx; tab2[13] = sk; tab2[15] = fy;
    const double rx = fx / c.K[9 * i], ry = fy / c.K[9 * i + 4];
    ok = ok && fin(fx) && fin(fy) && rx > c.focal_lo && rx < c.focal_hi && ry > c.focal_lo && ry < c.focal_hi;
  }
  return ok;
}
// phase "write": the pose of a free camera, the intrinsics of one with cam_focal; counts[14] = the groups that refine
BA_HD void cam_write_s(const CtxS& c, int buf, long i) {
  const double* tab = tab_of(c, buf, i);
  if (c.cam_free[i]) {
    double* T = c.T_out + 16 * i;
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) T[4 * r + k] = tab[3 * r + k];
      T[4 * r + 3] = tab[9 + r];
    }
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
  }
  if (c.cam_focal[i]) {
    double* K = c.K_out + 9 * i;
    K[0] = tab[12]; K[1] = tab[13]; K[2] = tab[14]; K[4] = tab[15]; K[5] = tab[16];
  }
}
BA_HD void ctrl_write_s(const CtxS& c) {
  ctrl_write<7>(c);
  c.counts[14] = c.cs->n_groups;
}

}  // namespace ba
