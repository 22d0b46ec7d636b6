// Global positioning (camera centres, points and one scale per observation from fixed rotations): what the host routine (position.hip)
// and the kernels (position_gpu.hip) share.  fp64, `+ - * /` and sqrt only, no contraction, compiled from this one text for both
// sides, so host and device take identical decisions and produce identical bits.  The rule is stated in include/loftr_global.h and
// DESIGN §27:
//   * the checks of a track, of an image's list, of the root and of a tree edge, and the error bits a failed check raises;
//   * one tree edge of one level of the start values, and the two passes that decide whether the tree is one;
//   * the bearing of an observation; which points, observations and cameras take part; the start value of a point and of a scale;
//   * the per-observation, per-point and per-camera steps of a Levenberg-Marquardt trial (the term of one observation in a camera's
//     sums; what the camera does with the finished sums), and what the owner of the scalars does when a sum arrives (feed, accept);
//   * the outputs of an observation, a point and a camera.
// A step is written for ONE item and reads only what an earlier phase wrote; the two sides differ only in how items are spread.
#pragma once
#include "../../include/loftr_global.h"
#include "bundle_core.h"

#pragma clang fp contract(off)

#define POS_HD __host__ __device__ inline

namespace pos {

constexpr int kCounts = 16;
constexpr int kInfo = 4;
constexpr int kChunk = ba::kChunk;          // osum: osum64 per chunk of 4096, then osum of the chunk sums (§18)
enum Count { kTrials = 0, kErrors = 1, kAccepted = 2, kPcgIters = 3, kActiveObs = 4, kActivePoints = 5, kFree = 6, kNegative = 7,
             kNoDirection = 8, kStatus = 9, kDepth = 10, kInGraph = 11, kChained = 12 };
enum : int { kBadImage = 1, kBadOffsets = 2, kBadGroups = 4, kBadRoot = 8, kBadTree = 16 };                     // error bits (counts[1])
enum CamState : uint8_t { kOutside = 0, kChainedOnly = 1, kSolved = 2, kRootCam = 3 };
enum : int { kConverged = 0, kMaxIters = 1, kStalled = 2, kNothing = 3 };
enum : int { kActCost0 = 0, kActRz0, kActPsp, kActRz, kActCostT };                                             // what a finished osum feeds
constexpr int kSetupSums = 10;              // a camera's sums of the set-up: M (6), sum w d^2, the right-hand side (3)
constexpr int kSpSums = 3;                  // ... and of one product S p

// what one thread owns: damping, flags, counters and the scalars of the conjugate gradients
struct Ctrl {
  int done, bad, pcg_done, status, n_trials, n_accepted, accepted_now, depth;
  long long n_pcg;
  unsigned long long step_bits;
  double lambda, cost, cost_t, cost0, rz, rz0, alpha, beta, last_step;
};

// the problem, its outputs and the workspace (layout below)
struct P {
  const long* offsets; long T; const int* image; const float* xy; long N; const long* cam_offsets; const int* cam_obs;
  const double* K; const double* R; const uint8_t* in_graph; int n, root;
  const int* tree_image; const double* tree_t; long Et;
  double huber, pcg_tol2, ftol;
  int max_iters, pcg_iters, min_cam_obs;
  double* centres; float* xyz; double* depth_scale; uint8_t* obs_state; uint8_t* cam_state; uint8_t* point_active;
  unsigned long long* counts; double* info;
  Ctrl* ctrl;
  double *v, *d, *dt, *wd2, *den, *e, *g, *er;                    // per observation: v, e, g [N,3]; the others [N]
  double *X, *Xt, *Ainv, *y, *u;                                  // per point: X, Xt, y, u [T,3]; Ainv [T,6]
  double *c, *ct, *M, *Minv, *x, *rr, *z, *pp, *Sp;               // per camera: M, Minv [n,6]; the others [n,3]
  double *gamma, *part, *red;                                     // gamma [Et,3]
  int *obs_track, *depth, *claim;
  uint8_t *usable, *active, *cstate, *nodir;                      // usable, active [N]; cstate [n]; nodir [Et]
};

POS_HD long chunks_of(long count) { return count > 0 ? (count + kChunk - 1) / kChunk : 1; }
POS_HD long part_items(long N, int n) { return N > 3L * n ? N : 3L * n; }
POS_HD bool sizes_ok(long T, long N, int n, long Et) { return tracks::sizes_ok(T, N, n) && n <= 0x3FFFFFFF && Et >= 0 && Et < (1L << 31); }

// carves the workspace; base == nullptr only measures
inline size_t layout(P& p, char* base) {
  size_t o = 0;
  const size_t N = (size_t)(p.N > 0 ? p.N : 1), T = (size_t)(p.T > 0 ? p.T : 1), n = (size_t)(p.n > 0 ? p.n : 1),
               Et = (size_t)(p.Et > 0 ? p.Et : 1), items = (size_t)part_items(p.N, p.n);
  auto take = [&](auto** ptr, size_t bytes) {
    const size_t at = tracks::carve(&o, bytes);
    if (base) *ptr = (std::remove_reference_t<decltype(*ptr)>)(base + at);
  };
  take(&p.ctrl, sizeof(Ctrl));
  take(&p.v, 8 * 3 * N); take(&p.d, 8 * N); take(&p.dt, 8 * N); take(&p.wd2, 8 * N); take(&p.den, 8 * N);
  take(&p.e, 8 * 3 * N); take(&p.g, 8 * 3 * N); take(&p.er, 8 * N);
  take(&p.X, 8 * 3 * T); take(&p.Xt, 8 * 3 * T); take(&p.Ainv, 8 * 6 * T); take(&p.y, 8 * 3 * T); take(&p.u, 8 * 3 * T);
  take(&p.c, 8 * 3 * n); take(&p.ct, 8 * 3 * n); take(&p.M, 8 * 6 * n); take(&p.Minv, 8 * 6 * n);
  take(&p.x, 8 * 3 * n); take(&p.rr, 8 * 3 * n); take(&p.z, 8 * 3 * n); take(&p.pp, 8 * 3 * n); take(&p.Sp, 8 * 3 * n);
  take(&p.gamma, 8 * 3 * Et);
  take(&p.part, 8 * (items > 0 ? items : 1));
  take(&p.red, 8 * 2 * (size_t)chunks_of((long)items));
  take(&p.obs_track, 4 * N); take(&p.depth, 4 * n); take(&p.claim, 4 * n);
  take(&p.usable, N); take(&p.active, N); take(&p.cstate, n); take(&p.nodir, Et);
  return o;
}

POS_HD double nan64() { return __builtin_nan(""); }
POS_HD unsigned long long bits_of(double v) { unsigned long long b; __builtin_memcpy(&b, &v, 8); return b; }
POS_HD double double_of(unsigned long long b) { double v; __builtin_memcpy(&v, &b, 8); return v; }
POS_HD bool fin3(const double* a) { return ba::fin(a[0]) && ba::fin(a[1]) && ba::fin(a[2]); }
POS_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// a maximum that several items may raise at once (the only kind of atomic the stage needs besides flags and counters)
POS_HD void raise_max(int* at, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(at, v);
#else
  if (*at < v) *at = v;
#endif
}

// §18's damping of a diagonal entry, as what is ADDED to it
POS_HD double damp_add(double a, double lambda) { return a == 0.0 ? lambda : a * lambda; }
// the inverse of the symmetric 3 x 3 matrix m (00 01 02 11 12 22) through its adjugate -> false unless its determinant is positive and finite
POS_HD bool inverse_sym3(const double* m, double* o) {
  const double c00 = m[3] * m[5] - m[4] * m[4], c01 = m[2] * m[4] - m[1] * m[5], c02 = m[1] * m[4] - m[2] * m[3];
  const double c11 = m[0] * m[5] - m[2] * m[2], c12 = m[1] * m[2] - m[0] * m[4], c22 = m[0] * m[3] - m[1] * m[1];
  const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
  const bool ok = det > 0.0 && ba::fin(det);
  const double s = ok ? det : 1.0;
  o[0] = c00 / s; o[1] = c01 / s; o[2] = c02 / s; o[3] = c11 / s; o[4] = c12 / s; o[5] = c22 / s;
  return ok;
}
POS_HD void mul_sym3(const double* m, const double* a, double* o) {
  o[0] = (m[0] * a[0] + m[1] * a[1]) + m[2] * a[2];
  o[1] = (m[1] * a[0] + m[3] * a[1]) + m[4] * a[2];
  o[2] = (m[2] * a[0] + m[4] * a[1]) + m[5] * a[2];
}

// ---- rule 1: checks ---------------------------------------------------------------------------------------------------------------------
// the error bits of track t; obs_track of its observations
POS_HD int track_check(const P& p, long t) {
  long b, e;
  if (!tracks::span(p.offsets, p.T, p.N, t, &b, &e)) return kBadOffsets;
  for (long o = b; o < e; ++o) p.obs_track[o] = (int)t;
  return tracks::images_ok(p.image, b, e, p.n) ? 0 : kBadImage;
}
// the error bits of image i's list; i == 0 also answers for the root.  Resets what the levels write.
POS_HD int cam_check(const P& p, int i) {
  int err = 0;
  if (i == 0 && (p.root < 0 || p.root >= p.n || !p.in_graph[p.root])) err |= kBadRoot;
  p.depth[i] = -1;
  p.claim[i] = 0;
  for (int k = 0; k < 3; ++k) p.c[3L * i + k] = 0.0;
  long b, e;
  if (!tracks::span(p.cam_offsets, p.n, p.N, i, &b, &e)) return err | kBadGroups;
  for (long k = b; k < e; ++k) {
    int o;
    if (tracks::group_slot(p.cam_obs, p.image, p.N, i, b, k, &o)) return err | kBadGroups;
  }
  return err;
}
// the error bits of tree edge e; its direction gamma = -R_b^T t / |t| (rule 4)
POS_HD int tree_check(const P& p, long e) {
  const int a = p.tree_image[2 * e], b = p.tree_image[2 * e + 1];
  double* gm = p.gamma + 3 * e;
  gm[0] = 0.0; gm[1] = 0.0; gm[2] = 0.0;
  p.nodir[e] = 1;
  if (a < 0 || a >= p.n || b < 0 || b >= p.n || a == b) return kBadTree;
  if (!p.in_graph[a] || !p.in_graph[b]) return kBadTree;
  const double* t = p.tree_t + 3 * e;
  const double* Rb = p.R + 9L * b;
  const double nt = sqrt(dot3(t, t));
  if (!fin3(t) || !ba::fin(nt) || !(nt > 0.0)) return 0;
  double g[3];
  for (int k = 0; k < 3; ++k) g[k] = -(((Rb[k] * t[0] + Rb[3 + k] * t[1]) + Rb[6 + k] * t[2]) / nt);
  if (!fin3(g)) return 0;
  gm[0] = g[0]; gm[1] = g[1]; gm[2] = g[2];
  p.nodir[e] = 0;
  return 0;
}

// ---- rule 4: start values of the cameras ------------------------------------------------------------------------------------------------
POS_HD void root_setup(const P& p) { p.depth[p.root] = 0; }
// tree edge e at level L: when one end was set at level L - 1 and the other is not set, the other takes its value -> 1, else 0
POS_HD int start_tree_edge(const P& p, long e, int L) {
  const int a = p.tree_image[2 * e], b = p.tree_image[2 * e + 1];
  const int da = p.depth[a], db = p.depth[b];
  const double* gm = p.gamma + 3 * e;
  if (da == L - 1 && db < 0) {
    for (int k = 0; k < 3; ++k) p.c[3L * b + k] = p.c[3L * a + k] + gm[k];
    p.depth[b] = L;
    return 1;
  }
  if (db == L - 1 && da < 0) {
    for (int k = 0; k < 3; ++k) p.c[3L * a + k] = p.c[3L * b + k] - gm[k];
    p.depth[a] = L;
    return 1;
  }
  return 0;
}
// after the last level: the deeper end of edge e, or -1 when its ends are not two reached images at adjacent levels
POS_HD int tree_child(const P& p, long e) {
  const int a = p.tree_image[2 * e], b = p.tree_image[2 * e + 1];
  const int da = p.depth[a], db = p.depth[b];
  if (da < 0 || db < 0) return -1;
  return db == da + 1 ? b : (da == db + 1 ? a : -1);
}
// ... first pass: the edge claims its deeper end -> its error bits
POS_HD int tree_claim(const P& p, long e) {
  const int ch = tree_child(p, e);
  if (ch < 0) return kBadTree;
  raise_max(p.claim + ch, (int)e + 1);
  return 0;
}
// ... second pass: no other edge claimed it
POS_HD int tree_verify(const P& p, long e) {
  const int ch = tree_child(p, e);
  return ch >= 0 && p.claim[ch] == (int)e + 1 ? 0 : kBadTree;
}
POS_HD bool cam_in_graph(const P& p, int i) { return p.in_graph[i] && p.depth[i] >= 0; }

// ---- rule 2: bearings; who takes part -----------------------------------------------------------------------------------------------------
// observation o: its bearing, whether it is usable
POS_HD void obs_bearing(const P& p, long o) {
  const int i = p.image[o];
  double* v = p.v + 3 * o;
  v[0] = 0.0; v[1] = 0.0; v[2] = 0.0;
  p.usable[o] = 0;
  p.active[o] = 0;
  p.d[o] = 0.0; p.dt[o] = 0.0;
  const double x = (double)p.xy[2 * o], y = (double)p.xy[2 * o + 1];
  if (!cam_in_graph(p, i) || !ba::fin(x) || !ba::fin(y)) return;
  const double* K = p.K + 9L * i;
  const double* R = p.R + 9L * i;
  const double rz = 1.0 / K[8], ry = (y - K[5] * rz) / K[4], rx = ((x - K[1] * ry) - K[2] * rz) / K[0];
  double w[3];
  for (int k = 0; k < 3; ++k) w[k] = (R[k] * rx + R[3 + k] * ry) + R[6 + k] * rz;
  const double nw = sqrt(dot3(w, w));
  w[0] = w[0] / nw; w[1] = w[1] / nw; w[2] = w[2] / nw;
  if (!fin3(w)) return;
  v[0] = w[0]; v[1] = w[1]; v[2] = w[2];
  p.usable[o] = 1;
}
// point t: active iff at least 2 usable observations; its observations' activity -> the number of active observations
POS_HD long track_setup(const P& p, long t) {
  long cnt = 0;
  for (long o = p.offsets[t]; o < p.offsets[t + 1]; ++o) cnt += p.usable[o];
  const bool act = cnt >= 2;
  p.point_active[t] = (uint8_t)act;
  for (long o = p.offsets[t]; o < p.offsets[t + 1]; ++o) p.active[o] = (uint8_t)(act && p.usable[o]);
  return act ? cnt : 0;
}
// rule 3: the state of camera i (after track_setup of every point)
POS_HD int cam_setup(const P& p, int i) {
  int st = kOutside;
  if (cam_in_graph(p, i)) {
    long cnt = 0;
    for (long k = p.cam_offsets[i]; k < p.cam_offsets[i + 1]; ++k) cnt += p.active[p.cam_obs[k]];
    st = i == p.root ? kRootCam : (cnt >= p.min_cam_obs ? kSolved : kChainedOnly);
  }
  p.cstate[i] = (uint8_t)st;
  for (int k = 0; k < 3; ++k) p.ct[3L * i + k] = p.c[3L * i + k];
  return st;
}
POS_HD bool cam_free(const P& p, int i) { return p.cstate[i] == kSolved; }
// rule 4: the start value of point t and of its observations' scales
POS_HD void point_start(const P& p, long t) {
  double s[3] = {0.0, 0.0, 0.0}, cnt = 0.0;
  double* X = p.X + 3 * t;
  for (long o = p.offsets[t]; o < p.offsets[t + 1]; ++o) {
    if (!p.active[o]) continue;
    const double* c = p.c + 3L * p.image[o];
    for (int k = 0; k < 3; ++k) s[k] = s[k] + (c[k] + p.v[3 * o + k]);
    cnt = cnt + 1.0;
  }
  for (int k = 0; k < 3; ++k) { X[k] = cnt > 0.0 ? s[k] / cnt : 0.0; p.Xt[3 * t + k] = X[k]; }
  for (long o = p.offsets[t]; o < p.offsets[t + 1]; ++o) {
    if (!p.active[o]) continue;
    const double* c = p.c + 3L * p.image[o];
    const double e[3] = {X[0] - c[0], X[1] - c[1], X[2] - c[2]};
    const double ee = dot3(e, e);
    p.d[o] = ee == 0.0 ? 0.0 : dot3(p.v + 3 * o, e) / ee;
    p.dt[o] = p.d[o];
  }
}

// ---- rule 5: one trial ------------------------------------------------------------------------------------------------------------------
// e = X - c, r = v - d e, the Huber weight and the cost term of observation o at (c, X, d) -> the cost term
POS_HD double obs_residual(const P& p, long o, const double* c, const double* X, const double* d, double* e, double* r, double* w) {
  const double* ci = c + 3L * p.image[o];
  const double* Xk = X + 3L * p.obs_track[o];
  for (int k = 0; k < 3; ++k) { e[k] = Xk[k] - ci[k]; r[k] = p.v[3 * o + k] - d[o] * e[k]; }
  const double sq = dot3(r, r), nr = sqrt(sq);
  if (p.huber > 0.0 && !(nr <= p.huber)) { *w = p.huber / nr; return (2.0 * p.huber) * nr - p.huber * p.huber; }
  *w = 1.0;
  return sq;
}
// the cost term of observation o at the state (trial == 0) or at the trial -> part
POS_HD void obs_eval(const P& p, long o, int trial) {
  double e[3], r[3], w, cost = 0.0;
  if (p.active[o]) cost = trial ? obs_residual(p, o, p.ct, p.Xt, p.dt, e, r, &w) : obs_residual(p, o, p.c, p.X, p.d, e, r, &w);
  p.part[o] = cost;
}
// observation o at the state: what the elimination of d_o leaves (w d^2, den, e, g, e.r)
POS_HD void obs_linearise(const P& p, long o) {
  double e[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0}, wd2 = 0.0, den = 1.0, er = 0.0;
  if (p.active[o]) {
    double r[3], w;
    obs_residual(p, o, p.c, p.X, p.d, e, r, &w);
    const double d = p.d[o], ee = dot3(e, e);
    wd2 = w * (d * d);
    den = ba::damped(ee, p.ctrl->lambda);                              // (e.e (1 + lambda), or lambda when e.e is 0: §18's damping)
    er = dot3(e, r);
    const double q = er / den, wd = w * d;
    for (int k = 0; k < 3; ++k) g[k] = wd * (r[k] - e[k] * q);
  }
  p.wd2[o] = wd2; p.den[o] = den; p.er[o] = er;
  for (int k = 0; k < 3; ++k) { p.e[3 * o + k] = e[k]; p.g[3 * o + k] = g[k]; }
}
// W_o a
POS_HD void obs_W(const P& p, long o, const double* a, double* out) {
  const double* e = p.e + 3 * o;
  const double q = dot3(e, a) / p.den[o];
  for (int k = 0; k < 3; ++k) out[k] = p.wd2[o] * (a[k] - e[k] * q);
}
// the six entries of W_o
POS_HD void obs_W6(const P& p, long o, double* m) {
  const double* e = p.e + 3 * o;
  const double wd2 = p.wd2[o], den = p.den[o];
  m[0] = wd2 * (1.0 - e[0] * e[0] / den); m[1] = wd2 * (0.0 - e[0] * e[1] / den); m[2] = wd2 * (0.0 - e[0] * e[2] / den);
  m[3] = wd2 * (1.0 - e[1] * e[1] / den); m[4] = wd2 * (0.0 - e[1] * e[2] / den); m[5] = wd2 * (1.0 - e[2] * e[2] / den);
}
// point t: A = sum W_o + damping, its inverse, y = A^-1 sum g_o -> false when A cannot be inverted
POS_HD bool point_factor(const P& p, long t) {
  double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0}, s = 0.0;
  double* y = p.y + 3 * t;
  y[0] = 0.0; y[1] = 0.0; y[2] = 0.0;
  if (!p.point_active[t]) return true;
  for (long o = p.offsets[t]; o < p.offsets[t + 1]; ++o) {
    double m[6];
    obs_W6(p, o, m);
    for (int k = 0; k < 6; ++k) A[k] = A[k] + m[k];
    for (int k = 0; k < 3; ++k) b[k] = b[k] + p.g[3 * o + k];
    s = s + p.wd2[o];
  }
  const double add = damp_add(s, p.ctrl->lambda);
  A[0] = A[0] + add; A[3] = A[3] + add; A[5] = A[5] + add;
  const bool ok = inverse_sym3(A, p.Ainv + 6 * t);
  mul_sym3(p.Ainv + 6 * t, b, y);
  return ok && fin3(y);
}
// point t: u = A^-1 sum W_o a_i over its observations, a = the cameras' vector src (p or x)
POS_HD void point_u(const P& p, long t, const double* src) {
  double s[3] = {0.0, 0.0, 0.0};
  double* u = p.u + 3 * t;
  if (p.point_active[t])
    for (long o = p.offsets[t]; o < p.offsets[t + 1]; ++o) {
      double w[3];
      obs_W(p, o, src + 3L * p.image[o], w);
      for (int k = 0; k < 3; ++k) s[k] = s[k] + w[k];
    }
  mul_sym3(p.Ainv + 6 * t, s, u);
  if (!p.point_active[t]) { u[0] = 0.0; u[1] = 0.0; u[2] = 0.0; }
}
// the term of observation o in its camera's set-up sums: W_o (6), w d^2, W_o y_k - g_o (3)
POS_HD void cam_term_setup(const P& p, long o, double* out) {
  double wy[3];
  obs_W6(p, o, out);
  out[6] = p.wd2[o];
  obs_W(p, o, p.y + 3L * p.obs_track[o], wy);
  for (int k = 0; k < 3; ++k) out[7 + k] = wy[k] - p.g[3 * o + k];
}
// camera i with its finished set-up sums: M, its inverse, and the conjugate gradients' start (x = 0, r = b, z = M^-1 r, p = z);
// part = r . z -> false when M cannot be inverted
POS_HD bool cam_finish_setup(const P& p, int i, const double* s) {
  const long j = 3L * i;
  bool ok = true;
  double z[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
  if (cam_free(p, i)) {
    double* M = p.M + 6L * i;
    const double add = damp_add(s[6], p.ctrl->lambda);
    for (int k = 0; k < 6; ++k) M[k] = s[k];
    M[0] = M[0] + add; M[3] = M[3] + add; M[5] = M[5] + add;
    ok = inverse_sym3(M, p.Minv + 6L * i);
    b[0] = s[7]; b[1] = s[8]; b[2] = s[9];
    mul_sym3(p.Minv + 6L * i, b, z);
    ok = ok && fin3(z);
  }
  for (int k = 0; k < 3; ++k) {
    p.x[j + k] = 0.0; p.rr[j + k] = b[k]; p.z[j + k] = z[k]; p.pp[j + k] = z[k]; p.Sp[j + k] = 0.0;
    p.part[j + k] = b[k] * z[k];
  }
  return ok;
}
// the term of observation o in its camera's sums of S p: W_o u_k
POS_HD void cam_term_Sp(const P& p, long o, double* out) { obs_W(p, o, p.u + 3L * p.obs_track[o], out); }
// camera i with the finished sums: (S p)_i = M_i p_i - sum; part = p . S p
POS_HD void cam_finish_Sp(const P& p, int i, const double* s) {
  const long j = 3L * i;
  double sp[3] = {0.0, 0.0, 0.0};
  if (cam_free(p, i)) {
    mul_sym3(p.M + 6L * i, p.pp + j, sp);
    for (int k = 0; k < 3; ++k) sp[k] = sp[k] - s[k];
  }
  for (int k = 0; k < 3; ++k) { p.Sp[j + k] = sp[k]; p.part[j + k] = p.pp[j + k] * sp[k]; }
}
// camera i: x += alpha p, r -= alpha S p, z = M^-1 r; part = r . z
POS_HD void cam_update(const P& p, int i) {
  const long j = 3L * i;
  if (!cam_free(p, i)) { p.part[j] = 0.0; p.part[j + 1] = 0.0; p.part[j + 2] = 0.0; return; }
  const double alpha = p.ctrl->alpha;
  for (int k = 0; k < 3; ++k) {
    p.x[j + k] = p.x[j + k] + alpha * p.pp[j + k];
    p.rr[j + k] = p.rr[j + k] - alpha * p.Sp[j + k];
  }
  mul_sym3(p.Minv + 6L * i, p.rr + j, p.z + j);
  for (int k = 0; k < 3; ++k) p.part[j + k] = p.rr[j + k] * p.z[j + k];
}
// camera i: p = z + beta p
POS_HD void cam_direction(const P& p, int i) {
  if (!cam_free(p, i)) return;
  const double beta = p.ctrl->beta;
  for (int k = 0; k < 3; ++k) p.pp[3L * i + k] = p.z[3L * i + k] + beta * p.pp[3L * i + k];
}
// camera i: the trial c + x -> |x|^2, or -1 for a step that is not finite
POS_HD double cam_apply(const P& p, int i) {
  const long j = 3L * i;
  if (!cam_free(p, i)) { for (int k = 0; k < 3; ++k) p.ct[j + k] = p.c[j + k]; return 0.0; }
  for (int k = 0; k < 3; ++k) p.ct[j + k] = p.c[j + k] + p.x[j + k];
  const double n2 = dot3(p.x + j, p.x + j);
  return ba::fin(n2) && fin3(p.ct + j) ? n2 : -1.0;
}
// point t (after point_u of x): the trial X + y + u -> false for a step that is not finite
POS_HD bool point_apply(const P& p, long t) {
  if (!p.point_active[t]) return true;
  for (int k = 0; k < 3; ++k) p.Xt[3 * t + k] = p.X[3 * t + k] + (p.y[3 * t + k] + p.u[3 * t + k]);
  return fin3(p.Xt + 3 * t);
}
// observation o (after cam_apply, point_apply): the trial d + (e.r - d e.(dX - dc)) / den -> false for a step that is not finite
POS_HD bool obs_apply(const P& p, long o) {
  if (!p.active[o]) return true;
  const long t = p.obs_track[o], j = 3L * p.image[o];
  const double dx[3] = {(p.y[3 * t] + p.u[3 * t]) - p.x[j], (p.y[3 * t + 1] + p.u[3 * t + 1]) - p.x[j + 1],
                        (p.y[3 * t + 2] + p.u[3 * t + 2]) - p.x[j + 2]};
  p.dt[o] = p.d[o] + (p.er[o] - p.d[o] * dot3(p.e + 3 * o, dx)) / p.den[o];
  return ba::fin(p.dt[o]);
}
// an accepted trial becomes the state
POS_HD bool commit_now(const P& p) { return p.ctrl->accepted_now != 0; }
POS_HD void cam_commit(const P& p, int i) { for (int k = 0; k < 3; ++k) p.c[3L * i + k] = p.ct[3L * i + k]; }
POS_HD void point_commit(const P& p, long t) { for (int k = 0; k < 3; ++k) p.X[3 * t + k] = p.Xt[3 * t + k]; }
POS_HD void obs_commit(const P& p, long o) { p.d[o] = p.dt[o]; }

// the owner of the scalars: its start, a finished sum, the end of a trial
POS_HD void ctrl_init(const P& p) {
  Ctrl& c = *p.ctrl;
  c.done = c.bad = c.pcg_done = c.n_trials = c.n_accepted = c.accepted_now = c.depth = 0;
  c.status = kMaxIters;
  c.n_pcg = 0;
  c.step_bits = 0;
  c.lambda = ba::kLambda0;
  c.cost = c.cost_t = c.cost0 = c.rz = c.rz0 = c.alpha = c.beta = c.last_step = 0.0;
}
POS_HD void feed(const P& p, int action, double v) {
  Ctrl& c = *p.ctrl;
  switch (action) {
    case kActCost0:
      c.cost = c.cost0 = v;
      if (p.counts[kActiveObs] == 0 || p.counts[kFree] == 0) { c.done = 1; c.status = kNothing; }
      else if (v == 0.0) { c.done = 1; c.status = kConverged; }             // nothing can lower a cost of exactly 0
      break;
    case kActRz0: c.rz = c.rz0 = v; if (!(v > 0.0)) c.pcg_done = 1; break;
    case kActPsp: c.alpha = c.rz / v; if (!(v > 0.0)) c.pcg_done = 1; else c.n_pcg += 1; break;
    case kActRz: c.beta = v / c.rz; c.rz = v; if (v <= p.pcg_tol2 * c.rz0) c.pcg_done = 1; break;
    case kActCostT: c.cost_t = v; break;
  }
}
POS_HD void accept(const P& p) {
  Ctrl& c = *p.ctrl;
  c.accepted_now = 0;
  if (c.done) return;
  c.n_trials += 1;
  if (!c.bad && c.cost_t < c.cost) {
    const double gain = c.cost - c.cost_t;
    c.cost = c.cost_t;
    c.n_accepted += 1;
    c.accepted_now = 1;
    c.last_step = sqrt(double_of(c.step_bits));
    c.lambda = c.lambda / 10.0 > ba::kLambdaMin ? c.lambda / 10.0 : ba::kLambdaMin;
    if (gain <= p.ftol * c.cost) { c.done = 1; c.status = kConverged; }
  } else {
    c.lambda = 10.0 * c.lambda;
    if (c.lambda > ba::kLambdaMax) { c.done = 1; c.status = kStalled; }
  }
  c.bad = 0;
  c.pcg_done = 0;
  c.step_bits = 0;
}
POS_HD bool refine_idle(const P& p) { return p.ctrl->done != 0; }
POS_HD bool pcg_idle(const P& p) { return p.ctrl->done != 0 || p.ctrl->pcg_done != 0; }

// ---- rule 7: outputs --------------------------------------------------------------------------------------------------------------------
// observation o -> 1 when it is active and ended with d <= 0
POS_HD int obs_write(const P& p, long o) {
  const bool act = p.active[o] != 0, neg = act && !(p.d[o] > 0.0);
  p.depth_scale[o] = act ? p.d[o] : 0.0;
  p.obs_state[o] = (uint8_t)(act ? (neg ? 2 : 1) : 0);
  return neg ? 1 : 0;
}
POS_HD void track_write(const P& p, long t) {
  for (int k = 0; k < 3; ++k) p.xyz[3 * t + k] = p.point_active[t] ? (float)p.X[3 * t + k] : (float)nan64();
}
POS_HD void cam_write(const P& p, int i) {
  p.cam_state[i] = p.cstate[i];
  for (int k = 0; k < 3; ++k) p.centres[3L * i + k] = p.cstate[i] != kOutside ? p.c[3L * i + k] : nan64();
}
// the counts and info the owner of the scalars holds
POS_HD void finish(const P& p) {
  const Ctrl& c = *p.ctrl;
  p.counts[kTrials] = (unsigned long long)c.n_trials;
  p.counts[kAccepted] = (unsigned long long)c.n_accepted;
  p.counts[kPcgIters] = (unsigned long long)c.n_pcg;
  p.counts[kStatus] = (unsigned long long)c.status;
  p.counts[kDepth] = (unsigned long long)c.depth;
  p.info[0] = c.cost0; p.info[1] = c.cost; p.info[2] = c.lambda; p.info[3] = c.last_step;
}

// ---- arguments --------------------------------------------------------------------------------------------------------------------------
struct Args {
  const long* offsets; long T; const int* obs_image; const float* obs_xy; long N; const long* cam_offsets; const int* cam_obs;
  const double* K; const double* R; const uint8_t* in_graph; int n_images, root; const int* tree_image; const double* tree_t; long Et;
  double huber; int max_iters, pcg_iters; double pcg_tol, ftol; int min_cam_obs;
  double* centres; float* xyz; double* depth_scale; uint8_t* obs_state; uint8_t* cam_state; uint8_t* point_active; long* counts;
  double* info;
};
inline int check_args(const Args& a) {
  if (!a.counts || !a.info || a.T < 0 || a.N < 0 || a.Et < 0 || a.n_images < 1 || !a.offsets || !a.cam_offsets || !a.K || !a.R ||
      !a.in_graph || !a.centres || !a.cam_state || (a.T == 0 && a.N > 0))
    return LOFTR_ERR_BAD_ARG;
  if (a.N > 0 && (!a.obs_image || !a.obs_xy || !a.cam_obs || !a.depth_scale || !a.obs_state)) return LOFTR_ERR_BAD_ARG;
  if (a.T > 0 && (!a.xyz || !a.point_active)) return LOFTR_ERR_BAD_ARG;
  if (a.Et > 0 && (!a.tree_image || !a.tree_t)) return LOFTR_ERR_BAD_ARG;
  if (!ba::fin(a.huber) || !(a.huber >= 0.0) || !(a.pcg_tol >= 0.0) || !(a.pcg_tol < 1.0) || !ba::fin(a.ftol) || !(a.ftol >= 0.0) ||
      a.max_iters < 0 || a.pcg_iters < 0 || a.min_cam_obs < 0)
    return LOFTR_ERR_BAD_ARG;
  if (!sizes_ok(a.T, a.N, a.n_images, a.Et) || a.max_iters > (1 << 16) || a.pcg_iters > (1 << 16)) return LOFTR_ERR_UNSUPPORTED;
  return LOFTR_OK;
}
inline P problem(const Args& a) {
  P p{};
  p.offsets = a.offsets; p.T = a.T; p.image = a.obs_image; p.xy = a.obs_xy; p.N = a.N; p.cam_offsets = a.cam_offsets; p.cam_obs = a.cam_obs;
  p.K = a.K; p.R = a.R; p.in_graph = a.in_graph; p.n = a.n_images; p.root = a.root; p.tree_image = a.tree_image; p.tree_t = a.tree_t;
  p.Et = a.Et; p.huber = a.huber; p.pcg_tol2 = a.pcg_tol * a.pcg_tol; p.ftol = a.ftol; p.max_iters = a.max_iters;
  p.pcg_iters = a.pcg_iters; p.min_cam_obs = a.min_cam_obs;
  p.centres = a.centres; p.xyz = a.xyz; p.depth_scale = a.depth_scale; p.obs_state = a.obs_state; p.cam_state = a.cam_state;
  p.point_active = a.point_active; p.counts = (unsigned long long*)a.counts; p.info = a.info;
  return p;
}

}  // namespace pos
