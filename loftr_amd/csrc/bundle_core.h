// Bundle adjustment of the triangulated model: the arithmetic and the per-item steps shared by the host routine (bundle.hip) and the GPU
// kernels (bundle_gpu.hip).  As in triangulate_core.h, every function here is compiled for both sides from this one text, fp64, without
// FMA contraction, and uses + - * / and sqrt only (correctly rounded on both sides), so that host and device take identical decisions and
// produce identical bits.  The rule is stated in include/loftr_hip.h and DESIGN §18; the checks of the track table, its error bits and
// the carving step of the workspace are tracks_core.h's.
//
// The run is a sequence of PHASES; a phase is a loop over tracks, over cameras or one single step, and a phase boundary is the only
// ordering (a kernel boundary on the device, the end of a loop on the host).  Every per-item step below reads only what earlier phases
// wrote, so the result does not depend on how a phase is spread over threads.  Every test is written so that a NaN takes the safe side.
//
// A MODE IS A ROW OF TRAITS (Pose, Focal, Shared, Radial and PriorOf<> below): fixed intrinsics, one focal step per camera
// (§18.1), one per group of cameras (§18.2), a radial coefficient per group next to it (§18.4), each with or without position priors
// on the camera centres (§18.3).  Every step that differs between modes is ONE name, a template on the mode, and decides what differs
// with `if constexpr` on a trait; no mode is reached through another "with a zero column", so each performs exactly its own operations
// and reads only its own arrays.  Where two modes take genuinely different arithmetic for a step (Shared's scalar group step against
// Radial's 2 x 2 one; the pinhole against the distorted projection) the two texts stand side by side inside the one template, never
// merged: the rounding of each is part of the result.  The argument superset of the entry points (Args), the context fill by traits,
// the one list of modes (with_mode) and the argument checks are at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/loftr_hip.h"
#include "tracks_core.h"

#pragma clang fp contract(off)

#define BA_HD __host__ __device__ inline

namespace ba {

constexpr int kCounts = 16;                // counts[]: see include/loftr_hip.h
constexpr int kCountsPrior = 24;           // ... of the entry points with position priors (§18.3): 16..20 are the prior's
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
  double *U, *gc, *Uf;                      // [n][21] sum A^T A, [n][6] sum A^T r, [n][21] factor of the damped U  (28, 7, 28 when S = 7)
  double *x, *r, *zc, *p, *Sp;              // [n][S] each: conjugate gradients over the cameras
  double *part, *part2, *red;               // [max(T, n)] x 2 terms of an osum, [2][ceil(max / 4096)] its chunk sums
  int* obs_track;                           // [N]
  uint8_t* cam_valid;                       // [n]
  Ctrl* ctrl;
};

// §18.1, focal refinement: the camera block is 7 wide (the seventh parameter is the relative focal step) and the problem carries the
// extra inputs and outputs.
struct Ctx7 : Ctx {
  const uint8_t* refine_focal; int min_focal_obs; double focal_lo, focal_hi;
  double* K_out; uint8_t* cam_focal;
};
// §18.2, one relative focal step per GROUP of cameras.  The unknowns are 6 per free camera and 1 per refining group; the system is
// E^T S7 E x = E^T b7, E copying a group's value into the seventh slot of its members with cam_focal.  The camera vectors keep §18.1's
// stride of 7: entries 0..5 are the pose part (read and written for a free camera only; +0 is used for any other), entry 6 of Sp is the
// camera's seventh entry BEFORE E^T (written for a member with cam_focal only), entry 6 of the others is unused.  The group vectors are
// [G].  A camera takes part when it is free or has cam_focal; the pose columns of A are +0 for a camera that is not free, the seventh
// is +0 for one without cam_focal.
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

// §18.4, one radial coefficient per group of cameras next to its focal step: x_d = x (1 + k r^2) on normalised coordinates.  The camera
// block is 8 wide (seventh the relative focal step, eighth the ADDITIVE radial step), the group carries two unknowns, focal first, and
// every group vector of CtxS holds two doubles per group ([G][2]; dg holds [n][3] the group's 2 x 2 block, then [n][3] its factor).  Only the Radial mode
// reads a k: no other mode is handed a zero coefficient.
struct CtrlR { int n_radial; };
struct CtxR : CtxS {
  const double* radial_in; const uint8_t* refine_radial; double radial_lo, radial_hi;
  double* radial_out; uint8_t *cam_radial, *group_radial;
  double* kr;                                     // [2][n]: a camera's k in the state and in the trial (ctrl->cur)
  double* ag;                                     // [2][n]: the radial step a group has taken so far, likewise
  CtrlR* cr;
};

// §18.3, position priors on the camera centres.  A prior couples no point, so it only adds to U, gc and the cost of its camera; what it
// needs is carried next to any of the three contexts, and only by the instantiations that have it.
struct CtrlP {
  double acc;                                // the tracks' sum of the cost, waiting for the cameras' (as CtrlS::acc waits for the groups')
  double pc0, pc, pc_t, sq0, sq, sq_t;       // sum of the prior shares / of |c - g|^2: at the start, of the state, of the trial
  unsigned long long n_prior;
};
struct Prior {
  const double *xyz, *sigma; const uint8_t* mask;   // [n,3], [n,3], [n]
  uint8_t* cam_prior;                               // [n]: the decision
  double *part, *part2;                             // [n] each: a camera's share of the cost, its |c - g|^2
  CtrlP* cp;
};
template <class Base> struct WithPrior : Base { Prior pr; };

// The MODES.  The sequence of phases (bundle.hip), the launch schedule (bundle_gpu.hip) and every per-item step that touches the
// camera block or the groups are written once, as templates on one of these: S is the stride of a camera's vectors and the width of its
// linearised block, W the width of what is factored, solved and updated per camera, kGroups whether the group phases exist, GW the
// unknowns per group (kTri<GW> the entries of a group's block).
// kPrior: whether the cameras carry position priors (§18.3); Base is the mode without them, whose kernels and steps serve every phase
// that the prior does not touch.
// kRadial: whether the projection is the distorted one of §18.4 and a group carries its radial step next to its focal step.
// A new mode supplies: its row here, its context (a struct that extends the one it builds on), its part of Args / fill / check_args /
// layout, its case in with_mode, its `if constexpr` branch in the steps that it changes, and a row of ops._BA_MODES.
struct Pose { static constexpr int S = 6, W = 6, GW = 1; static constexpr bool kGroups = false, kPrior = false, kRadial = false; using Ctx = ba::Ctx; using Base = Pose; };       // §18
struct Focal { static constexpr int S = 7, W = 7, GW = 1; static constexpr bool kGroups = false, kPrior = false, kRadial = false; using Ctx = ba::Ctx7; using Base = Focal; };    // §18.1
struct Shared { static constexpr int S = 7, W = 6, GW = 1; static constexpr bool kGroups = true, kPrior = false, kRadial = false; using Ctx = ba::CtxS; using Base = Shared; };   // §18.2
struct Radial { static constexpr int S = 8, W = 6, GW = 2; static constexpr bool kGroups = true, kPrior = false, kRadial = true; using Ctx = ba::CtxR; using Base = Radial; };    // §18.4
template <class M> struct PriorOf : M { static constexpr bool kPrior = true; using Ctx = WithPrior<typename M::Ctx>; using Base = M; };    // §18.3
using PoseP = PriorOf<Pose>;
using FocalP = PriorOf<Focal>;
using SharedP = PriorOf<Shared>;
template <int S> constexpr int kTri = S * (S + 1) / 2;      // entries of the upper triangle of a camera block: 21, 28 or 36
// the mode whose track steps (linearise, evaluate) a mode runs: they do not depend on the camera block, only on the projection
template <class Mode> using TrackMode = std::conditional_t<Mode::kRadial, Mode, Pose>;
// ... and whose camera setup it runs: that depends on what the camera carries (intrinsics to refine, a k), not on groups or priors
template <class Mode> using SetupMode = std::conditional_t<Mode::kRadial, Mode, std::conditional_t<Mode::S >= 7, Focal, Pose>>;
template <class Mode> BA_HD CtrlS* groups_ctrl(const typename Mode::Ctx& c) {
  if constexpr (Mode::kGroups) return c.cs;
  else return nullptr;
}

// carves the workspace; base may be null (then only the size counts) -> bytes.  What the groups add is sized by n (G <= n), so that the
// size does not depend on the grouping.
template <class Mode> inline size_t layout(typename Mode::Ctx& c, char* base) {
  constexpr int S = Mode::S;
  const size_t T = (size_t)c.T, n = (size_t)c.n, N = (size_t)c.N, m = (T > n ? T : n) + 1, ch = (m + kChunk - 1) / kChunk;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = tracks::carve(&off, bytes ? bytes : 1); return base ? base + at : nullptr; };
  c.ctrl = (Ctrl*)take(sizeof(Ctrl));
  c.tab = (double*)take(8 * 2 * n * kTab); c.quat = (double*)take(8 * 2 * n * 4); c.X = (double*)take(8 * 2 * T * 3);
  c.V = (double*)take(8 * T * 6); c.gp = (double*)take(8 * T * 3); c.Vf = (double*)take(8 * T * 6); c.z = (double*)take(8 * T * 3);
  c.U = (double*)take(8 * n * kTri<S>); c.gc = (double*)take(8 * n * S); c.Uf = (double*)take(8 * n * kTri<S>);
  c.x = (double*)take(8 * n * S); c.r = (double*)take(8 * n * S); c.zc = (double*)take(8 * n * S); c.p = (double*)take(8 * n * S);
  c.Sp = (double*)take(8 * n * S);
  c.part = (double*)take(8 * m); c.part2 = (double*)take(8 * m); c.red = (double*)take(8 * 2 * ch);
  c.obs_track = (int*)take(4 * N); c.cam_valid = (uint8_t*)take(n);
  if constexpr (Mode::kGroups) {
    constexpr size_t GW = Mode::GW, DW = Mode::kRadial ? 6 : 1;
    c.cs = (CtrlS*)take(sizeof(CtrlS));
    c.dg = (double*)take(8 * n * DW); c.xg = (double*)take(8 * n * GW); c.rg = (double*)take(8 * n * GW); c.zg = (double*)take(8 * n * GW);
    c.pg = (double*)take(8 * n * GW); c.Spg = (double*)take(8 * n * GW); c.partg = (double*)take(8 * n); c.sg = (double*)take(8 * 2 * n);
    c.cam_cnt = (int*)take(4 * n);
  }
  if constexpr (Mode::kRadial) {
    c.cr = (CtrlR*)take(sizeof(CtrlR));
    c.kr = (double*)take(8 * 2 * n); c.ag = (double*)take(8 * 2 * n);
  }
  if constexpr (Mode::kPrior) {
    c.pr.cp = (CtrlP*)take(sizeof(CtrlP));
    c.pr.part = (double*)take(8 * n); c.pr.part2 = (double*)take(8 * n);
  }
  return off;
}
template <class Mode> inline size_t workspace_bytes(long T, long N, int n) {
  if (!sizes_ok(T, N, n)) return 0;
  typename Mode::Ctx c{};
  c.T = T; c.N = N; c.n = n;
  return layout<Mode>(c, nullptr);
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

BA_HD double* kr_of(const CtxR& c, int buf, long i) { return c.kr + ((long)buf * c.n + i); }
// phase "camera setup", once, before any camera's decision is counted: the counter of the radial decisions starts at 0
template <class Mode> BA_HD void cam_setup_ctrl(const typename Mode::Ctx& c) {
  if constexpr (Mode::kRadial) c.cr->n_radial = 0;
}
// ... and per camera: validity, quaternion, both copies of the table; the output matrix starts as the input's bits.  The table holds
// R(q) for a valid camera that is not fixed and the input's R otherwise.  With a focal step (S >= 7) the output intrinsics start as the
// input's bits.  With a radial coefficient a valid camera whose k is not finite is not valid; both states start at the input's k and
// the output as its bits.
template <class Mode> BA_HD void cam_setup(const typename Mode::Ctx& c, long i) {
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
  if constexpr (Mode::S >= 7) {
    const uint64_t* ksrc = (const uint64_t*)(c.K + 9 * i);
    uint64_t* kdst = (uint64_t*)(c.K_out + 9 * i);
    for (int k = 0; k < 9; ++k) kdst[k] = ksrc[k];
  }
  if constexpr (Mode::kRadial) {
    const double k = c.radial_in[i];
    if (!fin(k)) c.cam_valid[i] = 0;
    *kr_of(c, 0, i) = k; *kr_of(c, 1, i) = k;
    *(uint64_t*)(c.radial_out + i) = *(const uint64_t*)(c.radial_in + i);
    c.cam_radial[i] = 0;
  }
}
// phase "camera groups", the last step of a camera with cnt active observations.  Focal: does it refine its focal?
BA_HD bool cam_focal_rule(const Ctx7& c, long i, bool is_free, long cnt) {
  return is_free && c.refine_focal[i] != 0 && cnt >= (long)c.min_focal_obs;
}
// Shared: does it carry its group's focal (its pose may be fixed)? -> error bits
BA_HD int cam_carry(const CtxS& c, long i, long cnt) {
  c.cam_cnt[i] = (c.cam_valid[i] != 0 && c.refine_focal[i] != 0 && cnt >= 1) ? (int)cnt : 0;
  c.cam_focal[i] = 0;
  const int g = c.cam_group[i];
  return g < 0 || g >= c.G ? kBadCamGroups : 0;
}
// phase "focal groups" (Shared): the span of group g (not empty) and slot k of its list -> error bits, *cnt = what the member carries.
// Ascending within a group, and groups in the order of their first members.  Reads nothing through a bad value.
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
BA_HD double* ag_of(const CtxR& c, int buf, long g) { return c.ag + ((long)buf * c.n + g); }
// How the members of a group are spread over workers: lane `lane` of kLanes takes every kLanes-th member; sum / any fold a value over
// the lanes (every lane receives the result), add / raise reach a counter / the error bits that other groups reach too.  The host takes
// the members one after another; the wave of bundle_gpu.hip folds with shuffles and reaches the counters with integer atomics.
struct OneLane {
  static constexpr int kLanes = 1;
  int lane = 0;
  BA_HD long sum(long v) const { return v; }
  BA_HD int any(int v) const { return v; }
  BA_HD void add(int* p, int v) const { *p += v; }
  BA_HD void raise(int* p, int v) const { *p |= v; }
};
// ... and the whole decision of group g (the group check of the schedule).  The slots are checked and counted (Radial: a member with
// refine_radial adds what it carries to the radial count as well); a group with a bad slot raises the error bits and decides nothing.
// It refines its focal when the total reaches min_focal_obs, and its factor starts at 1 in both states; a member has cam_focal when its
// group refines and it carries.  Radial: a group that refines its focal refines its radial coefficient when the radial count reaches
// min_focal_obs, its accumulated step starts at +0 in both states, and a member has cam_radial when its group does, it carries and it
// has refine_radial (cam_cnt is read, cam_focal is not: no lane waits for another).
template <class Mode, class Lanes> BA_HD void cgroup_decide(const typename Mode::Ctx& c, long g, const Lanes& w) {
  long b, e, total = 0, rtotal = 0;
  int err = 0;
  if (!cgroup_range(c, g, &b, &e)) { err = kBadCamGroups; b = e = 0; }
  for (long k = b + w.lane; k < e; k += Lanes::kLanes) {
    long cnt;
    err |= cgroup_slot(c, g, b, k, &cnt);
    total += cnt;
    if constexpr (Mode::kRadial) rtotal += cnt > 0 && c.refine_radial[c.group_cams[k]] != 0 ? cnt : 0;
  }
  err = w.any(err); total = w.sum(total);
  if constexpr (Mode::kRadial) rtotal = w.sum(rtotal);
  if (err) {
    if (w.lane == 0) w.raise(&c.ctrl->err, err);
    return;
  }
  const bool refines = total >= (long)c.min_focal_obs;
  long nf = 0;
  for (long k = b + w.lane; k < e; k += Lanes::kLanes) {
    const int i = c.group_cams[k];
    const bool fo = refines && c.cam_cnt[i] > 0;
    c.cam_focal[i] = (uint8_t)fo;
    nf += fo;
  }
  nf = w.sum(nf);
  if (w.lane == 0) {
    *sg_of(c, 0, g) = 1.0; *sg_of(c, 1, g) = 1.0;
    c.group_focal[g] = (uint8_t)refines;
    w.add(&c.cs->n_groups, (int)refines);
    w.add(&c.ctrl->n_focal, (int)nf);
  }
  if constexpr (Mode::kRadial) {
    const bool rr = refines && rtotal >= (long)c.min_focal_obs;
    long nr = 0;
    for (long k = b + w.lane; k < e; k += Lanes::kLanes) {
      const int i = c.group_cams[k];
      const bool ra = rr && c.cam_cnt[i] > 0 && c.refine_radial[i] != 0;
      c.cam_radial[i] = (uint8_t)ra;
      nr += ra;
    }
    nr = w.sum(nr);
    if (w.lane == 0) {
      *ag_of(c, 0, g) = 0.0; *ag_of(c, 1, g) = 0.0;
      c.group_radial[g] = (uint8_t)rr;
      w.add(&c.cr->n_radial, (int)nr);
    }
  }
}

// ---- §18.3: position priors ------------------------------------------------------------------------------------------------------------
// phase "camera groups", after cam_free of camera i is known: does it have a prior?  A NaN anywhere deactivates.
BA_HD bool cam_prior_rule(const Ctx& c, const Prior& p, long i) {
  bool ok = c.cam_free[i] != 0 && p.mask[i] != 0;
  for (int k = 0; k < 3; ++k) ok = ok && fin(p.xyz[3 * i + k]) && fin(p.sigma[3 * i + k]) && p.sigma[3 * i + k] > 0.0;
  return ok;
}
// d = c - g with the centre c = -R^T t, each of the three dot products summed left to right
BA_HD void prior_offset(const double* cam, const double* g, double* d) {
  for (int k = 0; k < 3; ++k) d[k] = -((cam[k] * cam[9] + cam[3 + k] * cam[10]) + cam[6 + k] * cam[11]) - g[k];
}
// the residual e [3] = d / sigma and its Jacobian J [3,6] = (-R^T [t]x, -R^T) with row k divided by sigma_k
BA_HD void prior_terms(const double* cam, const double* g, const double* sigma, double* e, double* J) {
  double d[3];
  prior_offset(cam, g, d);
  const double t0 = cam[9], t1 = cam[10], t2 = cam[11];
  for (int k = 0; k < 3; ++k) {
    const double r0 = cam[k], r1 = cam[3 + k], r2 = cam[6 + k], sg = sigma[k];      // column k of R
    e[k] = d[k] / sg;
    J[6 * k] = -(r1 * t2 - r2 * t1) / sg; J[6 * k + 1] = -(r2 * t0 - r0 * t2) / sg; J[6 * k + 2] = -(r0 * t1 - r1 * t0) / sg;
    J[6 * k + 3] = -r0 / sg; J[6 * k + 4] = -r1 / sg; J[6 * k + 5] = -r2 / sg;
  }
}
// phase "linearise cameras", after the osum64 of camera i has been stored: a camera with a prior adds J^T J to the leading 6 x 6 of U
// and J^T e to the first six of gc, entry by entry, each the sum of three products left to right.  One without performs no addition.
template <int S> BA_HD void cam_lin_prior(const Ctx& c, const Prior& p, int buf, long i) {
  if (!p.cam_prior[i]) return;
  double e[3], J[18];
  prior_terms(tab_of(c, buf, i), p.xyz + 3 * i, p.sigma + 3 * i, e, J);
  double* U = c.U + kTri<S> * i;
  double* g = c.gc + S * i;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = a; b < 6; ++b) {
      const int m = a * S - a * (a - 1) / 2 + (b - a);
      U[m] = U[m] + ((J[a] * J[b] + J[6 + a] * J[6 + b]) + J[12 + a] * J[12 + b]);
    }
    g[a] = g[a] + ((J[a] * e[0] + J[6 + a] * e[1]) + J[12 + a] * e[2]);
  }
}
// phase "evaluate", per camera at state `buf`: part = e0^2 + e1^2 + e2^2, part2 = |c - g|^2, left to right; +0 without a prior
BA_HD void cam_prior_eval(const Ctx& c, const Prior& p, int buf, long i) {
  double cost = 0.0, sq = 0.0;
  if (p.cam_prior[i]) {
    double d[3], e[3];
    prior_offset(tab_of(c, buf, i), p.xyz + 3 * i, d);
    for (int k = 0; k < 3; ++k) e[k] = d[k] / p.sigma[3 * i + k];
    cost = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    sq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  }
  p.part[i] = cost;
  p.part2[i] = sq;
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
// §18.4, the distorted projection, in this order: a = Y0 / Y2, b = Y1 / Y2, r2 = a a + b b, m = 1 + k r2, xd = a m, yd = b m,
// pixel = ((fx xd + skew yd) + cx, fy yd + cy)
BA_HD void residual_radial(const double* cam, double k, const double* Y, double u, double v, double* r) {
  const double a = Y[0] / Y[2], b = Y[1] / Y[2];
  const double r2 = a * a + b * b, m = 1.0 + k * r2, xd = a * m, yd = b * m;
  r[0] = ((cam[12] * xd + cam[13] * yd) + cam[14]) - u;
  r[1] = (cam[15] * yd + cam[16]) - v;
}
// ... and its Jacobians.  d(xd, yd)/d(a, b) = m I + 2k (a, b)(a, b)^T: jaa = m + 2k (a a), jab = 2k (a b), jbb = m + 2k (b b);
// d pixel/d(a, b): ua = fx jaa + skew jab, ub = fx jab + skew jbb, va = fy jab, vb = fy jbb; d pixel/dY = (ua / Y2, ub / Y2,
// -((ua a + ub b) / Y2)) and likewise for v, each times sw.  A [2,8]: the pose columns as in `jacobians` (the v row has no zero here),
// column 6 sw (fx xd + skew yd, fy yd) with `focal`, column 7 sw (fx (a r2) + skew (b r2), fy (b r2)) with `radial`, else +0.
BA_HD void jacobians_radial(const double* cam, double k, const double* P, const double* Y, double sw, bool focal, bool radial, double* A,
                            double* B) {
  const double fx = cam[12], sk = cam[13], fy = cam[15];
  const double a = Y[0] / Y[2], b = Y[1] / Y[2];
  const double r2 = a * a + b * b, m = 1.0 + k * r2, k2 = 2.0 * k;
  const double jaa = m + k2 * (a * a), jab = k2 * (a * b), jbb = m + k2 * (b * b);
  const double ua = fx * jaa + sk * jab, ub = fx * jab + sk * jbb, va = fy * jab, vb = fy * jbb;
  const double du[3] = {sw * (ua / Y[2]), sw * (ub / Y[2]), sw * -((ua * a + ub * b) / Y[2])};
  const double dv[3] = {sw * (va / Y[2]), sw * (vb / Y[2]), sw * -((va * a + vb * b) / Y[2])};
  A[0] = du[2] * P[1] - du[1] * P[2]; A[1] = du[0] * P[2] - du[2] * P[0]; A[2] = du[1] * P[0] - du[0] * P[1];
  A[3] = du[0]; A[4] = du[1]; A[5] = du[2];
  A[8] = dv[2] * P[1] - dv[1] * P[2]; A[9] = dv[0] * P[2] - dv[2] * P[0]; A[10] = dv[1] * P[0] - dv[0] * P[1];
  A[11] = dv[0]; A[12] = dv[1]; A[13] = dv[2];
  if (focal) {
    const double xd = a * m, yd = b * m;
    A[6] = sw * (fx * xd + sk * yd); A[14] = sw * (fy * yd);
  } else {
    A[6] = 0.0; A[14] = 0.0;
  }
  if (radial) {
    const double xr = a * r2, yr = b * r2;
    A[7] = sw * (fx * xr + sk * yr); A[15] = sw * (fy * yr);
  } else {
    A[7] = 0.0; A[15] = 0.0;
  }
  for (int j = 0; j < 3; ++j) {
    B[j] = (du[0] * cam[j] + du[1] * cam[3 + j]) + du[2] * cam[6 + j];
    B[3 + j] = (dv[0] * cam[j] + dv[1] * cam[3 + j]) + dv[2] * cam[6 + j];
  }
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
// the weighted A [2,S], B and residual rs of observation o of track t at state `buf`.  Shared: the pose columns of a camera that is not
// free are set to +0.
template <class Mode> BA_HD void obs_terms(const typename Mode::Ctx& c, int buf, long o, long t, double* A, double* B, double* rs) {
  constexpr int S = Mode::S;
  const double *cam = tab_of(c, buf, c.image[o]), *X = X_of(c, buf, t);
  bool focal = false;
  if constexpr (S >= 7) focal = c.cam_focal[c.image[o]] != 0;
  double P[3], Y[3], r[2], sw, rho, sq;
  transform(cam, X, P, Y);
  if constexpr (Mode::kRadial) {
    const double k = *kr_of(c, buf, c.image[o]);
    residual_radial(cam, k, Y, (double)c.xy[2 * o], (double)c.xy[2 * o + 1], r);
    loss(r, c.huber, &sw, &rho, &sq);
    jacobians_radial(cam, k, P, Y, sw, focal, c.cam_radial[c.image[o]] != 0, A, B);
  } else {
    residual(cam, Y, (double)c.xy[2 * o], (double)c.xy[2 * o + 1], r);
    loss(r, c.huber, &sw, &rho, &sq);
    jacobians<S>(cam, P, Y, sw, focal, A, B);
  }
  rs[0] = sw * r[0]; rs[1] = sw * r[1];
  if constexpr (Mode::kGroups)
    if (!c.cam_free[c.image[o]])
      for (int k = 0; k < 6; ++k) { A[k] = 0.0; A[S + k] = 0.0; }
}
// which cameras take part in the linear system: the free ones; Shared: those that are free or have cam_focal
template <class Mode> BA_HD bool takes_part(const typename Mode::Ctx& c, long i) {
  if constexpr (Mode::kGroups) return c.cam_free[i] != 0 || c.cam_focal[i] != 0;
  else return c.cam_free[i] != 0;
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
// a: the leading M x M block of an upper triangle stored row-major for width S (S (S + 1) / 2 entries); f: d [M] then the strict lower
// triangle of L row-major; false on a non-positive pivot.  The diagonal is damped here: a_ii (1 + lambda), or lambda when a_ii is zero.
BA_HD double damped(double d, double lambda) { return d == 0.0 ? lambda : d * (1.0 + lambda); }
template <int M, int S = M> BA_HD bool factor(const double* a, double lambda, double* f) {
  double L[M][M], d[M];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double s = damped(a[j * S - j * (j - 1) / 2], lambda);
#pragma unroll
    for (int k = 0; k < j; ++k) s = s - (L[j][k] * L[j][k]) * d[k];
    d[j] = s;
    ok = ok && s > 0.0;
#pragma unroll
    for (int i = j + 1; i < M; ++i) {
      double v = a[j * S - j * (j - 1) / 2 + (i - j)];
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
// phase "linearise tracks", per track: V = sum B^T B (upper triangle), gp = sum B^T rs, sequentially over the active observations.
// B does not depend on the width of the camera block, so one text (Mode = Pose) serves every mode with the pinhole projection.
template <class Mode = Pose> BA_HD void track_lin(const typename Mode::Ctx& c, int buf, long t) {
  double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
  if (c.point_active[t])
    for (long o = c.offsets[t]; o < c.offsets[t + 1]; ++o) {
      if (!c.obs_active[o]) continue;
      double A[2 * Mode::S], B[6], rs[2];
      obs_terms<Mode>(c, buf, o, t, A, B, rs);
      V[0] = V[0] + (B[0] * B[0] + B[3] * B[3]); V[1] = V[1] + (B[0] * B[1] + B[3] * B[4]); V[2] = V[2] + (B[0] * B[2] + B[3] * B[5]);
      V[3] = V[3] + (B[1] * B[1] + B[4] * B[4]); V[4] = V[4] + (B[1] * B[2] + B[4] * B[5]); V[5] = V[5] + (B[2] * B[2] + B[5] * B[5]);
      for (int k = 0; k < 3; ++k) g[k] = g[k] + (B[k] * rs[0] + B[3 + k] * rs[1]);
    }
  for (int k = 0; k < 6; ++k) c.V[6 * t + k] = V[k];
  for (int k = 0; k < 3; ++k) c.gp[3 * t + k] = g[k];
}
// phase "linearise cameras", one element of a camera's osum64: a [kTri<S> + S] += (A^T A upper triangle, A^T rs) of observation o
template <class Mode> BA_HD void cam_lin_term(const typename Mode::Ctx& c, int buf, long o, double* a) {
  constexpr int S = Mode::S;
  double A[2 * S], B[6], rs[2];
  obs_terms<Mode>(c, buf, o, c.obs_track[o], A, B, rs);
  int m = 0;
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int j = i; j < S; ++j) { a[m] = a[m] + (A[i] * A[j] + A[S + i] * A[S + j]); ++m; }
#pragma unroll
  for (int i = 0; i < S; ++i) a[kTri<S> + i] = a[kTri<S> + i] + (A[i] * rs[0] + A[S + i] * rs[1]);
}
// phase "linearise groups", one element of a group's osum64 of kTri<GW> values: member i with cam_focal adds U77 to d_g; Radial: (U77,
// U78, U88) to its group's block d [3] (U78 and U88 are +0 without cam_radial)
template <class Mode> BA_HD void group_lin_term(const typename Mode::Ctx& c, long i, double* a) {
  if (!c.cam_focal[i]) return;
  const double* U = c.U + kTri<Mode::S> * i;
  if constexpr (Mode::kRadial) { a[0] = a[0] + U[33]; a[1] = a[1] + U[34]; a[2] = a[2] + U[35]; }
  else a[0] = a[0] + U[27];
}
// phase "camera half", one element of a group's osum64 of GW values, E^T: member i adds its seventh entry of Sp with cam_focal;
// Radial: and its eighth with cam_radial
template <class Mode> BA_HD void group_half_term(const typename Mode::Ctx& c, long i, double* a) {
  if (c.cam_focal[i]) a[0] = a[0] + c.Sp[Mode::S * i + 6];
  if constexpr (Mode::kRadial)
    if (c.cam_radial[i]) a[1] = a[1] + c.Sp[8 * i + 7];
}

// ---- rule 6: the step ------------------------------------------------------------------------------------------------------------------
// phase "factor", per track / per free camera (the W x W block of U, damped -> Uf) / per refining group (the damped d_g must be
// positive) -> false on a non-positive pivot
BA_HD bool track_factor(const Ctx& c, long t, double lambda) {
  if (!c.point_active[t]) return true;
  double f[6];
  const bool ok = factor<3>(c.V + 6 * t, lambda, f);
  for (int k = 0; k < 6; ++k) c.Vf[6 * t + k] = f[k];
  return ok;
}
template <class Mode> BA_HD bool cam_factor(const Ctx& c, long i, double lambda) {
  constexpr int S = Mode::S, W = Mode::W;
  if (!c.cam_free[i]) return true;
  double f[kTri<W>];
  const bool ok = factor<W, S>(c.U + kTri<S> * i, lambda, f);
#pragma unroll
  for (int k = 0; k < kTri<W>; ++k) c.Uf[kTri<S> * i + k] = f[k];
  return ok;
}
// The group steps below are one name per step; Shared's scalar step (a division by the damped d_g) and Radial's 2 x 2 step (factor<2> /
// solve<2>) are two texts inside it: a 1 x 1 elimination in place of the division would round differently.
// Shared: the damped d_g must be positive.  Radial: the 2 x 2 L D L^T of the group's block, both diagonals damped here, once (a group
// that does not refine its radial has a block (d, 0; 0, 0), whose second pivot is lambda) -> the factor [3], kept behind the n blocks of dg
BA_HD double* dgf_of(const CtxS& c, long g) { return c.dg + 3 * ((long)c.n + g); }
template <class Mode> BA_HD bool group_factor(const CtxS& c, long g, double lambda) {
  if constexpr (Mode::kRadial) {
    if (!c.group_focal[g]) return true;
    double f[3];
    const bool ok = factor<2>(c.dg + 3 * g, lambda, f);
    for (int k = 0; k < 3; ++k) dgf_of(c, g)[k] = f[k];
    return ok;
  } else return !c.group_focal[g] || damped(c.dg[g], lambda) > 0.0;
}
// the vector of camera i as the operator sees it, out of x (step) or p: its S entries in place; Shared: the pose part of a free camera,
// its group's value when it has cam_focal (Radial: and its group's second value when it has cam_radial), else +0, formed in tmp [S]
template <class Mode> BA_HD const double* cam_vec(const typename Mode::Ctx& c, long i, bool step, double* tmp) {
  const double* vec = step ? c.x : c.p;
  if constexpr (!Mode::kGroups) return vec + Mode::S * i;
  else {
    const double* vecg = step ? c.xg : c.pg;
    const bool fr = c.cam_free[i] != 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) tmp[k] = fr ? vec[Mode::S * i + k] : 0.0;
    tmp[6] = c.cam_focal[i] ? vecg[Mode::GW * c.cam_group[i]] : 0.0;
    if constexpr (Mode::kRadial) tmp[7] = c.cam_radial[i] ? vecg[2 * c.cam_group[i] + 1] : 0.0;
    return tmp;
  }
}
// phase "track half", per track.  mode 0: z = Vd^-1 gp.  mode 1: z = Vd^-1 sum B^T (A p_c) over the active observations of the cameras
// that take part, sequentially.  mode 2 (back substitution): dX = Vd^-1 (-(gp + sum B^T (A x_c))), trial X' = X + dX -> false when not
// finite.
template <class Mode> BA_HD bool track_half(const typename Mode::Ctx& c, int buf, long t, int mode) {
  constexpr int S = Mode::S;
  if (!c.point_active[t]) return true;
  double s[3] = {0.0, 0.0, 0.0}, z[3];
  if (mode != 0)
    for (long o = c.offsets[t]; o < c.offsets[t + 1]; ++o) {
      const int im = c.image[o];
      if (!c.obs_active[o] || !takes_part<Mode>(c, im)) continue;
      double A[2 * S], B[6], rs[2], tmp[S < 7 ? 7 : S];
      obs_terms<Mode>(c, buf, o, t, A, B, rs);
      const double* v = cam_vec<Mode>(c, im, mode == 2, tmp);
      const double eu = dotm<S>(A, v), ev = dotm<S>(A + S, v);
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
// phase "camera half", one element of a camera's osum64: a [S] += A^T (B z_j) of observation o
template <class Mode> BA_HD void cam_half_term(const typename Mode::Ctx& c, int buf, long o, double* a) {
  constexpr int S = Mode::S;
  double A[2 * S], B[6], rs[2];
  const long t = c.obs_track[o];
  obs_terms<Mode>(c, buf, o, t, A, B, rs);
  const double* z = c.z + 3 * t;
  const double eu = (B[0] * z[0] + B[1] * z[1]) + B[2] * z[2], ev = (B[3] * z[0] + B[4] * z[1]) + B[5] * z[2];
#pragma unroll
  for (int k = 0; k < S; ++k) a[k] = a[k] + (A[k] * eu + A[S + k] * ev);
}
// ... and what follows the sum a [S] of camera i.  mode 0 (right-hand side): b = -(gc - a); a free camera starts its W entries (x = 0,
// r = b, zc = M^-1 r, p = zc, part = r . zc).  mode 1: rows 0..W-1 of Ud p - a for a free camera, part = p . Sp.  A camera that is not
// free has part = +0.  Shared: a member with cam_focal leaves b_7 (mode 0) or sum_{k<6} U_k7 p_k - a_7 (mode 1) in Sp[6] for its group;
// the group's own diagonal term is added once, at the group.
template <class Mode> BA_HD void cam_half_finish(const typename Mode::Ctx& c, long i, int mode, double lambda, const double* a) {
  constexpr int S = Mode::S, W = Mode::W;
  const bool fr = c.cam_free[i] != 0;
  bool fo = false, ra = false;
  if constexpr (Mode::kGroups) fo = c.cam_focal[i] != 0;
  if constexpr (Mode::kRadial) ra = c.cam_radial[i] != 0;
  if (!fr) c.part[i] = 0.0;
  if (!fr && !fo) return;
  double *x = c.x + S * i, *r = c.r + S * i, *zc = c.zc + S * i, *p = c.p + S * i, *Sp = c.Sp + S * i;
  if (mode == 0) {
    double b[S], zz[W];
#pragma unroll
    for (int k = 0; k < S; ++k) b[k] = -(c.gc[S * i + k] - a[k]);
    if (fr) {
#pragma unroll
      for (int k = 0; k < W; ++k) { x[k] = 0.0; r[k] = b[k]; }
      solve<W>(c.Uf + kTri<S> * i, b, zz);
#pragma unroll
      for (int k = 0; k < W; ++k) { zc[k] = zz[k]; p[k] = zz[k]; }
      c.part[i] = dotm<W>(b, zz);
    }
    if constexpr (Mode::kGroups)
      if (fo) Sp[6] = b[6];
    if constexpr (Mode::kRadial)
      if (ra) Sp[7] = b[7];
    return;
  }
  const double* U = c.U + kTri<S> * i;
  double pv[S], sp[W], tmp[S < 7 ? 7 : S];
  const double* v = cam_vec<Mode>(c, i, false, tmp);
#pragma unroll
  for (int k = 0; k < S; ++k) pv[k] = v[k];
  if (fr) {
#pragma unroll
    for (int row = 0; row < W; ++row) {
      double s = 0.0;
#pragma unroll
      for (int col = 0; col < S; ++col) {
        const int lo = row < col ? row : col, hi = row < col ? col : row;
        const double u = U[lo * S - lo * (lo - 1) / 2 + (hi - lo)];
        s = s + (row == col ? damped(u, lambda) : u) * pv[col];
      }
      sp[row] = s - a[row];
      Sp[row] = sp[row];
    }
    c.part[i] = dotm<W>(pv, sp);
  }
  if constexpr (Mode::kGroups)
    if (fo) {
      double s = 0.0;
#pragma unroll
      for (int col = 0; col < 6; ++col) s = s + U[col * S - col * (col - 1) / 2 + (6 - col)] * pv[col];
      Sp[6] = s - a[6];
    }
  if constexpr (Mode::kRadial)
    if (ra) {
      double s = 0.0;
#pragma unroll
      for (int col = 0; col < 6; ++col) s = s + U[col * S - col * (col - 1) / 2 + (7 - col)] * pv[col];
      Sp[7] = s - a[7];
    }
}
// ... and what follows the GW sums s of group g; a group that does not refine has partg = +0.  Shared.  mode 0: b_g = s; x = 0, r = b,
// z = r / d, p = z, partg = r z.  mode 1: Sp = d p + s, partg = p Sp (d: the damped d_g).  Radial: s = (focal, radial), the second
// taken as +0 when the group does not refine its radial.  mode 0: b = s; x = 0, r = b, z = D^-1 r by the factor, p = z, partg = r_0 z_0
// + r_1 z_1.  mode 1: Sp_0 = (d_00 p_0 + d_01 p_1) + s_0, Sp_1 = (d_01 p_0 + d_11 p_1) + s_1 with the damped diagonals, partg = p_0 Sp_0
// + p_1 Sp_1.
template <class Mode> BA_HD void group_half_finish(const typename Mode::Ctx& c, long g, int mode, double lambda, const double* s) {
  if (!c.group_focal[g]) { c.partg[g] = 0.0; return; }
  if constexpr (Mode::kRadial) {
    const double b[2] = {s[0], c.group_radial[g] ? s[1] : 0.0};
    double *x = c.xg + 2 * g, *r = c.rg + 2 * g, *z = c.zg + 2 * g, *p = c.pg + 2 * g, *Sp = c.Spg + 2 * g;
    if (mode == 0) {
      double zz[2];
      solve<2>(dgf_of(c, g), b, zz);
      for (int k = 0; k < 2; ++k) { x[k] = 0.0; r[k] = b[k]; z[k] = zz[k]; p[k] = zz[k]; }
      c.partg[g] = dotm<2>(b, zz);
      return;
    }
    const double* d = c.dg + 3 * g;
    const double sp[2] = {(damped(d[0], lambda) * p[0] + d[1] * p[1]) + b[0], (d[1] * p[0] + damped(d[2], lambda) * p[1]) + b[1]};
    Sp[0] = sp[0]; Sp[1] = sp[1];
    c.partg[g] = dotm<2>(p, sp);
  } else {
    const double d = damped(c.dg[g], lambda);
    if (mode == 0) {
      const double z = s[0] / d;
      c.xg[g] = 0.0; c.rg[g] = s[0]; c.zg[g] = z; c.pg[g] = z;
      c.partg[g] = s[0] * z;
      return;
    }
    const double sp = d * c.pg[g] + s[0];
    c.Spg[g] = sp;
    c.partg[g] = c.pg[g] * sp;
  }
}
// phase "update 1", per free camera over its W entries: x += alpha p, r -= alpha Sp, zc = M^-1 r, part = r . zc; per refining group
template <class Mode> BA_HD void cam_update1(const Ctx& c, long i, double alpha) {
  constexpr int S = Mode::S, W = Mode::W;
  if (!c.cam_free[i]) { c.part[i] = 0.0; return; }
  double r[W], zz[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    c.x[S * i + k] = c.x[S * i + k] + alpha * c.p[S * i + k];
    r[k] = c.r[S * i + k] - alpha * c.Sp[S * i + k];
    c.r[S * i + k] = r[k];
  }
  solve<W>(c.Uf + kTri<S> * i, r, zz);
#pragma unroll
  for (int k = 0; k < W; ++k) c.zc[S * i + k] = zz[k];
  c.part[i] = dotm<W>(r, zz);
}
template <class Mode> BA_HD void group_update1(const CtxS& c, long g, double alpha, double lambda) {
  if (!c.group_focal[g]) { c.partg[g] = 0.0; return; }
  if constexpr (Mode::kRadial) {                 // (the factor holds the damping)
    double r[2], zz[2];
    for (int k = 0; k < 2; ++k) {
      c.xg[2 * g + k] = c.xg[2 * g + k] + alpha * c.pg[2 * g + k];
      r[k] = c.rg[2 * g + k] - alpha * c.Spg[2 * g + k];
      c.rg[2 * g + k] = r[k];
    }
    solve<2>(dgf_of(c, g), r, zz);
    c.zg[2 * g] = zz[0]; c.zg[2 * g + 1] = zz[1];
    c.partg[g] = dotm<2>(r, zz);
  } else {
    c.xg[g] = c.xg[g] + alpha * c.pg[g];
    const double r = c.rg[g] - alpha * c.Spg[g], z = r / damped(c.dg[g], lambda);
    c.rg[g] = r; c.zg[g] = z;
    c.partg[g] = r * z;
  }
}
// phase "update 2", per free camera: p = zc + beta p; per refining group
template <class Mode> BA_HD void cam_update2(const Ctx& c, long i, double beta) {
  constexpr int S = Mode::S;
  if (!c.cam_free[i]) return;
  for (int k = 0; k < Mode::W; ++k) c.p[S * i + k] = c.zc[S * i + k] + beta * c.p[S * i + k];
}
template <class Mode> BA_HD void group_update2(const CtxS& c, long g, double beta) {
  if (!c.group_focal[g]) return;
  if constexpr (Mode::kRadial) {
    for (int k = 0; k < 2; ++k) c.pg[2 * g + k] = c.zg[2 * g + k] + beta * c.pg[2 * g + k];
  } else c.pg[g] = c.zg[g] + beta * c.pg[g];
}

// ---- rule 7: the trial -----------------------------------------------------------------------------------------------------------------
// phase "apply", per refining group: the factor of the trial s' = s (1 + delta_g); Radial: and its accumulated radial step a' = a + dk_g
template <class Mode> BA_HD void group_apply(const typename Mode::Ctx& c, int buf, long g) {
  if (c.group_focal[g]) *sg_of(c, 1 - buf, g) = *sg_of(c, buf, g) * (1.0 + c.xg[Mode::GW * g]);
  if constexpr (Mode::kRadial)
    if (c.group_radial[g]) *ag_of(c, 1 - buf, g) = *ag_of(c, buf, g) + c.xg[2 * g + 1];
}
// phase "apply", per camera.  A free camera: q' = normalise((1, omega / 2) (x) q), t' = t + dt into the other state -> false when not
// finite.  One with cam_focal: fx' = fx s, skew' = skew s, fy' = fy s with, Focal, s = 1 + delta on the values of the state, and, Shared,
// s = s_g (1 + delta_g) on the INPUT values (the camera forms s' itself, from the same two operands as group_apply), so that the members
// of a group leave with ONE factor on their input values however many trials were accepted -> false as well when fx' or fy' is not
// finite or fx' / fx_in or fy' / fy_in is not strictly inside (focal_lo, focal_hi); a NaN fails every test.  One with cam_radial (Radial):
// k' = k_in + (a_g + dk_g) on the INPUT value, the sum in brackets formed as group_apply forms it: one rounding on the input
// whatever the number of accepted trials -> false as well when k' is outside [radial_lo, radial_hi]
template <class Mode> BA_HD bool cam_apply(const typename Mode::Ctx& c, int buf, long i) {
  constexpr int S = Mode::S;
  bool ok = true;
  const double* tab = tab_of(c, buf, i);
  double* tab2 = tab_of(c, 1 - buf, i);
  const double* d = c.x + S * i;
  if (c.cam_free[i]) {
    const double* q = quat_of(c, buf, i);
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
  if constexpr (S >= 7) {
    if (c.cam_focal[i]) {                      // (Focal: only a free camera has cam_focal)
      const double* K = c.K + 9 * i;
      double s;
      const double* from;                      // fx and skew at 0 and 1; fy at 3 of the state table, at 4 of K
      if constexpr (Mode::kGroups) {
        const long g = c.cam_group[i];
        s = *sg_of(c, buf, g) * (1.0 + c.xg[Mode::GW * g]);
        from = K;
      } else {
        s = 1.0 + d[6];
        from = tab + 12;
      }
      const double fx = from[0] * s, sk = from[1] * s, fy = from[Mode::kGroups ? 4 : 3] * s;
      tab2[12] = fx; tab2[13] = sk; tab2[15] = fy;
      const double rx = fx / K[0], ry = fy / K[4];
      ok = ok && fin(fx) && fin(fy) && rx > c.focal_lo && rx < c.focal_hi && ry > c.focal_lo && ry < c.focal_hi;
    }
  }
  if constexpr (Mode::kRadial) {
    if (c.cam_radial[i]) {
      const long g = c.cam_group[i];
      const double k = c.radial_in[i] + (*ag_of(c, buf, g) + c.xg[2 * g + 1]);
      *kr_of(c, 1 - buf, i) = k;
      ok = ok && k >= c.radial_lo && k <= c.radial_hi;
    }
  }
  return ok;
}
// phase "evaluate", per track at state `buf`: part = sum rho, part2 = sum |r|^2 sequentially over the active observations
// -> false when an active observation is not in front of its camera
template <class Mode = Pose> BA_HD bool track_eval(const typename Mode::Ctx& c, int buf, long t) {
  double cost = 0.0, sq = 0.0;
  bool ok = true;
  if (c.point_active[t])
    for (long o = c.offsets[t]; o < c.offsets[t + 1]; ++o) {
      if (!c.obs_active[o]) continue;
      const double* cam = tab_of(c, buf, c.image[o]);
      double P[3], Y[3], r[2], sw, rho, s;
      ok = transform(cam, X_of(c, buf, t), P, Y) && ok;
      if constexpr (Mode::kRadial) residual_radial(cam, *kr_of(c, buf, c.image[o]), Y, (double)c.xy[2 * o], (double)c.xy[2 * o + 1], r);
      else residual(cam, Y, (double)c.xy[2 * o], (double)c.xy[2 * o + 1], r);
      loss(r, c.huber, &sw, &rho, &s);
      cost = cost + rho;
      sq = sq + s;
    }
  c.part[t] = cost;
  c.part2[t] = sq;
  return ok;
}

// ---- the single steps (one thread) -----------------------------------------------------------------------------------------------------
// cs: the scalars of the groups' sums, null without groups
BA_HD void ctrl_init(const Ctx& c, CtrlS* cs) {
  Ctrl& s = *c.ctrl;
  s.done = s.err = s.bad_f = s.bad_a = s.bad_e = s.pcg_done = s.cur = s.n_iters = s.n_accepted = s.n_focal = 0;
  s.fresh = 1;
  s.status = kMaxIters;
  s.n_pcg = 0;
  s.n_active_obs = s.n_active_pts = s.n_free = 0;
  s.lambda = kLambda0;
  s.cost = s.sq = s.cost_t = s.sq_t = s.cost0 = s.sq0 = s.rz = s.rz0 = s.psp = s.alpha = s.beta = 0.0;
  if (cs) { cs->acc = 0.0; cs->n_groups = 0; }
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
// ... with priors: the last level of a camera osum.  The cost is the tracks' sum (waiting in acc) plus the cameras', one addition,
// tracks first; the second sum is the report's |c - g|^2 and feeds nothing else.
BA_HD void ctrl_init_prior(const Prior& p) {
  CtrlP& q = *p.cp;
  q.acc = q.pc0 = q.pc = q.pc_t = q.sq0 = q.sq = q.sq_t = 0.0;
  q.n_prior = 0;
}
BA_HD void ctrl_feed_prior(const Ctx& c, const Prior& p, int action, double v) {
  CtrlP& q = *p.cp;
  switch (action) {
    case kActCost0: q.pc0 = q.pc = v; ctrl_feed(c, kActCost0, q.acc + v); break;
    case kActCostT: q.pc_t = v; ctrl_feed(c, kActCostT, q.acc + v); break;
    case kActSq0: q.sq0 = q.sq = v; break;
    case kActSqT: q.sq_t = v; break;
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
// ... with priors: an accepted trial takes its prior sums along
BA_HD void ctrl_accept_prior(const Ctx& c, const Prior& p) {
  const int before = c.ctrl->n_accepted;
  ctrl_accept(c);
  if (c.ctrl->n_accepted != before) { p.cp->pc = p.cp->pc_t; p.cp->sq = p.cp->sq_t; }
}
// phase "write": the pose of a free camera, the intrinsics of one with cam_focal (the other four entries of K_out keep the input's
// bits: cam_setup_focal), an active point, from the final state
template <class Mode> BA_HD void cam_write(const typename Mode::Ctx& c, int buf, long i) {
  const double* tab = tab_of(c, buf, i);
  if (c.cam_free[i]) {
    double* T = c.T_out + 16 * i;
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) T[4 * r + k] = tab[3 * r + k];
      T[4 * r + 3] = tab[9 + r];
    }
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
  }
  if constexpr (Mode::kRadial)
    if (c.cam_radial[i]) c.radial_out[i] = *kr_of(c, buf, i);
  if constexpr (Mode::S >= 7) {
    if (c.cam_focal[i]) {
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
template <class Mode> BA_HD void ctrl_write(const typename Mode::Ctx& c) {
  const Ctrl& s = *c.ctrl;
  long* k = c.counts;
  const double na = (double)s.n_active_obs;
  k[0] = s.status; k[1] = s.err; k[2] = s.n_iters; k[3] = s.n_accepted; k[4] = (long)s.n_pcg;
  k[5] = (long)s.n_active_obs; k[6] = (long)s.n_active_pts; k[7] = (long)s.n_free;
  k[8] = bits_of(s.cost0); k[9] = bits_of(s.cost);
  k[10] = bits_of(s.n_active_obs ? sqrt(s.sq0 / na) : 0.0); k[11] = bits_of(s.n_active_obs ? sqrt(s.sq / na) : 0.0);
  k[12] = bits_of(s.lambda); k[13] = 0; k[14] = 0; k[15] = 0;
  if constexpr (Mode::S >= 7) k[13] = s.n_focal;           // cameras that refine their focal
  if constexpr (Mode::kGroups) k[14] = c.cs->n_groups;     // groups that refine
  if constexpr (Mode::kRadial) k[15] = c.cr->n_radial;     // cameras that refine their radial coefficient
}

// counts[16..23] of the entry points with priors
BA_HD void ctrl_write_prior(const Ctx& c, const Prior& p) {
  const CtrlP& q = *p.cp;
  long* k = c.counts;
  const double np = (double)q.n_prior;
  k[16] = (long)q.n_prior; k[17] = bits_of(q.pc0); k[18] = bits_of(q.pc);
  k[19] = bits_of(q.n_prior ? sqrt(q.sq0 / np) : 0.0); k[20] = bits_of(q.n_prior ? sqrt(q.sq / np) : 0.0);
  k[21] = 0; k[22] = 0; k[23] = 0;
}

// ---- the entry points' side (host code of both files) ----------------------------------------------------------------------------------
// What the ten entry points take, as one superset; what a mode lacks stays NULL or 0.  Each part lists its members in the order of the C
// signature, so that an entry point is `Args a{{...}, {...}, ...}` with the parts it has.
struct Args {
  struct { const long* offsets; long T; const int* obs_image; const float* obs_xy; const uint8_t* obs_mask; long N; const float* xyz;
           const double *K, *T_cam_from_world; const uint8_t* fixed; int n_images; const long* cam_offsets; const int* cam_obs; } in;
  struct { double huber_px; int max_iters, pcg_iters; double pcg_tol, ftol; } par;
  struct { double* T_out; float* xyz_out; uint8_t *obs_active, *cam_free, *point_active; long* counts; } out;
  struct { const uint8_t* refine_focal; int min_focal_obs; double focal_lo, focal_hi; double* K_out; uint8_t* cam_focal; } focal;              // S >= 7
  struct { const int* cam_group; const long* group_offsets; const int* group_cams; int G; uint8_t* group_focal; } groups;                     // kGroups
  struct { const double* radial_in; const uint8_t* refine_radial; double radial_lo, radial_hi; double* radial_out;
           uint8_t *cam_radial, *group_radial; } radial;                                                                                      // kRadial
  struct { const double *xyz, *sigma; const uint8_t* mask; uint8_t* cam_prior; } prior;                                                       // kPrior
};
// the context of a mode out of the arguments: the problem, the parameters and the outputs every mode has, then what its traits add
template <class Mode> inline void fill(typename Mode::Ctx& c, const Args& a) {
  c.offsets = a.in.offsets; c.T = a.in.T; c.image = a.in.obs_image; c.xy = a.in.obs_xy; c.mask = a.in.obs_mask; c.N = a.in.N;
  c.xyz_in = a.in.xyz; c.K = a.in.K; c.Tin = a.in.T_cam_from_world; c.fixed = a.in.fixed; c.n = a.in.n_images;
  c.cam_offsets = a.in.cam_offsets; c.cam_obs = a.in.cam_obs;
  c.huber = a.par.huber_px; c.pcg_tol2 = a.par.pcg_tol * a.par.pcg_tol; c.ftol = a.par.ftol;
  c.T_out = a.out.T_out; c.xyz_out = a.out.xyz_out; c.obs_active = a.out.obs_active; c.cam_free = a.out.cam_free;
  c.point_active = a.out.point_active; c.counts = a.out.counts;
  if constexpr (Mode::S >= 7) {
    c.refine_focal = a.focal.refine_focal; c.min_focal_obs = a.focal.min_focal_obs; c.focal_lo = a.focal.focal_lo; c.focal_hi = a.focal.focal_hi;
    c.K_out = a.focal.K_out; c.cam_focal = a.focal.cam_focal;
  }
  if constexpr (Mode::kGroups) {
    c.cam_group = a.groups.cam_group; c.group_offsets = a.groups.group_offsets; c.group_cams = a.groups.group_cams; c.G = a.groups.G;
    c.group_focal = a.groups.group_focal;
  }
  if constexpr (Mode::kRadial) {
    c.radial_in = a.radial.radial_in; c.refine_radial = a.radial.refine_radial; c.radial_lo = a.radial.radial_lo; c.radial_hi = a.radial.radial_hi;
    c.radial_out = a.radial.radial_out; c.cam_radial = a.radial.cam_radial; c.group_radial = a.radial.group_radial;
  }
  if constexpr (Mode::kPrior) { c.pr.xyz = a.prior.xyz; c.pr.sigma = a.prior.sigma; c.pr.mask = a.prior.mask; c.pr.cam_prior = a.prior.cam_prior; }
}
// THE list of modes: f(Mode{}) for the mode of `kind` (the `mode` of the entry points with priors counts the same way) with or without
// priors, `unknown` for a combination that is no mode
enum : int { kKindPose = 0, kKindFocal, kKindShared, kKindRadial };
template <class R, class F> inline R with_mode(int kind, bool prior, R unknown, F f) {
  if (kind < kKindPose || kind > kKindRadial) return unknown;
  switch (kind + (prior ? 4 : 0)) {
    case kKindPose: return f(Pose{});
    case kKindFocal: return f(Focal{});
    case kKindShared: return f(Shared{});
    case kKindRadial: return f(Radial{});
    case 4 + kKindPose: return f(PoseP{});
    case 4 + kKindFocal: return f(FocalP{});
    case 4 + kKindShared: return f(SharedP{});
  }
  return unknown;
}
inline size_t workspace_bytes(int kind, bool prior, long T, long N, int n) {
  return with_mode(kind, prior, (size_t)0, [&](auto m) { return workspace_bytes<decltype(m)>(T, N, n); });
}
// the argument checks of every entry point -> LOFTR_OK when the run may start.  Limits are answered before a pointer is read;
// zero_counts: the host routines start from counts of zero (the kernels write them on the device).
template <class Mode> inline int check_args(const typename Mode::Ctx& c, int max_iters, int pcg_iters, double pcg_tol, bool zero_counts) {
  const long T = c.T, N = c.N;
  const int n = c.n;
  if constexpr (Mode::kRadial) {
    if (n > 0 && (!c.radial_in || !c.refine_radial || !c.radial_out || !c.cam_radial || !c.group_radial)) return LOFTR_ERR_BAD_ARG;
    if (!(fin(c.radial_lo) && fin(c.radial_hi) && c.radial_lo <= c.radial_hi)) return LOFTR_ERR_BAD_ARG;
  }
  if constexpr (Mode::S >= 7) {
    if (n > 0 && (!c.refine_focal || !c.K_out || !c.cam_focal)) return LOFTR_ERR_BAD_ARG;
    if (!(c.min_focal_obs >= 1 && fin(c.focal_lo) && fin(c.focal_hi) && c.focal_lo < 1.0 && 1.0 < c.focal_hi)) return LOFTR_ERR_BAD_ARG;
  }
  if constexpr (Mode::kPrior) {
    if (n > 0 && (!c.pr.xyz || !c.pr.sigma || !c.pr.mask || !c.pr.cam_prior)) return LOFTR_ERR_BAD_ARG;
  }
  if constexpr (Mode::kGroups) {
    if (n > 0 && (!c.cam_group || !c.group_cams || !c.group_focal)) return LOFTR_ERR_BAD_ARG;
    if (!c.group_offsets || c.G < 0 || c.G > n || (n > 0 && c.G == 0)) return LOFTR_ERR_BAD_ARG;
  }
  if (!c.offsets || !c.cam_offsets || !c.counts || T < 0 || N < 0 || n < 0) return LOFTR_ERR_BAD_ARG;
  if (T > 0 && (!c.xyz_in || !c.xyz_out || !c.point_active)) return LOFTR_ERR_BAD_ARG;
  if (N > 0 && (!c.image || !c.xy || !c.mask || !c.obs_active || !c.cam_obs)) return LOFTR_ERR_BAD_ARG;
  if (n > 0 && (!c.K || !c.Tin || !c.fixed || !c.T_out || !c.cam_free)) return LOFTR_ERR_BAD_ARG;
  if (!(c.huber >= 0.0 && fin(c.huber) && c.ftol >= 0.0 && fin(c.ftol) && pcg_tol >= 0.0 && pcg_tol < 1.0)) return LOFTR_ERR_BAD_ARG;
  if (max_iters < 0 || max_iters > LOFTR_BUNDLE_MAX_ITERS || pcg_iters < 1 || pcg_iters > LOFTR_BUNDLE_MAX_PCG) return LOFTR_ERR_BAD_ARG;
  if (!sizes_ok(T, N, n)) return LOFTR_ERR_UNSUPPORTED;
  if (zero_counts) for (int i = 0; i < (Mode::kPrior ? kCountsPrior : kCounts); ++i) c.counts[i] = 0;
  if (N > 0 && (T == 0 || n == 0)) return LOFTR_ERR_BAD_ARG;           // observations outside every track or camera
  return LOFTR_OK;
}

}  // namespace ba
