// View-graph calibration (one focal-length scale per camera from the fundamental matrices of all verified pairs): what the host
// routine (calib.hip) and the kernels (calib_gpu.hip) share.  fp64, `+ - * /` and sqrt only, no contraction, compiled from this one
// text for both sides, so host and device take identical decisions and produce identical bits.  The rule is stated in
// include/loftr_calib.h and DESIGN §28:
//   * the checks of an edge, an image, a group's span and an incidence slot, and the error bits a failed check raises;
//   * the centred, unit-norm fundamental matrix and the data weight of an edge; which groups are free;
//   * the residual rho of an edge at given scales and its two derivatives; the five scalars of its linearisation;
//   * the term of one incidence slot in its group's sums, what the group does with the finished sums, the per-group steps of the
//     conjugate gradients and of a Levenberg-Marquardt trial, and what the owner of the scalars does when a sum arrives;
//   * the outputs of an edge, an image and a group.
// A step is written for ONE item and reads only what an earlier phase wrote; the two sides differ only in how items are spread.
#pragma once
#include "../../include/loftr_calib.h"
#include "bundle_core.h"

#pragma clang fp contract(off)

#define VG_HD __host__ __device__ inline

namespace vg {

constexpr int kCounts = 16;
constexpr int kInfo = 4;
constexpr int kChunk = ba::kChunk;          // osum: osum64 per chunk of 4096, then osum of the chunk sums (§18)
enum Count { kTrials = 0, kErrors = 1, kAccepted = 2, kPcgIters = 3, kValidEdges = 4, kFreeGroups = 5, kOutliers = 6, kStatus = 7,
             kBoundRejects = 8 };
enum : int { kBadEdge = 1, kBadGroup = 2, kBadLists = 4, kBadStart = 8 };                                      // error bits (counts[1])
enum GroupState : uint8_t { kNoEdge = 0, kHeld = 1, kRefined = 2 };
enum EdgeState : uint8_t { kInvalid = 0, kOk = 1, kOutlier = 2 };
enum : int { kConverged = 0, kMaxIters = 1, kStalled = 2, kNothing = 3 };
enum : int { kActCost0 = 0, kActRz0, kActPap, kActRz, kActCostT };                                             // what a finished osum feeds
constexpr int kSetupSums = 2;               // a group's sums of the set-up: the diagonal, the right-hand side
constexpr int kApSums = 1;                  // ... and of one product A p

// what one thread owns: damping, flags, counters and the scalars of the conjugate gradients
struct Ctrl {
  int done, bad, oob, pcg_done, status, n_trials, n_accepted, accepted_now, n_bound;
  long long n_pcg;
  unsigned long long step_bits;
  double lambda, cost, cost_t, cost0, rz, rz0, alpha, beta, last_step;
};

// the problem, its outputs and the workspace (layout below)
struct P {
  const int* edge_image; const double* edge_F; const int* edge_weight; long E;
  const double* pp; const double* f0; const int* group; int n, G;
  const long* grp_offsets; const int* grp_inc;
  double loss2, max_resid, prior_weight, weight_cap, bound_lo, bound_hi, pcg_tol2, ftol;
  int min_edges, max_iters, pcg_iters;
  double* focal_scale; double* focal; double* edge_resid; uint8_t* edge_state; uint8_t* group_state;
  unsigned long long* counts; double* info;
  Ctrl* ctrl;
  double *Fp, *omega, *h;                                         // per edge: Fp [E,9], omega [E], h [E,5]
  double *m, *mt, *extra, *dtot, *x, *rr, *z, *dir, *Ap;          // per group [G]
  double *part, *red;                                             // part [E + G]
  int* n_inc;                                                     // per group: its valid incidences
  uint8_t *valid, *gstate;                                        // valid [E]; gstate [G]
};

VG_HD long chunks_of(long count) { return count > 0 ? (count + kChunk - 1) / kChunk : 1; }
VG_HD bool sizes_ok(long E, int n, int G) { return E >= 0 && E < (1L << 30) && n >= 1 && n <= 0x3FFFFFFF && G >= 1 && G <= n; }

// carves the workspace; base == nullptr only measures
inline size_t layout(P& p, char* base) {
  size_t o = 0;
  const size_t E = (size_t)(p.E > 0 ? p.E : 1), G = (size_t)(p.G > 0 ? p.G : 1), items = E + G;
  auto take = [&](auto** ptr, size_t bytes) {
    const size_t at = tracks::carve(&o, bytes);
    if (base) *ptr = (std::remove_reference_t<decltype(*ptr)>)(base + at);
  };
  take(&p.ctrl, sizeof(Ctrl));
  take(&p.Fp, 8 * 9 * E); take(&p.omega, 8 * E); take(&p.h, 8 * 5 * E);
  take(&p.m, 8 * G); take(&p.mt, 8 * G); take(&p.extra, 8 * G); take(&p.dtot, 8 * G); take(&p.x, 8 * G); take(&p.rr, 8 * G);
  take(&p.z, 8 * G); take(&p.dir, 8 * G); take(&p.Ap, 8 * G);
  take(&p.part, 8 * items);
  take(&p.red, 8 * 2 * (size_t)chunks_of((long)items));
  take(&p.n_inc, 4 * G);
  take(&p.valid, E); take(&p.gstate, G);
  return o;
}

VG_HD unsigned long long bits_of(double v) { unsigned long long b; __builtin_memcpy(&b, &v, 8); return b; }
VG_HD double double_of(unsigned long long b) { double v; __builtin_memcpy(&v, &b, 8); return v; }
VG_HD double dot9(const double* a, const double* b) {
  double s = a[0] * b[0];
  for (int k = 1; k < 9; ++k) s = s + a[k] * b[k];
  return s;
}
// o = a b and o = a b^T of 3 x 3 matrices (row-major), every entry (x0 y0 + x1 y1) + x2 y2
VG_HD void mul33(const double* a, const double* b, double* o) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[3 * r + c] = (a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c]) + a[3 * r + 2] * b[6 + c];
}
VG_HD void mul33t(const double* a, const double* b, double* o) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[3 * r + c] = (a[3 * r] * b[3 * c] + a[3 * r + 1] * b[3 * c + 1]) + a[3 * r + 2] * b[3 * c + 2];
}
// a counter that several items may raise at once (integer, so the order does not matter)
VG_HD void vg_count_one(int* at) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(at, 1);
#else
  *at += 1;
#endif
}
// §18's damping of a diagonal entry, as what is ADDED to it
VG_HD double vg_damp_add(double a, double lambda) { return a == 0.0 ? lambda : a * lambda; }

// ---- step 1: checks -------------------------------------------------------------------------------------------------------------------
VG_HD int vg_edge_check(const P& p, long e) {
  const int a = p.edge_image[2 * e], b = p.edge_image[2 * e + 1];
  return (a < 0 || a >= p.n || b < 0 || b >= p.n || a == b) ? kBadEdge : 0;
}
VG_HD int vg_image_check(const P& p, int i) {
  int err = 0;
  if (p.group[i] < 0 || p.group[i] >= p.G) err |= kBadGroup;
  const double f = p.f0[i];
  if (!ba::fin(f) || !(f > 0.0) || !ba::fin(p.pp[2L * i]) || !ba::fin(p.pp[2L * i + 1])) err |= kBadStart;
  return err;
}
// group g: its span of the incidence lists; resets what the set-up counts
VG_HD int vg_group_check(const P& p, int g) {
  long b, e;
  p.n_inc[g] = 0;
  return tracks::span(p.grp_offsets, p.G, 2 * p.E, g, &b, &e) ? 0 : kBadLists;
}
// slot k of the incidence lists: its code 2e + side names an edge end whose image's group owns the slot, above the slot before it.
// With spans that tile [0, 2E) this makes every list the stable ascending grouping.  Reads nothing through a bad value: an image or a
// group out of range is the other checks' to report.
VG_HD int vg_slot_check(const P& p, long k) {
  const int code = p.grp_inc[k];
  if (code < 0 || (long)code >= 2 * p.E) return kBadLists;
  const int img = p.edge_image[code];
  if (img < 0 || img >= p.n) return 0;
  const int g = p.group[img];
  if (g < 0 || g >= p.G) return 0;
  const long b = p.grp_offsets[g], e = p.grp_offsets[g + 1];
  if (k < b || k >= e) return kBadLists;
  if (k > b && k > 0 && !(p.grp_inc[k - 1] < code)) return kBadLists;
  return 0;
}

// ---- step 2: edges ---------------------------------------------------------------------------------------------------------------------
// edge e: F' = T_b^T F T_a scaled to unit Frobenius norm, its data weight, whether it is valid -> 1 when valid
VG_HD int vg_edge_setup(const P& p, long e) {
  double* Fp = p.Fp + 9 * e;
  for (int k = 0; k < 9; ++k) Fp[k] = 0.0;
  p.omega[e] = 0.0;
  p.valid[e] = 0;
  const int w = p.edge_weight[e];
  const double* F = p.edge_F + 9 * e;
  bool ok = w > 0;
  for (int k = 0; k < 9; ++k) ok = ok && ba::fin(F[k]);
  if (!ok) return 0;
  const int a = p.edge_image[2 * e], b = p.edge_image[2 * e + 1];
  const double ax = p.pp[2L * a], ay = p.pp[2L * a + 1], bx = p.pp[2L * b], by = p.pp[2L * b + 1];
  double M[9];
  for (int r = 0; r < 3; ++r) {                                          // F T_a: the third column takes the principal point of a
    M[3 * r] = F[3 * r]; M[3 * r + 1] = F[3 * r + 1];
    M[3 * r + 2] = (F[3 * r] * ax + F[3 * r + 1] * ay) + F[3 * r + 2];
  }
  for (int c = 0; c < 3; ++c) M[6 + c] = (bx * M[c] + by * M[3 + c]) + M[6 + c];   // T_b^T (.): the third row takes that of b
  const double nf = sqrt(dot9(M, M));
  if (!ba::fin(nf) || !(nf > 0.0)) return 0;
  for (int k = 0; k < 9; ++k) M[k] = M[k] / nf;
  for (int k = 0; k < 9; ++k) if (!ba::fin(M[k])) return 0;
  for (int k = 0; k < 9; ++k) Fp[k] = M[k];
  const double wd = (double)w;
  p.omega[e] = (wd < p.weight_cap ? wd : p.weight_cap) / p.weight_cap;
  p.valid[e] = 1;
  vg_count_one(p.n_inc + p.group[a]);
  vg_count_one(p.n_inc + p.group[b]);
  return 1;
}

// ---- step 3: groups --------------------------------------------------------------------------------------------------------------------
// group g (after vg_edge_setup of every edge): its state; the scale starts at 1
VG_HD int vg_group_setup(const P& p, int g) {
  const int cnt = p.n_inc[g];
  const int st = cnt == 0 ? kNoEdge : (cnt >= p.min_edges ? kRefined : kHeld);
  p.gstate[g] = (uint8_t)st;
  p.m[g] = 1.0; p.mt[g] = 1.0;
  p.extra[g] = 0.0; p.dtot[g] = 1.0; p.x[g] = 0.0; p.rr[g] = 0.0; p.z[g] = 0.0; p.dir[g] = 0.0; p.Ap[g] = 0.0;
  return st;
}
VG_HD bool vg_group_free(const P& p, int g) { return p.gstate[g] == kRefined; }

// ---- step 4: the residual --------------------------------------------------------------------------------------------------------------
// edge e at the scales m: Em = diag(f_b, f_b, 1) F' diag(f_a, f_a, 1), t = tr(Em Em^T), Nm = 2 Em Em^T Em - t Em, rho = Nm / t^(3/2)
// -> q = |rho|^2
VG_HD double vg_edge_rho(const P& p, long e, const double* m, double* Em, double* EEt, double* Nm, double* t_out, double* rho) {
  const int a = p.edge_image[2 * e], b = p.edge_image[2 * e + 1];
  const double fa = p.f0[a] * m[p.group[a]], fb = p.f0[b] * m[p.group[b]];
  const double* Fp = p.Fp + 9 * e;
  const double sr[3] = {fb, fb, 1.0}, sc[3] = {fa, fa, 1.0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Em[3 * r + c] = (sr[r] * Fp[3 * r + c]) * sc[c];
  mul33t(Em, Em, EEt);
  const double t = (EEt[0] + EEt[4]) + EEt[8];
  double MEm[9];
  mul33(EEt, Em, MEm);
  for (int k = 0; k < 9; ++k) Nm[k] = 2.0 * MEm[k] - t * Em[k];
  const double t32 = t * sqrt(t);
  for (int k = 0; k < 9; ++k) rho[k] = Nm[k] / t32;
  *t_out = t;
  return dot9(rho, rho);
}
// d rho for the derivative dE of Em (A = dE Em^T):
//   dN = 2 ((A + A^T) Em + Em Em^T dE) - 2 tr(A) Em - t dE,  dt = 2 tr(A),  d rho = dN / t^(3/2) - 1.5 N dt / t^(5/2)
VG_HD void vg_rho_derivative(const double* Em, const double* EEt, const double* Nm, double t, const double* dE, double* j) {
  double A[9], S[9], SE[9], MdE[9];
  mul33t(dE, Em, A);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) S[3 * r + c] = A[3 * r + c] + A[3 * c + r];
  mul33(S, Em, SE);
  mul33(EEt, dE, MdE);
  const double trA = (A[0] + A[4]) + A[8], dt = 2.0 * trA, st = sqrt(t), t32 = t * st, t52 = (t * t) * st;
  for (int k = 0; k < 9; ++k) {
    const double dN = (2.0 * (SE[k] + MdE[k]) - dt * Em[k]) - t * dE[k];
    j[k] = dN / t32 - ((1.5 * Nm[k]) * dt) / t52;
  }
}
// the cost term of an edge with data weight omega at q = |rho|^2 (Geman-McClure)
VG_HD double vg_edge_cost(const P& p, long e, double q) { return p.omega[e] * ((p.loss2 * q) / (p.loss2 + q)); }
// the cost term of edge e at the state (trial == 0) or at the trial -> part[e]
VG_HD void vg_edge_eval(const P& p, long e, int trial) {
  double term = 0.0;
  if (p.valid[e]) {
    double Em[9], EEt[9], Nm[9], rho[9], t;
    term = vg_edge_cost(p, e, vg_edge_rho(p, e, trial ? p.mt : p.m, Em, EEt, Nm, &t, rho));
  }
  p.part[e] = term;
}
// the prior's cost term of group g at the state or at the trial -> part[E + g]
VG_HD void vg_group_eval(const P& p, int g, int trial) {
  double term = 0.0;
  if (vg_group_free(p, g)) {
    const double d = (trial ? p.mt[g] : p.m[g]) - 1.0;
    term = p.prior_weight * (d * d);
  }
  p.part[p.E + g] = term;
}

// ---- step 6: the linearisation ---------------------------------------------------------------------------------------------------------
// edge e at the state: h_aa, h_ab, h_bb, g_a, g_b
VG_HD void vg_edge_linearise(const P& p, long e) {
  double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (p.valid[e]) {
    double Em[9], EEt[9], Nm[9], rho[9], t, dE[9], ja[9], jb[9];
    const double q = vg_edge_rho(p, e, p.m, Em, EEt, Nm, &t, rho);
    const int a = p.edge_image[2 * e], b = p.edge_image[2 * e + 1];
    const double ma = p.m[p.group[a]], mb = p.m[p.group[b]];
    for (int r = 0; r < 3; ++r) { dE[3 * r] = Em[3 * r] / ma; dE[3 * r + 1] = Em[3 * r + 1] / ma; dE[3 * r + 2] = 0.0; }
    vg_rho_derivative(Em, EEt, Nm, t, dE, ja);
    for (int c = 0; c < 3; ++c) { dE[c] = Em[c] / mb; dE[3 + c] = Em[3 + c] / mb; dE[6 + c] = 0.0; }
    vg_rho_derivative(Em, EEt, Nm, t, dE, jb);
    const double s = p.loss2 / (p.loss2 + q), w = p.omega[e] * (s * s);
    h[0] = w * dot9(ja, ja); h[1] = w * dot9(ja, jb); h[2] = w * dot9(jb, jb);
    h[3] = -(w * dot9(ja, rho)); h[4] = -(w * dot9(jb, rho));
  }
  for (int k = 0; k < 5; ++k) p.h[5 * e + k] = h[k];
}
// the group at the other end of the incidence `code`
VG_HD int vg_other_group(const P& p, int code) { return p.group[p.edge_image[code ^ 1]]; }
// the term of incidence `code` of group g in the set-up sums: the diagonal (the own term, and the cross term when both ends lie in
// g), the right-hand side
VG_HD void vg_term_setup(const P& p, int g, int code, double* out) {
  const double* h = p.h + 5L * (code >> 1);
  const int side = code & 1;
  const double own = side ? h[2] : h[0];
  out[0] = vg_other_group(p, code) == g ? own + h[1] : own;
  out[1] = side ? h[4] : h[3];
}
// ... in the sums of A p: h_ss p_g + h_ab p_other (a held group's p is 0)
VG_HD void vg_term_Ap(const P& p, int g, int code, double* out) {
  const double* h = p.h + 5L * (code >> 1);
  const int side = code & 1, og = vg_other_group(p, code);
  const double po = vg_group_free(p, og) ? p.dir[og] : 0.0;
  out[0] = (side ? h[2] : h[0]) * p.dir[g] + h[1] * po;
}
// group g with its finished set-up sums: the prior, the damping, and the conjugate gradients' start (x = 0, r = b, z = r / d, p = z);
// part = r z -> false when the damped diagonal is not positive
VG_HD bool vg_group_finish_setup(const P& p, int g, const double* s) {
  bool ok = true;
  double b = 0.0, z = 0.0;
  if (vg_group_free(p, g)) {
    const double D = s[0] + p.prior_weight, add = vg_damp_add(D, p.ctrl->lambda);
    p.extra[g] = p.prior_weight + add;
    p.dtot[g] = D + add;
    b = s[1] - p.prior_weight * (p.m[g] - 1.0);
    z = b / p.dtot[g];
    ok = p.dtot[g] > 0.0 && ba::fin(z);
  }
  p.x[g] = 0.0; p.rr[g] = b; p.z[g] = z; p.dir[g] = z; p.Ap[g] = 0.0;
  p.part[g] = b * z;
  return ok;
}
// group g with the finished sum: (A p)_g = sum + (prior + damping) p_g; part = p . A p
VG_HD void vg_group_finish_Ap(const P& p, int g, const double* s) {
  double ap = 0.0;
  if (vg_group_free(p, g)) ap = s[0] + p.extra[g] * p.dir[g];
  p.Ap[g] = ap;
  p.part[g] = p.dir[g] * ap;
}
// group g: x += alpha p, r -= alpha A p, z = r / d; part = r z
VG_HD void vg_group_update(const P& p, int g) {
  if (!vg_group_free(p, g)) { p.part[g] = 0.0; return; }
  const double alpha = p.ctrl->alpha;
  p.x[g] = p.x[g] + alpha * p.dir[g];
  p.rr[g] = p.rr[g] - alpha * p.Ap[g];
  p.z[g] = p.rr[g] / p.dtot[g];
  p.part[g] = p.rr[g] * p.z[g];
}
// group g: p = z + beta p
VG_HD void vg_group_direction(const P& p, int g) {
  if (vg_group_free(p, g)) p.dir[g] = p.z[g] + p.ctrl->beta * p.dir[g];
}
// group g: the trial m + x -> x^2, -1 for a step that is not finite, -2 for a trial outside (bound_lo, bound_hi)
VG_HD double vg_group_apply(const P& p, int g) {
  if (!vg_group_free(p, g)) { p.mt[g] = p.m[g]; return 0.0; }
  const double mt = p.m[g] + p.x[g], n2 = p.x[g] * p.x[g];
  p.mt[g] = mt;
  if (!ba::fin(n2) || !ba::fin(mt)) return -1.0;
  if (!(mt > p.bound_lo) || !(mt < p.bound_hi)) return -2.0;
  return n2;
}
// an accepted trial becomes the state
VG_HD bool vg_commit_now(const P& p) { return p.ctrl->accepted_now != 0; }
VG_HD void vg_group_commit(const P& p, int g) { p.m[g] = p.mt[g]; }

// ---- step 7: the owner of the scalars ----------------------------------------------------------------------------------------------------
VG_HD void vg_ctrl_init(const P& p) {
  Ctrl& c = *p.ctrl;
  c.done = c.bad = c.oob = c.pcg_done = c.n_trials = c.n_accepted = c.accepted_now = c.n_bound = 0;
  c.status = kMaxIters;
  c.n_pcg = 0;
  c.step_bits = 0;
  c.lambda = ba::kLambda0;
  c.cost = c.cost_t = c.cost0 = c.rz = c.rz0 = c.alpha = c.beta = c.last_step = 0.0;
}
VG_HD void vg_feed(const P& p, int action, double v) {
  Ctrl& c = *p.ctrl;
  switch (action) {
    case kActCost0:
      c.cost = c.cost0 = v;
      if (p.counts[kValidEdges] == 0 || p.counts[kFreeGroups] == 0) { c.done = 1; c.status = kNothing; }
      else if (v == 0.0) { c.done = 1; c.status = kConverged; }             // nothing can lower a cost of exactly 0
      break;
    case kActRz0: c.rz = c.rz0 = v; if (!(v > 0.0)) c.pcg_done = 1; break;
    case kActPap: c.alpha = c.rz / v; if (!(v > 0.0)) c.pcg_done = 1; else c.n_pcg += 1; break;
    case kActRz: c.beta = v / c.rz; c.rz = v; if (v <= p.pcg_tol2 * c.rz0) c.pcg_done = 1; break;
    case kActCostT: c.cost_t = v; break;
  }
}
// the end of a trial: ctrl_accept's schedule (§18), and a trial outside the bounds is rejected and counted
VG_HD void vg_accept(const P& p) {
  Ctrl& c = *p.ctrl;
  c.accepted_now = 0;
  if (c.done) return;
  c.n_trials += 1;
  if (c.oob) c.n_bound += 1;
  if (!c.bad && !c.oob && c.cost_t < c.cost) {
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
  c.oob = 0;
  c.pcg_done = 0;
  c.step_bits = 0;
}
VG_HD bool vg_refine_idle(const P& p) { return p.ctrl->done != 0; }
VG_HD bool vg_pcg_idle(const P& p) { return p.ctrl->done != 0 || p.ctrl->pcg_done != 0; }

// ---- step 8: outputs -------------------------------------------------------------------------------------------------------------------
// edge e -> 1 when it is an outlier
VG_HD int vg_edge_write(const P& p, long e) {
  double r = 0.0;
  int st = kInvalid;
  if (p.valid[e]) {
    double Em[9], EEt[9], Nm[9], rho[9], t;
    r = sqrt(vg_edge_rho(p, e, p.m, Em, EEt, Nm, &t, rho));
    st = r > p.max_resid ? kOutlier : kOk;
  }
  p.edge_resid[e] = r;
  p.edge_state[e] = (uint8_t)st;
  return st == kOutlier;
}
VG_HD void vg_image_write(const P& p, int i) { p.focal[i] = p.f0[i] * p.m[p.group[i]]; }
VG_HD void vg_group_write(const P& p, int g) { p.focal_scale[g] = p.m[g]; p.group_state[g] = p.gstate[g]; }
// the counts and info the owner of the scalars holds
VG_HD void vg_finish(const P& p) {
  const Ctrl& c = *p.ctrl;
  p.counts[kTrials] = (unsigned long long)c.n_trials;
  p.counts[kAccepted] = (unsigned long long)c.n_accepted;
  p.counts[kPcgIters] = (unsigned long long)c.n_pcg;
  p.counts[kStatus] = (unsigned long long)c.status;
  p.counts[kBoundRejects] = (unsigned long long)c.n_bound;
  p.info[0] = c.cost0; p.info[1] = c.cost; p.info[2] = c.lambda; p.info[3] = c.last_step;
}

// ---- arguments --------------------------------------------------------------------------------------------------------------------------
struct Args {
  const int* edge_image; const double* edge_F; const int* edge_weight; long E; const double* pp; const double* f0; const int* group;
  int n_images, n_groups; const long* grp_offsets; const int* grp_inc;
  double loss, max_resid, prior_weight; int weight_cap; double bound_lo, bound_hi; int min_edges, max_iters, pcg_iters; double pcg_tol, ftol;
  double* focal_scale; double* focal; double* edge_resid; uint8_t* edge_state; uint8_t* group_state; long* counts; double* info;
};
inline int vg_check_args(const Args& a) {
  if (!a.counts || !a.info || a.E < 0 || a.n_images < 1 || a.n_groups < 1 || a.n_groups > a.n_images || !a.pp || !a.f0 || !a.group ||
      !a.grp_offsets || !a.focal_scale || !a.focal || !a.group_state)
    return LOFTR_ERR_BAD_ARG;
  if (a.E > 0 && (!a.edge_image || !a.edge_F || !a.edge_weight || !a.grp_inc || !a.edge_resid || !a.edge_state)) return LOFTR_ERR_BAD_ARG;
  if (!ba::fin(a.loss) || !(a.loss > 0.0) || !ba::fin(a.max_resid) || !(a.max_resid >= 0.0) || !ba::fin(a.prior_weight) ||
      !(a.prior_weight >= 0.0) || a.weight_cap < 1 || !ba::fin(a.bound_hi) || !(a.bound_lo > 0.0) || !(a.bound_lo < 1.0) ||
      !(a.bound_hi > 1.0) || !(a.pcg_tol >= 0.0) || !(a.pcg_tol < 1.0) || !ba::fin(a.ftol) || !(a.ftol >= 0.0) || a.min_edges < 0 ||
      a.max_iters < 0 || a.pcg_iters < 0)
    return LOFTR_ERR_BAD_ARG;
  if (!sizes_ok(a.E, a.n_images, a.n_groups) || a.max_iters > (1 << 16) || a.pcg_iters > (1 << 16)) return LOFTR_ERR_UNSUPPORTED;
  return LOFTR_OK;
}
inline P vg_problem(const Args& a) {
  P p{};
  p.edge_image = a.edge_image; p.edge_F = a.edge_F; p.edge_weight = a.edge_weight; p.E = a.E; p.pp = a.pp; p.f0 = a.f0; p.group = a.group;
  p.n = a.n_images; p.G = a.n_groups; p.grp_offsets = a.grp_offsets; p.grp_inc = a.grp_inc;
  p.loss2 = a.loss * a.loss; p.max_resid = a.max_resid; p.prior_weight = a.prior_weight; p.weight_cap = (double)a.weight_cap;
  p.bound_lo = a.bound_lo; p.bound_hi = a.bound_hi; p.pcg_tol2 = a.pcg_tol * a.pcg_tol; p.ftol = a.ftol;
  p.min_edges = a.min_edges; p.max_iters = a.max_iters; p.pcg_iters = a.pcg_iters;
  p.focal_scale = a.focal_scale; p.focal = a.focal; p.edge_resid = a.edge_resid; p.edge_state = a.edge_state; p.group_state = a.group_state;
  p.counts = (unsigned long long*)a.counts; p.info = a.info;
  return p;
}

}  // namespace vg
