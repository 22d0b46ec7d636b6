// Rotation averaging over the view graph (global rotations from pairwise ones; the pairs that disagree): what the host routine
// (rotation.hip) and the kernels (rotation_gpu.hip) share.  fp64, `+ - * /` and sqrt only, no contraction, compiled from this one text
// for both sides, so host and device take identical decisions and produce identical bits.  The rule is stated in include/loftr_hip.h
// and DESIGN §26:
//   * the checks of an edge and of a node's adjacency list, and the error bits a failed check raises;
//   * which edges are valid, and the quaternion of an edge (bundle_core.h's Shepperd conversion, normalised there, once);
//   * one slot of an edge's cycle support; the 64-bit word of the spanning forest;
//   * one tree edge of one level of the start values;
//   * the per-edge and per-node steps of the Gauss-Newton refinement (residual and Geman-McClure weight, right-hand side and diagonal,
//     the conjugate gradients' per-node steps, apply, commit), and what the owner of the scalars does when a sum arrives (feed, decide);
//   * the verdict of an edge and the matrix of a node.
// A step is written for ONE item and reads only what an earlier phase wrote; the two sides differ only in how items are spread.
#pragma once
#include "bundle_core.h"

#pragma clang fp contract(off)

#define ROT_HD __host__ __device__ inline

namespace rot {

constexpr int kCounts = 16;
constexpr int kInfo = 4;
constexpr int kChunk = ba::kChunk;          // osum: osum64 per chunk of 4096, then osum of the chunk sums (§18)
enum Count { kInGraph = 0, kErrors = 1, kInvalidEdges = 2, kDuplicateEdges = 3, kUsedEdges = 4, kSupportSum = 5, kTreeEdges = 6,
             kTreeNoSupport = 7, kDepth = 8, kComponents = 9, kIters = 10, kPcgIters = 11, kOkEdges = 12, kOutlierEdges = 13, kStatus = 14,
             kRoot = 15 };
enum : int { kBadImage = 1, kSelfEdge = 2, kBadAdjacency = 4, kBadRoot = 8 };                                  // error bits (counts[1])
enum State : uint8_t { kInvalid = 0, kOutside = 1, kOk = 2, kOutlier = 3 };                                    // of an edge
enum : int { kConverged = 0, kMaxIters = 1, kStalled = 2, kNothing = 3 };
enum : int { kActCost = 0, kActRz0, kActPLp, kActRz, kActCostFinal };                                          // what a finished osum feeds
constexpr int kMaxSupport = 0xFFFF;
constexpr double kOrthoTol = 1e-3;

// what one thread owns: flags, counters and the scalars of the conjugate gradients
struct Ctrl {
  int done, bad, pcg_done, status, n_iters, have0, root, depth, n_tree;
  unsigned root_min;
  long long n_pcg;
  unsigned long long best_wsum, step_bits, chord_bits;
  double cost, cost0, rz, rz0, alpha, beta, last_step;
};

// the problem, its outputs and the workspace (layout below)
struct P {
  const int* edge_image; const double* edge_R; const int* edge_weight; long E; int n, root_arg;
  const long* adj_offsets; const int* adj_edge; const uint8_t* edge_use_in;
  double cos_half, d2, max_chord, step_tol, pcg_tol2;
  int max_iters, pcg_iters, rounds;
  double* R; uint8_t* in_graph; uint8_t* edge_state; double* edge_chord; int* support_out; uint8_t* tree_out; uint8_t* use_out;
  unsigned long long* counts; double* info;
  Ctrl* ctrl;
  double *q, *qn, *qt, *r3, *w, *diag, *x, *rr, *z, *pp, *Lp, *part, *red;   // q [E,4]; qn, qt [n,4]; r3 [E,3]; w [E]; the rest per node
  long long* wsum;
  unsigned long long* best;
  int *support, *depth, *label, *parent, *tree_list, *accepted;
  uint8_t *valid, *use, *tree;
};

ROT_HD long chunks_of(long count) { return count > 0 ? (count + kChunk - 1) / kChunk : 1; }
ROT_HD long part_items(long E, int n) { return E > 3L * n ? E : 3L * n; }

// sizes the routines index with int and pack into the word
ROT_HD bool sizes_ok(long E, int n) { return E >= 0 && n >= 0 && E <= 0x7FFFFFFEL && n <= 0x3FFFFFFF; }
// Boruvka rounds of the fixed schedule: ceil(log2 n) + 1
ROT_HD int rounds_of(int n) {
  int r = 0;
  while ((1L << r) < n) ++r;
  return r + 1;
}

// carves the workspace; base == nullptr only measures
inline size_t layout(P& p, char* base) {
  size_t o = 0;
  const size_t E = (size_t)(p.E > 0 ? p.E : 1), n = (size_t)(p.n > 0 ? p.n : 1);
  auto take = [&](auto** ptr, size_t bytes) {
    const size_t at = tracks::carve(&o, bytes);
    if (base) *ptr = (std::remove_reference_t<decltype(*ptr)>)(base + at);
  };
  take(&p.ctrl, sizeof(Ctrl));
  take(&p.q, sizeof(double) * 4 * E);
  take(&p.qn, sizeof(double) * 4 * n);
  take(&p.qt, sizeof(double) * 4 * n);
  take(&p.r3, sizeof(double) * 3 * E);
  take(&p.w, sizeof(double) * E);
  take(&p.diag, sizeof(double) * n);
  take(&p.x, sizeof(double) * 3 * n);
  take(&p.rr, sizeof(double) * 3 * n);
  take(&p.z, sizeof(double) * 3 * n);
  take(&p.pp, sizeof(double) * 3 * n);
  take(&p.Lp, sizeof(double) * 3 * n);
  take(&p.part, sizeof(double) * (size_t)(part_items(p.E, p.n) > 0 ? part_items(p.E, p.n) : 1));
  take(&p.red, sizeof(double) * 2 * (size_t)chunks_of(part_items(p.E, p.n)));
  take(&p.wsum, sizeof(long long) * n);
  take(&p.best, sizeof(unsigned long long) * n);
  take(&p.support, sizeof(int) * E);
  take(&p.depth, sizeof(int) * n);
  take(&p.label, sizeof(int) * n);
  take(&p.parent, sizeof(int) * n);
  take(&p.tree_list, sizeof(int) * n);
  take(&p.accepted, sizeof(int) * (size_t)rounds_of(p.n));
  take(&p.valid, E);
  take(&p.use, E);
  take(&p.tree, E);
  return o;
}

// ---- quaternions (w, x, y, z); R(a (x) b) = R(a) R(b) --------------------------------------------------------------------------------
ROT_HD void qmul(const double* a, const double* b, double* o) {
  o[0] = ((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3];
  o[1] = ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2];
  o[2] = ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1];
  o[3] = ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0];
}
ROT_HD void qnormalise(double* q) {
  const double nq = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  q[0] = q[0] / nq; q[1] = q[1] / nq; q[2] = q[2] / nq; q[3] = q[3] / nq;
}
ROT_HD double nan64() { return __builtin_nan(""); }
ROT_HD unsigned long long bits_of(double v) { unsigned long long b; __builtin_memcpy(&b, &v, 8); return b; }
ROT_HD double double_of(unsigned long long b) { double v; __builtin_memcpy(&v, &b, 8); return v; }

// the quaternion of edge e as the rotation that takes `from`'s frame to the other end's: stored, or conjugated when e is (other, from)
ROT_HD void edge_quat_from(const P& p, long e, int from, double* o) {
  const double* q = p.q + 4 * e;
  const bool stored = p.edge_image[2 * e] == from;
  o[0] = q[0];
  o[1] = stored ? q[1] : -q[1]; o[2] = stored ? q[2] : -q[2]; o[3] = stored ? q[3] : -q[3];
}
ROT_HD int other_end(const P& p, long e, int i) { return p.edge_image[2 * e] == i ? p.edge_image[2 * e + 1] : p.edge_image[2 * e]; }

// ---- rules 1, 2: checks, valid edges, quaternions -------------------------------------------------------------------------------------
// rule 2: edge e is valid
ROT_HD bool edge_valid(const P& p, long e) {
  const double* m = p.edge_R + 9 * e;
  if (!(p.edge_weight[e] > 0)) return false;
  for (int k = 0; k < 9; ++k) if (!ba::fin(m[k])) return false;
  const double det = (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
  if (!(det > 0.0)) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      const double g = ((m[i] * m[j] + m[3 + i] * m[3 + j]) + m[6 + i] * m[6 + j]) - (i == j ? 1.0 : 0.0);
      if (!(fabs(g) <= kOrthoTol)) return false;
    }
  return true;
}
// the error bits of edge e; its validity, whether it is used and its quaternion.  Reads nothing through edge_image.
ROT_HD int edge_setup(const P& p, long e) {
  int err = 0;
  const int a = p.edge_image[2 * e], b = p.edge_image[2 * e + 1];
  if (a < 0 || a >= p.n || b < 0 || b >= p.n) err |= kBadImage;
  if (a == b) err |= kSelfEdge;
  const bool valid = edge_valid(p, e);
  p.valid[e] = (uint8_t)valid;
  p.use[e] = (uint8_t)(valid && p.edge_use_in[e] != 0);
  p.tree[e] = 0;
  p.support[e] = 0;
  double* q = p.q + 4 * e;
  if (valid) {
    const double* m = p.edge_R + 9 * e;
    const double T[12] = {m[0], m[1], m[2], 0.0, m[3], m[4], m[5], 0.0, m[6], m[7], m[8], 0.0};
    ba::quat_from_matrix(T, q);
  } else {
    q[0] = 1.0; q[1] = 0.0; q[2] = 0.0; q[3] = 0.0;
  }
  return err;
}
// the error bits of node i's adjacency list (after edge_setup of every edge): offsets that ascend inside [0, 2E], slots that hold
// edges of i, neighbours ascending and edges ascending within a neighbour, at most one used edge per neighbour; wsum [i] = the sum of
// its used weights.  i == 0 also answers for the two ends of the offsets and for the root.
ROT_HD int node_check(const P& p, int i) {
  int err = 0;
  if (i == 0) {
    if (p.adj_offsets[0] != 0 || p.adj_offsets[p.n] != 2 * p.E) err |= kBadAdjacency;
    if (p.root_arg < -1 || p.root_arg >= p.n) err |= kBadRoot;
  }
  if (i >= p.n) return err;
  const long lo = p.adj_offsets[i], hi = p.adj_offsets[i + 1];
  long long wsum = 0;
  if (lo < 0 || hi < lo || hi > 2 * p.E) err |= kBadAdjacency;
  else {
    int nb_prev = -1, e_prev = -1, run_used = 0;
    for (long k = lo; k < hi; ++k) {
      const int e = p.adj_edge[k];
      if (e < 0 || e >= p.E) { err |= kBadAdjacency; break; }
      const int a = p.edge_image[2 * (long)e], b = p.edge_image[2 * (long)e + 1];
      if (a != i && b != i) { err |= kBadAdjacency; break; }
      const int nb = a == i ? b : a;
      if (k > lo && (nb < nb_prev || (nb == nb_prev && e <= e_prev))) { err |= kBadAdjacency; break; }
      run_used = (k > lo && nb == nb_prev ? run_used : 0) + p.use[e];
      if (run_used > 1) { err |= kBadAdjacency; break; }
      if (p.use[e]) wsum += p.edge_weight[e];
      nb_prev = nb; e_prev = e;
    }
  }
  p.wsum[i] = wsum;
  p.depth[i] = -1;
  p.label[i] = i;
  return err;
}

// ---- rule 3: cycle support ------------------------------------------------------------------------------------------------------------
// the used edge that joins node and nb, or -1: lower bound of nb in node's list, then the run of that neighbour
ROT_HD long find_used(const P& p, int node, int nb) {
  long lo = p.adj_offsets[node], hi = p.adj_offsets[node + 1];
  const long end = hi;
  while (lo < hi) {
    const long mid = lo + (hi - lo) / 2;
    if (other_end(p, p.adj_edge[mid], node) < nb) lo = mid + 1; else hi = mid;
  }
  for (long k = lo; k < end; ++k) {
    const long e = p.adj_edge[k];
    if (other_end(p, e, node) != nb) break;
    if (p.use[e]) return e;
  }
  return -1;
}
// slot k of a's list, for the used edge e = (a, b): 1 iff it is a used edge to a third node c that b also reaches by a used edge, and
// the cycle a -> b -> c -> a passes the test
ROT_HD int support_slot(const P& p, long e, long k) {
  const int a = p.edge_image[2 * e], b = p.edge_image[2 * e + 1];
  const long ea = p.adj_edge[k];
  if (!p.use[ea]) return 0;
  const int c = other_end(p, ea, a);
  if (c == b) return 0;
  const long eb = find_used(p, b, c);
  if (eb < 0) return 0;
  double q_bc[4], q_ca[4], t[4], cyc[4];
  edge_quat_from(p, eb, b, q_bc);
  edge_quat_from(p, ea, c, q_ca);
  qmul(q_bc, p.q + 4 * e, t);
  qmul(q_ca, t, cyc);
  return fabs(cyc[0]) >= p.cos_half ? 1 : 0;
}

// ---- rule 5: the word of the spanning forest ------------------------------------------------------------------------------------------
ROT_HD uint64_t word(const P& p, long e) {
  const int s = p.support[e], w = p.edge_weight[e];
  return ((uint64_t)(s < 0xFFFF ? s : 0xFFFF) << 48) | ((uint64_t)(w < 0xFFFF ? w : 0xFFFF) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)e);
}
ROT_HD long word_edge(uint64_t w) { return (long)(0xFFFFFFFFu - (uint32_t)w); }

// ---- rule 6: start values -------------------------------------------------------------------------------------------------------------
ROT_HD void root_setup(const P& p, int root) {
  p.ctrl->root = root;
  if (root < 0) return;
  p.depth[root] = 0;
  double* q = p.qn + 4 * (long)root;
  q[0] = 1.0; q[1] = 0.0; q[2] = 0.0; q[3] = 0.0;
}
// tree edge e at level L: when one end was set at level L - 1 and the other is not set, the other takes its value -> 1, else 0
ROT_HD int start_edge(const P& p, long e, int L) {
  const int a = p.edge_image[2 * e], b = p.edge_image[2 * e + 1];
  const int da = p.depth[a], db = p.depth[b];
  int parent, child;
  if (da == L - 1 && db < 0) { parent = a; child = b; }
  else if (db == L - 1 && da < 0) { parent = b; child = a; }
  else return 0;
  double qe[4], qc[4];
  edge_quat_from(p, e, parent, qe);
  qmul(qe, p.qn + 4 * (long)parent, qc);
  qnormalise(qc);
  double* o = p.qn + 4 * (long)child;
  o[0] = qc[0]; o[1] = qc[1]; o[2] = qc[2]; o[3] = qc[3];
  p.depth[child] = L;
  return 1;
}
// after the last level: the depth of the tree, and "nothing to do" when the root has no used edge
ROT_HD void start_finish(const P& p, int depth) {
  Ctrl& c = *p.ctrl;
  c.depth = depth;
  if (depth < 1) { c.done = 1; c.status = kNothing; }
}

// ---- rule 7: refinement ---------------------------------------------------------------------------------------------------------------
ROT_HD bool in_graph(const P& p, int i) { return p.depth[i] >= 0; }
ROT_HD bool edge_active(const P& p, long e) { return p.use[e] && in_graph(p, p.edge_image[2 * e]) && in_graph(p, p.edge_image[2 * e + 1]); }
ROT_HD bool node_free(const P& p, int i) { return in_graph(p, i) && i != p.ctrl->root; }

// r = 2 vec(conj(q_b) (x) q_ab (x) q_a) with the sign that makes the scalar part non-negative -> |r|^2
ROT_HD double residual(const P& p, long e, double* r) {
  const int a = p.edge_image[2 * e], b = p.edge_image[2 * e + 1];
  const double* qb = p.qn + 4 * (long)b;
  const double cb[4] = {qb[0], -qb[1], -qb[2], -qb[3]};
  double t[4], ee[4];
  qmul(p.q + 4 * e, p.qn + 4 * (long)a, t);
  qmul(cb, t, ee);
  const double s = ee[0] < 0.0 ? -2.0 : 2.0;
  r[0] = s * ee[1]; r[1] = s * ee[2]; r[2] = s * ee[3];
  return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
}
// residual, Geman-McClure weight and cost term of edge e at the state
ROT_HD void edge_eval(const P& p, long e) {
  double r[3] = {0.0, 0.0, 0.0}, w = 0.0, cost = 0.0;
  if (edge_active(p, e)) {
    const double r2 = residual(p, e, r);
    const double s = p.d2 / (p.d2 + r2), wt = (double)p.edge_weight[e];
    w = wt * (s * s);
    cost = wt * (s * r2);
  }
  p.r3[3 * e] = r[0]; p.r3[3 * e + 1] = r[1]; p.r3[3 * e + 2] = r[2];
  p.w[e] = w;
  p.part[e] = cost;
}
// node i: the diagonal and the right-hand side over its list in order, and the conjugate gradients' start (x = 0, r = g, z, p = z)
ROT_HD void node_rhs(const P& p, int i) {
  double d = 0.0, g[3] = {0.0, 0.0, 0.0};
  const bool fr = node_free(p, i);
  if (fr)
    for (long k = p.adj_offsets[i]; k < p.adj_offsets[i + 1]; ++k) {
      const long e = p.adj_edge[k];
      if (!p.use[e]) continue;
      const double w = p.w[e];
      d = d + w;
      if (p.edge_image[2 * e + 1] == i) for (int c = 0; c < 3; ++c) g[c] = g[c] + w * p.r3[3 * e + c];
      else for (int c = 0; c < 3; ++c) g[c] = g[c] - w * p.r3[3 * e + c];
    }
  p.diag[i] = d;
  for (int c = 0; c < 3; ++c) {
    const long j = 3L * i + c;
    const double z = fr && d > 0.0 ? g[c] / d : 0.0;
    p.x[j] = 0.0; p.rr[j] = g[c]; p.z[j] = z; p.pp[j] = z; p.Lp[j] = 0.0;
    p.part[j] = g[c] * z;
  }
}
// node i: (L p)_i over its list in order; part = p . L p
ROT_HD void node_Lp(const P& p, int i) {
  double s[3] = {0.0, 0.0, 0.0};
  if (node_free(p, i))
    for (long k = p.adj_offsets[i]; k < p.adj_offsets[i + 1]; ++k) {
      const long e = p.adj_edge[k];
      if (!p.use[e]) continue;
      const double w = p.w[e];
      const long j = other_end(p, e, i);
      for (int c = 0; c < 3; ++c) s[c] = s[c] + w * (p.pp[3L * i + c] - p.pp[3 * j + c]);
    }
  for (int c = 0; c < 3; ++c) {
    p.Lp[3L * i + c] = s[c];
    p.part[3L * i + c] = p.pp[3L * i + c] * s[c];
  }
}
// node i: x += alpha p, r -= alpha L p, z = r / diag; part = r . z
ROT_HD void node_update(const P& p, int i) {
  const bool fr = node_free(p, i);
  const double alpha = p.ctrl->alpha, d = p.diag[i];
  for (int c = 0; c < 3; ++c) {
    const long j = 3L * i + c;
    if (!fr) { p.part[j] = 0.0; continue; }
    p.x[j] = p.x[j] + alpha * p.pp[j];
    p.rr[j] = p.rr[j] - alpha * p.Lp[j];
    p.z[j] = d > 0.0 ? p.rr[j] / d : 0.0;
    p.part[j] = p.rr[j] * p.z[j];
  }
}
// node i: p = z + beta p
ROT_HD void node_direction(const P& p, int i) {
  if (!node_free(p, i)) return;
  const double beta = p.ctrl->beta;
  for (int c = 0; c < 3; ++c) p.pp[3L * i + c] = p.z[3L * i + c] + beta * p.pp[3L * i + c];
}
// node i: the trial q_i (x) (1, omega_i / 2), normalised -> |omega_i|^2, or -1 for a step that is not finite
ROT_HD double node_apply(const P& p, int i) {
  if (!in_graph(p, i)) return 0.0;
  const double* q = p.qn + 4 * (long)i;
  double* o = p.qt + 4 * (long)i;
  if (!node_free(p, i)) { o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3]; return 0.0; }
  const double* om = p.x + 3L * i;
  const double n2 = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2];
  const double dq[4] = {1.0, 0.5 * om[0], 0.5 * om[1], 0.5 * om[2]};
  double t[4];
  qmul(q, dq, t);
  qnormalise(t);
  o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3];
  return ba::fin(n2) && ba::fin(t[0]) && ba::fin(t[1]) && ba::fin(t[2]) && ba::fin(t[3]) ? n2 : -1.0;
}
// node i: the trial becomes the state (not after a step that was not finite)
ROT_HD void node_commit(const P& p, int i) {
  if (p.ctrl->bad || !in_graph(p, i)) return;
  for (int c = 0; c < 4; ++c) p.qn[4L * i + c] = p.qt[4L * i + c];
}
// the owner of the scalars receives a finished sum
ROT_HD void feed(const P& p, int action, double v) {
  Ctrl& c = *p.ctrl;
  if (action == kActCost || action == kActCostFinal) {
    c.cost = v;
    if (!c.have0) { c.cost0 = v; c.have0 = 1; }
    if (action == kActCostFinal && !c.done) c.status = kMaxIters;
  } else if (action == kActRz0) {
    c.rz0 = v; c.rz = v;
    c.pcg_done = v <= p.pcg_tol2 * v;
  } else if (action == kActPLp) {
    c.alpha = c.rz / v;
    ++c.n_pcg;
  } else {
    c.beta = v / c.rz;
    c.rz = v;
    c.pcg_done = v <= p.pcg_tol2 * c.rz0;
  }
}
// ... and closes an outer iteration after the commit
ROT_HD void decide(const P& p) {
  Ctrl& c = *p.ctrl;
  if (c.done) return;
  if (c.bad) { c.status = kStalled; c.done = 1; return; }
  ++c.n_iters;
  c.last_step = sqrt(double_of(c.step_bits));
  c.step_bits = 0;
  if (c.last_step < p.step_tol) { c.status = kConverged; c.done = 1; }
}
ROT_HD bool refine_idle(const P& p) { return p.ctrl->done != 0; }
ROT_HD bool pcg_idle(const P& p) { return p.ctrl->done != 0 || p.ctrl->pcg_done != 0; }

// ---- rule 8: verdict ------------------------------------------------------------------------------------------------------------------
// edge e: its state and its chord at the final state (NaN without a verdict); writes the per-edge outputs
ROT_HD int edge_verdict(const P& p, long e) {
  int st;
  double chord = nan64();
  if (!p.valid[e]) st = kInvalid;
  else if (!in_graph(p, p.edge_image[2 * e]) || !in_graph(p, p.edge_image[2 * e + 1])) st = kOutside;
  else {
    double r[3];
    chord = sqrt(residual(p, e, r));
    st = chord <= p.max_chord ? kOk : kOutlier;
  }
  p.edge_state[e] = (uint8_t)st;
  p.edge_chord[e] = chord;
  p.support_out[e] = p.support[e];
  p.tree_out[e] = p.tree[e];
  p.use_out[e] = p.use[e];
  return st;
}
// node i: its matrix (NaN outside the graph) and in_graph
ROT_HD void node_write(const P& p, int i) {
  double* R = p.R + 9L * i;
  const bool in = in_graph(p, i);
  p.in_graph[i] = (uint8_t)in;
  if (in) ba::matrix_from_quat(p.qn + 4L * i, R);
  else for (int k = 0; k < 9; ++k) R[k] = nan64();
}
// the counts and info the owner of the scalars holds
ROT_HD void finish(const P& p) {
  const Ctrl& c = *p.ctrl;
  p.counts[kDepth] = (unsigned long long)c.depth;
  p.counts[kIters] = (unsigned long long)c.n_iters;
  p.counts[kPcgIters] = (unsigned long long)c.n_pcg;
  p.counts[kStatus] = (unsigned long long)c.status;
  p.counts[kRoot] = (unsigned long long)(long long)c.root;
  p.info[0] = c.cost0; p.info[1] = c.cost; p.info[2] = c.last_step; p.info[3] = double_of(c.chord_bits);
}

// ---- arguments ------------------------------------------------------------------------------------------------------------------------
struct Args {
  const int* edge_image; const double* edge_R; const int* edge_weight; long E; int n_images, root;
  const long* adj_offsets; const int* adj_edge; const uint8_t* edge_use_in;
  double cycle_cos_half, loss_chord, max_chord, step_tol; int max_iters, pcg_iters; double pcg_tol;
  double* R; uint8_t* in_graph; uint8_t* edge_state; double* edge_chord; int* support; uint8_t* tree; uint8_t* edge_use; long* counts;
  double* info;
};
inline int check_args(const Args& a) {
  if (!a.counts || !a.info || a.E < 0 || a.n_images < 0 || !a.adj_offsets || (a.n_images == 0 && a.E > 0)) return LOFTR_ERR_BAD_ARG;
  if (a.E > 0 && (!a.edge_image || !a.edge_R || !a.edge_weight || !a.adj_edge || !a.edge_use_in || !a.edge_state || !a.edge_chord ||
                  !a.support || !a.tree || !a.edge_use))
    return LOFTR_ERR_BAD_ARG;
  if (a.n_images > 0 && (!a.R || !a.in_graph)) return LOFTR_ERR_BAD_ARG;
  if (!ba::fin(a.cycle_cos_half) || !ba::fin(a.loss_chord) || !(a.loss_chord > 0.0) || !ba::fin(a.max_chord) || !(a.max_chord >= 0.0) ||
      !ba::fin(a.step_tol) || !(a.step_tol >= 0.0) || !(a.pcg_tol >= 0.0) || !(a.pcg_tol < 1.0) || a.max_iters < 0 || a.pcg_iters < 0)
    return LOFTR_ERR_BAD_ARG;
  if (!sizes_ok(a.E, a.n_images) || a.max_iters > (1 << 16) || a.pcg_iters > (1 << 16)) return LOFTR_ERR_UNSUPPORTED;
  return LOFTR_OK;
}
inline P problem(const Args& a) {
  P p{};
  p.edge_image = a.edge_image; p.edge_R = a.edge_R; p.edge_weight = a.edge_weight; p.E = a.E; p.n = a.n_images; p.root_arg = a.root;
  p.adj_offsets = a.adj_offsets; p.adj_edge = a.adj_edge; p.edge_use_in = a.edge_use_in;
  p.cos_half = a.cycle_cos_half; p.d2 = a.loss_chord * a.loss_chord; p.max_chord = a.max_chord; p.step_tol = a.step_tol;
  p.pcg_tol2 = a.pcg_tol * a.pcg_tol; p.max_iters = a.max_iters; p.pcg_iters = a.pcg_iters; p.rounds = rounds_of(a.n_images);
  p.R = a.R; p.in_graph = a.in_graph; p.edge_state = a.edge_state; p.edge_chord = a.edge_chord; p.support_out = a.support;
  p.tree_out = a.tree; p.use_out = a.edge_use; p.counts = (unsigned long long*)a.counts; p.info = a.info;
  return p;
}

}  // namespace rot
