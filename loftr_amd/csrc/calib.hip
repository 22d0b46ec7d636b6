// View-graph calibration, host routine (plain C++ on host arrays, double precision): one focal-length scale per camera from the
// fundamental matrices of all verified pairs at once (the contract is in include/loftr_calib.h).  What the view-graph
// calibration step of a global SfM pipeline does; this is a statement of the published idea as an order-defined rule, NOT of
// anybody's source.  PARITY UNPINNED.
// This function DEFINES the result: loftr_calibrate_view_graph (calib_gpu.hip) reproduces it bit for bit, which is why every per-item
// step lives in calib_core.h and this file is only the sequence of phases and the order-defined sums.
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "calib_core.h"

#pragma clang fp contract(off)

using namespace vg;

namespace {

// §18's osum64 of `count` terms: 64 accumulators taken in turn, folded 32, 16, ..., 1
double osum64(const double* v, long count) {
  double a[64];
  for (int l = 0; l < 64; ++l) a[l] = 0.0;
  for (long e = 0; e < count; ++e) a[e % 64] = a[e % 64] + v[e];
  for (int s = 32; s >= 1; s >>= 1)
    for (int l = 0; l < s; ++l) a[l] = a[l] + a[l + s];
  return a[0];
}
// §18's osum of v[0 .. count): osum64 per chunk of 4096, then osum of the chunk sums
double osum(const double* v, long count) {
  std::vector<double> cur(v, v + count), next;
  for (;;) {
    const long chunks = chunks_of((long)cur.size());
    next.assign((size_t)chunks, 0.0);
    for (long b = 0; b < chunks; ++b) {
      const long lo = b * kChunk, len = std::min((long)cur.size() - lo, (long)kChunk);
      next[(size_t)b] = osum64(cur.data() + lo, std::max(len, 0L));
    }
    if (chunks <= 1) return next[0];
    cur.swap(next);
  }
}
// the osum64 of K-vectors over group g's incidence list: term(code, out[K]) of the k-th slot goes to accumulator k % 64
template <int K, class Term> void group_osum64(const P& p, int g, Term term, double* out) {
  double a[64][K];
  for (int l = 0; l < 64; ++l) for (int k = 0; k < K; ++k) a[l][k] = 0.0;
  const long b = p.grp_offsets[g], e = p.grp_offsets[g + 1];
  for (long s = b; s < e; ++s) {
    double t[K];
    term(p.grp_inc[s], t);
    for (int k = 0; k < K; ++k) a[(s - b) % 64][k] = a[(s - b) % 64][k] + t[k];
  }
  for (int s = 32; s >= 1; s >>= 1)
    for (int l = 0; l < s; ++l) for (int k = 0; k < K; ++k) a[l][k] = a[l][k] + a[l + s][k];
  for (int k = 0; k < K; ++k) out[k] = a[0][k];
}

}  // namespace

extern "C" int loftr_calib_abi_version(void) { return LOFTR_CALIB_ABI_VERSION; }

extern "C" int loftr_calibrate_view_graph_host(const int* edge_image, const double* edge_F, const int* edge_weight, long E, const double* pp,
                                               const double* f0, const int* group, int n_images, int n_groups, const long* grp_offsets,
                                               const int* grp_inc, double loss, double max_resid, double prior_weight, int weight_cap,
                                               double bound_lo, double bound_hi, int min_edges, int max_iters, int pcg_iters, double pcg_tol,
                                               double ftol, double* focal_scale, double* focal, double* edge_resid, uint8_t* edge_state,
                                               uint8_t* group_state, long* counts, double* info) {
  const Args a{edge_image, edge_F, edge_weight, E, pp, f0, group, n_images, n_groups, grp_offsets, grp_inc, loss, max_resid, prior_weight,
               weight_cap, bound_lo, bound_hi, min_edges, max_iters, pcg_iters, pcg_tol, ftol, focal_scale, focal, edge_resid, edge_state,
               group_state, counts, info};
  const int st = vg_check_args(a);
  if (st != LOFTR_OK) return st;
  P p = vg_problem(a);
  std::vector<char> ws(layout(p, nullptr), 0);
  layout(p, ws.data());
  const int n = p.n, G = p.G;
  Ctrl& c = *p.ctrl;
  for (int k = 0; k < kCounts; ++k) counts[k] = 0;
  for (int k = 0; k < kInfo; ++k) info[k] = 0.0;
  memset(focal_scale, 0, sizeof(double) * (size_t)G);
  memset(group_state, 0, (size_t)G);
  memset(focal, 0, sizeof(double) * (size_t)n);
  if (E > 0) { memset(edge_resid, 0, sizeof(double) * (size_t)E); memset(edge_state, 0, (size_t)E); }
  vg_ctrl_init(p);

  // step 1: checks
  int err = 0;
  for (long e = 0; e < E; ++e) err |= vg_edge_check(p, e);
  for (int i = 0; i < n; ++i) err |= vg_image_check(p, i);
  for (int g = 0; g < G; ++g) err |= vg_group_check(p, g);
  for (long k = 0; k < 2 * E; ++k) err |= vg_slot_check(p, k);
  counts[kErrors] = err;
  if (err) return LOFTR_ERR_BAD_ARG;

  // steps 2, 3: edges, groups, the cost of the start values
  for (long e = 0; e < E; ++e) counts[kValidEdges] += vg_edge_setup(p, e);
  for (int g = 0; g < G; ++g) counts[kFreeGroups] += vg_group_setup(p, g) == kRefined;
  for (long e = 0; e < E; ++e) vg_edge_eval(p, e, 0);
  for (int g = 0; g < G; ++g) vg_group_eval(p, g, 0);
  vg_feed(p, kActCost0, osum(p.part, E + G));

  // steps 4 to 7: refinement
  auto dot = [&](int action) { vg_feed(p, action, osum(p.part, G)); };
  for (int it = 0; it < max_iters && !vg_refine_idle(p); ++it) {
    for (long e = 0; e < E; ++e) vg_edge_linearise(p, e);
    for (int g = 0; g < G; ++g) {
      double s[kSetupSums] = {};
      if (vg_group_free(p, g)) group_osum64<kSetupSums>(p, g, [&](int code, double* out) { vg_term_setup(p, g, code, out); }, s);
      if (!vg_group_finish_setup(p, g, s)) c.bad = 1;
    }
    dot(kActRz0);
    for (int k = 0; k < pcg_iters && !vg_pcg_idle(p); ++k) {
      for (int g = 0; g < G; ++g) {
        double s[kApSums] = {};
        if (vg_group_free(p, g)) group_osum64<kApSums>(p, g, [&](int code, double* out) { vg_term_Ap(p, g, code, out); }, s);
        vg_group_finish_Ap(p, g, s);
      }
      dot(kActPap);
      if (vg_pcg_idle(p)) break;
      for (int g = 0; g < G; ++g) vg_group_update(p, g);
      dot(kActRz);
      if (vg_pcg_idle(p)) break;
      for (int g = 0; g < G; ++g) vg_group_direction(p, g);
    }
    double step2 = 0.0;
    for (int g = 0; g < G; ++g) {
      const double v = vg_group_apply(p, g);
      if (v == -1.0) c.bad = 1;
      else if (v == -2.0) c.oob = 1;
      else if (v > step2) step2 = v;
    }
    c.step_bits = bits_of(step2);
    for (long e = 0; e < E; ++e) vg_edge_eval(p, e, 1);
    for (int g = 0; g < G; ++g) vg_group_eval(p, g, 1);
    vg_feed(p, kActCostT, osum(p.part, E + G));
    vg_accept(p);
    if (vg_commit_now(p))
      for (int g = 0; g < G; ++g) vg_group_commit(p, g);
  }

  // step 8: outputs
  for (long e = 0; e < E; ++e) counts[kOutliers] += vg_edge_write(p, e);
  for (int i = 0; i < n; ++i) vg_image_write(p, i);
  for (int g = 0; g < G; ++g) vg_group_write(p, g);
  vg_finish(p);
  return LOFTR_OK;
}
