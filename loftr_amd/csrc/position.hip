// Global positioning, host routine (plain C++ on host arrays, double precision): with one rotation per image fixed, the camera centres,
// the points and one scale per observation from the tracks, all at once (the contract is in include/loftr_global.h).  What
// the global-positioning stage of a global SfM pipeline does (Pan et al., "Global Structure-from-Motion Revisited"); this is a statement
// of the published idea as an order-defined rule, NOT of anybody's source.  PARITY UNPINNED.
// This function DEFINES the result: loftr_global_positions (position_gpu.hip) reproduces it bit for bit, which is why every per-item
// step lives in position_core.h and this file is only the sequence of phases, the breadth-first levels and the order-defined sums.
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "position_core.h"

#pragma clang fp contract(off)

using namespace pos;

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
// the osum64 of K-vectors over camera i's list: term(o, out[K]) of the k-th observation goes to accumulator k % 64
template <int K, class Term> void cam_osum64(const P& p, int i, Term term, double* out) {
  double a[64][K];
  for (int l = 0; l < 64; ++l) for (int k = 0; k < K; ++k) a[l][k] = 0.0;
  const long b = p.cam_offsets[i], e = p.cam_offsets[i + 1];
  for (long s = b; s < e; ++s) {
    double t[K];
    term(p.cam_obs[s], t);
    for (int k = 0; k < K; ++k) a[(s - b) % 64][k] = a[(s - b) % 64][k] + t[k];
  }
  for (int s = 32; s >= 1; s >>= 1)
    for (int l = 0; l < s; ++l) for (int k = 0; k < K; ++k) a[l][k] = a[l][k] + a[l + s][k];
  for (int k = 0; k < K; ++k) out[k] = a[0][k];
}

}  // namespace

extern "C" int loftr_global_abi_version(void) { return LOFTR_GLOBAL_ABI_VERSION; }

extern "C" int loftr_global_positions_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, long N,
                                           const long* cam_offsets, const int* cam_obs, const double* K, const double* R,
                                           const uint8_t* in_graph, int n_images, int root, const int* tree_image, const double* tree_t,
                                           long Et, double huber, int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_cam_obs,
                                           double* centres, float* xyz, double* depth_scale, uint8_t* obs_state, uint8_t* cam_state,
                                           uint8_t* point_active, long* counts, double* info) {
  const Args a{offsets, T, obs_image, obs_xy, N, cam_offsets, cam_obs, K, R, in_graph, n_images, root, tree_image, tree_t, Et, huber,
               max_iters, pcg_iters, pcg_tol, ftol, min_cam_obs, centres, xyz, depth_scale, obs_state, cam_state, point_active, counts, info};
  const int st = check_args(a);
  if (st != LOFTR_OK) return st;
  P p = problem(a);
  std::vector<char> ws(layout(p, nullptr), 0);
  layout(p, ws.data());
  const int n = p.n;
  Ctrl& c = *p.ctrl;
  for (int k = 0; k < kCounts; ++k) counts[k] = 0;
  for (int k = 0; k < kInfo; ++k) info[k] = 0.0;
  memset(centres, 0, sizeof(double) * 3 * (size_t)n);
  memset(cam_state, 0, (size_t)n);
  if (N > 0) { memset(depth_scale, 0, sizeof(double) * (size_t)N); memset(obs_state, 0, (size_t)N); }
  if (T > 0) { memset(xyz, 0, sizeof(float) * 3 * (size_t)T); memset(point_active, 0, (size_t)T); }
  ctrl_init(p);

  // rule 1: checks
  int err = 0;
  for (long t = 0; t < T; ++t) err |= track_check(p, t);
  for (int i = 0; i < n; ++i) err |= cam_check(p, i);
  for (long e = 0; e < Et; ++e) err |= tree_check(p, e);
  counts[kErrors] = err;
  if (err) return LOFTR_ERR_BAD_ARG;

  // rule 4: the cameras' start values, level by level; then whether the tree is one
  root_setup(p);
  int depth = 0;
  for (int L = 1; L <= n; ++L) {
    int set = 0;
    for (long e = 0; e < Et; ++e) set |= start_tree_edge(p, e, L);
    if (!set) break;
    depth = L;
  }
  c.depth = depth;
  for (long e = 0; e < Et; ++e) err |= tree_claim(p, e);
  for (long e = 0; e < Et; ++e) err |= tree_verify(p, e);
  counts[kErrors] = err;
  if (err) return LOFTR_ERR_BAD_ARG;

  // rules 2, 3, 4: bearings, who takes part, the start values of points and scales
  for (long o = 0; o < N; ++o) obs_bearing(p, o);
  for (long t = 0; t < T; ++t) {
    const long cnt = track_setup(p, t);
    counts[kActiveObs] += cnt;
    counts[kActivePoints] += cnt > 0;
  }
  for (int i = 0; i < n; ++i) {
    const int s = cam_setup(p, i);
    counts[kInGraph] += s != kOutside;
    counts[kFree] += s == kSolved;
    counts[kChained] += s == kChainedOnly;
  }
  for (long e = 0; e < Et; ++e) counts[kNoDirection] += p.nodir[e];
  for (long t = 0; t < T; ++t) point_start(p, t);

  // rule 5: refinement
  auto dot = [&](int action) { feed(p, action, osum(p.part, 3L * n)); };
  for (long o = 0; o < N; ++o) obs_eval(p, o, 0);
  feed(p, kActCost0, osum(p.part, N));
  for (int it = 0; it < max_iters && !refine_idle(p); ++it) {
    for (long o = 0; o < N; ++o) obs_linearise(p, o);
    for (long t = 0; t < T; ++t) if (!point_factor(p, t)) c.bad = 1;
    for (int i = 0; i < n; ++i) {
      double s[kSetupSums] = {};
      if (cam_free(p, i)) cam_osum64<kSetupSums>(p, i, [&](long o, double* out) { cam_term_setup(p, o, out); }, s);
      if (!cam_finish_setup(p, i, s)) c.bad = 1;
    }
    dot(kActRz0);
    for (int k = 0; k < pcg_iters && !pcg_idle(p); ++k) {
      for (long t = 0; t < T; ++t) point_u(p, t, p.pp);
      for (int i = 0; i < n; ++i) {
        double s[kSpSums] = {};
        if (cam_free(p, i)) cam_osum64<kSpSums>(p, i, [&](long o, double* out) { cam_term_Sp(p, o, out); }, s);
        cam_finish_Sp(p, i, s);
      }
      dot(kActPsp);
      if (pcg_idle(p)) break;
      for (int i = 0; i < n; ++i) cam_update(p, i);
      dot(kActRz);
      if (pcg_idle(p)) break;
      for (int i = 0; i < n; ++i) cam_direction(p, i);
    }
    double step2 = 0.0;
    for (int i = 0; i < n; ++i) {
      const double v = cam_apply(p, i);
      if (v < 0.0) c.bad = 1;
      else if (v > step2) step2 = v;
    }
    c.step_bits = bits_of(step2);
    for (long t = 0; t < T; ++t) point_u(p, t, p.x);
    for (long t = 0; t < T; ++t) if (!point_apply(p, t)) c.bad = 1;
    for (long o = 0; o < N; ++o) if (!obs_apply(p, o)) c.bad = 1;
    for (long o = 0; o < N; ++o) obs_eval(p, o, 1);
    feed(p, kActCostT, osum(p.part, N));
    accept(p);
    if (commit_now(p)) {
      for (int i = 0; i < n; ++i) cam_commit(p, i);
      for (long t = 0; t < T; ++t) point_commit(p, t);
      for (long o = 0; o < N; ++o) obs_commit(p, o);
    }
  }

  // rule 7: outputs
  for (long o = 0; o < N; ++o) counts[kNegative] += obs_write(p, o);
  for (long t = 0; t < T; ++t) track_write(p, t);
  for (int i = 0; i < n; ++i) cam_write(p, i);
  finish(p);
  return LOFTR_OK;
}
