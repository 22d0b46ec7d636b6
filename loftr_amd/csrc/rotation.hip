// Rotation averaging over the view graph, host routine (plain C++ on host arrays, double precision): the pairwise rotations of the image
// pairs as a graph; cycle support per edge, a maximum spanning forest that prefers supported edges, start values along the tree, a
// robust (Geman-McClure) Gauss-Newton refinement of one rotation per image, and a verdict per pair (the contract is in
// include/loftr_hip.h).  What the rotation-averaging stage of a global SfM pipeline does (Chatterjee and Govindu, "Efficient and Robust
// Large-Scale Rotation Averaging"; Zach et al., "Disambiguating Visual Relations Using Loop Constraints"); none of those pipelines is
// in this image, so this is a statement of the published idea as an order-defined rule, NOT of their source.  PARITY UNPINNED.
// This function DEFINES the result: loftr_rotation_averaging (rotation_gpu.hip) reproduces it bit for bit, which is why every per-item
// step lives in rotation_core.h and this file is only the sequence of phases, Kruskal's forest and the order-defined sums.
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/loftr_hip.h"
#include "rotation_core.h"

#pragma clang fp contract(off)

using namespace rot;

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

int find(std::vector<int>& up, int i) {
  while (up[(size_t)i] != i) {
    up[(size_t)i] = up[(size_t)up[(size_t)i]];
    i = up[(size_t)i];
  }
  return i;
}

}  // namespace

extern "C" int loftr_rotation_averaging_host(const int* edge_image, const double* edge_R, const int* edge_weight, long E, int n_images, int root,
                                             const long* adj_offsets, const int* adj_edge, const uint8_t* edge_use_in, double cycle_cos_half,
                                             double loss_chord, double max_chord, double step_tol, int max_iters, int pcg_iters, double pcg_tol,
                                             double* R, uint8_t* in_graph_out, uint8_t* edge_state, double* edge_chord, int* support,
                                             uint8_t* tree, uint8_t* edge_use, long* counts, double* info) {
  const Args a{edge_image, edge_R, edge_weight, E, n_images, root, adj_offsets, adj_edge, edge_use_in, cycle_cos_half, loss_chord, max_chord,
               step_tol, max_iters, pcg_iters, pcg_tol, R, in_graph_out, edge_state, edge_chord, support, tree, edge_use, counts, info};
  const int st = check_args(a);
  if (st != LOFTR_OK) return st;
  P p = problem(a);
  std::vector<char> ws(layout(p, nullptr), 0);
  layout(p, ws.data());
  const int n = p.n;
  Ctrl& c = *p.ctrl;

  // rules 1, 2: checks, valid and used edges, quaternions
  int err = 0;
  for (long e = 0; e < E; ++e) err |= edge_setup(p, e);
  for (int i = 0; i < std::max(n, 1); ++i) err |= node_check(p, i);
  for (int k = 0; k < kCounts; ++k) counts[k] = 0;
  counts[kErrors] = err;
  if (err) return LOFTR_ERR_BAD_ARG;
  for (int k = 0; k < kInfo; ++k) info[k] = 0.0;

  // rule 3: cycle support
  for (long e = 0; e < E; ++e) {
    if (!p.use[e]) continue;
    const int u = edge_image[2 * e];
    int s = 0;
    for (long k = adj_offsets[u]; k < adj_offsets[u + 1]; ++k) s += support_slot(p, e, k);
    p.support[e] = std::min(s, kMaxSupport);
  }

  // rule 4: the root
  int r = root;
  if (r < 0)
    for (int i = 0; i < n; ++i)
      if (r < 0 || p.wsum[i] > p.wsum[r]) r = i;
  root_setup(p, r);

  // rule 5: the maximum spanning forest under the strict order of the words (Kruskal)
  std::vector<uint64_t> words;
  for (long e = 0; e < E; ++e) if (p.use[e]) words.push_back(word(p, e));
  std::sort(words.begin(), words.end(), [](uint64_t x, uint64_t y) { return x > y; });
  std::vector<int> up((size_t)n);
  for (int i = 0; i < n; ++i) up[(size_t)i] = i;
  std::vector<int> tree_list;
  for (uint64_t w : words) {
    const long e = word_edge(w);
    const int x = find(up, edge_image[2 * e]), y = find(up, edge_image[2 * e + 1]);
    if (x == y) continue;
    up[(size_t)std::max(x, y)] = std::min(x, y);
    p.tree[e] = 1;
    tree_list.push_back((int)e);
  }

  // rule 6: start values, level by level
  int depth = 0;
  if (r >= 0)
    for (int L = 1; L <= n; ++L) {
      int set = 0;
      for (int e : tree_list) set |= start_edge(p, e, L);
      if (!set) break;
      depth = L;
    }
  start_finish(p, depth);

  // rule 7: refinement
  auto eval = [&](int action) {
    for (long e = 0; e < E; ++e) edge_eval(p, e);
    feed(p, action, osum(p.part, E));
  };
  auto dot = [&](int action) { feed(p, action, osum(p.part, 3L * n)); };
  for (int it = 0; it < max_iters && !refine_idle(p); ++it) {
    eval(kActCost);
    for (int i = 0; i < n; ++i) node_rhs(p, i);
    dot(kActRz0);
    for (int k = 0; k < pcg_iters && !pcg_idle(p); ++k) {
      for (int i = 0; i < n; ++i) node_Lp(p, i);
      dot(kActPLp);
      for (int i = 0; i < n; ++i) node_update(p, i);
      dot(kActRz);
      if (pcg_idle(p)) break;
      for (int i = 0; i < n; ++i) node_direction(p, i);
    }
    double step2 = 0.0;
    for (int i = 0; i < n; ++i) {
      const double v = node_apply(p, i);
      if (v < 0.0) c.bad = 1;
      else if (v > step2) step2 = v;
    }
    c.step_bits = bits_of(step2);
    for (int i = 0; i < n; ++i) node_commit(p, i);
    decide(p);
  }
  eval(kActCostFinal);

  // rule 8: verdict
  double chord = 0.0;
  for (long e = 0; e < E; ++e) {
    const int s = edge_verdict(p, e);
    counts[kInvalidEdges] += s == kInvalid;
    counts[kDuplicateEdges] += p.valid[e] && !p.use[e];
    counts[kUsedEdges] += p.use[e];
    counts[kSupportSum] += p.support[e];
    counts[kTreeEdges] += p.tree[e];
    counts[kTreeNoSupport] += p.tree[e] && p.support[e] == 0;
    counts[kOkEdges] += s == kOk;
    counts[kOutlierEdges] += s == kOutlier;
    if (s == kOk && edge_chord[e] > chord) chord = edge_chord[e];
  }
  c.chord_bits = bits_of(chord);
  for (int i = 0; i < n; ++i) {
    node_write(p, i);
    counts[kInGraph] += in_graph(p, i);
    counts[kComponents] += find(up, i) == i;
  }
  finish(p);
  return LOFTR_OK;
}
