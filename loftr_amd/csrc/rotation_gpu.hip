// Rotation averaging on the GPU (gfx950, wave64): loftr_rotation_averaging_host (rotation.hip) with the same result bit for bit (DESIGN
// §26).  Every per-item step is rotation_core.h's, compiled from the same text; what this file adds is only how the work is spread
// over threads.  A fixed schedule on the caller's stream, nothing read back:
//   memsets, rot_init_kernel    the counts and the scalars to 0;
//   rot_edge_setup_kernel       (thread per edge)  error bits 1 and 2, valid / used, the quaternion;
//   rot_node_check_kernel       (thread per node)  error bits 4 and 8, the sum of used weights and its maximum (64-bit atomicMax);
//   rot_support_kernel          (wave per edge)  a used edge's lanes take the slots of its first end's list in steps of 64; a lane
//                               looks its third node up in the other end's list by bisection; the votes are counted by ballot;
//   rot_root_kernel, rot_root_setup_kernel   the lowest image that holds the maximum (atomicMin); the root's start value;
//   per Boruvka round (ceil(log2 n) + 1 of them): a memset of best, then
//     rot_propose_kernel        (thread per edge)  an edge between two components does two unsigned 64-bit atomicMax into best;
//     rot_link_kernel           (thread per node)  a component's best edge enters the tree and the component points at the other one
//                               (a pair that chose each other: the lower label stays a root);
//     rot_jump_kernel           ceil(log2 n) launches of parent <- parent[parent]; the last one writes the labels;
//   rot_tree_list_kernel        (thread per edge)  the tree edges take slots of one list;
//   rot_start_kernel            ONE workgroup of 1024 loops over the levels of the tree with a block barrier; a level visits the tree
//                               edges with one end set at the level before and the other end not set;
//   per outer iteration: rot_eval_kernel (thread per edge), rot_node_kernel (thread per node, its list in order) for the right-hand
//     side, per conjugate-gradient iteration for L p, the update and the direction, each dot product by rot_osum_kernel (a wave per
//     4096 terms, one launch per level; lane 0 of the last level feeds the scalars); rot_apply_kernel (the largest step by a 64-bit
//     atomicMax of its bits), rot_node_kernel for the commit, rot_decide_kernel (one thread);
//   rot_eval_kernel + osum once more for the final cost, rot_write_kernel (thread per edge / node), rot_finish_kernel (one thread).
// A launch reads only what an earlier launch wrote.  Every launch after the checks returns at once when counts[1] is set, so nothing is
// read through a bad value and no output but the counts is written; the refinement's launches return at once when it has ended, the
// conjugate gradients' when they have.  No persistent or waiting kernel, no graph, no grid-wide barrier.  Integer atomics only.  Plain
// C++, ordinary vector stores.
#include <algorithm>
#include "rotation_core.h"
#include "stage_timer.h"

#pragma clang fp contract(off)

namespace {

using namespace rot;
typedef unsigned long long u64;

constexpr int kBlock = 256;
constexpr int kStartBlock = 1024;
inline unsigned blocks_of(long n, int per = kBlock) { return (unsigned)std::max((n + per - 1) / per, 1L); }

__device__ __forceinline__ bool bad_input(const P& p) { return p.counts[kErrors] != 0; }
__device__ __forceinline__ void add_votes(u64* counts, int slot, bool v) {
  const unsigned n = (unsigned)__popcll(__ballot(v));
  if (threadIdx.x % 64 == 0 && n) atomicAdd(counts + slot, (u64)n);
}

__global__ void rot_init_kernel(P p) {
  p.ctrl->root_min = 0xFFFFFFFFu;
  p.ctrl->root = -1;
}
// no image: the checks that remain, and "nothing to do" (no workspace)
__global__ void rot_empty_kernel(P p) {
  const int err = node_check(p, 0);
  if (err) p.counts[kErrors] = (u64)err;
  else {
    p.counts[kStatus] = (u64)kNothing;
    p.counts[kRoot] = (u64)(long long)-1;
  }
}

// grid ceil(E / 256) x 256
__global__ void __launch_bounds__(kBlock) rot_edge_setup_kernel(P p) {
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= p.E) return;
  const int err = edge_setup(p, e);
  if (err) atomicOr(p.counts + kErrors, (u64)err);
}

// grid ceil(max(n, 1) / 256) x 256
__global__ void __launch_bounds__(kBlock) rot_node_check_kernel(P p) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (p.n > 1 ? p.n : 1)) return;
  const int err = node_check(p, (int)i);
  if (err) atomicOr(p.counts + kErrors, (u64)err);
  else if (i < p.n) atomicMax(&p.ctrl->best_wsum, (u64)p.wsum[i]);
}

// a wave per edge, grid ceil(E / 4) x 256
__global__ void __launch_bounds__(kBlock) rot_support_kernel(P p) {
  if (bad_input(p)) return;
  const long e = (long)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (e >= p.E || !p.use[e]) return;                                              // (uniform in the wave)
  const int a = p.edge_image[2 * e];
  const long lo = p.adj_offsets[a], hi = p.adj_offsets[a + 1];
  int s = 0;
  for (long k0 = lo; k0 < hi; k0 += 64) {
    const long k = k0 + lane;
    s += __popcll(__ballot(k < hi && support_slot(p, e, k) != 0));
    if (s > kMaxSupport) s = kMaxSupport;
  }
  if (lane == 0) p.support[e] = s;
}

// grid ceil(n / 256) x 256
__global__ void __launch_bounds__(kBlock) rot_root_kernel(P p) {
  if (bad_input(p) || p.root_arg >= 0) return;
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i < p.n && (u64)p.wsum[i] == p.ctrl->best_wsum) atomicMin(&p.ctrl->root_min, (unsigned)i);
}
__global__ void rot_root_setup_kernel(P p) {
  if (bad_input(p)) return;
  root_setup(p, p.root_arg >= 0 ? p.root_arg : (p.n > 0 ? (int)p.ctrl->root_min : -1));
}

// the rounds' gate: a bad input, or a round before this one that accepted nothing (the same in every thread)
__device__ __forceinline__ bool round_idle(const P& p, int r) { return bad_input(p) || (r > 0 && p.accepted[r - 1] == 0); }

// grid ceil(E / 256) x 256
__global__ void __launch_bounds__(kBlock) rot_propose_kernel(P p, int r) {
  if (round_idle(p, r)) return;
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= p.E || !p.use[e]) return;
  const int la = p.label[p.edge_image[2 * e]], lb = p.label[p.edge_image[2 * e + 1]];
  if (la == lb) return;
  const u64 w = (u64)word(p, e);
  atomicMax(p.best + la, w);
  atomicMax(p.best + lb, w);
}

// grid ceil(n / 256) x 256
__global__ void __launch_bounds__(kBlock) rot_link_kernel(P p, int r) {
  if (round_idle(p, r)) return;
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  int up = p.label[i];
  if (up == (int)i && p.best[i] != 0) {
    const u64 w = p.best[i];
    const long e = word_edge((uint64_t)w);
    const int la = p.label[p.edge_image[2 * e]], lb = p.label[p.edge_image[2 * e + 1]];
    const int d = la == (int)i ? lb : la;
    p.tree[e] = 1;
    up = p.best[d] == w && (int)i < d ? (int)i : d;
    atomicAdd(p.accepted + r, 1);
  }
  p.parent[i] = up;
}

// grid ceil(n / 256) x 256.  In place: whatever a thread reads is an ancestor, so every launch at least doubles the distance covered.
__global__ void __launch_bounds__(kBlock) rot_jump_kernel(P p, int r, int last) {
  if (round_idle(p, r)) return;
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  const int up = p.parent[p.parent[i]];
  p.parent[i] = up;
  if (last) p.label[i] = up;
}

// grid ceil(E / 256) x 256
__global__ void __launch_bounds__(kBlock) rot_tree_list_kernel(P p) {
  if (bad_input(p)) return;
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e < p.E && p.tree[e]) p.tree_list[atomicAdd(&p.ctrl->n_tree, 1)] = (int)e;
}

// ONE workgroup of 1024.  A level reads the depths and values the level before wrote: the block-scope fence orders a thread's global
// writes before the barrier, after which the other threads of the workgroup read them.
__global__ void __launch_bounds__(kStartBlock) rot_start_kernel(P p) {
  if (bad_input(p)) return;
  const int n_tree = p.ctrl->n_tree;
  int depth = 0;
  if (p.ctrl->root >= 0)
    for (int L = 1; L <= p.n; ++L) {
      int set = 0;
      for (int k = threadIdx.x; k < n_tree; k += kStartBlock) set |= start_edge(p, p.tree_list[k], L);
      __threadfence_block();
      if (!__syncthreads_or(set)) break;
      depth = L;
    }
  if (threadIdx.x == 0) start_finish(p, depth);
}

// grid ceil(E / 256) x 256; final: the evaluation after the last iteration, which an ended refinement does not skip
__global__ void __launch_bounds__(kBlock) rot_eval_kernel(P p, int final) {
  if (bad_input(p) || (!final && refine_idle(p))) return;
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e < p.E) edge_eval(p, e);
}

// §18's osum64 of the elements [0, len) over the 64 lanes of a wave: lane l takes l, l + 64, ..., then the lanes are folded
__device__ __forceinline__ double wave_osum64(const double* v, long len, int lane) {
  double a = 0.0;
  for (long k = lane; k < len; k += 64) a = a + v[k];
  for (int s = 32; s >= 1; s >>= 1) {
    const double o = __shfl_down(a, s, 64);
    if (lane < s) a = a + o;
  }
  return a;
}
// one level of an osum: a wave per chunk of 4096, grid chunks x 64; on the last level lane 0 feeds the sum
__global__ void __launch_bounds__(64) rot_osum_kernel(P p, const double* in, long count, double* out, int action, int gate) {
  if (bad_input(p) || (gate == 1 && refine_idle(p)) || (gate == 2 && pcg_idle(p))) return;
  const int lane = threadIdx.x;
  const long lo = (long)blockIdx.x * kChunk, len = count - lo < kChunk ? count - lo : kChunk;
  const double a = wave_osum64(in + lo, len > 0 ? len : 0, lane);
  if (lane == 0) {
    if (action >= 0) feed(p, action, a);
    else out[blockIdx.x] = a;
  }
}

enum : int { kStepRhs = 0, kStepLp, kStepUpdate, kStepDirection, kStepCommit };
// grid ceil(n / 256) x 256: one per-node step of the refinement
__global__ void __launch_bounds__(kBlock) rot_node_kernel(P p, int step) {
  if (bad_input(p) || (step == kStepRhs || step == kStepCommit ? refine_idle(p) : pcg_idle(p))) return;
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  if (step == kStepRhs) node_rhs(p, (int)i);
  else if (step == kStepLp) node_Lp(p, (int)i);
  else if (step == kStepUpdate) node_update(p, (int)i);
  else if (step == kStepDirection) node_direction(p, (int)i);
  else node_commit(p, (int)i);
}

// grid ceil(n / 256) x 256
__global__ void __launch_bounds__(kBlock) rot_apply_kernel(P p) {
  if (bad_input(p) || refine_idle(p)) return;
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  const double v = node_apply(p, (int)i);
  if (v < 0.0) atomicOr(&p.ctrl->bad, 1);
  else if (v > 0.0) atomicMax(&p.ctrl->step_bits, (u64)bits_of(v));              // (the bits of doubles >= 0 order as the doubles do)
}
__global__ void rot_decide_kernel(P p) {
  if (!bad_input(p)) decide(p);
}

// grid ceil(max(E, n) / 256) x 256
__global__ void __launch_bounds__(kBlock) rot_write_kernel(P p) {
  if (bad_input(p)) return;                                                      // uniform: no output but the counts
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool edge = i < p.E, node = i < p.n;
  const int st = edge ? edge_verdict(p, i) : -1;
  if (st == kOk) atomicMax(&p.ctrl->chord_bits, (u64)bits_of(p.edge_chord[i]));
  if (node) node_write(p, (int)i);
  add_votes(p.counts, kInvalidEdges, st == kInvalid);
  add_votes(p.counts, kDuplicateEdges, edge && p.valid[i] && !p.use[i]);
  add_votes(p.counts, kUsedEdges, edge && p.use[i]);
  add_votes(p.counts, kTreeEdges, edge && p.tree[i]);
  add_votes(p.counts, kTreeNoSupport, edge && p.tree[i] && p.support[i] == 0);
  add_votes(p.counts, kOkEdges, st == kOk);
  add_votes(p.counts, kOutlierEdges, st == kOutlier);
  add_votes(p.counts, kInGraph, node && in_graph(p, (int)i));
  add_votes(p.counts, kComponents, node && p.label[i] == (int)i);
  long s = edge ? p.support[i] : 0;                                               // the sum of support: per wave first
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x % 64 == 0 && s) atomicAdd(p.counts + kSupportSum, (u64)s);
}
__global__ void rot_finish_kernel(P p) {
  if (!bad_input(p)) finish(p);
}

}  // namespace

extern "C" size_t loftr_rotation_averaging_workspace_bytes(long E, int n_images) {
  if (!sizes_ok(E, n_images) || n_images == 0) return 0;
  P p{};
  p.E = E; p.n = n_images;
  return layout(p, nullptr);
}

extern "C" int loftr_rotation_averaging(const int* edge_image, const double* edge_R, const int* edge_weight, long E, int n_images, int root,
                                        const long* adj_offsets, const int* adj_edge, const uint8_t* edge_use_in, double cycle_cos_half,
                                        double loss_chord, double max_chord, double step_tol, int max_iters, int pcg_iters, double pcg_tol,
                                        double* R, uint8_t* in_graph_out, uint8_t* edge_state, double* edge_chord, int* support, uint8_t* tree,
                                        uint8_t* edge_use, long* counts, double* info, void* ws, size_t ws_bytes, float* stage_ms,
                                        void* stream) {
  const Args a{edge_image, edge_R, edge_weight, E, n_images, root, adj_offsets, adj_edge, edge_use_in, cycle_cos_half, loss_chord, max_chord,
               step_tol, max_iters, pcg_iters, pcg_tol, R, in_graph_out, edge_state, edge_chord, support, tree, edge_use, counts, info};
  const int st = check_args(a);
  if (st != LOFTR_OK) return st;
  P p = problem(a);
  hipStream_t s = (hipStream_t)stream;
  const int n = n_images;
  if (n == 0) {                                                                    // (check_args: then E == 0)
    if (hipMemsetAsync(counts, 0, sizeof(long) * kCounts, s) != hipSuccess || hipMemsetAsync(info, 0, sizeof(double) * kInfo, s) != hipSuccess)
      return LOFTR_ERR_LAUNCH;
    hipLaunchKernelGGL(rot_empty_kernel, dim3(1), dim3(1), 0, s, p);
    LOFTR_CHECK_LAUNCH();
    if (stage_ms) for (int k = 0; k < LOFTR_ROTATION_STAGES; ++k) stage_ms[k] = 0.f;
    return LOFTR_OK;
  }
  LOFTR_CHECK_ARG(ws != nullptr);
  if (ws_bytes < layout(p, nullptr)) return LOFTR_ERR_WORKSPACE;
  layout(p, (char*)ws);
  const unsigned nbe = blocks_of(E), nbn = blocks_of(n), nbw = blocks_of(std::max(E, (long)n));
  StageTimer timer(stage_ms, LOFTR_ROTATION_STAGES, s);
  auto fill = [s](void* ptr, int v, size_t bytes) { return hipMemsetAsync(ptr, v, bytes, s) == hipSuccess; };
  // the levels of an osum of part[0 .. count) into `action`
  auto osum = [&](long count, int action, int gate) {
    const double* in = p.part;
    double* out = p.red;
    const long half = chunks_of(part_items(E, n));
    for (int level = 0;; ++level) {
      const long chunks = chunks_of(count);
      const bool last = chunks <= 1;
      hipLaunchKernelGGL(rot_osum_kernel, dim3((unsigned)chunks), dim3(64), 0, s, p, in, count, out, last ? action : -1, gate);
      if (last) break;
      in = out;
      out = p.red + (level % 2 == 0 ? half : 0);
      count = chunks;
    }
  };
  auto nodes = [&](int step) { hipLaunchKernelGGL(rot_node_kernel, dim3(nbn), dim3(kBlock), 0, s, p, step); };

  timer.mark();
  if (!fill(counts, 0, sizeof(long) * kCounts) || !fill(info, 0, sizeof(double) * kInfo) || !fill(p.ctrl, 0, sizeof(Ctrl)) ||
      !fill(p.accepted, 0, sizeof(int) * (size_t)p.rounds))
    return LOFTR_ERR_LAUNCH;
  hipLaunchKernelGGL(rot_init_kernel, dim3(1), dim3(1), 0, s, p);
  if (E > 0) hipLaunchKernelGGL(rot_edge_setup_kernel, dim3(nbe), dim3(kBlock), 0, s, p);
  hipLaunchKernelGGL(rot_node_check_kernel, dim3(nbn), dim3(kBlock), 0, s, p);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  if (E > 0) hipLaunchKernelGGL(rot_support_kernel, dim3(blocks_of(E, kBlock / 64)), dim3(kBlock), 0, s, p);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  if (n > 0) hipLaunchKernelGGL(rot_root_kernel, dim3(nbn), dim3(kBlock), 0, s, p);
  hipLaunchKernelGGL(rot_root_setup_kernel, dim3(1), dim3(1), 0, s, p);
  LOFTR_CHECK_LAUNCH();
  if (E > 0 && n > 0) {
    int jumps = 0;
    while ((1L << jumps) < n) ++jumps;
    for (int r = 0; r < p.rounds; ++r) {
      if (!fill(p.best, 0, sizeof(u64) * (size_t)n)) return LOFTR_ERR_LAUNCH;
      hipLaunchKernelGGL(rot_propose_kernel, dim3(nbe), dim3(kBlock), 0, s, p, r);
      hipLaunchKernelGGL(rot_link_kernel, dim3(nbn), dim3(kBlock), 0, s, p, r);
      for (int j = 0; j < std::max(jumps, 1); ++j)
        hipLaunchKernelGGL(rot_jump_kernel, dim3(nbn), dim3(kBlock), 0, s, p, r, j + 1 >= jumps ? 1 : 0);
      LOFTR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(rot_tree_list_kernel, dim3(nbe), dim3(kBlock), 0, s, p);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  hipLaunchKernelGGL(rot_start_kernel, dim3(1), dim3(kStartBlock), 0, s, p);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  if (E > 0 && n > 0)
    for (int it = 0; it < max_iters; ++it) {
      hipLaunchKernelGGL(rot_eval_kernel, dim3(nbe), dim3(kBlock), 0, s, p, 0);
      osum(E, kActCost, 1);
      nodes(kStepRhs);
      osum(3L * n, kActRz0, 1);
      for (int k = 0; k < pcg_iters; ++k) {
        nodes(kStepLp);
        osum(3L * n, kActPLp, 2);
        nodes(kStepUpdate);
        osum(3L * n, kActRz, 2);
        nodes(kStepDirection);
      }
      hipLaunchKernelGGL(rot_apply_kernel, dim3(nbn), dim3(kBlock), 0, s, p);
      nodes(kStepCommit);
      hipLaunchKernelGGL(rot_decide_kernel, dim3(1), dim3(1), 0, s, p);
      LOFTR_CHECK_LAUNCH();
    }
  if (E > 0) hipLaunchKernelGGL(rot_eval_kernel, dim3(nbe), dim3(kBlock), 0, s, p, 1);
  osum(E, kActCostFinal, 0);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  hipLaunchKernelGGL(rot_write_kernel, dim3(nbw), dim3(kBlock), 0, s, p);
  hipLaunchKernelGGL(rot_finish_kernel, dim3(1), dim3(1), 0, s, p);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  return timer.finish();
}
