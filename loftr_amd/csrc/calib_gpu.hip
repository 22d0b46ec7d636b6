// View-graph calibration on the GPU (gfx950, wave64): loftr_calibrate_view_graph_host (calib.hip) with the same result bit for bit
// (DESIGN §28).  Every per-item step is calib_core.h's, compiled from the same text; what this file adds is only how the work is
// spread over threads.  A fixed schedule on the caller's stream that depends on E, n, G and the iteration limits only, nothing read
// back:
//   memsets of the outputs, vg_init_kernel (one thread);
//   vg_check_kernel         (thread per edge / image / group / incidence slot)  the error bits of step 1;
//   vg_edge_setup_kernel    (thread per edge)  F', the data weight, the groups' valid incidences (integer atomic adds);
//   vg_group_setup_kernel   (thread per group) free or held;
//   vg_cost_kernel + osum   the cost of the start values;
//   per trial: vg_linearise_kernel (thread per edge: the residual, its two derivatives, the five scalars),
//     vg_group_sums_kernel<set-up> (a WAVE per group: the lanes stride the group's incidence list in osum64 order and are folded by
//     shuffles; lane 0 finishes the group), osum -> r.z; per conjugate-gradient iteration vg_group_sums_kernel<A p>, osum -> p.Ap,
//     vg_group_kernel (thread per group) for the update, osum -> r.z, vg_group_kernel for the direction; then vg_group_kernel for the
//     trial scales (the largest step by a 64-bit atomicMax of its bits), vg_cost_kernel at the trial, osum -> the trial's cost,
//     vg_accept_kernel (one thread), vg_commit_kernel;
//   vg_write_kernel (thread per edge / image / group), vg_finish_kernel (one thread).
// A launch reads only what an earlier launch wrote.  Every launch after the checks returns at once when counts[1] is set, so nothing
// is read through a bad value and no output but the counts is written; a trial's launches return at once when the refinement has
// ended, the conjugate gradients' when they have.  No persistent or waiting kernel, no graph, no grid-wide barrier.  Integer atomics
// only (flags, counters, one maximum).  Plain C++, ordinary vector stores.
#include <algorithm>
#include "calib_core.h"
#include "stage_timer.h"

#pragma clang fp contract(off)

namespace {

using namespace vg;
typedef unsigned long long u64;

constexpr int kBlock = 256;
inline unsigned blocks_of(long n, int per = kBlock) { return (unsigned)std::max((n + per - 1) / per, 1L); }

__device__ __forceinline__ bool bad_input(const P& p) { return p.counts[kErrors] != 0; }
__device__ __forceinline__ void add_votes(u64* counts, int slot, bool v) {
  const unsigned n = (unsigned)__popcll(__ballot(v));
  if (threadIdx.x % 64 == 0 && n) atomicAdd(counts + slot, (u64)n);
}

__global__ void vg_init_kernel(P p) { vg_ctrl_init(p); }

// grid ceil(max(2E, n, G) / 256) x 256
__global__ void __launch_bounds__(kBlock) vg_check_kernel(P p) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  int err = 0;
  if (i < p.E) err |= vg_edge_check(p, i);
  if (i < p.n) err |= vg_image_check(p, (int)i);
  if (i < p.G) err |= vg_group_check(p, (int)i);
  if (i < 2 * p.E) err |= vg_slot_check(p, i);
  if (err) atomicOr(p.counts + kErrors, (u64)err);
}

// grid ceil(E / 256) x 256
__global__ void __launch_bounds__(kBlock) vg_edge_setup_kernel(P p) {
  if (bad_input(p)) return;
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  const int v = e < p.E ? vg_edge_setup(p, e) : 0;
  add_votes(p.counts, kValidEdges, v != 0);
}
// grid ceil(G / 256) x 256
__global__ void __launch_bounds__(kBlock) vg_group_setup_kernel(P p) {
  if (bad_input(p)) return;
  const long g = (long)blockIdx.x * kBlock + threadIdx.x;
  const int s = g < p.G ? vg_group_setup(p, (int)g) : -1;
  add_votes(p.counts, kFreeGroups, s == kRefined);
}

// grid ceil(max(E, G) / 256) x 256: the cost terms at the state (gate 0) or at the trial (gate 1)
__global__ void __launch_bounds__(kBlock) vg_cost_kernel(P p, int trial) {
  if (bad_input(p) || (trial && vg_refine_idle(p))) return;
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i < p.E) vg_edge_eval(p, i, trial);
  if (i < p.G) vg_group_eval(p, (int)i, trial);
}

// one level of an osum: a wave per chunk of 4096, grid chunks x 64; on the last level lane 0 feeds the sum
__global__ void __launch_bounds__(64) vg_osum_kernel(P p, const double* in, long count, double* out, int action, int gate) {
  if (bad_input(p) || (gate == 1 && vg_refine_idle(p)) || (gate == 2 && vg_pcg_idle(p))) return;
  const int lane = threadIdx.x;
  const long lo = (long)blockIdx.x * kChunk, left = count - lo, len = left < kChunk ? (left > 0 ? left : 0) : kChunk;
  double a = 0.0;
  for (long k = lane; k < len; k += 64) a = a + in[lo + k];
  for (int s = 32; s >= 1; s >>= 1) {
    const double o = __shfl_down(a, s, 64);
    if (lane < s) a = a + o;
  }
  if (lane == 0) {
    if (action >= 0) vg_feed(p, action, a);
    else out[blockIdx.x] = a;
  }
}

// grid ceil(E / 256) x 256
__global__ void __launch_bounds__(kBlock) vg_linearise_kernel(P p) {
  if (bad_input(p) || vg_refine_idle(p)) return;
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e < p.E) vg_edge_linearise(p, e);
}

// a WAVE per group, grid ceil(G / 4) x 256: §18's osum64 of the K sums over the group's incidence list (lane l takes the slots l,
// l + 64, ... in order, then the lanes are folded with the host's pairs); lane 0 finishes the group
template <int K, bool kSetup> __global__ void __launch_bounds__(kBlock) vg_group_sums_kernel(P p) {
  if (bad_input(p) || (kSetup ? vg_refine_idle(p) : vg_pcg_idle(p))) return;
  const long g = (long)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (g >= p.G) return;                                                           // (uniform in the wave)
  double a[K];
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = 0.0;
  if (vg_group_free(p, (int)g)) {                                                 // (uniform in the wave)
    const long b = p.grp_offsets[g], e = p.grp_offsets[g + 1];
    for (long s = b + lane; s < e; s += 64) {
      double t[K];
      if constexpr (kSetup) vg_term_setup(p, (int)g, p.grp_inc[s], t);
      else vg_term_Ap(p, (int)g, p.grp_inc[s], t);
#pragma unroll
      for (int k = 0; k < K; ++k) a[k] = a[k] + t[k];
    }
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double o = __shfl_down(a[k], s, 64);
        if (lane < s) a[k] = a[k] + o;
      }
    }
  }
  if (lane != 0) return;
  if constexpr (kSetup) { if (!vg_group_finish_setup(p, (int)g, a)) atomicOr(&p.ctrl->bad, 1); }
  else vg_group_finish_Ap(p, (int)g, a);
}

enum : int { kStepUpdate = 0, kStepDirection, kStepApply };
// grid ceil(G / 256) x 256: one per-group step
__global__ void __launch_bounds__(kBlock) vg_group_kernel(P p, int step) {
  if (bad_input(p) || (step == kStepApply ? vg_refine_idle(p) : vg_pcg_idle(p))) return;
  const long g = (long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= p.G) return;
  if (step == kStepUpdate) vg_group_update(p, (int)g);
  else if (step == kStepDirection) vg_group_direction(p, (int)g);
  else {
    const double v = vg_group_apply(p, (int)g);
    if (v == -1.0) atomicOr(&p.ctrl->bad, 1);
    else if (v == -2.0) atomicOr(&p.ctrl->oob, 1);
    else if (v > 0.0) atomicMax(&p.ctrl->step_bits, (u64)bits_of(v));               // (the bits of doubles >= 0 order as the doubles do)
  }
}
__global__ void vg_accept_kernel(P p) {
  if (!bad_input(p)) vg_accept(p);
}
// grid ceil(G / 256) x 256
__global__ void __launch_bounds__(kBlock) vg_commit_kernel(P p) {
  if (bad_input(p) || !vg_commit_now(p)) return;
  const long g = (long)blockIdx.x * kBlock + threadIdx.x;
  if (g < p.G) vg_group_commit(p, (int)g);
}

// grid ceil(max(E, n, G) / 256) x 256
__global__ void __launch_bounds__(kBlock) vg_write_kernel(P p) {
  if (bad_input(p)) return;                                                      // uniform: no output but the counts
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  const int out = i < p.E ? vg_edge_write(p, i) : 0;
  if (i < p.n) vg_image_write(p, (int)i);
  if (i < p.G) vg_group_write(p, (int)i);
  add_votes(p.counts, kOutliers, out != 0);
}
__global__ void vg_finish_kernel(P p) {
  if (!bad_input(p)) vg_finish(p);
}

}  // namespace

extern "C" size_t loftr_calibrate_view_graph_workspace_bytes(long E, int n_images, int n_groups) {
  if (!sizes_ok(E, n_images, n_groups)) return 0;
  P p{};
  p.E = E; p.n = n_images; p.G = n_groups;
  return layout(p, nullptr);
}

extern "C" int loftr_calibrate_view_graph(const int* edge_image, const double* edge_F, const int* edge_weight, long E, const double* pp,
                                          const double* f0, const int* group, int n_images, int n_groups, const long* grp_offsets,
                                          const int* grp_inc, double loss, double max_resid, double prior_weight, int weight_cap,
                                          double bound_lo, double bound_hi, int min_edges, int max_iters, int pcg_iters, double pcg_tol,
                                          double ftol, double* focal_scale, double* focal, double* edge_resid, uint8_t* edge_state,
                                          uint8_t* group_state, long* counts, double* info, void* ws, size_t ws_bytes, float* stage_ms,
                                          void* stream) {
  const Args a{edge_image, edge_F, edge_weight, E, pp, f0, group, n_images, n_groups, grp_offsets, grp_inc, loss, max_resid, prior_weight,
               weight_cap, bound_lo, bound_hi, min_edges, max_iters, pcg_iters, pcg_tol, ftol, focal_scale, focal, edge_resid, edge_state,
               group_state, counts, info};
  const int st = vg_check_args(a);
  if (st != LOFTR_OK) return st;
  P p = vg_problem(a);
  hipStream_t s = (hipStream_t)stream;
  const int n = n_images, G = n_groups;
  LOFTR_CHECK_ARG(ws != nullptr);
  if (ws_bytes < layout(p, nullptr)) return LOFTR_ERR_WORKSPACE;
  layout(p, (char*)ws);
  const unsigned nbe = blocks_of(E), nbg = blocks_of(G), nbw = blocks_of(G, kBlock / 64), nbc = blocks_of(std::max(E, (long)G)),
                 nba = blocks_of(std::max(std::max(E, (long)n), (long)G));
  StageTimer timer(stage_ms, LOFTR_CALIB_STAGES, s);
  auto fill = [s](void* ptr, size_t bytes) { return bytes == 0 || hipMemsetAsync(ptr, 0, bytes, s) == hipSuccess; };
  // the levels of an osum of part[0 .. count) into `action`
  auto osum = [&](long count, int action, int gate) {
    const double* in = p.part;
    double* out = p.red;
    const long half = chunks_of(E + G);
    for (int level = 0;; ++level) {
      const long chunks = chunks_of(count);
      const bool last = chunks <= 1;
      hipLaunchKernelGGL(vg_osum_kernel, dim3((unsigned)chunks), dim3(64), 0, s, p, in, count, out, last ? action : -1, gate);
      if (last) break;
      in = out;
      out = p.red + (level % 2 == 0 ? half : 0);
      count = chunks;
    }
  };
  auto groups = [&](int step) { hipLaunchKernelGGL(vg_group_kernel, dim3(nbg), dim3(kBlock), 0, s, p, step); };

  timer.mark();
  if (!fill(counts, sizeof(long) * kCounts) || !fill(info, sizeof(double) * kInfo) || !fill(focal_scale, sizeof(double) * (size_t)G) ||
      !fill(group_state, (size_t)G) || !fill(focal, sizeof(double) * (size_t)n) || !fill(edge_resid, sizeof(double) * (size_t)E) ||
      !fill(edge_state, (size_t)E))
    return LOFTR_ERR_LAUNCH;
  hipLaunchKernelGGL(vg_init_kernel, dim3(1), dim3(1), 0, s, p);
  hipLaunchKernelGGL(vg_check_kernel, dim3(blocks_of(std::max(std::max(2 * E, (long)n), (long)G))), dim3(kBlock), 0, s, p);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  if (E > 0) hipLaunchKernelGGL(vg_edge_setup_kernel, dim3(nbe), dim3(kBlock), 0, s, p);
  hipLaunchKernelGGL(vg_group_setup_kernel, dim3(nbg), dim3(kBlock), 0, s, p);
  hipLaunchKernelGGL(vg_cost_kernel, dim3(nbc), dim3(kBlock), 0, s, p, 0);
  osum(E + G, kActCost0, 0);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  if (E > 0)
    for (int it = 0; it < max_iters; ++it) {
      hipLaunchKernelGGL(vg_linearise_kernel, dim3(nbe), dim3(kBlock), 0, s, p);
      hipLaunchKernelGGL((vg_group_sums_kernel<kSetupSums, true>), dim3(nbw), dim3(kBlock), 0, s, p);
      osum(G, kActRz0, 1);
      for (int k = 0; k < pcg_iters; ++k) {
        hipLaunchKernelGGL((vg_group_sums_kernel<kApSums, false>), dim3(nbw), dim3(kBlock), 0, s, p);
        osum(G, kActPap, 2);
        groups(kStepUpdate);
        osum(G, kActRz, 2);
        groups(kStepDirection);
      }
      groups(kStepApply);
      hipLaunchKernelGGL(vg_cost_kernel, dim3(nbc), dim3(kBlock), 0, s, p, 1);
      osum(E + G, kActCostT, 1);
      hipLaunchKernelGGL(vg_accept_kernel, dim3(1), dim3(1), 0, s, p);
      hipLaunchKernelGGL(vg_commit_kernel, dim3(nbg), dim3(kBlock), 0, s, p);
      LOFTR_CHECK_LAUNCH();
    }
  timer.mark();
  hipLaunchKernelGGL(vg_write_kernel, dim3(nba), dim3(kBlock), 0, s, p);
  hipLaunchKernelGGL(vg_finish_kernel, dim3(1), dim3(1), 0, s, p);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  return timer.finish();
}
