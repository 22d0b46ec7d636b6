// Global positioning on the GPU (gfx950, wave64): loftr_global_positions_host (position.hip) with the same result bit for bit (DESIGN
// §27).  Every per-item step is position_core.h's, compiled from the same text; what this file adds is only how the work is spread
// over threads.  A fixed schedule on the caller's stream that depends on the sizes and the iteration limits only, nothing read back:
//   memsets of the outputs, pos_init_kernel (one thread);
//   pos_check_kernel            (thread per track / image / tree edge)  the error bits of rule 1, obs_track, the edges' directions;
//   pos_start_kernel            ONE workgroup of 1024 loops over the levels of the tree with a block barrier, then the two passes that
//                               decide whether the tree is one (the deeper end of an edge by a 32-bit atomicMax);
//   pos_bearing_kernel (thread per observation), pos_track_setup_kernel (thread per point), pos_cam_setup_kernel (thread per image),
//   pos_point_start_kernel (thread per point), pos_eval_kernel + osum for the cost of the start values;
//   per trial: pos_linearise_kernel (thread per observation), pos_point_factor_kernel (thread per point, CSR order),
//     pos_cam_sums_kernel<set-up> (a WAVE per image: the lanes stride the image's list in osum64 order and are folded by shuffles; lane
//     0 finishes the camera), osum -> r.z; per conjugate-gradient iteration pos_point_u_kernel (thread per point), pos_cam_sums_kernel
//     <S p>, osum -> p.Sp, pos_cam_kernel (thread per image) for the update, osum -> r.z, pos_cam_kernel for the direction; then
//     pos_cam_kernel for the trial centres (the largest step by a 64-bit atomicMax of its bits), pos_point_u_kernel of x,
//     pos_point_apply_kernel, pos_obs_apply_kernel (the trial scale and the trial's cost term), osum -> the trial's cost,
//     pos_accept_kernel (one thread), pos_commit_kernel;
//   pos_write_kernel (thread per observation / point / image), pos_finish_kernel (one thread).
// A launch reads only what an earlier launch wrote.  Every launch after the checks returns at once when counts[1] is set, so nothing is
// read through a bad value and no output but the counts is written; a trial's launches return at once when the refinement has ended,
// the conjugate gradients' when they have.  No persistent or waiting kernel, no graph, no grid-wide barrier.  Integer atomics only
// (flags, counters, two maxima).  Plain C++, ordinary vector stores.
#include <algorithm>
#include "position_core.h"
#include "stage_timer.h"

#pragma clang fp contract(off)

namespace {

using namespace pos;
typedef unsigned long long u64;

constexpr int kBlock = 256;
constexpr int kStartBlock = 1024;
inline unsigned blocks_of(long n, int per = kBlock) { return (unsigned)std::max((n + per - 1) / per, 1L); }

__device__ __forceinline__ bool bad_input(const P& p) { return p.counts[kErrors] != 0; }
__device__ __forceinline__ void add_votes(u64* counts, int slot, bool v) {
  const unsigned n = (unsigned)__popcll(__ballot(v));
  if (threadIdx.x % 64 == 0 && n) atomicAdd(counts + slot, (u64)n);
}
__device__ __forceinline__ void raise_bad(const P& p) { atomicOr(&p.ctrl->bad, 1); }

__global__ void pos_init_kernel(P p) { ctrl_init(p); }

// grid ceil(max(T, n, Et) / 256) x 256
__global__ void __launch_bounds__(kBlock) pos_check_kernel(P p) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  int err = 0;
  if (i < p.T) err |= track_check(p, i);
  if (i < p.n) err |= cam_check(p, (int)i);
  if (i < p.Et) err |= tree_check(p, i);
  if (err) atomicOr(p.counts + kErrors, (u64)err);
}

// ONE workgroup of 1024.  A level reads the depths and centres the level before wrote: the block-scope fence orders a thread's global
// writes before the barrier, after which the other threads of the workgroup read them.
// In a tree every image is set by exactly one edge, so no two threads write the same centre.  An input that is NOT a tree (a cycle) can
// have two edges of one level write different centres to one image at once: a plain write-write race on doubles, inside the workspace.
// It is harmless by construction, not by luck: both edges write the same depth, so the levels stay defined; the two passes below then
// raise kBadTree on every path (one of the two edges does not hold its claim), and every later launch returns before it reads a
// centre, so no output but the counts is written.
__global__ void __launch_bounds__(kStartBlock) pos_start_kernel(P p) {
  if (bad_input(p)) return;
  if (threadIdx.x == 0) root_setup(p);
  __threadfence_block();
  __syncthreads();
  int depth = 0;
  for (int L = 1; L <= p.n; ++L) {
    int set = 0;
    for (long e = threadIdx.x; e < p.Et; e += kStartBlock) set |= start_tree_edge(p, e, L);
    __threadfence_block();
    if (!__syncthreads_or(set)) break;
    depth = L;
  }
  int err = 0;
  for (long e = threadIdx.x; e < p.Et; e += kStartBlock) err |= tree_claim(p, e);
  __threadfence_block();
  __syncthreads();
  for (long e = threadIdx.x; e < p.Et; e += kStartBlock) err |= tree_verify(p, e);
  if (err) atomicOr(p.counts + kErrors, (u64)err);
  if (threadIdx.x == 0) p.ctrl->depth = depth;
}

// grid ceil(N / 256) x 256
__global__ void __launch_bounds__(kBlock) pos_bearing_kernel(P p) {
  if (bad_input(p)) return;
  const long o = (long)blockIdx.x * kBlock + threadIdx.x;
  if (o < p.N) obs_bearing(p, o);
}
// grid ceil(T / 256) x 256
__global__ void __launch_bounds__(kBlock) pos_track_setup_kernel(P p) {
  if (bad_input(p)) return;
  const long t = (long)blockIdx.x * kBlock + threadIdx.x;
  const long cnt = t < p.T ? track_setup(p, t) : 0;
  add_votes(p.counts, kActivePoints, cnt > 0);
  long s = cnt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x % 64 == 0 && s) atomicAdd(p.counts + kActiveObs, (u64)s);
}
// grid ceil(max(n, Et) / 256) x 256
__global__ void __launch_bounds__(kBlock) pos_cam_setup_kernel(P p) {
  if (bad_input(p)) return;
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  const int s = i < p.n ? cam_setup(p, (int)i) : -1;
  add_votes(p.counts, kInGraph, s > kOutside);
  add_votes(p.counts, kFree, s == kSolved);
  add_votes(p.counts, kChained, s == kChainedOnly);
  add_votes(p.counts, kNoDirection, i < p.Et && p.nodir[i]);
}
// grid ceil(T / 256) x 256
__global__ void __launch_bounds__(kBlock) pos_point_start_kernel(P p) {
  if (bad_input(p)) return;
  const long t = (long)blockIdx.x * kBlock + threadIdx.x;
  if (t < p.T) point_start(p, t);
}

// grid ceil(N / 256) x 256: the cost terms at the start values
__global__ void __launch_bounds__(kBlock) pos_eval_kernel(P p) {
  if (bad_input(p)) return;
  const long o = (long)blockIdx.x * kBlock + threadIdx.x;
  if (o < p.N) obs_eval(p, o, 0);
}

// one level of an osum: a wave per chunk of 4096, grid chunks x 64; on the last level lane 0 feeds the sum
__global__ void __launch_bounds__(64) pos_osum_kernel(P p, const double* in, long count, double* out, int action, int gate) {
  if (bad_input(p) || (gate == 1 && refine_idle(p)) || (gate == 2 && pcg_idle(p))) return;
  const int lane = threadIdx.x;
  const long lo = (long)blockIdx.x * kChunk, left = count - lo, len = left < kChunk ? (left > 0 ? left : 0) : kChunk;
  double a = 0.0;
  for (long k = lane; k < len; k += 64) a = a + in[lo + k];
  for (int s = 32; s >= 1; s >>= 1) {
    const double o = __shfl_down(a, s, 64);
    if (lane < s) a = a + o;
  }
  if (lane == 0) {
    if (action >= 0) feed(p, action, a);
    else out[blockIdx.x] = a;
  }
}

// grid ceil(N / 256) x 256
__global__ void __launch_bounds__(kBlock) pos_linearise_kernel(P p) {
  if (bad_input(p) || refine_idle(p)) return;
  const long o = (long)blockIdx.x * kBlock + threadIdx.x;
  if (o < p.N) obs_linearise(p, o);
}
// grid ceil(T / 256) x 256
__global__ void __launch_bounds__(kBlock) pos_point_factor_kernel(P p) {
  if (bad_input(p) || refine_idle(p)) return;
  const long t = (long)blockIdx.x * kBlock + threadIdx.x;
  if (t < p.T && !point_factor(p, t)) raise_bad(p);
}
// grid ceil(T / 256) x 256: u of the direction p (which == 0, inside the conjugate gradients) or of the step x
__global__ void __launch_bounds__(kBlock) pos_point_u_kernel(P p, int which) {
  if (bad_input(p) || (which == 0 ? pcg_idle(p) : refine_idle(p))) return;
  const long t = (long)blockIdx.x * kBlock + threadIdx.x;
  if (t < p.T) point_u(p, t, which == 0 ? p.pp : p.x);
}

// a WAVE per image, grid ceil(n / 4) x 256: §18's osum64 of the K sums over the image's list (lane l takes the slots l, l + 64, ...
// in order, then the lanes are folded); lane 0 finishes the camera
template <int K, bool kSetup> __global__ void __launch_bounds__(kBlock) pos_cam_sums_kernel(P p) {
  if (bad_input(p) || (kSetup ? refine_idle(p) : pcg_idle(p))) return;
  const long i = (long)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (i >= p.n) return;                                                           // (uniform in the wave)
  double a[K];
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = 0.0;
  if (cam_free(p, (int)i)) {                                                      // (uniform in the wave)
    const long b = p.cam_offsets[i], e = p.cam_offsets[i + 1];
    for (long s = b + lane; s < e; s += 64) {
      double t[K];
      if constexpr (kSetup) cam_term_setup(p, p.cam_obs[s], t);
      else cam_term_Sp(p, p.cam_obs[s], t);
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
  if constexpr (kSetup) { if (!cam_finish_setup(p, (int)i, a)) raise_bad(p); }
  else cam_finish_Sp(p, (int)i, a);
}

enum : int { kStepUpdate = 0, kStepDirection, kStepApply };
// grid ceil(n / 256) x 256: one per-camera step
__global__ void __launch_bounds__(kBlock) pos_cam_kernel(P p, int step) {
  if (bad_input(p) || (step == kStepApply ? refine_idle(p) : pcg_idle(p))) return;
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  if (step == kStepUpdate) cam_update(p, (int)i);
  else if (step == kStepDirection) cam_direction(p, (int)i);
  else {
    const double v = cam_apply(p, (int)i);
    if (v < 0.0) raise_bad(p);
    else if (v > 0.0) atomicMax(&p.ctrl->step_bits, (u64)bits_of(v));             // (the bits of doubles >= 0 order as the doubles do)
  }
}
// grid ceil(T / 256) x 256
__global__ void __launch_bounds__(kBlock) pos_point_apply_kernel(P p) {
  if (bad_input(p) || refine_idle(p)) return;
  const long t = (long)blockIdx.x * kBlock + threadIdx.x;
  if (t < p.T && !point_apply(p, t)) raise_bad(p);
}
// grid ceil(N / 256) x 256: the trial scale, then the trial's cost term
__global__ void __launch_bounds__(kBlock) pos_obs_apply_kernel(P p) {
  if (bad_input(p) || refine_idle(p)) return;
  const long o = (long)blockIdx.x * kBlock + threadIdx.x;
  if (o >= p.N) return;
  if (!obs_apply(p, o)) raise_bad(p);
  obs_eval(p, o, 1);
}
__global__ void pos_accept_kernel(P p) {
  if (!bad_input(p)) accept(p);
}
// grid ceil(max(N, T, n) / 256) x 256
__global__ void __launch_bounds__(kBlock) pos_commit_kernel(P p) {
  if (bad_input(p) || !commit_now(p)) return;
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i < p.n) cam_commit(p, (int)i);
  if (i < p.T) point_commit(p, i);
  if (i < p.N) obs_commit(p, i);
}

// grid ceil(max(N, T, n) / 256) x 256
__global__ void __launch_bounds__(kBlock) pos_write_kernel(P p) {
  if (bad_input(p)) return;                                                      // uniform: no output but the counts
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  const int neg = i < p.N ? obs_write(p, i) : 0;
  if (i < p.T) track_write(p, i);
  if (i < p.n) cam_write(p, (int)i);
  add_votes(p.counts, kNegative, neg != 0);
}
__global__ void pos_finish_kernel(P p) {
  if (!bad_input(p)) finish(p);
}

}  // namespace

extern "C" size_t loftr_global_positions_workspace_bytes(long T, long N, int n_images, long Et) {
  if (!sizes_ok(T, N, n_images, Et) || n_images < 1) return 0;
  P p{};
  p.T = T; p.N = N; p.n = n_images; p.Et = Et;
  return layout(p, nullptr);
}

extern "C" int loftr_global_positions(const long* offsets, long T, const int* obs_image, const float* obs_xy, long N, const long* cam_offsets,
                                      const int* cam_obs, const double* K, const double* R, const uint8_t* in_graph, int n_images, int root,
                                      const int* tree_image, const double* tree_t, long Et, double huber, int max_iters, int pcg_iters,
                                      double pcg_tol, double ftol, int min_cam_obs, double* centres, float* xyz, double* depth_scale,
                                      uint8_t* obs_state, uint8_t* cam_state, uint8_t* point_active, long* counts, double* info, void* ws,
                                      size_t ws_bytes, float* stage_ms, void* stream) {
  const Args a{offsets, T, obs_image, obs_xy, N, cam_offsets, cam_obs, K, R, in_graph, n_images, root, tree_image, tree_t, Et, huber,
               max_iters, pcg_iters, pcg_tol, ftol, min_cam_obs, centres, xyz, depth_scale, obs_state, cam_state, point_active, counts, info};
  const int st = check_args(a);
  if (st != LOFTR_OK) return st;
  P p = problem(a);
  hipStream_t s = (hipStream_t)stream;
  const int n = n_images;
  LOFTR_CHECK_ARG(ws != nullptr);
  if (ws_bytes < layout(p, nullptr)) return LOFTR_ERR_WORKSPACE;
  layout(p, (char*)ws);
  const unsigned nbo = blocks_of(N), nbt = blocks_of(T), nbn = blocks_of(n), nbw = blocks_of(n, kBlock / 64),
                 nba = blocks_of(std::max(std::max(N, T), (long)n));
  StageTimer timer(stage_ms, LOFTR_POSITION_STAGES, s);
  auto fill = [s](void* ptr, size_t bytes) { return bytes == 0 || hipMemsetAsync(ptr, 0, bytes, s) == hipSuccess; };
  // the levels of an osum of part[0 .. count) into `action`
  auto osum = [&](long count, int action, int gate) {
    const double* in = p.part;
    double* out = p.red;
    const long half = chunks_of(part_items(N, n));
    for (int level = 0;; ++level) {
      const long chunks = chunks_of(count);
      const bool last = chunks <= 1;
      hipLaunchKernelGGL(pos_osum_kernel, dim3((unsigned)chunks), dim3(64), 0, s, p, in, count, out, last ? action : -1, gate);
      if (last) break;
      in = out;
      out = p.red + (level % 2 == 0 ? half : 0);
      count = chunks;
    }
  };
  auto cams = [&](int step) { hipLaunchKernelGGL(pos_cam_kernel, dim3(nbn), dim3(kBlock), 0, s, p, step); };
  auto points_u = [&](int which) { hipLaunchKernelGGL(pos_point_u_kernel, dim3(nbt), dim3(kBlock), 0, s, p, which); };

  timer.mark();
  if (!fill(counts, sizeof(long) * kCounts) || !fill(info, sizeof(double) * kInfo) || !fill(centres, sizeof(double) * 3 * (size_t)n) ||
      !fill(cam_state, (size_t)n) || !fill(depth_scale, sizeof(double) * (size_t)N) || !fill(obs_state, (size_t)N) ||
      !fill(xyz, sizeof(float) * 3 * (size_t)T) || !fill(point_active, (size_t)T))
    return LOFTR_ERR_LAUNCH;
  hipLaunchKernelGGL(pos_init_kernel, dim3(1), dim3(1), 0, s, p);
  hipLaunchKernelGGL(pos_check_kernel, dim3(blocks_of(std::max(std::max(T, Et), (long)n))), dim3(kBlock), 0, s, p);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  hipLaunchKernelGGL(pos_start_kernel, dim3(1), dim3(kStartBlock), 0, s, p);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  if (N > 0) hipLaunchKernelGGL(pos_bearing_kernel, dim3(nbo), dim3(kBlock), 0, s, p);
  if (T > 0) hipLaunchKernelGGL(pos_track_setup_kernel, dim3(nbt), dim3(kBlock), 0, s, p);
  hipLaunchKernelGGL(pos_cam_setup_kernel, dim3(blocks_of(std::max((long)n, Et))), dim3(kBlock), 0, s, p);
  if (T > 0) hipLaunchKernelGGL(pos_point_start_kernel, dim3(nbt), dim3(kBlock), 0, s, p);
  if (N > 0) hipLaunchKernelGGL(pos_eval_kernel, dim3(nbo), dim3(kBlock), 0, s, p);
  osum(N, kActCost0, 0);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  if (N > 0)
    for (int it = 0; it < max_iters; ++it) {
      hipLaunchKernelGGL(pos_linearise_kernel, dim3(nbo), dim3(kBlock), 0, s, p);
      hipLaunchKernelGGL(pos_point_factor_kernel, dim3(nbt), dim3(kBlock), 0, s, p);
      hipLaunchKernelGGL((pos_cam_sums_kernel<kSetupSums, true>), dim3(nbw), dim3(kBlock), 0, s, p);
      osum(3L * n, kActRz0, 1);
      for (int k = 0; k < pcg_iters; ++k) {
        points_u(0);
        hipLaunchKernelGGL((pos_cam_sums_kernel<kSpSums, false>), dim3(nbw), dim3(kBlock), 0, s, p);
        osum(3L * n, kActPsp, 2);
        cams(kStepUpdate);
        osum(3L * n, kActRz, 2);
        cams(kStepDirection);
      }
      cams(kStepApply);
      points_u(1);
      hipLaunchKernelGGL(pos_point_apply_kernel, dim3(nbt), dim3(kBlock), 0, s, p);
      hipLaunchKernelGGL(pos_obs_apply_kernel, dim3(nbo), dim3(kBlock), 0, s, p);
      osum(N, kActCostT, 1);
      hipLaunchKernelGGL(pos_accept_kernel, dim3(1), dim3(1), 0, s, p);
      hipLaunchKernelGGL(pos_commit_kernel, dim3(nba), dim3(kBlock), 0, s, p);
      LOFTR_CHECK_LAUNCH();
    }
  timer.mark();
  hipLaunchKernelGGL(pos_write_kernel, dim3(nba), dim3(kBlock), 0, s, p);
  hipLaunchKernelGGL(pos_finish_kernel, dim3(1), dim3(1), 0, s, p);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  return timer.finish();
}
