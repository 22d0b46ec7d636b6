// Bundle adjustment on the GPU: loftr_bundle_adjust_host (bundle.hip) with the same result bit for bit.  Every phase of
// the host routine is one kernel here, every per-item step is bundle_core.h's, compiled from the same text, fp64 without FMA
// contraction; what this file adds is only how a phase is spread over threads:
//   a thread per track      setup, linearise, track half of S p, back substitution, evaluate (the sums of a track run sequentially in
//                           that one thread, as §16's refit);
//   a wave per camera       groups check, linearise, camera half of S p: lane l accumulates slots l, l + 64, ... of the camera's list
//                           and the 64 lanes are folded 32, 16, ..., 1 with shuffles -- osum64 exactly as the host's 64-entry array;
//   a wave per 4096 terms   osum over tracks or cameras, one launch per level; lane 0 of the last level hands the sum to ctrl_feed;
//   a thread per camera     factor, the two updates of the conjugate gradients, apply;
//   one thread              init, accept: the owner of lambda, the counters and the flags.
// The whole run is a FIXED launch schedule on the caller's stream: max_iters trials of pcg_iters iterations each.  A kernel whose phase
// the host routine would not run (the run has stopped, the conjugate gradients have stopped, the step is already rejected, an error bit
// is up) returns at once on a flag in device memory; a flag is only ever read by kernels launched after the one that wrote it.  No
// readback, no grid-wide barrier, no persistent kernel, no captured graph: a kernel boundary is the only device-wide ordering.
// Floating-point values cross lanes only as exact copies (shuffles); atomics are integer only.  Plain C++, ordinary vector stores.
#include <algorithm>
#include <vector>
#include "common.h"
#include "bundle_core.h"

#pragma clang fp contract(off)

namespace {

using namespace ba;

constexpr int kThreads = 256;
enum : int { kSkipBadF = 1, kSkipBadA = 2, kSkipBadE = 4, kSkipPcg = 8, kNeedFresh = 16 };
enum : int { kClsSetup = 0, kClsLinearise, kClsFactor, kClsTrackHalf, kClsCamHalf, kClsOsum, kClsUpdate, kClsApply, kClsEvaluate, kClsAccept,
             kClsWrite, kClsCount };
static_assert(kClsCount == LOFTR_BUNDLE_CLASSES, "kernel classes out of step with include/loftr_hip.h");

__device__ __forceinline__ bool skipped(const Ctx& c, int flags) {
  const Ctrl& s = *c.ctrl;
  return s.done || s.err || ((flags & kSkipBadF) && s.bad_f) || ((flags & kSkipBadA) && s.bad_a) || ((flags & kSkipBadE) && s.bad_e) ||
         ((flags & kSkipPcg) && s.pcg_done) || ((flags & kNeedFresh) && !s.fresh);
}

// osum64 of camera i's list over the 64 lanes of a wave: a [M] of lane 0 is the sum
template <int M, class F> __device__ __forceinline__ void wave_osum64(const Ctx& c, long i, int lane, F term, double* a) {
#pragma unroll
  for (int m = 0; m < M; ++m) a[m] = 0.0;
  const long b = c.cam_offsets[i], e = c.cam_offsets[i + 1];
  for (long k = b + lane; k < e; k += 64) {
    const long o = c.cam_obs[k];
    if (c.obs_active[o]) term(o, a);
  }
  for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const double v = __shfl_down(a[m], s, 64);
      if (lane < s) a[m] = a[m] + v;
    }
}

__global__ void ba_init_kernel(Ctx c) { ctrl_init(c); }

// grid ceil(n / 256) x 256
template <int M> __global__ void __launch_bounds__(kThreads) ba_cam_setup_kernel(CtxT<M> c) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i < c.n) {
    cam_setup(c, i);
    if constexpr (M == 7) cam_setup_focal(c, i);
  }
}

// grid ceil(T / 256) x 256
__global__ void __launch_bounds__(kThreads) ba_track_setup_kernel(Ctx c) {
  __shared__ unsigned s_cnt[3];                                          // active observations, active points, error bits
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t < c.T) {
    long cnt;
    const int err = track_setup(c, t, &cnt);
    if (cnt) { atomicAdd(&s_cnt[0], (unsigned)cnt); atomicAdd(&s_cnt[1], 1u); }
    if (err) atomicOr(&s_cnt[2], (unsigned)err);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_cnt[0]) atomicAdd(&c.ctrl->n_active_obs, (unsigned long long)s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&c.ctrl->n_active_pts, (unsigned long long)s_cnt[1]);
    if (s_cnt[2]) atomicOr(&c.ctrl->err, (int)s_cnt[2]);
  }
}

// a wave per camera, grid ceil(n / 4) x 256.  Reads the observation arrays only through checked indices, so it needs no flag.
template <int M> __global__ void __launch_bounds__(kThreads) ba_groups_kernel(CtxT<M> c) {
  const long i = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (i >= c.n) return;
  long b, e;
  int err = 0, cnt = 0;
  if (!group_range(c, i, &b, &e)) { err = kBadGroups; b = e = 0; }
  for (long k = b + lane; k < e; k += 64) {
    bool active;
    err |= group_check(c, i, b, k, &active);
    cnt += active;
  }
  for (int m = 32; m >= 1; m >>= 1) { err |= __shfl_xor(err, m, 64); cnt += __shfl_xor(cnt, m, 64); }
  if (lane == 0) {
    const bool fr = !c.fixed[i] && c.cam_valid[i] && cnt >= 1;
    c.cam_free[i] = (uint8_t)fr;
    if (fr) atomicAdd(&c.ctrl->n_free, 1ull);
    if (err) atomicOr(&c.ctrl->err, err);
    if constexpr (M == 7) {
      const bool fo = cam_focal_rule(c, i, fr, cnt);
      c.cam_focal[i] = (uint8_t)fo;
      if (fo) atomicAdd(&c.ctrl->n_focal, 1);
    }
  }
}

// grid ceil(T / 256) x 256; other = 0 evaluates the state, 1 the trial
__global__ void __launch_bounds__(kThreads) ba_evaluate_kernel(Ctx c, int other, int flags) {
  if (skipped(c, flags)) return;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t < c.T && !track_eval(c, c.ctrl->cur ^ other, t)) atomicOr(&c.ctrl->bad_e, 1);
}

// one level of an osum: a wave per chunk of 4096, grid ceil(count / 4096) (at least 1) x 64; action >= 0 on the last level
__global__ void __launch_bounds__(64) ba_osum_kernel(Ctx c, const double* in, long count, double* out, int action, int flags) {
  if (skipped(c, flags)) return;
  const int lane = threadIdx.x;
  const long lo = (long)blockIdx.x * kChunk, len = count - lo < kChunk ? count - lo : kChunk;
  double a = 0.0;
  for (long e = lane; e < len; e += 64) a = a + in[lo + e];
  for (int s = 32; s >= 1; s >>= 1) {
    const double v = __shfl_down(a, s, 64);
    if (lane < s) a = a + v;
  }
  if (lane == 0) {
    if (action >= 0) ctrl_feed(c, action, a);
    else out[blockIdx.x] = a;
  }
}

template <int M> __global__ void __launch_bounds__(kThreads) ba_track_lin_kernel(CtxT<M> c, int flags) {
  if (skipped(c, flags)) return;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t < c.T) track_lin<M>(c, c.ctrl->cur, t);
}

// a wave per camera, grid ceil(n / 4) x 256
template <int M> __global__ void __launch_bounds__(kThreads) ba_cam_lin_kernel(CtxT<M> c, int flags) {
  if (skipped(c, flags)) return;
  const long i = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64, cur = c.ctrl->cur;
  if (i >= c.n || !c.cam_free[i]) return;
  constexpr int kU = kTri<M>;
  double a[kU + M];
  wave_osum64<kU + M>(c, i, lane, [&](long o, double* acc) { cam_lin_term<M>(c, cur, o, acc); }, a);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kU; ++k) c.U[kU * i + k] = a[k];
#pragma unroll
    for (int k = 0; k < M; ++k) c.gc[M * i + k] = a[kU + k];
  }
}

// threads [0, T): tracks, [T, T + n): cameras; grid ceil((T + n) / 256) x 256
template <int M> __global__ void __launch_bounds__(kThreads) ba_factor_kernel(Ctx c, int flags) {
  if (skipped(c, flags)) return;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  const double lambda = c.ctrl->lambda;
  bool ok = true;
  if (id < c.T) ok = track_factor(c, id, lambda);
  else if (id < c.T + c.n) ok = cam_factor<M>(c, id - c.T, lambda);
  if (!ok) atomicOr(&c.ctrl->bad_f, 1);
}

// mode 0: z = Vd^-1 gp; mode 1: the track half of S p
template <int M> __global__ void __launch_bounds__(kThreads) ba_track_half_kernel(CtxT<M> c, int mode, int flags) {
  if (skipped(c, flags)) return;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t < c.T) track_half<M>(c, c.ctrl->cur, t, mode, c.p);
}

// a wave per camera, grid ceil(n / 4) x 256.  mode 0: the right-hand side and the start of the conjugate gradients; mode 1: S p
template <int M> __global__ void __launch_bounds__(kThreads) ba_cam_half_kernel(CtxT<M> c, int mode, int flags) {
  if (skipped(c, flags)) return;
  const long i = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64, cur = c.ctrl->cur;
  if (i >= c.n) return;
  double a[M];
#pragma unroll
  for (int k = 0; k < M; ++k) a[k] = 0.0;
  if (c.cam_free[i]) wave_osum64<M>(c, i, lane, [&](long o, double* acc) { cam_half_term<M>(c, cur, o, acc); }, a);
  if (lane == 0) cam_half_finish<M>(c, i, mode, c.ctrl->lambda, a);
}

template <int M> __global__ void __launch_bounds__(kThreads) ba_update_kernel(Ctx c, int which, int flags) {
  if (skipped(c, flags)) return;
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= c.n) return;
  if (which == 1) cam_update1<M>(c, i, c.ctrl->alpha);
  else cam_update2<M>(c, i, c.ctrl->beta);
}

// threads [0, T): back substitution of the tracks, [T, T + n): the cameras' trial poses
template <int M> __global__ void __launch_bounds__(kThreads) ba_apply_kernel(CtxT<M> c, int flags) {
  if (skipped(c, flags)) return;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  const int cur = c.ctrl->cur;
  bool ok = true;
  if (id < c.T) ok = track_half<M>(c, cur, id, 2, c.x);
  else if (id < c.T + c.n) ok = cam_apply<M>(c, cur, id - c.T);
  if (!ok) atomicOr(&c.ctrl->bad_a, 1);
}

__global__ void ba_accept_kernel(Ctx c) { ctrl_accept(c); }

// threads [0, T): points, [T, T + n): cameras; thread 0 also writes the counts.  Runs whatever the flags say.
template <int M> __global__ void __launch_bounds__(kThreads) ba_write_kernel(CtxT<M> c) {
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  const int cur = c.ctrl->cur;
  if (!c.ctrl->err) {
    if (id < c.T) track_write(c, cur, id);
    else if (id < c.T + c.n) cam_write<M>(c, cur, id - c.T);
  }
  if (id == 0) ctrl_write<M>(c);
}

// the argument checks of both entry points
int check_args(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N, const float* xyz,
               const double* K, const double* T_cam_from_world, const uint8_t* fixed, int n_images, const long* cam_offsets,
               const int* cam_obs, double huber_px, int max_iters, int pcg_iters, double pcg_tol, double ftol, double* T_out, float* xyz_out,
               uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active, long* counts, void* ws) {
  LOFTR_CHECK_ARG(offsets && cam_offsets && counts && ws && T >= 0 && N >= 0 && n_images >= 0);
  LOFTR_CHECK_ARG(T == 0 || (xyz && xyz_out && point_active));
  LOFTR_CHECK_ARG(N == 0 || (obs_image && obs_xy && obs_mask && obs_active && cam_obs));
  LOFTR_CHECK_ARG(n_images == 0 || (K && T_cam_from_world && fixed && T_out && cam_free));
  LOFTR_CHECK_ARG(huber_px >= 0.0 && fin(huber_px) && ftol >= 0.0 && fin(ftol) && pcg_tol >= 0.0 && pcg_tol < 1.0);
  LOFTR_CHECK_ARG(max_iters >= 0 && max_iters <= LOFTR_BUNDLE_MAX_ITERS && pcg_iters >= 1 && pcg_iters <= LOFTR_BUNDLE_MAX_PCG);
  LOFTR_CHECK_ARG((T > 0 && n_images > 0) || N == 0);                  // observations outside every track or camera
  if (!sizes_ok(T, N, n_images)) return LOFTR_ERR_UNSUPPORTED;
  return LOFTR_OK;
}

// the fixed launch schedule; c holds the problem and the result
template <int M> int run(CtxT<M>& c, int max_iters, int pcg_iters, void* ws, size_t ws_bytes, float* class_ms, long* class_launches,
                         void* stream) {
  if (ws_bytes < layout<M>(c, nullptr)) return LOFTR_ERR_WORKSPACE;
  layout<M>(c, (char*)ws);
  hipStream_t s = (hipStream_t)stream;
  const long n = c.n, T = c.T;
  const bool timed = class_ms != nullptr;
  std::vector<hipEvent_t> ev;
  std::vector<int> ev_cls;
  long launches[kClsCount] = {0};
  bool failed = false;
  auto mark = [&]() {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess || hipEventRecord(e, s) != hipSuccess) failed = true;
    else ev.push_back(e);
  };
  auto after = [&](int cls) {
    if (hipGetLastError() != hipSuccess) failed = true;
    launches[cls] += 1;
    if (timed && !failed) { mark(); ev_cls.push_back(cls); }
  };
  auto blocks = [](long items, long per) { return dim3((unsigned)(items > 0 ? (items + per - 1) / per : 1)); };
  const Ctx& b = c;                                                     // what the kernels without a camera block take
  // osum of v[0 .. count) into ctrl_feed(action): one launch per level
  auto osum = [&](const double* v, long count, int action, int flags) {
    const double* in = v;
    double* out = c.red;
    for (;;) {
      const long chunks = count > 0 ? (count + kChunk - 1) / kChunk : 1;
      hipLaunchKernelGGL(ba_osum_kernel, dim3((unsigned)chunks), dim3(64), 0, s, b, in, count, out, chunks == 1 ? action : -1, flags);
      after(kClsOsum);
      if (chunks == 1) return;
      in = out;
      out = out == c.red ? c.red + ((std::max(T, n) + 1 + kChunk - 1) / kChunk) : c.red;
      count = chunks;
    }
  };
  if (timed) mark();
  hipLaunchKernelGGL(ba_init_kernel, dim3(1), dim3(1), 0, s, b); after(kClsSetup);
  hipLaunchKernelGGL(ba_cam_setup_kernel<M>, blocks(n, kThreads), dim3(kThreads), 0, s, c); after(kClsSetup);
  hipLaunchKernelGGL(ba_track_setup_kernel, blocks(T, kThreads), dim3(kThreads), 0, s, b); after(kClsSetup);
  hipLaunchKernelGGL(ba_groups_kernel<M>, blocks(n, 4), dim3(kThreads), 0, s, c); after(kClsSetup);
  hipLaunchKernelGGL(ba_evaluate_kernel, blocks(T, kThreads), dim3(kThreads), 0, s, b, 0, 0); after(kClsEvaluate);
  osum(c.part, T, kActCost0, 0);
  osum(c.part2, T, kActSq0, 0);
  for (int it = 0; it < max_iters && !failed; ++it) {
    hipLaunchKernelGGL(ba_track_lin_kernel<M>, blocks(T, kThreads), dim3(kThreads), 0, s, c, kNeedFresh); after(kClsLinearise);
    hipLaunchKernelGGL(ba_cam_lin_kernel<M>, blocks(n, 4), dim3(kThreads), 0, s, c, kNeedFresh); after(kClsLinearise);
    hipLaunchKernelGGL(ba_factor_kernel<M>, blocks(T + n, kThreads), dim3(kThreads), 0, s, b, 0); after(kClsFactor);
    hipLaunchKernelGGL(ba_track_half_kernel<M>, blocks(T, kThreads), dim3(kThreads), 0, s, c, 0, kSkipBadF); after(kClsTrackHalf);
    hipLaunchKernelGGL(ba_cam_half_kernel<M>, blocks(n, 4), dim3(kThreads), 0, s, c, 0, kSkipBadF); after(kClsCamHalf);
    osum(c.part, n, kActRz0, kSkipBadF);
    for (int pi = 0; pi < pcg_iters && !failed; ++pi) {
      const int f = kSkipBadF | kSkipPcg;
      hipLaunchKernelGGL(ba_track_half_kernel<M>, blocks(T, kThreads), dim3(kThreads), 0, s, c, 1, f); after(kClsTrackHalf);
      hipLaunchKernelGGL(ba_cam_half_kernel<M>, blocks(n, 4), dim3(kThreads), 0, s, c, 1, f); after(kClsCamHalf);
      osum(c.part, n, kActPsp, f);
      hipLaunchKernelGGL(ba_update_kernel<M>, blocks(n, kThreads), dim3(kThreads), 0, s, b, 1, f); after(kClsUpdate);
      osum(c.part, n, kActRz, f);
      hipLaunchKernelGGL(ba_update_kernel<M>, blocks(n, kThreads), dim3(kThreads), 0, s, b, 2, f); after(kClsUpdate);
    }
    hipLaunchKernelGGL(ba_apply_kernel<M>, blocks(T + n, kThreads), dim3(kThreads), 0, s, c, kSkipBadF); after(kClsApply);
    hipLaunchKernelGGL(ba_evaluate_kernel, blocks(T, kThreads), dim3(kThreads), 0, s, b, 1, kSkipBadF | kSkipBadA); after(kClsEvaluate);
    osum(c.part, T, kActCostT, kSkipBadF | kSkipBadA | kSkipBadE);
    osum(c.part2, T, kActSqT, kSkipBadF | kSkipBadA | kSkipBadE);
    hipLaunchKernelGGL(ba_accept_kernel, dim3(1), dim3(1), 0, s, b); after(kClsAccept);
  }
  hipLaunchKernelGGL(ba_write_kernel<M>, blocks(T + n, kThreads), dim3(kThreads), 0, s, c); after(kClsWrite);
  if (class_launches) for (int k = 0; k < kClsCount; ++k) class_launches[k] = launches[k];
  if (timed) {
    if (hipStreamSynchronize(s) != hipSuccess) failed = true;
    std::vector<float> ms[kClsCount];
    for (size_t k = 0; k + 1 < ev.size() && !failed; ++k) {
      float v = 0.f;
      if (hipEventElapsedTime(&v, ev[k], ev[k + 1]) == hipSuccess) ms[ev_cls[k]].push_back(v);
    }
    for (int k = 0; k < kClsCount; ++k) {                             // per class: the median launch, then the total
      std::sort(ms[k].begin(), ms[k].end());
      float total = 0.f;
      for (float v : ms[k]) total += v;
      class_ms[2 * k] = ms[k].empty() ? 0.f : ms[k][ms[k].size() / 2];
      class_ms[2 * k + 1] = total;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
  }
  return failed ? LOFTR_ERR_LAUNCH : LOFTR_OK;
}

// ---- §18.2: one focal step per group of cameras.  New kernels for every phase that touches the camera block or the groups; the phases
// that do not (init of the scalars aside: track setup, evaluate, the track linearisation, the osum of the cost, accept) are the ones above.
// A wave per group folds its members exactly as a wave per camera folds its observations.

// osum64 of group g's list over the 64 lanes of a wave: member i adds v[stride i] when it has cam_focal; the sum is lane 0's
__device__ __forceinline__ double wave_gsum64(const CtxS& c, long g, int lane, const double* v, long stride) {
  double a = 0.0;
  const long b = c.group_offsets[g], e = c.group_offsets[g + 1];
  for (long k = b + lane; k < e; k += 64) group_term(c, c.group_cams[k], v, stride, &a);
  for (int s = 32; s >= 1; s >>= 1) {
    const double w = __shfl_down(a, s, 64);
    if (lane < s) a = a + w;
  }
  return a;
}

__global__ void ba_init_shared_kernel(CtxS c) { shared_init(c); }

// a wave per camera, grid ceil(n / 4) x 256: ba_groups_kernel, and what the camera carries for its group
__global__ void __launch_bounds__(kThreads) ba_groups_shared_kernel(CtxS c) {
  const long i = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (i >= c.n) return;
  long b, e;
  int err = 0, cnt = 0;
  if (!group_range(c, i, &b, &e)) { err = kBadGroups; b = e = 0; }
  for (long k = b + lane; k < e; k += 64) {
    bool active;
    err |= group_check(c, i, b, k, &active);
    cnt += active;
  }
  for (int m = 32; m >= 1; m >>= 1) { err |= __shfl_xor(err, m, 64); cnt += __shfl_xor(cnt, m, 64); }
  if (lane == 0) {
    const bool fr = !c.fixed[i] && c.cam_valid[i] && cnt >= 1;
    c.cam_free[i] = (uint8_t)fr;
    if (fr) atomicAdd(&c.ctrl->n_free, 1ull);
    err |= cam_carry(c, i, cnt);
    if (err) atomicOr(&c.ctrl->err, err);
  }
}

// a wave per group, grid ceil(G / 4) x 256: the check of the group arrays and the count.  Reads them only through checked indices, and
// writes cam_focal only when the whole list of the group has passed, so it needs no flag.
__global__ void __launch_bounds__(kThreads) ba_cgroups_kernel(CtxS c) {
  const long g = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (g >= c.G) return;
  long b, e, total = 0;
  int err = 0;
  if (!cgroup_range(c, g, &b, &e)) { err = kBadCamGroups; b = e = 0; }
  for (long k = b + lane; k < e; k += 64) {
    long cnt;
    err |= cgroup_slot(c, g, b, k, &cnt);
    total += cnt;
  }
  for (int m = 32; m >= 1; m >>= 1) { err |= __shfl_xor(err, m, 64); total += __shfl_xor(total, m, 64); }
  if (err) {
    if (lane == 0) atomicOr(&c.ctrl->err, err);
    return;
  }
  const bool refines = lane == 0 ? cgroup_rule(c, g, total) : total >= (long)c.min_focal_obs;
  int nf = 0;
  for (long k = b + lane; k < e; k += 64) {
    const int i = c.group_cams[k];
    const bool fo = refines && c.cam_cnt[i] > 0;
    c.cam_focal[i] = (uint8_t)fo;
    nf += fo;
  }
  for (int m = 32; m >= 1; m >>= 1) nf += __shfl_xor(nf, m, 64);
  if (lane == 0) {
    c.group_focal[g] = (uint8_t)refines;
    if (refines) atomicAdd(&c.cs->n_groups, 1);
    if (nf) atomicAdd(&c.ctrl->n_focal, nf);
  }
}

// a wave per live camera, grid ceil(n / 4) x 256
__global__ void __launch_bounds__(kThreads) ba_cam_lin_shared_kernel(CtxS c, int flags) {
  if (skipped(c, flags)) return;
  const long i = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64, cur = c.ctrl->cur;
  if (i >= c.n || !live(c, i)) return;
  double a[35];
  wave_osum64<35>(c, i, lane, [&](long o, double* acc) { cam_lin_term_s(c, cur, o, acc); }, a);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 28; ++k) c.U[28 * i + k] = a[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) c.gc[7 * i + k] = a[28 + k];
  }
}

// a wave per refining group, grid ceil(G / 4) x 256: d_g = the sum of U77 over its members
__global__ void __launch_bounds__(kThreads) ba_group_lin_kernel(CtxS c, int flags) {
  if (skipped(c, flags)) return;
  const long g = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (g >= c.G || !c.group_focal[g]) return;
  const double d = wave_gsum64(c, g, lane, c.U + 27, 28);
  if (lane == 0) c.dg[g] = d;
}

// threads [0, T): tracks, [T, T + n): cameras, [T + n, T + n + G): groups
__global__ void __launch_bounds__(kThreads) ba_factor_shared_kernel(CtxS c, int flags) {
  if (skipped(c, flags)) return;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  const double lambda = c.ctrl->lambda;
  bool ok = true;
  if (id < c.T) ok = track_factor(c, id, lambda);
  else if (id < c.T + c.n) ok = cam_factor_s(c, id - c.T, lambda);
  else if (id < c.T + c.n + c.G) ok = group_factor(c, id - c.T - c.n, lambda);
  if (!ok) atomicOr(&c.ctrl->bad_f, 1);
}

__global__ void __launch_bounds__(kThreads) ba_track_half_shared_kernel(CtxS c, int mode, int flags) {
  if (skipped(c, flags)) return;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t < c.T) track_half_s(c, c.ctrl->cur, t, mode, c.p, c.pg);
}

// a wave per camera, grid ceil(n / 4) x 256
__global__ void __launch_bounds__(kThreads) ba_cam_half_shared_kernel(CtxS c, int mode, int flags) {
  if (skipped(c, flags)) return;
  const long i = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64, cur = c.ctrl->cur;
  if (i >= c.n) return;
  double a[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) a[k] = 0.0;
  if (live(c, i)) wave_osum64<7>(c, i, lane, [&](long o, double* acc) { cam_half_term_s(c, cur, o, acc); }, a);
  if (lane == 0) cam_half_finish_s(c, i, mode, c.ctrl->lambda, a);
}

// a wave per group, grid ceil(G / 4) x 256: E^T of the cameras' seventh entries, then the group's own step
__global__ void __launch_bounds__(kThreads) ba_group_half_kernel(CtxS c, int mode, int flags) {
  if (skipped(c, flags)) return;
  const long g = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (g >= c.G) return;
  double s = 0.0;
  if (c.group_focal[g]) s = wave_gsum64(c, g, lane, c.Sp + 6, 7);
  if (lane == 0) group_half_finish(c, g, mode, c.ctrl->lambda, s);
}

// ba_osum_kernel for a dot product of two halves: the cameras' sum waits (action kActStore), the groups' is added to it and fed
__global__ void __launch_bounds__(64) ba_osum_shared_kernel(CtxS c, const double* in, long count, double* out, int action, int flags) {
  if (skipped(c, flags)) return;
  const int lane = threadIdx.x;
  const long lo = (long)blockIdx.x * kChunk, len = count - lo < kChunk ? count - lo : kChunk;
  double a = 0.0;
  for (long e = lane; e < len; e += 64) a = a + in[lo + e];
  for (int s = 32; s >= 1; s >>= 1) {
    const double v = __shfl_down(a, s, 64);
    if (lane < s) a = a + v;
  }
  if (lane == 0) {
    if (action == kActStore) c.cs->acc = a;
    else if (action >= 0) ctrl_feed(c, action, c.cs->acc + a);
    else out[blockIdx.x] = a;
  }
}

// threads [0, n): cameras, [n, n + G): groups (the scalar update of a group)
__global__ void __launch_bounds__(kThreads) ba_update_shared_kernel(CtxS c, int which, int flags) {
  if (skipped(c, flags)) return;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  if (id < c.n) {
    if (which == 1) cam_update1_s(c, id, c.ctrl->alpha);
    else cam_update2_s(c, id, c.ctrl->beta);
  } else if (id < c.n + c.G) {
    if (which == 1) group_update1(c, id - c.n, c.ctrl->alpha, c.ctrl->lambda);
    else group_update2(c, id - c.n, c.ctrl->beta);
  }
}

__global__ void __launch_bounds__(kThreads) ba_apply_shared_kernel(CtxS c, int flags) {
  if (skipped(c, flags)) return;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  const int cur = c.ctrl->cur;
  bool ok = true;
  if (id < c.T) ok = track_half_s(c, cur, id, 2, c.x, c.xg);
  else if (id < c.T + c.n) ok = cam_apply_s(c, cur, id - c.T);
  else if (id < c.T + c.n + c.G) group_apply(c, cur, id - c.T - c.n);
  if (!ok) atomicOr(&c.ctrl->bad_a, 1);
}

__global__ void __launch_bounds__(kThreads) ba_write_shared_kernel(CtxS c) {
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  const int cur = c.ctrl->cur;
  if (!c.ctrl->err) {
    if (id < c.T) track_write(c, cur, id);
    else if (id < c.T + c.n) cam_write_s(c, cur, id - c.T);
  }
  if (id == 0) ctrl_write_s(c);
}

// the fixed launch schedule of §18.2
int run_shared(CtxS& c, int max_iters, int pcg_iters, void* ws, size_t ws_bytes, float* class_ms, long* class_launches, void* stream) {
  if (ws_bytes < layout_shared(c, nullptr)) return LOFTR_ERR_WORKSPACE;
  layout_shared(c, (char*)ws);
  hipStream_t s = (hipStream_t)stream;
  const long n = c.n, T = c.T, G = c.G;
  const bool timed = class_ms != nullptr;
  std::vector<hipEvent_t> ev;
  std::vector<int> ev_cls;
  long launches[kClsCount] = {0};
  bool failed = false;
  auto mark = [&]() {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess || hipEventRecord(e, s) != hipSuccess) failed = true;
    else ev.push_back(e);
  };
  auto after = [&](int cls) {
    if (hipGetLastError() != hipSuccess) failed = true;
    launches[cls] += 1;
    if (timed && !failed) { mark(); ev_cls.push_back(cls); }
  };
  auto blocks = [](long items, long per) { return dim3((unsigned)(items > 0 ? (items + per - 1) / per : 1)); };
  const Ctx& b = c;
  double* red2 = c.red + ((std::max(T, n) + 1 + kChunk - 1) / kChunk);
  // osum of v[0 .. count): one launch per level; `pair` = the shared kernel (kActStore, or a feed that adds the stored half)
  auto osum = [&](const double* v, long count, int action, int flags, bool pair) {
    const double* in = v;
    double* out = c.red;
    for (;;) {
      const long chunks = count > 0 ? (count + kChunk - 1) / kChunk : 1;
      const int act = chunks == 1 ? action : -1;
      if (pair) hipLaunchKernelGGL(ba_osum_shared_kernel, dim3((unsigned)chunks), dim3(64), 0, s, c, in, count, out, act, flags);
      else hipLaunchKernelGGL(ba_osum_kernel, dim3((unsigned)chunks), dim3(64), 0, s, b, in, count, out, act, flags);
      after(kClsOsum);
      if (chunks == 1) return;
      in = out;
      out = out == c.red ? red2 : c.red;
      count = chunks;
    }
  };
  auto dot = [&](int action, int flags) { osum(c.part, n, kActStore, flags, true); osum(c.partg, G, action, flags, true); };
  auto camera_half = [&](int mode, int flags) {
    hipLaunchKernelGGL(ba_cam_half_shared_kernel, blocks(n, 4), dim3(kThreads), 0, s, c, mode, flags); after(kClsCamHalf);
    hipLaunchKernelGGL(ba_group_half_kernel, blocks(G, 4), dim3(kThreads), 0, s, c, mode, flags); after(kClsCamHalf);
  };
  if (timed) mark();
  hipLaunchKernelGGL(ba_init_shared_kernel, dim3(1), dim3(1), 0, s, c); after(kClsSetup);
  hipLaunchKernelGGL(ba_cam_setup_kernel<7>, blocks(n, kThreads), dim3(kThreads), 0, s, (const Ctx7&)c); after(kClsSetup);
  hipLaunchKernelGGL(ba_track_setup_kernel, blocks(T, kThreads), dim3(kThreads), 0, s, b); after(kClsSetup);
  hipLaunchKernelGGL(ba_groups_shared_kernel, blocks(n, 4), dim3(kThreads), 0, s, c); after(kClsSetup);
  hipLaunchKernelGGL(ba_cgroups_kernel, blocks(G, 4), dim3(kThreads), 0, s, c); after(kClsSetup);
  hipLaunchKernelGGL(ba_evaluate_kernel, blocks(T, kThreads), dim3(kThreads), 0, s, b, 0, 0); after(kClsEvaluate);
  osum(c.part, T, kActCost0, 0, false);
  osum(c.part2, T, kActSq0, 0, false);
  for (int it = 0; it < max_iters && !failed; ++it) {
    hipLaunchKernelGGL(ba_track_lin_kernel<6>, blocks(T, kThreads), dim3(kThreads), 0, s, b, kNeedFresh); after(kClsLinearise);
    hipLaunchKernelGGL(ba_cam_lin_shared_kernel, blocks(n, 4), dim3(kThreads), 0, s, c, kNeedFresh); after(kClsLinearise);
    hipLaunchKernelGGL(ba_group_lin_kernel, blocks(G, 4), dim3(kThreads), 0, s, c, kNeedFresh); after(kClsLinearise);
    hipLaunchKernelGGL(ba_factor_shared_kernel, blocks(T + n + G, kThreads), dim3(kThreads), 0, s, c, 0); after(kClsFactor);
    hipLaunchKernelGGL(ba_track_half_shared_kernel, blocks(T, kThreads), dim3(kThreads), 0, s, c, 0, kSkipBadF); after(kClsTrackHalf);
    camera_half(0, kSkipBadF);
    dot(kActRz0, kSkipBadF);
    for (int pi = 0; pi < pcg_iters && !failed; ++pi) {
      const int f = kSkipBadF | kSkipPcg;
      hipLaunchKernelGGL(ba_track_half_shared_kernel, blocks(T, kThreads), dim3(kThreads), 0, s, c, 1, f); after(kClsTrackHalf);
      camera_half(1, f);
      dot(kActPsp, f);
      hipLaunchKernelGGL(ba_update_shared_kernel, blocks(n + G, kThreads), dim3(kThreads), 0, s, c, 1, f); after(kClsUpdate);
      dot(kActRz, f);
      hipLaunchKernelGGL(ba_update_shared_kernel, blocks(n + G, kThreads), dim3(kThreads), 0, s, c, 2, f); after(kClsUpdate);
    }
    hipLaunchKernelGGL(ba_apply_shared_kernel, blocks(T + n + G, kThreads), dim3(kThreads), 0, s, c, kSkipBadF); after(kClsApply);
    hipLaunchKernelGGL(ba_evaluate_kernel, blocks(T, kThreads), dim3(kThreads), 0, s, b, 1, kSkipBadF | kSkipBadA); after(kClsEvaluate);
    osum(c.part, T, kActCostT, kSkipBadF | kSkipBadA | kSkipBadE, false);
    osum(c.part2, T, kActSqT, kSkipBadF | kSkipBadA | kSkipBadE, false);
    hipLaunchKernelGGL(ba_accept_kernel, dim3(1), dim3(1), 0, s, b); after(kClsAccept);
  }
  hipLaunchKernelGGL(ba_write_shared_kernel, blocks(T + n, kThreads), dim3(kThreads), 0, s, c); after(kClsWrite);
  if (class_launches) for (int k = 0; k < kClsCount; ++k) class_launches[k] = launches[k];
  if (timed) {
    if (hipStreamSynchronize(s) != hipSuccess) failed = true;
    std::vector<float> ms[kClsCount];
    for (size_t k = 0; k + 1 < ev.size() && !failed; ++k) {
      float v = 0.f;
      if (hipEventElapsedTime(&v, ev[k], ev[k + 1]) == hipSuccess) ms[ev_cls[k]].push_back(v);
    }
    for (int k = 0; k < kClsCount; ++k) {
      std::sort(ms[k].begin(), ms[k].end());
      float total = 0.f;
      for (float v : ms[k]) total += v;
      class_ms[2 * k] = ms[k].empty() ? 0.f : ms[k][ms[k].size() / 2];
      class_ms[2 * k + 1] = total;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
  }
  return failed ? LOFTR_ERR_LAUNCH : LOFTR_OK;
}

}  // namespace

extern "C" size_t loftr_bundle_adjust_shared_workspace_bytes(long T, long N, int n_images) {
  if (!sizes_ok(T, N, n_images)) return 0;
  CtxS c{};
  c.T = T; c.N = N; c.n = n_images;
  return layout_shared(c, nullptr);
}

extern "C" int loftr_bundle_adjust_shared(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                          long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                          const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                          const int* cam_group, const long* group_offsets, const int* group_cams, int G, double huber_px,
                                          int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs, double focal_lo,
                                          double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free,
                                          uint8_t* point_active, double* K_out, uint8_t* cam_focal, uint8_t* group_focal, long* counts,
                                          void* ws, size_t ws_bytes, float* class_ms, long* class_launches, void* stream) {
  LOFTR_CHECK_ARG(n_images <= 0 || (refine_focal && K_out && cam_focal && cam_group && group_cams && group_focal));
  LOFTR_CHECK_ARG(group_offsets && G >= 0 && G <= n_images && (n_images <= 0 || G > 0));
  LOFTR_CHECK_ARG(min_focal_obs >= 1 && fin(focal_lo) && fin(focal_hi) && focal_lo < 1.0 && 1.0 < focal_hi);
  const int st = check_args(offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs,
                            huber_px, max_iters, pcg_iters, pcg_tol, ftol, T_out, xyz_out, obs_active, cam_free, point_active, counts, ws);
  if (st != LOFTR_OK) return st;
  CtxS c{};
  c.offsets = offsets; c.T = T; c.image = obs_image; c.xy = obs_xy; c.mask = obs_mask; c.N = N;
  c.xyz_in = xyz; c.K = K; c.Tin = T_cam_from_world; c.fixed = fixed; c.n = n_images; c.cam_offsets = cam_offsets; c.cam_obs = cam_obs;
  c.huber = huber_px; c.pcg_tol2 = pcg_tol * pcg_tol; c.ftol = ftol;
  c.T_out = T_out; c.xyz_out = xyz_out; c.obs_active = obs_active; c.cam_free = cam_free; c.point_active = point_active; c.counts = counts;
  c.refine_focal = refine_focal; c.min_focal_obs = min_focal_obs; c.focal_lo = focal_lo; c.focal_hi = focal_hi;
  c.K_out = K_out; c.cam_focal = cam_focal;
  c.cam_group = cam_group; c.group_offsets = group_offsets; c.group_cams = group_cams; c.G = G; c.group_focal = group_focal;
  return run_shared(c, max_iters, pcg_iters, ws, ws_bytes, class_ms, class_launches, stream);
}

extern "C" size_t loftr_bundle_adjust_workspace_bytes(long T, long N, int n_images) {
  if (!sizes_ok(T, N, n_images)) return 0;
  Ctx c{};
  c.T = T; c.N = N; c.n = n_images;
  return layout<6>(c, nullptr);
}

extern "C" size_t loftr_bundle_adjust_focal_workspace_bytes(long T, long N, int n_images) {
  if (!sizes_ok(T, N, n_images)) return 0;
  Ctx c{};
  c.T = T; c.N = N; c.n = n_images;
  return layout<7>(c, nullptr);
}

extern "C" int loftr_bundle_adjust(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                                   const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed, int n_images,
                                   const long* cam_offsets, const int* cam_obs, double huber_px, int max_iters, int pcg_iters, double pcg_tol,
                                   double ftol, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active,
                                   long* counts, void* ws, size_t ws_bytes, float* class_ms, long* class_launches, void* stream) {
  const int st = check_args(offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs,
                            huber_px, max_iters, pcg_iters, pcg_tol, ftol, T_out, xyz_out, obs_active, cam_free, point_active, counts, ws);
  if (st != LOFTR_OK) return st;
  Ctx c{};
  c.offsets = offsets; c.T = T; c.image = obs_image; c.xy = obs_xy; c.mask = obs_mask; c.N = N;
  c.xyz_in = xyz; c.K = K; c.Tin = T_cam_from_world; c.fixed = fixed; c.n = n_images; c.cam_offsets = cam_offsets; c.cam_obs = cam_obs;
  c.huber = huber_px; c.pcg_tol2 = pcg_tol * pcg_tol; c.ftol = ftol;
  c.T_out = T_out; c.xyz_out = xyz_out; c.obs_active = obs_active; c.cam_free = cam_free; c.point_active = point_active; c.counts = counts;
  return run<6>(c, max_iters, pcg_iters, ws, ws_bytes, class_ms, class_launches, stream);
}

extern "C" int loftr_bundle_adjust_focal(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                         long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                         const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                         double huber_px, int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs,
                                         double focal_lo, double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active,
                                         uint8_t* cam_free, uint8_t* point_active, double* K_out, uint8_t* cam_focal, long* counts, void* ws,
                                         size_t ws_bytes, float* class_ms, long* class_launches, void* stream) {
  LOFTR_CHECK_ARG(n_images <= 0 || (refine_focal && K_out && cam_focal));
  LOFTR_CHECK_ARG(min_focal_obs >= 1 && fin(focal_lo) && fin(focal_hi) && focal_lo < 1.0 && 1.0 < focal_hi);
  const int st = check_args(offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs,
                            huber_px, max_iters, pcg_iters, pcg_tol, ftol, T_out, xyz_out, obs_active, cam_free, point_active, counts, ws);
  if (st != LOFTR_OK) return st;
  Ctx7 c{};
  c.offsets = offsets; c.T = T; c.image = obs_image; c.xy = obs_xy; c.mask = obs_mask; c.N = N;
  c.xyz_in = xyz; c.K = K; c.Tin = T_cam_from_world; c.fixed = fixed; c.n = n_images; c.cam_offsets = cam_offsets; c.cam_obs = cam_obs;
  c.huber = huber_px; c.pcg_tol2 = pcg_tol * pcg_tol; c.ftol = ftol;
  c.T_out = T_out; c.xyz_out = xyz_out; c.obs_active = obs_active; c.cam_free = cam_free; c.point_active = point_active; c.counts = counts;
  c.refine_focal = refine_focal; c.min_focal_obs = min_focal_obs; c.focal_lo = focal_lo; c.focal_hi = focal_hi;
  c.K_out = K_out; c.cam_focal = cam_focal;
  return run<7>(c, max_iters, pcg_iters, ws, ws_bytes, class_ms, class_launches, stream);
}
