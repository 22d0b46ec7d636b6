// Bundle adjustment on the GPU: the host routines of bundle.hip with the same result bit for bit (DESIGN §18 .. §18.5).
// Every phase of the host sequence is one kernel here, every per-item step is bundle_core.h's, compiled from the same text, fp64 without
// FMA contraction.  As on the host there is ONE schedule, run<Mode>, with one event / launch accounting; every kernel whose phase
// differs between modes is a template on the mode that names its class: the mode itself where the prior acts, its Base where it does
// not, TrackMode for the track phases (the projection alone tells them apart), SetupMode for the camera setup.  The group kernels and
// launches of the grouped modes are `if constexpr (kGroups)` in the schedule.  What this file adds is only how a phase is spread over
// threads:
//   a thread per track      setup, linearise, track half of S p, back substitution, evaluate (the sums of a track run sequentially in
//                           that one thread, as §16's refit);
//   a wave per camera       groups check, linearise, camera half of S p: lane l accumulates slots l, l + 64, ... of the camera's list
//                           and the 64 lanes are folded 32, 16, ..., 1 with shuffles -- osum64 exactly as the host's 64-entry array;
//   a wave per group        (kGroups) the group check, the sums of its block, the group half: the members folded as a camera's observations;
//   a wave per 4096 terms   osum over tracks, cameras or groups, one launch per level; lane 0 of the last level hands the sum to ctrl_feed;
//   a thread per camera     factor, the two updates of the conjugate gradients, apply (kGroups: the groups in the threads after them);
//   one thread              init, accept: the owner of lambda, the counters and the flags.
// The whole run is a FIXED launch schedule on the caller's stream: max_iters trials of pcg_iters iterations each.  A kernel whose phase
// the host routine would not run (the run has stopped, the conjugate gradients have stopped, the step is already rejected, an error bit
// is up) returns at once on a flag in device memory; a flag is only ever read by kernels launched after the one that wrote it.  No
// readback, no grid-wide barrier, no persistent kernel, no captured graph: a kernel boundary is the only device-wide ordering.
// Floating-point values cross lanes only as exact copies (shuffles); atomics are integer only.  Plain C++, ordinary vector stores.
// Position priors (§18.3) are a trait of the mode: PoseP, FocalP and SharedP run the same schedule; the decision is taken by the lane
// that ends ba_groups_kernel, the additions to U and gc by the lane that ends ba_cam_lin_kernel, a thread per camera evaluates the
// prior of a state (ba_prior_eval_kernel), the levels of the cameras' osum follow it (ba_prior_osum_kernel), and every kernel that the
// prior does not touch is the one of the mode without it (it takes the Base context by value: a wider kernel argument alone cost time,
// profiles/bundle_refactor_bench.txt).  Radial (§18.4) runs §18.2's schedule launch for launch, as one more instantiation.
#include <algorithm>
#include <type_traits>
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

// osum64 of the elements [b, e) over the 64 lanes of a wave: lane l takes b + l, b + l + 64, ... with term(k, a), then the lanes are
// folded; a [M] of lane 0 is the sum
template <int M, class F> __device__ __forceinline__ void wave_osum64(long b, long e, int lane, F term, double* a) {
#pragma unroll
  for (int m = 0; m < M; ++m) a[m] = 0.0;
  for (long k = b + lane; k < e; k += 64) term(k, a);
  for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const double v = __shfl_down(a[m], s, 64);
      if (lane < s) a[m] = a[m] + v;
    }
}
// ... of camera i's list: an inactive slot adds nothing
template <int M, class F> __device__ __forceinline__ void wave_cam_sum(const Ctx& c, long i, int lane, F term, double* a) {
  wave_osum64<M>(c.cam_offsets[i], c.cam_offsets[i + 1], lane, [&](long k, double* acc) {
    const long o = c.cam_obs[k];
    if (c.obs_active[o]) term(o, acc);
  }, a);
}
// ... of group g's list: term(i, a) adds member i
template <int M, class F> __device__ __forceinline__ void wave_group_sum(const CtxS& c, long g, int lane, F term, double* a) {
  wave_osum64<M>(c.group_offsets[g], c.group_offsets[g + 1], lane, [&](long k, double* acc) { term(c.group_cams[k], acc); }, a);
}
// the wave as the workers of a group's decision (OneLane of the core is the host's): folds with shuffles, integer atomics
struct WaveLanes {
  static constexpr int kLanes = 64;
  int lane;
  __device__ long sum(long v) const { for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64); return v; }
  __device__ int any(int v) const { for (int m = 32; m >= 1; m >>= 1) v |= __shfl_xor(v, m, 64); return v; }
  __device__ void add(int* p, int v) const { if (v) atomicAdd(p, v); }
  __device__ void raise(int* p, int v) const { atomicOr(p, v); }
};

// what the factor and update kernels take: the base of the context (their steps need no more), with groups the groups' vectors too
// (the group steps of these two phases read nothing beyond CtxS in any mode)
template <class Mode> using StepCtx = std::conditional_t<Mode::kGroups, CtxS, Ctx>;

__global__ void ba_init_kernel(Ctx c, CtrlS* cs) { ctrl_init(c, cs); }
__global__ void ba_prior_init_kernel(Prior p) { ctrl_init_prior(p); }

// grid ceil(n / 256) x 256; Mode: Pose, Focal or Radial (SetupMode).  Thread 0 owns what the phase resets.
template <class Mode> __global__ void __launch_bounds__(kThreads) ba_cam_setup_kernel(typename Mode::Ctx c) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) cam_setup_ctrl<Mode>(c);
  if (i < c.n) cam_setup<Mode>(c, i);
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

// a wave per camera, grid ceil(n / 4) x 256.  Reads the observation arrays only through checked indices, so it needs no flag.  The last
// step: Focal, whether the camera refines its focal; Shared, what it carries for its group.
template <class Mode> __global__ void __launch_bounds__(kThreads) ba_groups_kernel(typename Mode::Ctx c) {
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
    if constexpr (Mode::kPrior) {
      const bool pr = cam_prior_rule(c, c.pr, i);
      c.pr.cam_prior[i] = (uint8_t)pr;
      if (pr) atomicAdd(&c.pr.cp->n_prior, 1ull);
    }
    if constexpr (Mode::kGroups) err |= cam_carry(c, i, cnt);
    if (err) atomicOr(&c.ctrl->err, err);
    if constexpr (Mode::S == 7 && !Mode::kGroups) {
      const bool fo = cam_focal_rule(c, i, fr, cnt);
      c.cam_focal[i] = (uint8_t)fo;
      if (fo) atomicAdd(&c.ctrl->n_focal, 1);
    }
  }
}

// A wave per group, grid ceil(G / 4) x 256: the check of the group arrays, the counts and the decisions (cgroup_decide); a wave per
// group folds its members exactly as a wave per camera folds its observations.  Reads the arrays only through checked indices, and
// writes cam_focal only when the whole list of the group has passed, so it needs no flag.
template <class Mode> __global__ void __launch_bounds__(kThreads) ba_cgroups_kernel(typename Mode::Ctx c) {
  const long g = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  if (g < c.G) cgroup_decide<Mode>(c, g, WaveLanes{(int)(threadIdx.x % 64)});
}

// grid ceil(T / 256) x 256; other = 0 evaluates the state, 1 the trial.  TMode: Pose or Radial (TrackMode), the projection
template <class TMode> __global__ void __launch_bounds__(kThreads) ba_evaluate_kernel(typename TMode::Ctx c, int other, int flags) {
  if (skipped(c, flags)) return;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t < c.T && !track_eval<TMode>(c, c.ctrl->cur ^ other, t)) atomicOr(&c.ctrl->bad_e, 1);
}

// one level of an osum: a wave per chunk of 4096, grid ceil(count / 4096) (at least 1) x 64.  On the last level action >= 0 feeds the
// sum, or with acc the sum that waits there plus this one (a dot product of two halves), and kActStore leaves it in acc to wait.
__global__ void __launch_bounds__(64) ba_osum_kernel(Ctx c, const double* in, long count, double* out, int action, double* acc, int flags) {
  if (skipped(c, flags)) return;
  const int lane = threadIdx.x;
  const long lo = (long)blockIdx.x * kChunk, len = count - lo < kChunk ? count - lo : kChunk;
  double a;
  wave_osum64<1>(0, len, lane, [&](long e, double* s) { s[0] = s[0] + in[lo + e]; }, &a);
  if (lane == 0) {
    if (action == kActStore) *acc = a;
    else if (action >= 0) ctrl_feed(c, action, acc ? *acc + a : a);
    else out[blockIdx.x] = a;
  }
}

// §18.3.  A thread per camera, grid ceil(n / 256) x 256: its share of the cost and |c - g|^2 at the state (other = 0) or the trial
__global__ void __launch_bounds__(kThreads) ba_prior_eval_kernel(Ctx c, Prior p, int other, int flags) {
  if (skipped(c, flags)) return;
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i < c.n) cam_prior_eval(c, p, c.ctrl->cur ^ other, i);
}
// ... and one level of a cameras' osum, as ba_osum_kernel; the last level feeds the owner of the prior's scalars
__global__ void __launch_bounds__(64) ba_prior_osum_kernel(Ctx c, Prior p, const double* in, long count, double* out, int action, int flags) {
  if (skipped(c, flags)) return;
  const int lane = threadIdx.x;
  const long lo = (long)blockIdx.x * kChunk, len = count - lo < kChunk ? count - lo : kChunk;
  double a;
  wave_osum64<1>(0, len, lane, [&](long e, double* s) { s[0] = s[0] + in[lo + e]; }, &a);
  if (lane == 0) {
    if (action >= 0) ctrl_feed_prior(c, p, action, a);
    else out[blockIdx.x] = a;
  }
}

template <class TMode> __global__ void __launch_bounds__(kThreads) ba_track_lin_kernel(typename TMode::Ctx c, int flags) {
  if (skipped(c, flags)) return;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t < c.T) track_lin<TMode>(c, c.ctrl->cur, t);
}

// a wave per camera that takes part, grid ceil(n / 4) x 256
template <class Mode> __global__ void __launch_bounds__(kThreads) ba_cam_lin_kernel(typename Mode::Ctx c, int flags) {
  if (skipped(c, flags)) return;
  const long i = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64, cur = c.ctrl->cur;
  if (i >= c.n || !takes_part<Mode>(c, i)) return;
  constexpr int S = Mode::S, kU = kTri<S>;
  double a[kU + S];
  wave_cam_sum<kU + S>(c, i, lane, [&](long o, double* acc) { cam_lin_term<Mode>(c, cur, o, acc); }, a);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kU; ++k) c.U[kU * i + k] = a[k];
#pragma unroll
    for (int k = 0; k < S; ++k) c.gc[S * i + k] = a[kU + k];
    if constexpr (Mode::kPrior) cam_lin_prior<S>(c, c.pr, cur, i);
  }
}

// A wave per refining group, grid ceil(G / 4) x 256: d_g = the sum of U77 over its members (Radial: the three sums of its 2 x 2 block)
template <class Mode> __global__ void __launch_bounds__(kThreads) ba_group_lin_kernel(typename Mode::Ctx c, int flags) {
  if (skipped(c, flags)) return;
  const long g = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (g >= c.G || !c.group_focal[g]) return;
  constexpr int kD = kTri<Mode::GW>;
  double d[kD];
  wave_group_sum<kD>(c, g, lane, [&](long i, double* acc) { group_lin_term<Mode>(c, i, acc); }, d);
  if (lane == 0)
    for (int k = 0; k < kD; ++k) c.dg[kD * g + k] = d[k];
}

// threads [0, T): tracks, [T, T + n): cameras, Shared [T + n, T + n + G): groups; grid ceil of that / 256 x 256
template <class Mode> __global__ void __launch_bounds__(kThreads) ba_factor_kernel(StepCtx<Mode> c, int flags) {
  if (skipped(c, flags)) return;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  const double lambda = c.ctrl->lambda;
  bool ok = true;
  if (id < c.T) ok = track_factor(c, id, lambda);
  else if (id < c.T + c.n) ok = cam_factor<Mode>(c, id - c.T, lambda);
  else if constexpr (Mode::kGroups) {
    if (id < c.T + c.n + c.G) ok = group_factor<Mode>(c, id - c.T - c.n, lambda);
  }
  if (!ok) atomicOr(&c.ctrl->bad_f, 1);
}

// mode 0: z = Vd^-1 gp; mode 1: the track half of S p
template <class Mode> __global__ void __launch_bounds__(kThreads) ba_track_half_kernel(typename Mode::Ctx c, int mode, int flags) {
  if (skipped(c, flags)) return;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t < c.T) track_half<Mode>(c, c.ctrl->cur, t, mode);
}

// a wave per camera, grid ceil(n / 4) x 256.  mode 0: the right-hand side and the start of the conjugate gradients; mode 1: S p
template <class Mode> __global__ void __launch_bounds__(kThreads) ba_cam_half_kernel(typename Mode::Ctx c, int mode, int flags) {
  if (skipped(c, flags)) return;
  const long i = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64, cur = c.ctrl->cur;
  if (i >= c.n) return;
  constexpr int S = Mode::S;
  double a[S];
#pragma unroll
  for (int k = 0; k < S; ++k) a[k] = 0.0;
  if (takes_part<Mode>(c, i)) wave_cam_sum<S>(c, i, lane, [&](long o, double* acc) { cam_half_term<Mode>(c, cur, o, acc); }, a);
  if (lane == 0) cam_half_finish<Mode>(c, i, mode, c.ctrl->lambda, a);
}

// A wave per group, grid ceil(G / 4) x 256: E^T of the cameras' seventh (Radial: and eighth) entries, then the group's own step
template <class Mode> __global__ void __launch_bounds__(kThreads) ba_group_half_kernel(typename Mode::Ctx c, int mode, int flags) {
  if (skipped(c, flags)) return;
  const long g = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (g >= c.G) return;
  double s[Mode::GW];
#pragma unroll
  for (int k = 0; k < Mode::GW; ++k) s[k] = 0.0;
  if (c.group_focal[g]) wave_group_sum<Mode::GW>(c, g, lane, [&](long i, double* acc) { group_half_term<Mode>(c, i, acc); }, s);
  if (lane == 0) group_half_finish<Mode>(c, g, mode, c.ctrl->lambda, s);
}

// threads [0, n): cameras, Shared [n, n + G): groups (the scalar update of a group)
template <class Mode> __global__ void __launch_bounds__(kThreads) ba_update_kernel(StepCtx<Mode> c, int which, int flags) {
  if (skipped(c, flags)) return;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  if (id < c.n) {
    if (which == 1) cam_update1<Mode>(c, id, c.ctrl->alpha);
    else cam_update2<Mode>(c, id, c.ctrl->beta);
  } else if constexpr (Mode::kGroups) {
    if (id >= c.n + c.G) return;
    if (which == 1) group_update1<Mode>(c, id - c.n, c.ctrl->alpha, c.ctrl->lambda);
    else group_update2<Mode>(c, id - c.n, c.ctrl->beta);
  }
}

// threads [0, T): back substitution of the tracks, [T, T + n): the cameras' trial poses and focals, Shared [T + n, T + n + G): the groups
template <class Mode> __global__ void __launch_bounds__(kThreads) ba_apply_kernel(typename Mode::Ctx c, int flags) {
  if (skipped(c, flags)) return;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  const int cur = c.ctrl->cur;
  bool ok = true;
  if (id < c.T) ok = track_half<Mode>(c, cur, id, 2);
  else if (id < c.T + c.n) ok = cam_apply<Mode>(c, cur, id - c.T);
  else if constexpr (Mode::kGroups) {
    if (id < c.T + c.n + c.G) group_apply<Mode>(c, cur, id - c.T - c.n);
  }
  if (!ok) atomicOr(&c.ctrl->bad_a, 1);
}

__global__ void ba_accept_kernel(Ctx c) { ctrl_accept(c); }
__global__ void ba_prior_accept_kernel(Ctx c, Prior p) { ctrl_accept_prior(c, p); }

// threads [0, T): points, [T, T + n): cameras; thread 0 also writes the counts.  Runs whatever the flags say.
template <class Mode> __global__ void __launch_bounds__(kThreads) ba_write_kernel(typename Mode::Ctx c) {
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  const int cur = c.ctrl->cur;
  if (!c.ctrl->err) {
    if (id < c.T) track_write(c, cur, id);
    else if (id < c.T + c.n) cam_write<Mode>(c, cur, id - c.T);
  }
  if (id == 0) {
    ctrl_write<Mode>(c);
    if constexpr (Mode::kPrior) ctrl_write_prior(c, c.pr);
  }
}

// the fixed launch schedule of every mode; c holds the problem and the result.  The phases that do not touch the camera block or the
// groups (track setup, accept, the osum; evaluate and the track linearisation per projection) are one kernel for all modes, on the
// base of the context.
template <class Mode> int run(typename Mode::Ctx& c, int max_iters, int pcg_iters, double pcg_tol, void* ws, size_t ws_bytes, float* class_ms,
                              long* class_launches, void* stream) {
  constexpr bool kGroups = Mode::kGroups, kPrior = Mode::kPrior;
  using BaseMode = typename Mode::Base;                                 // the kernels of the phases that the prior does not touch
  using TMode = TrackMode<Mode>;                                        // ... of the track phases: the projection alone tells them apart
  LOFTR_CHECK_ARG(ws);
  const int st = check_args<Mode>(c, max_iters, pcg_iters, pcg_tol, false);
  if (st != LOFTR_OK) return st;
  if (ws_bytes < layout<Mode>(c, nullptr)) return LOFTR_ERR_WORKSPACE;
  layout<Mode>(c, (char*)ws);
  hipStream_t s = (hipStream_t)stream;
  const long n = c.n, T = c.T;
  long G = 0;
  double* acc = nullptr;                                                // where the cameras' half of a dot product waits for the groups'
  if constexpr (kGroups) { G = c.G; acc = &c.cs->acc; }
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
  const dim3 threads(kThreads);
  const Ctx& b = c;                                                     // what the kernels of all modes take
  const typename BaseMode::Ctx& cb = c;                                 // ... and those of the mode, without the prior
  const typename TMode::Ctx& tb = c;                                    // ... those of the track phases
  const typename SetupMode<Mode>::Ctx& sb = c;                          // ... and the camera setup
  Prior pr{};
  if constexpr (kPrior) pr = c.pr;
  double* red2 = c.red + ((std::max(T, n) + 1 + kChunk - 1) / kChunk);
  // the levels of an osum of v[0 .. count): launch(chunks, in, count, out, last) once per level
  auto levels = [&](const double* v, long count, auto launch) {
    const double* in = v;
    double* out = c.red;
    for (;;) {
      const long chunks = count > 0 ? (count + kChunk - 1) / kChunk : 1;
      launch(dim3((unsigned)chunks), in, count, out, chunks == 1);
      after(kClsOsum);
      if (chunks == 1) return;
      in = out;
      out = out == c.red ? red2 : c.red;
      count = chunks;
    }
  };
  // osum of v[0 .. count) into `action` (ba_osum_kernel)
  auto osum = [&](const double* v, long count, int action, double* wait, int flags) {
    levels(v, count, [&](dim3 grid, const double* in, long cnt, double* out, bool last) {
      hipLaunchKernelGGL(ba_osum_kernel, grid, dim3(64), 0, s, b, in, cnt, out, last ? action : -1, wait, flags);
    });
  };
  // ... of the cameras' prior terms v[0 .. n) into `action` (ba_prior_osum_kernel)
  auto prior_osum = [&](const double* v, int action, int flags) {
    levels(v, n, [&](dim3 grid, const double* in, long cnt, double* out, bool last) {
      hipLaunchKernelGGL(ba_prior_osum_kernel, grid, dim3(64), 0, s, b, pr, in, cnt, out, last ? action : -1, flags);
    });
  };
  // a dot product over the unknowns: the cameras' terms, and with groups the groups' terms added to their sum
  auto dot = [&](int action, int flags) {
    if constexpr (kGroups) {
      osum(c.part, n, kActStore, acc, flags);
      osum(c.partg, G, action, acc, flags);
    } else osum(c.part, n, action, nullptr, flags);
  };
  auto camera_half = [&](int mode, int flags) {
    hipLaunchKernelGGL(ba_cam_half_kernel<BaseMode>, blocks(n, 4), threads, 0, s, cb, mode, flags); after(kClsCamHalf);
    if constexpr (kGroups) { hipLaunchKernelGGL(ba_group_half_kernel<BaseMode>, blocks(G, 4), threads, 0, s, cb, mode, flags); after(kClsCamHalf); }
  };
  // evaluate the state (other = 0) or the trial, then its cost and sum of |r|^2: the tracks' osum, with priors the cameras' added to it
  auto evaluate = [&](int other, int cost, int sq, int flags) {
    hipLaunchKernelGGL(ba_evaluate_kernel<TMode>, blocks(T, kThreads), threads, 0, s, tb, other, flags); after(kClsEvaluate);
    const int f = other ? flags | kSkipBadE : flags;
    if constexpr (kPrior) {
      hipLaunchKernelGGL(ba_prior_eval_kernel, blocks(n, kThreads), threads, 0, s, b, pr, other, flags); after(kClsEvaluate);
      osum(c.part, T, kActStore, &pr.cp->acc, f);
      prior_osum(pr.part, cost, f);
      osum(c.part2, T, sq, nullptr, f);
      prior_osum(pr.part2, sq, f);
    } else {
      osum(c.part, T, cost, nullptr, f);
      osum(c.part2, T, sq, nullptr, f);
    }
  };
  if (timed) mark();
  hipLaunchKernelGGL(ba_init_kernel, dim3(1), dim3(1), 0, s, b, groups_ctrl<Mode>(c)); after(kClsSetup);
  if constexpr (kPrior) { hipLaunchKernelGGL(ba_prior_init_kernel, dim3(1), dim3(1), 0, s, pr); after(kClsSetup); }
  hipLaunchKernelGGL(ba_cam_setup_kernel<SetupMode<Mode>>, blocks(n, kThreads), threads, 0, s, sb); after(kClsSetup);
  hipLaunchKernelGGL(ba_track_setup_kernel, blocks(T, kThreads), threads, 0, s, b); after(kClsSetup);
  hipLaunchKernelGGL(ba_groups_kernel<Mode>, blocks(n, 4), threads, 0, s, c); after(kClsSetup);
  if constexpr (kGroups) { hipLaunchKernelGGL(ba_cgroups_kernel<BaseMode>, blocks(G, 4), threads, 0, s, cb); after(kClsSetup); }
  evaluate(0, kActCost0, kActSq0, 0);
  for (int it = 0; it < max_iters && !failed; ++it) {
    hipLaunchKernelGGL(ba_track_lin_kernel<TMode>, blocks(T, kThreads), threads, 0, s, tb, kNeedFresh); after(kClsLinearise);
    hipLaunchKernelGGL(ba_cam_lin_kernel<Mode>, blocks(n, 4), threads, 0, s, c, kNeedFresh); after(kClsLinearise);
    if constexpr (kGroups) { hipLaunchKernelGGL(ba_group_lin_kernel<BaseMode>, blocks(G, 4), threads, 0, s, cb, kNeedFresh); after(kClsLinearise); }
    hipLaunchKernelGGL(ba_factor_kernel<BaseMode>, blocks(T + n + G, kThreads), threads, 0, s, cb, 0); after(kClsFactor);
    hipLaunchKernelGGL(ba_track_half_kernel<BaseMode>, blocks(T, kThreads), threads, 0, s, cb, 0, kSkipBadF); after(kClsTrackHalf);
    camera_half(0, kSkipBadF);
    dot(kActRz0, kSkipBadF);
    for (int pi = 0; pi < pcg_iters && !failed; ++pi) {
      const int f = kSkipBadF | kSkipPcg;
      hipLaunchKernelGGL(ba_track_half_kernel<BaseMode>, blocks(T, kThreads), threads, 0, s, cb, 1, f); after(kClsTrackHalf);
      camera_half(1, f);
      dot(kActPsp, f);
      hipLaunchKernelGGL(ba_update_kernel<BaseMode>, blocks(n + G, kThreads), threads, 0, s, cb, 1, f); after(kClsUpdate);
      dot(kActRz, f);
      hipLaunchKernelGGL(ba_update_kernel<BaseMode>, blocks(n + G, kThreads), threads, 0, s, cb, 2, f); after(kClsUpdate);
    }
    hipLaunchKernelGGL(ba_apply_kernel<BaseMode>, blocks(T + n + G, kThreads), threads, 0, s, cb, kSkipBadF); after(kClsApply);
    evaluate(1, kActCostT, kActSqT, kSkipBadF | kSkipBadA);
    if constexpr (kPrior) hipLaunchKernelGGL(ba_prior_accept_kernel, dim3(1), dim3(1), 0, s, b, pr);
    else hipLaunchKernelGGL(ba_accept_kernel, dim3(1), dim3(1), 0, s, b);
    after(kClsAccept);
  }
  hipLaunchKernelGGL(ba_write_kernel<Mode>, blocks(T + n, kThreads), threads, 0, s, c); after(kClsWrite);
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

template <class Mode> int enter(const Args& a, void* ws, size_t ws_bytes, float* class_ms, long* class_launches, void* stream) {
  typename Mode::Ctx c{};
  fill<Mode>(c, a);
  return run<Mode>(c, a.par.max_iters, a.par.pcg_iters, a.par.pcg_tol, ws, ws_bytes, class_ms, class_launches, stream);
}

}  // namespace

extern "C" size_t loftr_bundle_adjust_workspace_bytes(long T, long N, int n_images) { return workspace_bytes(kKindPose, false, T, N, n_images); }
extern "C" size_t loftr_bundle_adjust_focal_workspace_bytes(long T, long N, int n_images) { return workspace_bytes(kKindFocal, false, T, N, n_images); }
extern "C" size_t loftr_bundle_adjust_shared_workspace_bytes(long T, long N, int n_images) { return workspace_bytes(kKindShared, false, T, N, n_images); }
extern "C" size_t loftr_bundle_adjust_radial_workspace_bytes(long T, long N, int n_images) { return workspace_bytes(kKindRadial, false, T, N, n_images); }
extern "C" size_t loftr_bundle_adjust_prior_workspace_bytes(long T, long N, int n_images, int mode) { return workspace_bytes(mode, true, T, N, n_images); }

extern "C" int loftr_bundle_adjust(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                                   const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed, int n_images,
                                   const long* cam_offsets, const int* cam_obs, double huber_px, int max_iters, int pcg_iters, double pcg_tol,
                                   double ftol, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active,
                                   long* counts, void* ws, size_t ws_bytes, float* class_ms, long* class_launches, void* stream) {
  return enter<Pose>({{offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs},
                      {huber_px, max_iters, pcg_iters, pcg_tol, ftol}, {T_out, xyz_out, obs_active, cam_free, point_active, counts}},
                     ws, ws_bytes, class_ms, class_launches, stream);
}

extern "C" int loftr_bundle_adjust_focal(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                         long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                         const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                         double huber_px, int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs,
                                         double focal_lo, double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active,
                                         uint8_t* cam_free, uint8_t* point_active, double* K_out, uint8_t* cam_focal, long* counts, void* ws,
                                         size_t ws_bytes, float* class_ms, long* class_launches, void* stream) {
  return enter<Focal>({{offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs},
                       {huber_px, max_iters, pcg_iters, pcg_tol, ftol}, {T_out, xyz_out, obs_active, cam_free, point_active, counts},
                       {refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal}},
                      ws, ws_bytes, class_ms, class_launches, stream);
}

extern "C" int loftr_bundle_adjust_shared(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                          long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                          const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                          const int* cam_group, const long* group_offsets, const int* group_cams, int G, double huber_px,
                                          int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs, double focal_lo,
                                          double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free,
                                          uint8_t* point_active, double* K_out, uint8_t* cam_focal, uint8_t* group_focal, long* counts,
                                          void* ws, size_t ws_bytes, float* class_ms, long* class_launches, void* stream) {
  return enter<Shared>({{offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs},
                        {huber_px, max_iters, pcg_iters, pcg_tol, ftol}, {T_out, xyz_out, obs_active, cam_free, point_active, counts},
                        {refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal}, {cam_group, group_offsets, group_cams, G, group_focal}},
                       ws, ws_bytes, class_ms, class_launches, stream);
}

extern "C" int loftr_bundle_adjust_radial(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                          long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                          const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                          const int* cam_group, const long* group_offsets, const int* group_cams, int G,
                                          const double* radial_in, const uint8_t* refine_radial, double huber_px, int max_iters, int pcg_iters,
                                          double pcg_tol, double ftol, int min_focal_obs, double focal_lo, double focal_hi, double radial_lo,
                                          double radial_hi, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free,
                                          uint8_t* point_active, double* K_out, uint8_t* cam_focal, uint8_t* group_focal, double* radial_out,
                                          uint8_t* cam_radial, uint8_t* group_radial, long* counts, void* ws, size_t ws_bytes, float* class_ms,
                                          long* class_launches, void* stream) {
  return enter<Radial>({{offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs},
                        {huber_px, max_iters, pcg_iters, pcg_tol, ftol}, {T_out, xyz_out, obs_active, cam_free, point_active, counts},
                        {refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal}, {cam_group, group_offsets, group_cams, G, group_focal},
                        {radial_in, refine_radial, radial_lo, radial_hi, radial_out, cam_radial, group_radial}},
                       ws, ws_bytes, class_ms, class_launches, stream);
}

// with position priors on the camera centres (§18.3): mode 0 pose, 1 focal, 2 shared; the focal and group arguments are ignored below
// their mode
extern "C" int loftr_bundle_adjust_prior(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                         long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                         const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                         const int* cam_group, const long* group_offsets, const int* group_cams, int G,
                                         const double* prior_xyz, const double* prior_sigma, const uint8_t* prior_mask, int mode,
                                         double huber_px, int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs,
                                         double focal_lo, double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active,
                                         uint8_t* cam_free, uint8_t* point_active, double* K_out, uint8_t* cam_focal, uint8_t* group_focal,
                                         uint8_t* cam_prior, long* counts, void* ws, size_t ws_bytes, float* class_ms, long* class_launches,
                                         void* stream) {
  const Args a{{offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs},
               {huber_px, max_iters, pcg_iters, pcg_tol, ftol}, {T_out, xyz_out, obs_active, cam_free, point_active, counts},
               {refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal}, {cam_group, group_offsets, group_cams, G, group_focal}, {},
               {prior_xyz, prior_sigma, prior_mask, cam_prior}};
  return with_mode(mode, true, (int)LOFTR_ERR_BAD_ARG, [&](auto m) { return enter<decltype(m)>(a, ws, ws_bytes, class_ms, class_launches, stream); });
}
