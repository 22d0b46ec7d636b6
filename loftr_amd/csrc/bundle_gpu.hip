// Bundle adjustment on the GPU: the three host routines of bundle.hip with the same result bit for bit.
// Every phase of the host sequence is one kernel here, every per-item step is bundle_core.h's, compiled from the same text, fp64 without
// FMA contraction.  As on the host there is ONE schedule, run<Mode>, with one event / launch accounting, and the kernels that touch the
// camera block are templates on the mode (Pose, Focal, Shared); the group kernels and launches of Shared are `if constexpr` in it.  What
// this file adds is only how a phase is spread over threads:
//   a thread per track      setup, linearise, track half of S p, back substitution, evaluate (the sums of a track run sequentially in
//                           that one thread, as §16's refit);
//   a wave per camera       groups check, linearise, camera half of S p: lane l accumulates slots l, l + 64, ... of the camera's list
//                           and the 64 lanes are folded 32, 16, ..., 1 with shuffles -- osum64 exactly as the host's 64-entry array;
//   a wave per group        (Shared) the group check, the sum of U77, the group half: the members folded as a camera's observations;
//   a wave per 4096 terms   osum over tracks, cameras or groups, one launch per level; lane 0 of the last level hands the sum to ctrl_feed;
//   a thread per camera     factor, the two updates of the conjugate gradients, apply (Shared: the groups in the threads after them);
//   one thread              init, accept: the owner of lambda, the counters and the flags.
// The whole run is a FIXED launch schedule on the caller's stream: max_iters trials of pcg_iters iterations each.  A kernel whose phase
// the host routine would not run (the run has stopped, the conjugate gradients have stopped, the step is already rejected, an error bit
// is up) returns at once on a flag in device memory; a flag is only ever read by kernels launched after the one that wrote it.  No
// readback, no grid-wide barrier, no persistent kernel, no captured graph: a kernel boundary is the only device-wide ordering.
// Floating-point values cross lanes only as exact copies (shuffles); atomics are integer only.  Plain C++, ordinary vector stores.
// Position priors (§18.3) are a trait of the mode: PoseP, FocalP and SharedP run the same schedule; the decision is taken by the lane
// that ends ba_groups_kernel, the additions to U and gc by the lane that ends ba_cam_lin_kernel, a thread per camera evaluates the
// prior of a state (ba_prior_eval_kernel), the levels of the cameras' osum follow it (ba_prior_osum_kernel), and every kernel that the
// prior does not touch is the one of the mode without it.
// Radial (§18.4) runs §18.2's schedule launch for launch: a kernel of its own stands where a kernel without a mode stood (camera
// setup, the group check, evaluate, the track linearisation, the group sums), the templates get one more instantiation.
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
// ... of group g's list: member i adds v[stride i] when it has cam_focal
__device__ __forceinline__ double wave_group_sum(const CtxS& c, long g, int lane, const double* v, long stride) {
  double a;
  wave_osum64<1>(c.group_offsets[g], c.group_offsets[g + 1], lane, [&](long k, double* acc) { group_term(c, c.group_cams[k], v, stride, acc); }, &a);
  return a;
}

// what the factor and update kernels take: the base of the context (their steps need no more), with groups the groups' vectors too
// (Radial: its group steps of these two phases read nothing beyond CtxS)
template <class Mode> using StepCtx = std::conditional_t<Mode::kGroups, CtxS, Ctx>;

__global__ void ba_init_kernel(Ctx c, CtrlS* cs) { ctrl_init(c, cs); }
__global__ void ba_prior_init_kernel(Prior p) { ctrl_init_prior(p); }

// Radial.  grid ceil(n / 256) x 256: the setup of the other modes, then the camera's k; thread 0 owns the radial counter
__global__ void __launch_bounds__(kThreads) ba_cam_setup_radial_kernel(CtxR c) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) c.cr->n_radial = 0;
  if (i < c.n) {
    cam_setup(c, i);
    cam_setup_focal(c, i);
    cam_setup_radial(c, i);
  }
}

// grid ceil(n / 256) x 256
template <int S> __global__ void __launch_bounds__(kThreads) ba_cam_setup_kernel(std::conditional_t<S == 7, Ctx7, Ctx> c) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i < c.n) {
    cam_setup(c, i);
    if constexpr (S == 7) cam_setup_focal(c, i);
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

// Shared.  A wave per group, grid ceil(G / 4) x 256: the check of the group arrays and the count; a wave per group folds its members
// exactly as a wave per camera folds its observations.  Reads the arrays only through checked indices, and writes cam_focal only when
// the whole list of the group has passed, so it needs no flag.
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
// Radial.  The same kernel (its text is kept apart so that the device code of ba_cgroups_kernel stays what it was), and then the
// radial decision of the group and of its members from the same counts.
__global__ void __launch_bounds__(kThreads) ba_cgroups_radial_kernel(CtxR c) {
  const long g = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (g >= c.G) return;
  long b, e, total = 0, rtotal = 0;
  int err = 0;
  if (!cgroup_range(c, g, &b, &e)) { err = kBadCamGroups; b = e = 0; }
  for (long k = b + lane; k < e; k += 64) {
    long cnt;
    err |= cgroup_slot(c, g, b, k, &cnt);
    total += cnt;
    rtotal += cgroup_slot_radial(c, k, cnt);
  }
  for (int m = 32; m >= 1; m >>= 1) { err |= __shfl_xor(err, m, 64); total += __shfl_xor(total, m, 64); }
  for (int m = 32; m >= 1; m >>= 1) rtotal += __shfl_xor(rtotal, m, 64);
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
  {                                                                      // (cam_cnt is read, cam_focal is not: no lane waits for another)
    const bool rr = lane == 0 ? cgroup_rule_radial(c, g, refines, rtotal) : refines && rtotal >= (long)c.min_focal_obs;
    int nr = 0;
    for (long k = b + lane; k < e; k += 64) {
      const int i = c.group_cams[k];
      const bool ra = cam_radial_rule(c, i, rr);
      c.cam_radial[i] = (uint8_t)ra;
      nr += ra;
    }
    for (int m = 32; m >= 1; m >>= 1) nr += __shfl_xor(nr, m, 64);
    if (lane == 0) {
      c.group_radial[g] = (uint8_t)rr;
      if (nr) atomicAdd(&c.cr->n_radial, nr);
    }
  }
}

// grid ceil(T / 256) x 256; other = 0 evaluates the state, 1 the trial
__global__ void __launch_bounds__(kThreads) ba_evaluate_kernel(Ctx c, int other, int flags) {
  if (skipped(c, flags)) return;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t < c.T && !track_eval(c, c.ctrl->cur ^ other, t)) atomicOr(&c.ctrl->bad_e, 1);
}
// Radial: ... through the distorted projection
__global__ void __launch_bounds__(kThreads) ba_evaluate_radial_kernel(CtxR c, int other, int flags) {
  if (skipped(c, flags)) return;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t < c.T && !track_eval<Radial>(c, c.ctrl->cur ^ other, t)) atomicOr(&c.ctrl->bad_e, 1);
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

__global__ void __launch_bounds__(kThreads) ba_track_lin_kernel(Ctx c, int flags) {
  if (skipped(c, flags)) return;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t < c.T) track_lin(c, c.ctrl->cur, t);
}
__global__ void __launch_bounds__(kThreads) ba_track_lin_radial_kernel(CtxR c, int flags) {
  if (skipped(c, flags)) return;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t < c.T) track_lin<Radial>(c, c.ctrl->cur, t);
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

// Shared.  A wave per refining group, grid ceil(G / 4) x 256: d_g = the sum of U77 over its members
__global__ void __launch_bounds__(kThreads) ba_group_lin_kernel(CtxS c, int flags) {
  if (skipped(c, flags)) return;
  const long g = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (g >= c.G || !c.group_focal[g]) return;
  const double d = wave_group_sum(c, g, lane, c.U + 27, 28);
  if (lane == 0) c.dg[g] = d;
}
// Radial.  ... the three sums of its 2 x 2 block
__global__ void __launch_bounds__(kThreads) ba_group_lin_radial_kernel(CtxR c, int flags) {
  if (skipped(c, flags)) return;
  const long g = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (g >= c.G || !c.group_focal[g]) return;
  double d[3];
  wave_osum64<3>(c.group_offsets[g], c.group_offsets[g + 1], lane, [&](long k, double* acc) { group_term_block(c, c.group_cams[k], acc); }, d);
  if (lane == 0)
    for (int k = 0; k < 3; ++k) c.dg[3 * g + k] = d[k];
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
    if (id < c.T + c.n + c.G) {
      if constexpr (Mode::kRadial) ok = group_factor_radial(c, id - c.T - c.n, lambda);
      else ok = group_factor(c, id - c.T - c.n, lambda);
    }
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

// Shared.  A wave per group, grid ceil(G / 4) x 256: E^T of the cameras' seventh entries, then the group's own step
__global__ void __launch_bounds__(kThreads) ba_group_half_kernel(CtxS c, int mode, int flags) {
  if (skipped(c, flags)) return;
  const long g = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (g >= c.G) return;
  double s = 0.0;
  if (c.group_focal[g]) s = wave_group_sum(c, g, lane, c.Sp + 6, 7);
  if (lane == 0) group_half_finish(c, g, mode, c.ctrl->lambda, s);
}
// Radial.  ... of the seventh and eighth entries
__global__ void __launch_bounds__(kThreads) ba_group_half_radial_kernel(CtxR c, int mode, int flags) {
  if (skipped(c, flags)) return;
  const long g = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (g >= c.G) return;
  double s[2] = {0.0, 0.0};
  if (c.group_focal[g])
    wave_osum64<2>(c.group_offsets[g], c.group_offsets[g + 1], lane, [&](long k, double* acc) { group_term_pair(c, c.group_cams[k], acc); }, s);
  if (lane == 0) group_half_finish_radial(c, g, mode, c.ctrl->lambda, s);
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
    if constexpr (Mode::kRadial) {
      if (which == 1) group_update1_radial(c, id - c.n, c.ctrl->alpha);
      else group_update2_radial(c, id - c.n, c.ctrl->beta);
    } else {
      if (which == 1) group_update1(c, id - c.n, c.ctrl->alpha, c.ctrl->lambda);
      else group_update2(c, id - c.n, c.ctrl->beta);
    }
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
    if (id < c.T + c.n + c.G) {
      if constexpr (Mode::kRadial) group_apply_radial(c, cur, id - c.T - c.n);
      else group_apply(c, cur, id - c.T - c.n);
    }
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
// groups (track setup, evaluate, the track linearisation, accept, the osum) are one kernel for all modes, on the base of the context.
template <class Mode> int run(typename Mode::Ctx& c, int max_iters, int pcg_iters, double pcg_tol, void* ws, size_t ws_bytes, float* class_ms,
                              long* class_launches, void* stream) {
  constexpr bool kGroups = Mode::kGroups, kPrior = Mode::kPrior, kRadial = Mode::kRadial;
  using BaseMode = typename Mode::Base;                                 // the kernels of the phases that the prior does not touch
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
  Prior pr{};
  if constexpr (kPrior) pr = c.pr;
  double* red2 = c.red + ((std::max(T, n) + 1 + kChunk - 1) / kChunk);
  // osum of v[0 .. count) into `action` (ba_osum_kernel): one launch per level
  auto osum = [&](const double* v, long count, int action, double* wait, int flags) {
    const double* in = v;
    double* out = c.red;
    for (;;) {
      const long chunks = count > 0 ? (count + kChunk - 1) / kChunk : 1;
      hipLaunchKernelGGL(ba_osum_kernel, dim3((unsigned)chunks), dim3(64), 0, s, b, in, count, out, chunks == 1 ? action : -1, wait, flags);
      after(kClsOsum);
      if (chunks == 1) return;
      in = out;
      out = out == c.red ? red2 : c.red;
      count = chunks;
    }
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
    if constexpr (kRadial) { hipLaunchKernelGGL(ba_group_half_radial_kernel, blocks(G, 4), threads, 0, s, cb, mode, flags); after(kClsCamHalf); }
    else if constexpr (kGroups) { hipLaunchKernelGGL(ba_group_half_kernel, blocks(G, 4), threads, 0, s, cb, mode, flags); after(kClsCamHalf); }
  };
  // osum of the cameras' prior terms v[0 .. n) into `action` (ba_prior_osum_kernel): one launch per level
  auto prior_osum = [&](const double* v, int action, int flags) {
    const double* in = v;
    double* out = c.red;
    long count = n;
    for (;;) {
      const long chunks = count > 0 ? (count + kChunk - 1) / kChunk : 1;
      hipLaunchKernelGGL(ba_prior_osum_kernel, dim3((unsigned)chunks), dim3(64), 0, s, b, pr, in, count, out, chunks == 1 ? action : -1, flags);
      after(kClsOsum);
      if (chunks == 1) return;
      in = out;
      out = out == c.red ? red2 : c.red;
      count = chunks;
    }
  };
  // evaluate the state (other = 0) or the trial, then its cost and sum of |r|^2: the tracks' osum, with priors the cameras' added to it
  auto evaluate = [&](int other, int cost, int sq, int flags) {
    if constexpr (kRadial) hipLaunchKernelGGL(ba_evaluate_radial_kernel, blocks(T, kThreads), threads, 0, s, cb, other, flags);
    else hipLaunchKernelGGL(ba_evaluate_kernel, blocks(T, kThreads), threads, 0, s, b, other, flags);
    after(kClsEvaluate);
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
  if constexpr (kRadial) hipLaunchKernelGGL(ba_cam_setup_radial_kernel, blocks(n, kThreads), threads, 0, s, cb);
  else hipLaunchKernelGGL(ba_cam_setup_kernel<Mode::S>, blocks(n, kThreads), threads, 0, s, cb);
  after(kClsSetup);
  hipLaunchKernelGGL(ba_track_setup_kernel, blocks(T, kThreads), threads, 0, s, b); after(kClsSetup);
  hipLaunchKernelGGL(ba_groups_kernel<Mode>, blocks(n, 4), threads, 0, s, c); after(kClsSetup);
  if constexpr (kRadial) { hipLaunchKernelGGL(ba_cgroups_radial_kernel, blocks(G, 4), threads, 0, s, cb); after(kClsSetup); }
  else if constexpr (kGroups) { hipLaunchKernelGGL(ba_cgroups_kernel, blocks(G, 4), threads, 0, s, cb); after(kClsSetup); }
  evaluate(0, kActCost0, kActSq0, 0);
  for (int it = 0; it < max_iters && !failed; ++it) {
    if constexpr (kRadial) hipLaunchKernelGGL(ba_track_lin_radial_kernel, blocks(T, kThreads), threads, 0, s, cb, kNeedFresh);
    else hipLaunchKernelGGL(ba_track_lin_kernel, blocks(T, kThreads), threads, 0, s, b, kNeedFresh);
    after(kClsLinearise);
    hipLaunchKernelGGL(ba_cam_lin_kernel<Mode>, blocks(n, 4), threads, 0, s, c, kNeedFresh); after(kClsLinearise);
    if constexpr (kRadial) { hipLaunchKernelGGL(ba_group_lin_radial_kernel, blocks(G, 4), threads, 0, s, cb, kNeedFresh); after(kClsLinearise); }
    else if constexpr (kGroups) { hipLaunchKernelGGL(ba_group_lin_kernel, blocks(G, 4), threads, 0, s, cb, kNeedFresh); after(kClsLinearise); }
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

}  // namespace

extern "C" size_t loftr_bundle_adjust_workspace_bytes(long T, long N, int n_images) { return workspace_bytes<Pose>(T, N, n_images); }
extern "C" size_t loftr_bundle_adjust_focal_workspace_bytes(long T, long N, int n_images) { return workspace_bytes<Focal>(T, N, n_images); }
extern "C" size_t loftr_bundle_adjust_shared_workspace_bytes(long T, long N, int n_images) { return workspace_bytes<Shared>(T, N, n_images); }

extern "C" int loftr_bundle_adjust(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                                   const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed, int n_images,
                                   const long* cam_offsets, const int* cam_obs, double huber_px, int max_iters, int pcg_iters, double pcg_tol,
                                   double ftol, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active,
                                   long* counts, void* ws, size_t ws_bytes, float* class_ms, long* class_launches, void* stream) {
  Ctx c{};
  fill(c, offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs, huber_px, pcg_tol, ftol,
       T_out, xyz_out, obs_active, cam_free, point_active, counts);
  return run<Pose>(c, max_iters, pcg_iters, pcg_tol, ws, ws_bytes, class_ms, class_launches, stream);
}

extern "C" int loftr_bundle_adjust_focal(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                         long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                         const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                         double huber_px, int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs,
                                         double focal_lo, double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active,
                                         uint8_t* cam_free, uint8_t* point_active, double* K_out, uint8_t* cam_focal, long* counts, void* ws,
                                         size_t ws_bytes, float* class_ms, long* class_launches, void* stream) {
  Ctx7 c{};
  fill(c, offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs, huber_px, pcg_tol, ftol,
       T_out, xyz_out, obs_active, cam_free, point_active, counts);
  fill_focal(c, refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal);
  return run<Focal>(c, max_iters, pcg_iters, pcg_tol, ws, ws_bytes, class_ms, class_launches, stream);
}

extern "C" int loftr_bundle_adjust_shared(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                          long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                          const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                          const int* cam_group, const long* group_offsets, const int* group_cams, int G, double huber_px,
                                          int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs, double focal_lo,
                                          double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free,
                                          uint8_t* point_active, double* K_out, uint8_t* cam_focal, uint8_t* group_focal, long* counts,
                                          void* ws, size_t ws_bytes, float* class_ms, long* class_launches, void* stream) {
  CtxS c{};
  fill(c, offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs, huber_px, pcg_tol, ftol,
       T_out, xyz_out, obs_active, cam_free, point_active, counts);
  fill_focal(c, refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal);
  fill_groups(c, cam_group, group_offsets, group_cams, G, group_focal);
  return run<Shared>(c, max_iters, pcg_iters, pcg_tol, ws, ws_bytes, class_ms, class_launches, stream);
}

extern "C" size_t loftr_bundle_adjust_radial_workspace_bytes(long T, long N, int n_images) { return workspace_bytes<Radial>(T, N, n_images); }

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
  CtxR c{};
  fill(c, offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs, huber_px, pcg_tol, ftol,
       T_out, xyz_out, obs_active, cam_free, point_active, counts);
  fill_focal(c, refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal);
  fill_groups(c, cam_group, group_offsets, group_cams, G, group_focal);
  fill_radial(c, radial_in, refine_radial, radial_lo, radial_hi, radial_out, cam_radial, group_radial);
  return run<Radial>(c, max_iters, pcg_iters, pcg_tol, ws, ws_bytes, class_ms, class_launches, stream);
}

// with position priors on the camera centres (§18.3): mode 0 pose, 1 focal, 2 shared
namespace {
template <class F> auto with_prior_mode(int mode, F go) -> decltype(go(PoseP{})) {
  switch (mode) {
    case 0: return go(PoseP{});
    case 1: return go(FocalP{});
    case 2: return go(SharedP{});
  }
  return decltype(go(PoseP{}))(0);
}
}  // namespace

extern "C" size_t loftr_bundle_adjust_prior_workspace_bytes(long T, long N, int n_images, int mode) {
  return with_prior_mode(mode, [&](auto m) { return workspace_bytes<decltype(m)>(T, N, n_images); });
}

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
  if (mode < 0 || mode > 2) return LOFTR_ERR_BAD_ARG;
  return with_prior_mode(mode, [&](auto m) {
    using Mode = decltype(m);
    typename Mode::Ctx c{};
    fill(c, offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs, huber_px, pcg_tol,
         ftol, T_out, xyz_out, obs_active, cam_free, point_active, counts);
    if constexpr (Mode::S == 7) fill_focal(c, refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal);
    if constexpr (Mode::kGroups) fill_groups(c, cam_group, group_offsets, group_cams, G, group_focal);
    fill_prior(c.pr, prior_xyz, prior_sigma, prior_mask, cam_prior);
    return run<Mode>(c, max_iters, pcg_iters, pcg_tol, ws, ws_bytes, class_ms, class_launches, stream);
  });
}
