// Bundle adjustment of the triangulated model (host code, double precision): Levenberg-Marquardt over camera poses (6 DoF; intrinsics
// fixed, or with §18.1 one relative focal step per camera) and points on the pixel reprojection error, optional Huber loss, the
// point-eliminated Schur system solved by preconditioned conjugate gradients without forming it (the contract is in
// include/loftr_hip.h).  What Ceres / COLMAP's bundle adjuster is used for after triangulation; neither is in this image, so this is a
// statement of the published method (Triggs et al., "Bundle Adjustment -- A Modern Synthesis"; Agarwal et al., "Bundle Adjustment in
// the Large"), NOT of their source.  PARITY UNPINNED against them.
// These functions DEFINE the result: loftr_bundle_adjust / _focal / _shared (bundle_gpu.hip) reproduce it bit for bit, which is why all
// the arithmetic, every per-item step, the context fill and the argument checks live in bundle_core.h and why this file is only the
// sequence of phases and the order-defined sums.  The sequence is ONE template, run<Mode>, and the three entry points are its three
// instantiations: Pose (§18), Focal (§18.1: one focal step per camera), Shared (§18.2: one per group of cameras, whose group phases
// are `if constexpr` in the sequence).  Position priors on the camera centres (§18.3) are a trait of the mode as well: PoseP, FocalP and
// SharedP run the same sequence with the prior's steps, loftr_bundle_adjust_prior_host picks one by `mode`.  Radial (§18.4) is the
// grouped mode with an 8-wide camera block and two unknowns per group, the second an additive step of one radial coefficient; its
// steps stand behind `if constexpr (kRadial)` in the same sequence, and it alone reads the distorted projection.
#include <stdint.h>
#include <vector>
#include "../../include/loftr_hip.h"
#include "bundle_core.h"

#pragma clang fp contract(off)

using namespace ba;

namespace {

// osum64 of `count` elements of M values each: term(e, a) adds element e into the M accumulators a
template <int M, class F> void osum64(long count, F term, double* out) {
  double a[64][M];
  for (int l = 0; l < 64; ++l) for (int m = 0; m < M; ++m) a[l][m] = 0.0;
  for (long e = 0; e < count; ++e) term(e, a[e % 64]);
  for (int s = 32; s >= 1; s >>= 1)
    for (int l = 0; l < s; ++l) for (int m = 0; m < M; ++m) a[l][m] = a[l][m] + a[l + s][m];
  for (int m = 0; m < M; ++m) out[m] = a[0][m];
}
// osum of v[0 .. count): osum64 per chunk of 4096, then osum of the chunk sums
double osum(const double* v, long count) {
  std::vector<double> cur(v, v + count), next;
  for (;;) {
    const long chunks = (long)((cur.size() + kChunk - 1) / kChunk);
    next.assign((size_t)(chunks > 0 ? chunks : 1), 0.0);
    for (long b = 0; b < (chunks > 0 ? chunks : 1); ++b) {
      const long lo = b * kChunk, len = (long)cur.size() - lo < kChunk ? (long)cur.size() - lo : kChunk;
      const double* src = cur.data() + lo;
      osum64<1>(len > 0 ? len : 0, [&](long e, double* a) { a[0] = a[0] + src[e]; }, &next[(size_t)b]);
    }
    if (chunks <= 1) return next[0];
    cur.swap(next);
  }
}

// a camera's osum64: element l is slot l of its list; an inactive slot adds nothing
template <int W, class F> void cam_sum(const Ctx& c, long i, F term, double* out) {
  const long b = c.cam_offsets[i];
  osum64<W>(c.cam_offsets[i + 1] - b, [&](long e, double* a) { const long o = c.cam_obs[b + e]; if (c.obs_active[o]) term(o, a); }, out);
}
// a group's osum64: element l is the l-th member
double group_sum(const CtxS& c, long g, const double* v, long stride) {
  const long b = c.group_offsets[g];
  double out;
  osum64<1>(c.group_offsets[g + 1] - b, [&](long e, double* a) { group_term(c, c.group_cams[b + e], v, stride, a); }, &out);
  return out;
}

// Radial: a group's osum64 of M values per member
template <int M, class F> void group_sum_radial(const CtxR& c, long g, F term, double* out) {
  const long b = c.group_offsets[g];
  osum64<M>(c.group_offsets[g + 1] - b, [&](long e, double* a) { term(c.group_cams[b + e], a); }, out);
}

// the sequence of phases of every mode; c holds the problem and the result.  The group phases exist for Shared and Radial only.
template <class Mode> int run(typename Mode::Ctx& c, int max_iters, int pcg_iters, double pcg_tol) {
  constexpr int S = Mode::S, kU = kTri<S>;
  constexpr bool kGroups = Mode::kGroups, kRadial = Mode::kRadial;
  using TMode = TrackMode<Mode>;
  const int st = check_args<Mode>(c, max_iters, pcg_iters, pcg_tol, true);
  if (st != LOFTR_OK) return st;
  const long T = c.T, n = c.n;
  std::vector<char> ws(layout<Mode>(c, nullptr), 0);
  layout<Mode>(c, ws.data());
  Ctrl& s = *c.ctrl;
  ctrl_init(c, groups_ctrl<Mode>(c));
  if constexpr (Mode::kPrior) ctrl_init_prior(c.pr);
  if constexpr (kRadial) c.cr->n_radial = 0;
  for (long i = 0; i < n; ++i) {
    cam_setup(c, i);
    if constexpr (S >= 7) cam_setup_focal(c, i);
    if constexpr (kRadial) cam_setup_radial(c, i);
  }
  for (long t = 0; t < T; ++t) {
    long cnt;
    s.err |= track_setup(c, t, &cnt);
    s.n_active_obs += (unsigned long long)cnt;
    s.n_active_pts += cnt > 0;
  }
  if (s.err) return LOFTR_ERR_BAD_ARG;
  for (long i = 0; i < n; ++i) {
    if constexpr (S >= 7) c.cam_focal[i] = 0;
    long b, e, cnt = 0;
    if (!group_range(c, i, &b, &e)) { s.err |= kBadGroups; continue; }
    for (long k = b; k < e; ++k) {
      bool active;
      s.err |= group_check(c, i, b, k, &active);
      cnt += active;
    }
    c.cam_free[i] = (uint8_t)(!c.fixed[i] && c.cam_valid[i] && cnt >= 1);
    s.n_free += c.cam_free[i];
    if constexpr (Mode::kPrior) {
      c.pr.cam_prior[i] = (uint8_t)cam_prior_rule(c, c.pr, i);
      c.pr.cp->n_prior += c.pr.cam_prior[i];
    }
    if constexpr (kGroups) s.err |= cam_carry(c, i, cnt);
    else if constexpr (S == 7) {
      c.cam_focal[i] = (uint8_t)cam_focal_rule(c, i, c.cam_free[i] != 0, cnt);
      s.n_focal += c.cam_focal[i];
    }
  }
  if (s.err) return LOFTR_ERR_BAD_ARG;
  if constexpr (kGroups) {
    for (long g = 0; g < c.G; ++g) {
      long b, e, total = 0, rtotal = 0;
      int err = 0;
      if (!cgroup_range(c, g, &b, &e)) { s.err |= kBadCamGroups; continue; }
      for (long k = b; k < e; ++k) {
        long cnt;
        err |= cgroup_slot(c, g, b, k, &cnt);
        total += cnt;
        if constexpr (kRadial) rtotal += cgroup_slot_radial(c, k, cnt);
      }
      s.err |= err;
      if (err) continue;
      const bool refines = cgroup_rule(c, g, total);
      c.group_focal[g] = (uint8_t)refines;
      c.cs->n_groups += refines;
      for (long k = b; k < e; ++k) {
        const int i = c.group_cams[k];
        c.cam_focal[i] = (uint8_t)(refines && c.cam_cnt[i] > 0);
        s.n_focal += c.cam_focal[i];
      }
      if constexpr (kRadial) {
        const bool rr = cgroup_rule_radial(c, g, refines, rtotal);
        c.group_radial[g] = (uint8_t)rr;
        for (long k = b; k < e; ++k) {
          const int i = c.group_cams[k];
          c.cam_radial[i] = (uint8_t)cam_radial_rule(c, i, rr);
          c.cr->n_radial += c.cam_radial[i];
        }
      }
    }
    if (s.err) return LOFTR_ERR_BAD_ARG;
  }

  // a dot product over the unknowns: the cameras' osum, and with groups the groups' osum added to it
  auto dot = [&]() {
    const double cams = osum(c.part, n);
    if constexpr (kGroups) return cams + osum(c.partg, c.G);
    else return cams;
  };
  auto evaluate = [&](int buf) {
    bool ok = true;
    for (long t = 0; t < T; ++t) ok = track_eval<TMode>(c, buf, t) && ok;
    if constexpr (Mode::kPrior)
      for (long i = 0; i < n; ++i) cam_prior_eval(c, c.pr, buf, i);
    return ok;
  };
  // the cost and the sum of |r|^2 of what `evaluate` left: the tracks' osum, with priors the cameras' osum added to it (and the
  // cameras' |c - g|^2 for the report)
  auto feed_cost = [&](int cost, int sq) {
    if constexpr (Mode::kPrior) {
      c.pr.cp->acc = osum(c.part, T);
      ctrl_feed_prior(c, c.pr, cost, osum(c.pr.part, n));
      ctrl_feed(c, sq, osum(c.part2, T));
      ctrl_feed_prior(c, c.pr, sq, osum(c.pr.part2, n));
    } else {
      ctrl_feed(c, cost, osum(c.part, T));
      ctrl_feed(c, sq, osum(c.part2, T));
    }
  };
  evaluate(0);
  feed_cost(kActCost0, kActSq0);

  for (int it = 0; it < max_iters && !s.done; ++it) {
    const int cur = s.cur;
    if (s.fresh) {
      for (long t = 0; t < T; ++t) track_lin<TMode>(c, cur, t);
      for (long i = 0; i < n; ++i) {
        if (!takes_part<Mode>(c, i)) continue;
        double a[kU + S];
        cam_sum<kU + S>(c, i, [&](long o, double* acc) { cam_lin_term<Mode>(c, cur, o, acc); }, a);
        for (int k = 0; k < kU; ++k) c.U[kU * i + k] = a[k];
        for (int k = 0; k < S; ++k) c.gc[S * i + k] = a[kU + k];
        if constexpr (Mode::kPrior) cam_lin_prior<S>(c, c.pr, cur, i);
      }
      if constexpr (kRadial) {
        for (long g = 0; g < c.G; ++g)
          if (c.group_focal[g]) group_sum_radial<3>(c, g, [&](long i, double* a) { group_term_block(c, i, a); }, c.dg + 3 * g);
      } else if constexpr (kGroups)
        for (long g = 0; g < c.G; ++g) if (c.group_focal[g]) c.dg[g] = group_sum(c, g, c.U + 27, 28);
    }
    const double lambda = s.lambda;
    for (long t = 0; t < T; ++t) if (!track_factor(c, t, lambda)) s.bad_f = 1;
    for (long i = 0; i < n; ++i) if (!cam_factor<Mode>(c, i, lambda)) s.bad_f = 1;
    if constexpr (kRadial) {
      for (long g = 0; g < c.G; ++g) if (!group_factor_radial(c, g, lambda)) s.bad_f = 1;
    } else if constexpr (kGroups)
      for (long g = 0; g < c.G; ++g) if (!group_factor(c, g, lambda)) s.bad_f = 1;
    auto camera_half = [&](int mode) {
      for (long i = 0; i < n; ++i) {
        double a[S];
        for (int k = 0; k < S; ++k) a[k] = 0.0;
        if (takes_part<Mode>(c, i)) cam_sum<S>(c, i, [&](long o, double* acc) { cam_half_term<Mode>(c, cur, o, acc); }, a);
        cam_half_finish<Mode>(c, i, mode, lambda, a);
      }
      if constexpr (kRadial) {
        for (long g = 0; g < c.G; ++g) {
          double sg[2] = {0.0, 0.0};
          if (c.group_focal[g]) group_sum_radial<2>(c, g, [&](long i, double* a) { group_term_pair(c, i, a); }, sg);
          group_half_finish_radial(c, g, mode, lambda, sg);
        }
      } else if constexpr (kGroups)
        for (long g = 0; g < c.G; ++g) group_half_finish(c, g, mode, lambda, c.group_focal[g] ? group_sum(c, g, c.Sp + 6, 7) : 0.0);
    };
    if (!s.bad_f) {
      for (long t = 0; t < T; ++t) track_half<Mode>(c, cur, t, 0);
      camera_half(0);
      ctrl_feed(c, kActRz0, dot());
      for (int pi = 0; pi < pcg_iters && !s.pcg_done; ++pi) {
        for (long t = 0; t < T; ++t) track_half<Mode>(c, cur, t, 1);
        camera_half(1);
        ctrl_feed(c, kActPsp, dot());
        if (s.pcg_done) break;
        for (long i = 0; i < n; ++i) cam_update1<Mode>(c, i, s.alpha);
        if constexpr (kRadial) {
          for (long g = 0; g < c.G; ++g) group_update1_radial(c, g, s.alpha);
        } else if constexpr (kGroups)
          for (long g = 0; g < c.G; ++g) group_update1(c, g, s.alpha, lambda);
        ctrl_feed(c, kActRz, dot());
        if (s.pcg_done) break;
        for (long i = 0; i < n; ++i) cam_update2<Mode>(c, i, s.beta);
        if constexpr (kRadial) {
          for (long g = 0; g < c.G; ++g) group_update2_radial(c, g, s.beta);
        } else if constexpr (kGroups)
          for (long g = 0; g < c.G; ++g) group_update2(c, g, s.beta);
      }
      for (long i = 0; i < n; ++i) if (!cam_apply<Mode>(c, cur, i)) s.bad_a = 1;
      if constexpr (kRadial) {
        for (long g = 0; g < c.G; ++g) group_apply_radial(c, cur, g);
      } else if constexpr (kGroups)
        for (long g = 0; g < c.G; ++g) group_apply(c, cur, g);
      for (long t = 0; t < T; ++t) if (!track_half<Mode>(c, cur, t, 2)) s.bad_a = 1;
    }
    if (!s.bad_f && !s.bad_a) {
      if (!evaluate(1 - cur)) s.bad_e = 1;
      if (!s.bad_e) feed_cost(kActCostT, kActSqT);
    }
    if constexpr (Mode::kPrior) ctrl_accept_prior(c, c.pr);
    else ctrl_accept(c);
  }
  for (long i = 0; i < n; ++i) cam_write<Mode>(c, s.cur, i);
  for (long t = 0; t < T; ++t) track_write(c, s.cur, t);
  ctrl_write<Mode>(c);
  if constexpr (Mode::kPrior) ctrl_write_prior(c, c.pr);
  return LOFTR_OK;
}

}  // namespace

extern "C" int loftr_bundle_adjust_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                                        const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed, int n_images,
                                        const long* cam_offsets, const int* cam_obs, double huber_px, int max_iters, int pcg_iters,
                                        double pcg_tol, double ftol, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free,
                                        uint8_t* point_active, long* counts) {
  Ctx c{};
  fill(c, offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs, huber_px, pcg_tol, ftol,
       T_out, xyz_out, obs_active, cam_free, point_active, counts);
  return run<Pose>(c, max_iters, pcg_iters, pcg_tol);
}

extern "C" int loftr_bundle_adjust_focal_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                              long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                              const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                              double huber_px, int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs,
                                              double focal_lo, double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active,
                                              uint8_t* cam_free, uint8_t* point_active, double* K_out, uint8_t* cam_focal, long* counts) {
  Ctx7 c{};
  fill(c, offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs, huber_px, pcg_tol, ftol,
       T_out, xyz_out, obs_active, cam_free, point_active, counts);
  fill_focal(c, refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal);
  return run<Focal>(c, max_iters, pcg_iters, pcg_tol);
}

extern "C" int loftr_bundle_adjust_shared_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                               long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                               const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                               const int* cam_group, const long* group_offsets, const int* group_cams, int G, double huber_px,
                                               int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs, double focal_lo,
                                               double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free,
                                               uint8_t* point_active, double* K_out, uint8_t* cam_focal, uint8_t* group_focal, long* counts) {
  CtxS c{};
  fill(c, offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs, huber_px, pcg_tol, ftol,
       T_out, xyz_out, obs_active, cam_free, point_active, counts);
  fill_focal(c, refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal);
  fill_groups(c, cam_group, group_offsets, group_cams, G, group_focal);
  return run<Shared>(c, max_iters, pcg_iters, pcg_tol);
}

// one focal step and one radial coefficient per group of cameras (§18.4)
extern "C" int loftr_bundle_adjust_radial_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                               long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                               const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                               const int* cam_group, const long* group_offsets, const int* group_cams, int G,
                                               const double* radial_in, const uint8_t* refine_radial, double huber_px, int max_iters,
                                               int pcg_iters, double pcg_tol, double ftol, int min_focal_obs, double focal_lo, double focal_hi,
                                               double radial_lo, double radial_hi, double* T_out, float* xyz_out, uint8_t* obs_active,
                                               uint8_t* cam_free, uint8_t* point_active, double* K_out, uint8_t* cam_focal, uint8_t* group_focal,
                                               double* radial_out, uint8_t* cam_radial, uint8_t* group_radial, long* counts) {
  CtxR c{};
  fill(c, offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs, huber_px, pcg_tol, ftol,
       T_out, xyz_out, obs_active, cam_free, point_active, counts);
  fill_focal(c, refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal);
  fill_groups(c, cam_group, group_offsets, group_cams, G, group_focal);
  fill_radial(c, radial_in, refine_radial, radial_lo, radial_hi, radial_out, cam_radial, group_radial);
  return run<Radial>(c, max_iters, pcg_iters, pcg_tol);
}

// with position priors on the camera centres (§18.3): mode 0 pose, 1 focal, 2 shared; the focal and group arguments are ignored below
// their mode
extern "C" int loftr_bundle_adjust_prior_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                              long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                              const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                              const int* cam_group, const long* group_offsets, const int* group_cams, int G,
                                              const double* prior_xyz, const double* prior_sigma, const uint8_t* prior_mask, int mode,
                                              double huber_px, int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs,
                                              double focal_lo, double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active,
                                              uint8_t* cam_free, uint8_t* point_active, double* K_out, uint8_t* cam_focal, uint8_t* group_focal,
                                              uint8_t* cam_prior, long* counts) {
  auto go = [&](auto m) {
    using Mode = decltype(m);
    typename Mode::Ctx c{};
    fill(c, offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs, huber_px, pcg_tol,
         ftol, T_out, xyz_out, obs_active, cam_free, point_active, counts);
    if constexpr (Mode::S == 7) fill_focal(c, refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal);
    if constexpr (Mode::kGroups) fill_groups(c, cam_group, group_offsets, group_cams, G, group_focal);
    fill_prior(c.pr, prior_xyz, prior_sigma, prior_mask, cam_prior);
    return run<Mode>(c, max_iters, pcg_iters, pcg_tol);
  };
  switch (mode) {
    case 0: return go(PoseP{});
    case 1: return go(FocalP{});
    case 2: return go(SharedP{});
  }
  return LOFTR_ERR_BAD_ARG;
}
