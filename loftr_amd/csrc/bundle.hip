// Bundle adjustment of the triangulated model (host code, double precision): Levenberg-Marquardt over camera poses (6 DoF; intrinsics
// fixed, or with §18.1 one relative focal step per camera) and points on the pixel reprojection error, optional Huber loss, the
// point-eliminated Schur system solved by preconditioned conjugate gradients without forming it (the contract is in
// include/loftr_hip.h).  What Ceres / COLMAP's bundle adjuster is used for after triangulation; neither is in this image, so this is a
// statement of the published method (Triggs et al., "Bundle Adjustment -- A Modern Synthesis"; Agarwal et al., "Bundle Adjustment in
// the Large"), NOT of their source.  PARITY UNPINNED against them.
// These functions DEFINE the result: the kernels of bundle_gpu.hip reproduce it bit for bit, which is why all the arithmetic, every
// per-item step, the context fill and the argument checks live in bundle_core.h and why this file is only the sequence of phases and
// the order-defined sums.  The sequence is ONE template, run<Mode>, and a mode is a row of traits (bundle_core.h): Pose
// (§18), Focal (§18.1: one focal step per camera), Shared (§18.2: one per group of cameras), Radial (§18.4: the grouped mode with an
// 8-wide camera block and two unknowns per group, the second an additive step of one radial coefficient), and PoseP, FocalP, SharedP
// (§18.3: position priors on the camera centres).  The sequence asks the traits only WHETHER a phase has a group part (kGroups) or a
// prior part (kPrior); what that part is in a mode is the core's `<Mode>` step.  An entry point builds the arguments' superset (Args)
// and enters its mode; loftr_bundle_adjust_prior_host picks one by `mode` through the one list of modes (with_mode).
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
// a group's osum64 of M values per member: element l is the l-th member
template <int M, class F> void group_sum(const CtxS& c, long g, F term, double* out) {
  const long b = c.group_offsets[g];
  osum64<M>(c.group_offsets[g + 1] - b, [&](long e, double* a) { term(c.group_cams[b + e], a); }, out);
}

// the sequence of phases of every mode; c holds the problem and the result.  The group phases exist for the modes with kGroups only;
// what a group step is in a mode is the core's business.
template <class Mode> int run(typename Mode::Ctx& c, int max_iters, int pcg_iters, double pcg_tol) {
  constexpr int S = Mode::S, kU = kTri<S>, GW = Mode::GW, kD = kTri<GW>;
  constexpr bool kGroups = Mode::kGroups;
  using TMode = TrackMode<Mode>;
  const int st = check_args<Mode>(c, max_iters, pcg_iters, pcg_tol, true);
  if (st != LOFTR_OK) return st;
  const long T = c.T, n = c.n;
  std::vector<char> ws(layout<Mode>(c, nullptr), 0);
  layout<Mode>(c, ws.data());
  Ctrl& s = *c.ctrl;
  ctrl_init(c, groups_ctrl<Mode>(c));
  if constexpr (Mode::kPrior) ctrl_init_prior(c.pr);
  cam_setup_ctrl<Mode>(c);
  for (long i = 0; i < n; ++i) cam_setup<Mode>(c, i);
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
    for (long g = 0; g < c.G; ++g) cgroup_decide<Mode>(c, g, OneLane{});
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
      if constexpr (kGroups)
        for (long g = 0; g < c.G; ++g)
          if (c.group_focal[g]) group_sum<kD>(c, g, [&](long i, double* a) { group_lin_term<Mode>(c, i, a); }, c.dg + kD * g);
    }
    const double lambda = s.lambda;
    for (long t = 0; t < T; ++t) if (!track_factor(c, t, lambda)) s.bad_f = 1;
    for (long i = 0; i < n; ++i) if (!cam_factor<Mode>(c, i, lambda)) s.bad_f = 1;
    if constexpr (kGroups)
      for (long g = 0; g < c.G; ++g) if (!group_factor<Mode>(c, g, lambda)) s.bad_f = 1;
    auto camera_half = [&](int mode) {
      for (long i = 0; i < n; ++i) {
        double a[S];
        for (int k = 0; k < S; ++k) a[k] = 0.0;
        if (takes_part<Mode>(c, i)) cam_sum<S>(c, i, [&](long o, double* acc) { cam_half_term<Mode>(c, cur, o, acc); }, a);
        cam_half_finish<Mode>(c, i, mode, lambda, a);
      }
      if constexpr (kGroups)
        for (long g = 0; g < c.G; ++g) {
          double sg[GW];
          for (int k = 0; k < GW; ++k) sg[k] = 0.0;
          if (c.group_focal[g]) group_sum<GW>(c, g, [&](long i, double* a) { group_half_term<Mode>(c, i, a); }, sg);
          group_half_finish<Mode>(c, g, mode, lambda, sg);
        }
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
        if constexpr (kGroups)
          for (long g = 0; g < c.G; ++g) group_update1<Mode>(c, g, s.alpha, lambda);
        ctrl_feed(c, kActRz, dot());
        if (s.pcg_done) break;
        for (long i = 0; i < n; ++i) cam_update2<Mode>(c, i, s.beta);
        if constexpr (kGroups)
          for (long g = 0; g < c.G; ++g) group_update2<Mode>(c, g, s.beta);
      }
      for (long i = 0; i < n; ++i) if (!cam_apply<Mode>(c, cur, i)) s.bad_a = 1;
      if constexpr (kGroups)
        for (long g = 0; g < c.G; ++g) group_apply<Mode>(c, cur, g);
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

template <class Mode> int enter(const Args& a) {
  typename Mode::Ctx c{};
  fill<Mode>(c, a);
  return run<Mode>(c, a.par.max_iters, a.par.pcg_iters, a.par.pcg_tol);
}

}  // namespace

extern "C" int loftr_bundle_adjust_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                                        const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed, int n_images,
                                        const long* cam_offsets, const int* cam_obs, double huber_px, int max_iters, int pcg_iters,
                                        double pcg_tol, double ftol, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free,
                                        uint8_t* point_active, long* counts) {
  return enter<Pose>({{offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs},
                      {huber_px, max_iters, pcg_iters, pcg_tol, ftol}, {T_out, xyz_out, obs_active, cam_free, point_active, counts}});
}

extern "C" int loftr_bundle_adjust_focal_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                              long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                              const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                              double huber_px, int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs,
                                              double focal_lo, double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active,
                                              uint8_t* cam_free, uint8_t* point_active, double* K_out, uint8_t* cam_focal, long* counts) {
  return enter<Focal>({{offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs},
                       {huber_px, max_iters, pcg_iters, pcg_tol, ftol}, {T_out, xyz_out, obs_active, cam_free, point_active, counts},
                       {refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal}});
}

extern "C" int loftr_bundle_adjust_shared_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                               long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                               const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                               const int* cam_group, const long* group_offsets, const int* group_cams, int G, double huber_px,
                                               int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs, double focal_lo,
                                               double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free,
                                               uint8_t* point_active, double* K_out, uint8_t* cam_focal, uint8_t* group_focal, long* counts) {
  return enter<Shared>({{offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs},
                        {huber_px, max_iters, pcg_iters, pcg_tol, ftol}, {T_out, xyz_out, obs_active, cam_free, point_active, counts},
                        {refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal},
                        {cam_group, group_offsets, group_cams, G, group_focal}});
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
  return enter<Radial>({{offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs},
                        {huber_px, max_iters, pcg_iters, pcg_tol, ftol}, {T_out, xyz_out, obs_active, cam_free, point_active, counts},
                        {refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal},
                        {cam_group, group_offsets, group_cams, G, group_focal},
                        {radial_in, refine_radial, radial_lo, radial_hi, radial_out, cam_radial, group_radial}});
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
  const Args a{{offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs},
               {huber_px, max_iters, pcg_iters, pcg_tol, ftol}, {T_out, xyz_out, obs_active, cam_free, point_active, counts},
               {refine_focal, min_focal_obs, focal_lo, focal_hi, K_out, cam_focal},
               {cam_group, group_offsets, group_cams, G, group_focal}, {}, {prior_xyz, prior_sigma, prior_mask, cam_prior}};
  return with_mode(mode, true, (int)LOFTR_ERR_BAD_ARG, [&](auto m) { return enter<decltype(m)>(a); });
}
