// Bundle adjustment of the triangulated model (host code, double precision): Levenberg-Marquardt over camera poses (6 DoF; intrinsics
// fixed, or with §18.1 one relative focal step per camera) and points on the pixel reprojection error, optional Huber loss, the
// point-eliminated Schur system solved by preconditioned conjugate gradients without forming it (the contract is in
// include/loftr_hip.h).  What Ceres / COLMAP's bundle adjuster is used for after triangulation; neither is in this image, so this is a
// statement of the published method (Triggs et al., "Bundle Adjustment -- A Modern Synthesis"; Agarwal et al., "Bundle Adjustment in
// the Large"), NOT of their source.  PARITY UNPINNED against them.
// These functions DEFINE the result: loftr_bundle_adjust / loftr_bundle_adjust_focal (bundle_gpu.hip) reproduce it bit for bit, which is
// why all the arithmetic and every per-item step live in bundle_core.h and why this file is only the sequence of phases and the
// order-defined sums.  The sequence is one template on the width M of the camera block: 6 (poses) or 7 (poses and focal); run_shared is
// §18.2's, with one focal step per group of cameras (loftr_bundle_adjust_shared_host).
#include <stdint.h>
#include <type_traits>
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

// the argument checks of both entry points -> LOFTR_OK when the run may start (counts are zero then)
int check_args(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N, const float* xyz,
               const double* K, const double* T_cam_from_world, const uint8_t* fixed, int n_images, const long* cam_offsets,
               const int* cam_obs, double huber_px, int max_iters, int pcg_iters, double pcg_tol, double ftol, double* T_out, float* xyz_out,
               uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active, long* counts) {
  if (!offsets || !cam_offsets || !counts || T < 0 || N < 0 || n_images < 0) return LOFTR_ERR_BAD_ARG;
  if (T > 0 && (!xyz || !xyz_out || !point_active)) return LOFTR_ERR_BAD_ARG;
  if (N > 0 && (!obs_image || !obs_xy || !obs_mask || !obs_active || !cam_obs)) return LOFTR_ERR_BAD_ARG;
  if (n_images > 0 && (!K || !T_cam_from_world || !fixed || !T_out || !cam_free)) return LOFTR_ERR_BAD_ARG;
  if (!(huber_px >= 0.0 && fin(huber_px) && ftol >= 0.0 && fin(ftol) && pcg_tol >= 0.0 && pcg_tol < 1.0)) return LOFTR_ERR_BAD_ARG;
  if (max_iters < 0 || max_iters > LOFTR_BUNDLE_MAX_ITERS || pcg_iters < 1 || pcg_iters > LOFTR_BUNDLE_MAX_PCG) return LOFTR_ERR_BAD_ARG;
  if (T >= (1L << 31) || N >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  for (int i = 0; i < kCounts; ++i) counts[i] = 0;
  if (T == 0 && N > 0) return LOFTR_ERR_BAD_ARG;
  if (n_images == 0 && N > 0) return LOFTR_ERR_BAD_ARG;
  return LOFTR_OK;
}

// the sequence of phases; c holds the problem and the result
template <int M> int run(CtxT<M>& c, int max_iters, int pcg_iters) {
  constexpr int kU = kTri<M>;
  const long T = c.T, n = c.n;
  const long* cam_offsets = c.cam_offsets;
  const int* cam_obs = c.cam_obs;
  const uint8_t *fixed = c.fixed, *obs_active = c.obs_active;
  uint8_t* cam_free = c.cam_free;
  std::vector<char> ws(layout<M>(c, nullptr), 0);
  layout<M>(c, ws.data());
  Ctrl& s = *c.ctrl;
  ctrl_init(c);
  for (long i = 0; i < n; ++i) {
    cam_setup(c, i);
    if constexpr (M == 7) cam_setup_focal(c, i);
  }
  for (long t = 0; t < T; ++t) {
    long cnt;
    s.err |= track_setup(c, t, &cnt);
    s.n_active_obs += (unsigned long long)cnt;
    s.n_active_pts += cnt > 0;
  }
  if (s.err) return LOFTR_ERR_BAD_ARG;
  for (long i = 0; i < n; ++i) {
    if constexpr (M == 7) c.cam_focal[i] = 0;
    long b, e, cnt = 0;
    if (!group_range(c, i, &b, &e)) { s.err |= kBadGroups; continue; }
    for (long k = b; k < e; ++k) {
      bool active;
      s.err |= group_check(c, i, b, k, &active);
      cnt += active;
    }
    cam_free[i] = (uint8_t)(!fixed[i] && c.cam_valid[i] && cnt >= 1);
    s.n_free += cam_free[i];
    if constexpr (M == 7) {
      c.cam_focal[i] = (uint8_t)cam_focal_rule(c, i, cam_free[i] != 0, cnt);
      s.n_focal += c.cam_focal[i];
    }
  }
  if (s.err) return LOFTR_ERR_BAD_ARG;

  // a camera's osum64: element l is slot l of its list; an inactive slot adds nothing
  auto cam_sum = [&](long i, auto tag, auto term, double* out) {
    constexpr int W = decltype(tag)::value;
    const long b = cam_offsets[i];
    osum64<W>(cam_offsets[i + 1] - b, [&](long e, double* a) { const long o = cam_obs[b + e]; if (obs_active[o]) term(o, a); }, out);
  };
  auto evaluate = [&](int buf) {
    bool ok = true;
    for (long t = 0; t < T; ++t) ok = track_eval(c, buf, t) && ok;
    return ok;
  };
  evaluate(0);
  ctrl_feed(c, kActCost0, osum(c.part, T));
  ctrl_feed(c, kActSq0, osum(c.part2, T));

  for (int it = 0; it < max_iters && !s.done; ++it) {
    const int cur = s.cur;
    if (s.fresh) {
      for (long t = 0; t < T; ++t) track_lin<M>(c, cur, t);
      for (long i = 0; i < n; ++i) {
        if (!cam_free[i]) continue;
        double a[kU + M];
        cam_sum(i, std::integral_constant<int, kU + M>{}, [&](long o, double* acc) { cam_lin_term<M>(c, cur, o, acc); }, a);
        for (int k = 0; k < kU; ++k) c.U[kU * i + k] = a[k];
        for (int k = 0; k < M; ++k) c.gc[M * i + k] = a[kU + k];
      }
    }
    const double lambda = s.lambda;
    for (long t = 0; t < T; ++t) if (!track_factor(c, t, lambda)) s.bad_f = 1;
    for (long i = 0; i < n; ++i) if (!cam_factor<M>(c, i, lambda)) s.bad_f = 1;
    auto camera_half = [&](int mode) {
      for (long i = 0; i < n; ++i) {
        double a[M];
        for (int k = 0; k < M; ++k) a[k] = 0.0;
        if (cam_free[i]) cam_sum(i, std::integral_constant<int, M>{}, [&](long o, double* acc) { cam_half_term<M>(c, cur, o, acc); }, a);
        cam_half_finish<M>(c, i, mode, lambda, a);
      }
    };
    if (!s.bad_f) {
      for (long t = 0; t < T; ++t) track_half<M>(c, cur, t, 0, nullptr);
      camera_half(0);
      ctrl_feed(c, kActRz0, osum(c.part, n));
      for (int pi = 0; pi < pcg_iters && !s.pcg_done; ++pi) {
        for (long t = 0; t < T; ++t) track_half<M>(c, cur, t, 1, c.p);
        camera_half(1);
        ctrl_feed(c, kActPsp, osum(c.part, n));
        if (s.pcg_done) break;
        for (long i = 0; i < n; ++i) cam_update1<M>(c, i, s.alpha);
        ctrl_feed(c, kActRz, osum(c.part, n));
        if (s.pcg_done) break;
        for (long i = 0; i < n; ++i) cam_update2<M>(c, i, s.beta);
      }
      for (long i = 0; i < n; ++i) if (!cam_apply<M>(c, cur, i)) s.bad_a = 1;
      for (long t = 0; t < T; ++t) if (!track_half<M>(c, cur, t, 2, c.x)) s.bad_a = 1;
    }
    if (!s.bad_f && !s.bad_a) {
      if (!evaluate(1 - cur)) s.bad_e = 1;
      if (!s.bad_e) {
        ctrl_feed(c, kActCostT, osum(c.part, T));
        ctrl_feed(c, kActSqT, osum(c.part2, T));
      }
    }
    ctrl_accept(c);
  }
  for (long i = 0; i < n; ++i) cam_write<M>(c, s.cur, i);
  for (long t = 0; t < T; ++t) track_write(c, s.cur, t);
  ctrl_write<M>(c);
  return LOFTR_OK;
}

// §18.2: the sequence of phases with one focal step per group of cameras
int run_shared(CtxS& c, int max_iters, int pcg_iters) {
  const long T = c.T, n = c.n, G = c.G;
  const long* cam_offsets = c.cam_offsets;
  const int* cam_obs = c.cam_obs;
  const uint8_t *fixed = c.fixed, *obs_active = c.obs_active;
  uint8_t* cam_free = c.cam_free;
  std::vector<char> ws(layout_shared(c, nullptr), 0);
  layout_shared(c, ws.data());
  Ctrl& s = *c.ctrl;
  shared_init(c);
  for (long i = 0; i < n; ++i) { cam_setup(c, i); cam_setup_focal(c, i); }
  for (long t = 0; t < T; ++t) {
    long cnt;
    s.err |= track_setup(c, t, &cnt);
    s.n_active_obs += (unsigned long long)cnt;
    s.n_active_pts += cnt > 0;
  }
  if (s.err) return LOFTR_ERR_BAD_ARG;
  for (long i = 0; i < n; ++i) {
    c.cam_focal[i] = 0;
    long b, e, cnt = 0;
    if (!group_range(c, i, &b, &e)) { s.err |= kBadGroups; continue; }
    for (long k = b; k < e; ++k) {
      bool active;
      s.err |= group_check(c, i, b, k, &active);
      cnt += active;
    }
    cam_free[i] = (uint8_t)(!fixed[i] && c.cam_valid[i] && cnt >= 1);
    s.n_free += cam_free[i];
    s.err |= cam_carry(c, i, cnt);
  }
  if (s.err) return LOFTR_ERR_BAD_ARG;
  for (long g = 0; g < G; ++g) {
    long b, e, total = 0;
    int err = 0;
    if (!cgroup_range(c, g, &b, &e)) { s.err |= kBadCamGroups; continue; }
    for (long k = b; k < e; ++k) {
      long cnt;
      err |= cgroup_slot(c, g, b, k, &cnt);
      total += cnt;
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
  }
  if (s.err) return LOFTR_ERR_BAD_ARG;

  auto cam_sum = [&](long i, auto tag, auto term, double* out) {
    constexpr int W = decltype(tag)::value;
    const long b = cam_offsets[i];
    osum64<W>(cam_offsets[i + 1] - b, [&](long e, double* a) { const long o = cam_obs[b + e]; if (obs_active[o]) term(o, a); }, out);
  };
  // a group's osum64: element l is the l-th member
  auto group_sum = [&](long g, const double* v, long stride) {
    const long b = c.group_offsets[g];
    double out;
    osum64<1>(c.group_offsets[g + 1] - b, [&](long e, double* a) { group_term(c, c.group_cams[b + e], v, stride, a); }, &out);
    return out;
  };
  auto dot = [&]() { const double cams = osum(c.part, n); return cams + osum(c.partg, G); };
  auto evaluate = [&](int buf) {
    bool ok = true;
    for (long t = 0; t < T; ++t) ok = track_eval(c, buf, t) && ok;
    return ok;
  };
  evaluate(0);
  ctrl_feed(c, kActCost0, osum(c.part, T));
  ctrl_feed(c, kActSq0, osum(c.part2, T));

  for (int it = 0; it < max_iters && !s.done; ++it) {
    const int cur = s.cur;
    if (s.fresh) {
      for (long t = 0; t < T; ++t) track_lin<6>(c, cur, t);
      for (long i = 0; i < n; ++i) {
        if (!live(c, i)) continue;
        double a[35];
        cam_sum(i, std::integral_constant<int, 35>{}, [&](long o, double* acc) { cam_lin_term_s(c, cur, o, acc); }, a);
        for (int k = 0; k < 28; ++k) c.U[28 * i + k] = a[k];
        for (int k = 0; k < 7; ++k) c.gc[7 * i + k] = a[28 + k];
      }
      for (long g = 0; g < G; ++g) if (c.group_focal[g]) c.dg[g] = group_sum(g, c.U + 27, 28);
    }
    const double lambda = s.lambda;
    for (long t = 0; t < T; ++t) if (!track_factor(c, t, lambda)) s.bad_f = 1;
    for (long i = 0; i < n; ++i) if (!cam_factor_s(c, i, lambda)) s.bad_f = 1;
    for (long g = 0; g < G; ++g) if (!group_factor(c, g, lambda)) s.bad_f = 1;
    auto camera_half = [&](int mode) {
      for (long i = 0; i < n; ++i) {
        double a[7];
        for (int k = 0; k < 7; ++k) a[k] = 0.0;
        if (live(c, i)) cam_sum(i, std::integral_constant<int, 7>{}, [&](long o, double* acc) { cam_half_term_s(c, cur, o, acc); }, a);
        cam_half_finish_s(c, i, mode, lambda, a);
      }
      for (long g = 0; g < G; ++g) group_half_finish(c, g, mode, lambda, c.group_focal[g] ? group_sum(g, c.Sp + 6, 7) : 0.0);
    };
    if (!s.bad_f) {
      for (long t = 0; t < T; ++t) track_half_s(c, cur, t, 0, nullptr, nullptr);
      camera_half(0);
      ctrl_feed(c, kActRz0, dot());
      for (int pi = 0; pi < pcg_iters && !s.pcg_done; ++pi) {
        for (long t = 0; t < T; ++t) track_half_s(c, cur, t, 1, c.p, c.pg);
        camera_half(1);
        ctrl_feed(c, kActPsp, dot());
        if (s.pcg_done) break;
        for (long i = 0; i < n; ++i) cam_update1_s(c, i, s.alpha);
        for (long g = 0; g < G; ++g) group_update1(c, g, s.alpha, lambda);
        ctrl_feed(c, kActRz, dot());
        if (s.pcg_done) break;
        for (long i = 0; i < n; ++i) cam_update2_s(c, i, s.beta);
        for (long g = 0; g < G; ++g) group_update2(c, g, s.beta);
      }
      for (long i = 0; i < n; ++i) if (!cam_apply_s(c, cur, i)) s.bad_a = 1;
      for (long g = 0; g < G; ++g) group_apply(c, cur, g);
      for (long t = 0; t < T; ++t) if (!track_half_s(c, cur, t, 2, c.x, c.xg)) s.bad_a = 1;
    }
    if (!s.bad_f && !s.bad_a) {
      if (!evaluate(1 - cur)) s.bad_e = 1;
      if (!s.bad_e) {
        ctrl_feed(c, kActCostT, osum(c.part, T));
        ctrl_feed(c, kActSqT, osum(c.part2, T));
      }
    }
    ctrl_accept(c);
  }
  for (long i = 0; i < n; ++i) cam_write_s(c, s.cur, i);
  for (long t = 0; t < T; ++t) track_write(c, s.cur, t);
  ctrl_write_s(c);
  return LOFTR_OK;
}

}  // namespace

extern "C" int loftr_bundle_adjust_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                                        const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed, int n_images,
                                        const long* cam_offsets, const int* cam_obs, double huber_px, int max_iters, int pcg_iters,
                                        double pcg_tol, double ftol, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free,
                                        uint8_t* point_active, long* counts) {
  const int st = check_args(offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs,
                            huber_px, max_iters, pcg_iters, pcg_tol, ftol, T_out, xyz_out, obs_active, cam_free, point_active, counts);
  if (st != LOFTR_OK) return st;
  Ctx c{};
  c.offsets = offsets; c.T = T; c.image = obs_image; c.xy = obs_xy; c.mask = obs_mask; c.N = N;
  c.xyz_in = xyz; c.K = K; c.Tin = T_cam_from_world; c.fixed = fixed; c.n = n_images; c.cam_offsets = cam_offsets; c.cam_obs = cam_obs;
  c.huber = huber_px; c.pcg_tol2 = pcg_tol * pcg_tol; c.ftol = ftol;
  c.T_out = T_out; c.xyz_out = xyz_out; c.obs_active = obs_active; c.cam_free = cam_free; c.point_active = point_active; c.counts = counts;
  return run<6>(c, max_iters, pcg_iters);
}

extern "C" int loftr_bundle_adjust_focal_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                              long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                              const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                              double huber_px, int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs,
                                              double focal_lo, double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active,
                                              uint8_t* cam_free, uint8_t* point_active, double* K_out, uint8_t* cam_focal, long* counts) {
  if (n_images > 0 && (!refine_focal || !K_out || !cam_focal)) return LOFTR_ERR_BAD_ARG;
  if (!(min_focal_obs >= 1 && fin(focal_lo) && fin(focal_hi) && focal_lo < 1.0 && 1.0 < focal_hi)) return LOFTR_ERR_BAD_ARG;
  const int st = check_args(offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs,
                            huber_px, max_iters, pcg_iters, pcg_tol, ftol, T_out, xyz_out, obs_active, cam_free, point_active, counts);
  if (st != LOFTR_OK) return st;
  Ctx7 c{};
  c.offsets = offsets; c.T = T; c.image = obs_image; c.xy = obs_xy; c.mask = obs_mask; c.N = N;
  c.xyz_in = xyz; c.K = K; c.Tin = T_cam_from_world; c.fixed = fixed; c.n = n_images; c.cam_offsets = cam_offsets; c.cam_obs = cam_obs;
  c.huber = huber_px; c.pcg_tol2 = pcg_tol * pcg_tol; c.ftol = ftol;
  c.T_out = T_out; c.xyz_out = xyz_out; c.obs_active = obs_active; c.cam_free = cam_free; c.point_active = point_active; c.counts = counts;
  c.refine_focal = refine_focal; c.min_focal_obs = min_focal_obs; c.focal_lo = focal_lo; c.focal_hi = focal_hi;
  c.K_out = K_out; c.cam_focal = cam_focal;
  return run<7>(c, max_iters, pcg_iters);
}

extern "C" int loftr_bundle_adjust_shared_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask,
                                               long N, const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                               const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                               const int* cam_group, const long* group_offsets, const int* group_cams, int G, double huber_px,
                                               int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs, double focal_lo,
                                               double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free,
                                               uint8_t* point_active, double* K_out, uint8_t* cam_focal, uint8_t* group_focal, long* counts) {
  if (n_images > 0 && (!refine_focal || !K_out || !cam_focal || !cam_group || !group_cams || !group_focal)) return LOFTR_ERR_BAD_ARG;
  if (!group_offsets || G < 0 || G > n_images || (n_images > 0 && G == 0)) return LOFTR_ERR_BAD_ARG;
  if (!(min_focal_obs >= 1 && fin(focal_lo) && fin(focal_hi) && focal_lo < 1.0 && 1.0 < focal_hi)) return LOFTR_ERR_BAD_ARG;
  const int st = check_args(offsets, T, obs_image, obs_xy, obs_mask, N, xyz, K, T_cam_from_world, fixed, n_images, cam_offsets, cam_obs,
                            huber_px, max_iters, pcg_iters, pcg_tol, ftol, T_out, xyz_out, obs_active, cam_free, point_active, counts);
  if (st != LOFTR_OK) return st;
  CtxS c{};
  c.offsets = offsets; c.T = T; c.image = obs_image; c.xy = obs_xy; c.mask = obs_mask; c.N = N;
  c.xyz_in = xyz; c.K = K; c.Tin = T_cam_from_world; c.fixed = fixed; c.n = n_images; c.cam_offsets = cam_offsets; c.cam_obs = cam_obs;
  c.huber = huber_px; c.pcg_tol2 = pcg_tol * pcg_tol; c.ftol = ftol;
  c.T_out = T_out; c.xyz_out = xyz_out; c.obs_active = obs_active; c.cam_free = cam_free; c.point_active = point_active; c.counts = counts;
  c.refine_focal = refine_focal; c.min_focal_obs = min_focal_obs; c.focal_lo = focal_lo; c.focal_hi = focal_hi;
  c.K_out = K_out; c.cam_focal = cam_focal;
  c.cam_group = cam_group; c.group_offsets = group_offsets; c.group_cams = group_cams; c.G = G; c.group_focal = group_focal;
  return run_shared(c, max_iters, pcg_iters);
}
