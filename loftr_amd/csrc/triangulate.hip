// Triangulation of tracks from known camera poses (host code, double precision): for every track of a keypoint atlas, a 3D point from
// its observations -- two-ray midpoints over a fixed enumeration of observation pairs, scored by pixel reprojection error, the best one
// refitted by Gauss-Newton over its inliers (the contract is in include/loftr_hip.h).  What COLMAP's / hloc's point
// triangulator does with database poses; neither is in this image, so this is a statement of the published method (midpoint
// initialisation, robust selection, non-linear refinement), NOT of their source.  PARITY UNPINNED against them.
// This function DEFINES the result: loftr_triangulate_tracks (triangulate_gpu.hip) reproduces it bit for bit, which is why all the
// arithmetic lives in triangulate_core.h and why the refit's sums run in ascending observation order.
#include <stdint.h>
#include <vector>
#include "../../include/loftr_hip.h"
#include "triangulate_core.h"

#pragma clang fp contract(off)

using namespace tri;

extern "C" int loftr_triangulation_pairs(int L, int* pairs, int* n) {
  if (!pairs || !n || L < 0) return LOFTR_ERR_BAD_ARG;
  *n = n_pairs(L);
  for (int h = 0; h < *n; ++h) {
    long i, j;
    pair_at(L, h, &i, &j);
    pairs[2 * h] = (int)i;
    pairs[2 * h + 1] = (int)j;
  }
  return LOFTR_OK;
}

extern "C" int loftr_triangulate_tracks_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, long N, const double* K,
                                             const double* T_cam_from_world, int n_images, double thresh_px, double cos_min_angle,
                                             float* xyz, int* n_inliers, float* rms_px, float* tri_cos, uint8_t* status, uint8_t* obs_inlier,
                                             long* counts) {
  if (!offsets || !counts || T < 0 || N < 0 || n_images < 0) return LOFTR_ERR_BAD_ARG;
  if (T > 0 && (!xyz || !n_inliers || !rms_px || !tri_cos || !status)) return LOFTR_ERR_BAD_ARG;
  if (N > 0 && (!obs_image || !obs_xy || !obs_inlier)) return LOFTR_ERR_BAD_ARG;
  if (n_images > 0 && (!K || !T_cam_from_world)) return LOFTR_ERR_BAD_ARG;
  if (!(thresh_px >= 0.0 && cos_min_angle >= -1.0 && cos_min_angle <= 1.0)) return LOFTR_ERR_BAD_ARG;
  if (T >= (1L << 31) || N >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  for (int i = 0; i < kCounts; ++i) counts[i] = 0;
  if (T == 0 && (offsets[0] != 0 || N != 0)) return LOFTR_ERR_BAD_ARG;
  for (long t = 0, b, e; t < T; ++t)
    if (!tracks::span(offsets, T, N, t, &b, &e) || !tracks::images_ok(obs_image, b, e, n_images)) return LOFTR_ERR_BAD_ARG;
  std::vector<double> tab((size_t)kCam * (size_t)n_images);
  for (int i = 0; i < n_images; ++i) cam_table(K + 9 * (size_t)i, T_cam_from_world + 16 * (size_t)i, &tab[(size_t)kCam * i]);
  const Obs o{tab.data(), obs_image, obs_xy, thresh_px * thresh_px, cos_min_angle};
  const Out w{xyz, n_inliers, rms_px, tri_cos, status};
  for (long t = 0; t < T; ++t) {
    const long o0 = offsets[t], L = offsets[t + 1] - o0;
    uint8_t* bits = obs_inlier + o0;
    double X[3] = {0.0, 0.0, 0.0}, rms = 0.0, min_cos = 2.0;
    long cnt = 0;
    int st = -1;
    bool bad = false;
    for (long k = 0; k < L; ++k) bad = bad || !cam_valid(&tab[(size_t)kCam * obs_image[o0 + k]]);
    if (L < 2) st = kTooShort;
    else if (bad) st = kBadCamera;
    else {
      const int nh = n_pairs(L);
      unsigned long long best = 0;
      for (int h = 0; h < nh; ++h) {
        const unsigned long long word = hyp_word(o, o0, L, h);
        if (word > best) best = word;
      }
      if (best == 0) st = kNoHypothesis;
      else {
        hyp_point(o, o0, L, (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)), X);
        cnt = refit_track(o, o0, L, X, bits, &rms);
        for (int h = 0; h < nh; ++h) {
          double cs;
          if (pair_cos(o, o0, L, h, X, bits, &cs) && cs < min_cos) min_cos = cs;
        }
        st = min_cos > cos_min_angle ? kSmallAngle : kOk;
      }
    }
    if (st != kOk) for (long k = 0; k < L; ++k) bits[k] = 0;
    write_track(w, t, st, X, cnt, rms, min_cos, min_cos != 2.0);
    counts[st] += 1;
    if (st == kOk) counts[6] += cnt;
  }
  return LOFTR_OK;
}
