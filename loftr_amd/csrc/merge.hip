// Track merging, host routine (plain C++ on host arrays, double precision): every row of a track table that has a 3D point is projected
// into every posed image it does not visit; where it lands on a keypoint held by another row with a point, the two rows share no image
// and every defining observation of both lies within the threshold of their weighted point, the pair is a candidate; two rows that are
// each other's best candidate become one (the contract is in include/loftr_hip.h).  The step COLMAP runs next to
// CompleteTracks after every adjustment (MergeTracks); COLMAP is not in this image, so this is a statement of the published idea, NOT
// of its source.  PARITY UNPINNED against it.
// This function DEFINES the result: loftr_merge_tracks (merge_gpu.hip) reproduces it bit for bit, which is why every per-item step
// lives in merge_core.h.  It is written as rows x images in order with a plain array of best keys.
#include <stdint.h>
#include <vector>
#include "../../include/loftr_hip.h"
#include "merge_core.h"

#pragma clang fp contract(off)

using namespace merge;

extern "C" int loftr_merge_tracks_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                                       const float* xyz, const uint8_t* status, const long* kp_offsets, const float* keypoints,
                                       const int* kp_cell, const int* kp_row, long K, const double* Kmat, const double* T_cam_from_world,
                                       const uint8_t* posed, int n_images, float inv, int gh, int gw, double thresh_px, int reach,
                                       int* row_into, float* merge_r2, int* kp_row_new, long* counts) {
  if (!offsets || !kp_offsets || !counts || T < 0 || N < 0 || K < 0 || n_images < 0 || gh < 0 || gw < 0) return LOFTR_ERR_BAD_ARG;
  if (T > 0 && (!xyz || !status || !row_into || !merge_r2)) return LOFTR_ERR_BAD_ARG;
  if (N > 0 && (!obs_image || !obs_xy || !obs_mask)) return LOFTR_ERR_BAD_ARG;
  if (K > 0 && (!keypoints || !kp_cell || !kp_row || !kp_row_new)) return LOFTR_ERR_BAD_ARG;
  if (n_images > 0 && (!Kmat || !T_cam_from_world || !posed)) return LOFTR_ERR_BAD_ARG;
  if (!(thresh_px >= 0.0) || !tri::fin(thresh_px) || reach < 0 || reach > complete::kMaxReach) return LOFTR_ERR_BAD_ARG;
  if ((T == 0 && N != 0) || (n_images == 0 && K != 0)) return LOFTR_ERR_BAD_ARG;      // observations / keypoints outside every row / image
  if (!complete::sizes_ok(T, N, K, n_images) || !complete::grid_ok(gh, gw)) return LOFTR_ERR_UNSUPPORTED;
  std::vector<double> tab((size_t)tri::kCam * (size_t)n_images);
  const In a{{offsets, T, obs_image, N, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, tab.data(), posed, n_images, inv, gh, gw,
              thresh_px * thresh_px, reach}, obs_xy, obs_mask};
  if (T == 0 && offsets[0] != 0) return LOFTR_ERR_BAD_ARG;
  if (n_images == 0 && kp_offsets[0] != 0) return LOFTR_ERR_BAD_ARG;
  int err = 0;
  for (long t = 0; t < T; ++t) err |= complete::check_row(a.c, t);
  for (int i = 0; i < n_images; ++i) err |= complete::check_image(a.c, i);
  for (long k = 0; k < K; ++k) err |= complete::check_keypoint(a.c, k);
  for (int c = 0; c < kCounts; ++c) counts[c] = 0;
  counts[kErrors] = err;
  if (err) return LOFTR_ERR_BAD_ARG;
  for (int i = 0; i < n_images; ++i) tri::cam_table(Kmat + 9 * (size_t)i, T_cam_from_world + 16 * (size_t)i, &tab[(size_t)tri::kCam * i]);
  std::vector<uint64_t> best((size_t)T, kNoPartner);
  for (long j = 0; j < T; ++j) {
    double X[3];
    if (!complete::source(a.c, j, X)) continue;
    ++counts[kSources];
    long cur = offsets[j];
    const long end = offsets[j + 1];
    for (int i = 0; i < n_images; ++i) {
      while (cur < end && obs_image[cur] < i) ++cur;                                   // the merge walk over the row's ascending images
      if (!complete::target_image(a.c, i) || (cur < end && obs_image[cur] == i)) continue;
      ++counts[kPairs];
      const long m = meet(a, i, j, X);
      if (m < 0) continue;
      ++counts[kMeetings];
      uint32_t bits = 0;
      const int verdict = judge(a, j, m, &bits);
      counts[kDisjoint] += (verdict & 1) != 0;
      if (!(verdict & 2)) continue;
      ++counts[kAccepted];
      const uint64_t kj = key(bits, m), km = key(bits, j);
      if (kj < best[(size_t)j]) best[(size_t)j] = kj;
      if (km < best[(size_t)m]) best[(size_t)m] = km;
    }
  }
  const float nanf_ = __builtin_nanf("");
  for (long j = 0; j < T; ++j) {
    bool merged;
    float r2 = nanf_;
    const long into = survivor(best.data(), j, &merged, &r2);
    row_into[j] = (int)into;
    merge_r2[j] = merged ? r2 : nanf_;
    counts[kMerged] += merged && into == j;                                            // a pair is counted once, at its lower row
  }
  for (long k = 0; k < K; ++k) {
    const int row = kp_row[k];
    kp_row_new[k] = row < 0 ? row : row_into[row];
    counts[kRelabelled] += kp_row_new[k] != row;
  }
  return LOFTR_OK;
}
