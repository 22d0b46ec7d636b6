// Track completion, host routine (plain C++ on host arrays, double precision): every row of a track table that has a 3D point is
// projected into every posed image it does not visit yet and claims the nearest free atlas keypoint within the threshold; a keypoint
// claimed by several rows goes to the nearest, then to the lowest row (the contract is in include/loftr_hip.h).  The step
// COLMAP runs after every adjustment (CompleteTracks); COLMAP is not in this image, so this is a statement of the published idea
// (reproject, search, extend the track), NOT of its source.  PARITY UNPINNED against it.
// This function DEFINES the result: loftr_complete_tracks (complete_gpu.hip) reproduces it bit for bit, which is why the arithmetic
// and the candidate order live in complete_core.h.  It is written as rows x images in order with a plain array of claims.
#include <stdint.h>
#include <vector>
#include "../../include/loftr_hip.h"
#include "complete_core.h"

#pragma clang fp contract(off)

using namespace complete;

extern "C" int loftr_complete_tracks_host(const long* offsets, long T, const int* obs_image, long N, const float* xyz, const uint8_t* status,
                                          const long* kp_offsets, const float* keypoints, const int* kp_cell, const int* kp_row, long K,
                                          const double* Kmat, const double* T_cam_from_world, const uint8_t* posed, int n_images, float inv,
                                          int gh, int gw, double thresh_px, int reach, int* kp_row_new, float* link_r2, long* counts) {
  if (!offsets || !kp_offsets || !counts || T < 0 || N < 0 || K < 0 || n_images < 0 || gh < 0 || gw < 0) return LOFTR_ERR_BAD_ARG;
  if (T > 0 && (!xyz || !status)) return LOFTR_ERR_BAD_ARG;
  if (N > 0 && !obs_image) return LOFTR_ERR_BAD_ARG;
  if (K > 0 && (!keypoints || !kp_cell || !kp_row || !kp_row_new || !link_r2)) return LOFTR_ERR_BAD_ARG;
  if (n_images > 0 && (!Kmat || !T_cam_from_world || !posed)) return LOFTR_ERR_BAD_ARG;
  if (!(thresh_px >= 0.0) || !tri::fin(thresh_px) || reach < 0 || reach > kMaxReach) return LOFTR_ERR_BAD_ARG;
  if ((T == 0 && N != 0) || (n_images == 0 && K != 0)) return LOFTR_ERR_BAD_ARG;      // observations / keypoints outside every row / image
  if (!sizes_ok(T, N, K, n_images) || !grid_ok(gh, gw)) return LOFTR_ERR_UNSUPPORTED;
  std::vector<double> tab((size_t)tri::kCam * (size_t)n_images);
  const In a{offsets, T, obs_image, N, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, tab.data(), posed, n_images, inv, gh, gw,
             thresh_px * thresh_px, reach};
  if (T == 0 && offsets[0] != 0) return LOFTR_ERR_BAD_ARG;
  if (n_images == 0 && kp_offsets[0] != 0) return LOFTR_ERR_BAD_ARG;
  int err = 0;
  for (long t = 0; t < T; ++t) err |= check_row(a, t);
  for (int i = 0; i < n_images; ++i) err |= check_image(a, i);
  for (long k = 0; k < K; ++k) err |= check_keypoint(a, k);
  for (int c = 0; c < kCounts; ++c) counts[c] = 0;
  counts[kErrors] = err;
  if (err) return LOFTR_ERR_BAD_ARG;
  for (int i = 0; i < n_images; ++i) tri::cam_table(Kmat + 9 * (size_t)i, T_cam_from_world + 16 * (size_t)i, &tab[(size_t)tri::kCam * i]);
  std::vector<uint64_t> claim((size_t)K, kNoClaim);
  for (long j = 0; j < T; ++j) {
    double X[3];
    if (!source(a, j, X)) continue;
    ++counts[kSources];
    long cur = offsets[j];
    const long end = offsets[j + 1];
    for (int i = 0; i < n_images; ++i) {
      while (cur < end && obs_image[cur] < i) ++cur;                                   // the merge walk over the row's ascending images
      if (!target_image(a, i) || (cur < end && obs_image[cur] == i)) continue;
      ++counts[kPairs];
      uint32_t bits;
      int flags;
      const long k = propose(a, i, X, &bits, &flags);
      counts[kInside] += (flags & kFlagInside) != 0;
      counts[kBlocked] += (flags & kFlagBlocked) != 0;
      if (k < 0) continue;
      ++counts[kProposals];
      const uint64_t mine = key(bits, j);
      if (mine < claim[(size_t)k]) claim[(size_t)k] = mine;
    }
  }
  const float nanf_ = __builtin_nanf("");
  for (long k = 0; k < K; ++k) {
    const bool won = claim[(size_t)k] != kNoClaim;
    kp_row_new[k] = won ? key_row(claim[(size_t)k]) : kp_row[k];
    link_r2[k] = won ? key_r2(claim[(size_t)k]) : nanf_;
    counts[kLinks] += won;
  }
  counts[kLost] = counts[kProposals] - counts[kLinks];
  return LOFTR_OK;
}
