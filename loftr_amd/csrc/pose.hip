// Relative pose from matches: five-point essential matrix inside RANSAC + cheirality (host code, double precision).
//
// Replaces: estimate_pose (src/utils/metrics.py:72-98) = cv2.findEssentialMat(kpts0, kpts1, I, threshold, prob, RANSAC)
// followed by cv2.recoverPose(E, kpts0, kpts1, I, 1e9, mask) on intrinsics-normalised key points -- the pose step of the
// reference's test_step (compute_pose_errors, metrics.py:101-136).  OpenCV is a CPU library and is not in this image, so
// this is a restatement of the published algorithms, NOT of OpenCV's source:
//   * D. Nister, "An efficient solution to the five-point relative pose problem", PAMI 2004: the 4-dimensional null
//     space of the epipolar constraints, the ten cubic constraints (det E = 0, 2 E E^T E - tr(E E^T) E = 0) eliminated
//     by Gauss-Jordan to a 3x3 polynomial matrix in z whose determinant is a tenth-degree polynomial;
//   * RANSAC with the Sampson distance (squared, against threshold^2), adaptive iteration count from the confidence,
//     at most 1000 iterations -- the parameters cv2.findEssentialMat documents;
//   * the four (R, t) decompositions of E disambiguated by triangulating the inliers (positive depth in both views,
//     depth < 1e9), as cv2.recoverPose documents.
// The arithmetic lives in pose_core.h, one text for this file and for the batched GPU estimator (pose_gpu.hip), which reproduces this
// function's result bit for bit.
// PARITY UNPINNED: the random sampling sequence (and therefore the selected hypothesis on noisy data) cannot match
// OpenCV's; the tests check the solver on exact data and the recovered pose on synthetic scenes with known ground truth.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/loftr_hip.h"
#include "pose_core.h"

#pragma clang fp contract(off)

namespace {

using namespace pose;

const PolarTable& table() { static const PolarTable t = polar_table<10>(); return t; }

// squared Sampson distance of every correspondence; returns the number below thr2
long score(const double* E, const double* q0, const double* q1, long n, double thr2, uint8_t* mask) {
  long cnt = 0;
  for (long i = 0; i < n; ++i) {
    const bool in = sampson_in(E, q0[2 * i], q0[2 * i + 1], q1[2 * i], q1[2 * i + 1], thr2);
    if (mask) mask[i] = in;
    cnt += in;
  }
  return cnt;
}

// cheirality: number of inliers in front of both cameras for (R, t), marked in good
long cheirality(const double* R, const double* t, const double* q0, const double* q1, long n, const uint8_t* in, double dist,
                uint8_t* good) {
  long cnt = 0;
  for (long i = 0; i < n; ++i) {
    good[i] = in[i] && in_front(R, t, q0[2 * i], q0[2 * i + 1], q1[2 * i], q1[2 * i + 1], dist);
    cnt += good[i];
  }
  return cnt;
}

}  // namespace

extern "C" int loftr_five_point(const double* q0, const double* q1, int n, double* E_out, int* n_solutions) {
  if (!q0 || !q1 || !E_out || !n_solutions || n < 5) return LOFTR_ERR_BAD_ARG;
  double Es[kSol * 9];
  const int ns = five_point(q0, q1, 2, nullptr, n, Es, table());
  memcpy(E_out, Es, sizeof(double) * 9 * ns);
  *n_solutions = ns;
  return LOFTR_OK;
}

extern "C" int loftr_estimate_pose(const float* kpts0, const float* kpts1, long M, const float* K0, const float* K1,
                                   float thresh_px, float conf, unsigned seed, float* R_out, float* t_out,
                                   uint8_t* inliers_out, long* n_inliers) {
  if (!kpts0 || !kpts1 || !K0 || !K1 || !R_out || !t_out || !inliers_out || !n_inliers || M < 0) return LOFTR_ERR_BAD_ARG;
  *n_inliers = -1;                                           // "None" of the reference: too few points / no model
  if (M < kSample) return LOFTR_OK;
  std::vector<double> q0(2 * M), q1(2 * M);
  for (long i = 0; i < M; ++i) {                             // (kpts - [cx, cy]) / [fx, fy]        metrics.py:76-77
    q0[2 * i] = ((double)kpts0[2 * i] - K0[2]) / K0[0]; q0[2 * i + 1] = ((double)kpts0[2 * i + 1] - K0[5]) / K0[4];
    q1[2 * i] = ((double)kpts1[2 * i] - K1[2]) / K1[0]; q1[2 * i + 1] = ((double)kpts1[2 * i + 1] - K1[5]) / K1[4];
  }
  const double thr2 = sampson_thr2(thresh_px, K0, K1);       //                                      metrics.py:80
  const PolarTable& tab = table();
  Rng rng(seed);
  double bestE[9] = {0};
  long best = 0;
  int iters = kIters;
  for (int it = 0; it < iters; ++it) {
    int idx[kSample];
    draw_sample(rng, M, kSample, idx);
    double Es[kSol * 9];
    const int ns = five_point(q0.data(), q1.data(), 2, idx, kSample, Es, tab);
    for (int s = 0; s < ns; ++s) {
      const long cnt = score(Es + 9 * s, q0.data(), q1.data(), M, thr2, nullptr);
      if (cnt > best) {
        best = cnt;
        memcpy(bestE, Es + 9 * s, sizeof(bestE));
        iters = adaptive_iters(cnt, M, kSample, conf, it, iters);
      }
    }
  }
  if (best < kSample) return LOFTR_OK;
  std::vector<uint8_t> in(M), good(M), bestgood(M);
  score(bestE, q0.data(), q1.data(), M, thr2, in.data());
  double Rs[4][9], ts[4][3];
  pose_candidates(bestE, Rs, ts);
  long bestc = -1; int bi = 0;
  for (int c = 0; c < 4; ++c) {                               // the sequential vote: the first maximum wins
    const long cnt = cheirality(Rs[c], ts[c], q0.data(), q1.data(), M, in.data(), 1e9, good.data());
    if (cnt > bestc) { bestc = cnt; bi = c; bestgood = good; }
  }
  if (bestc <= 0) return LOFTR_OK;                            // recoverPose found no point in front of both cameras
  for (int i = 0; i < 9; ++i) R_out[i] = (float)Rs[bi][i];
  for (int i = 0; i < 3; ++i) t_out[i] = (float)ts[bi][i];
  memcpy(inliers_out, bestgood.data(), (size_t)M);
  *n_inliers = bestc;
  return LOFTR_OK;
}
