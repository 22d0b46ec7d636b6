// Absolute pose (camera resection, PnP) from 2D-3D matches: P3P inside RANSAC + a Gauss-Newton refit on the pixel reprojection error
// (host code, double precision).  The metric counterpart of loftr_estimate_pose (pose.hip): what cv2.solvePnPRansac / pycolmap's
// absolute pose estimation are used for when one image of the pair comes with a depth map (InLoc, Aachen, RGB-D re-localisation).
// Neither library is in this image, so this is a restatement of the published algorithms, NOT of their source:
//   * P3P: Grunert's quartic in the depth ratio as in Haralick et al.'s review (IJCV 1994), its real positive roots by the Aberth-
//     Ehrlich finder of the five-point solver, a Newton polish of the three distances, and the rigid motion from the orthonormal
//     frames of the two point triples; (near-)collinear world points and coincident bearings give no solution;
//   * RANSAC with loftr_estimate_pose's sampler (xorshift64*, duplicate rejection), cap (1000) and adaptive stop (exponent 3);
//     residual: squared reprojection error in pixels, positive depth required;
//   * a Gauss-Newton refit (left rotation increment through a normalised quaternion, additive translation, 5 steps) over the inliers
//     of the best hypothesis, adopted when it keeps at least as many inliers and repeated on the adopted model's inliers while the
//     set strictly grows (at most 4 fits), exactly as loftr_estimate_geometry does.
// This function DEFINES the result: loftr_estimate_absolute_pose_batched (absolute_pose_gpu.hip) reproduces it bit for bit, which is
// why all the arithmetic lives in absolute_pose_core.h and why the refit's sums have a fixed order (256 strided partials, then a
// pairwise tree).  PARITY UNPINNED against OpenCV's solvePnPRansac: own sampling sequence, own degeneracy tests.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/loftr_hip.h"
#include "absolute_pose_core.h"

#pragma clang fp contract(off)

namespace {

using namespace absp;

const PolarTable& table() { static const PolarTable t = polar_table<4>(); return t; }

// pts [n,8]: world point (3), pixel (2), unit bearing (3)
long score(const Cam& cam, const double* R, const double* t, const double* pts, long n, double thr2, uint8_t* mask) {
  long cnt = 0;
  for (long i = 0; i < n; ++i) {
    const bool in = is_inlier(cam, R, t, pts + 8 * i, pts[8 * i + 3], pts[8 * i + 4], thr2);
    if (mask) mask[i] = in;
    cnt += in;
  }
  return cnt;
}

// Gauss-Newton fit on the matches with in[i] != 0, from (R, t); the fit replaces them on success
bool refit(const Cam& cam, const double* pts, long n, const uint8_t* in, double* R, double* t) {
  std::vector<double> part((size_t)kLanes * kSums);
  double col[kLanes], sums[kSums], fR[9], fT[3];
  memcpy(fR, R, sizeof(fR));
  memcpy(fT, t, sizeof(fT));
  for (int it = 0; it < kGnIters; ++it) {
    std::fill(part.begin(), part.end(), 0.0);
    for (long i = 0; i < n; ++i) if (in[i]) accum27(cam, fR, fT, pts + 8 * i, pts[8 * i + 3], pts[8 * i + 4], &part[(size_t)(i % kLanes) * kSums]);
    for (int q = 0; q < kSums; ++q) {
      for (int k = 0; k < kLanes; ++k) col[k] = part[(size_t)k * kSums + q];
      sums[q] = tree(col);
    }
    if (!gn_step(sums, fR, fT)) return false;
  }
  memcpy(R, fR, sizeof(fR));
  memcpy(t, fT, sizeof(fT));
  return true;
}

}  // namespace

extern "C" int loftr_p3p(const double* X, const double* bearings, double* R_out, double* t_out, int* n_solutions) {
  if (!X || !bearings || !R_out || !t_out || !n_solutions) return LOFTR_ERR_BAD_ARG;
  double f[9];
  for (int i = 0; i < 3; ++i) {                                  // unit bearings, whatever the caller's scale
    const double* b = bearings + 3 * i;
    const double n = sqrt(dot3(b, b));
    for (int k = 0; k < 3; ++k) f[3 * i + k] = n > 0 ? b[k] / n : 0.0;
  }
  double poses[kPose * kSol];
  const int ns = p3p(X, f, poses, table());
  for (int k = 0; k < ns; ++k) {
    memcpy(R_out + 9 * k, poses + kPose * k, sizeof(double) * 9);
    memcpy(t_out + 3 * k, poses + kPose * k + 9, sizeof(double) * 3);
  }
  *n_solutions = ns;
  return LOFTR_OK;
}

extern "C" int loftr_estimate_absolute_pose(const float* pts3d, const float* kpts, long M, const float* K, float thresh_px, float conf,
                                            unsigned seed, float* R_out, float* t_out, uint8_t* inliers_out, long* n_inliers) {
  if (!R_out || !t_out || !n_inliers || !K || M < 0 || (M > 0 && (!pts3d || !kpts || !inliers_out))) return LOFTR_ERR_BAD_ARG;
  *n_inliers = -1;
  for (int i = 0; i < 9; ++i) R_out[i] = 0.f;
  for (int i = 0; i < 3; ++i) t_out[i] = 0.f;
  if (M > 0) memset(inliers_out, 0, (size_t)M);
  if (M < 3) return LOFTR_OK;
  const Cam cam = cam_from_K(K);
  std::vector<double> pts(8 * (size_t)M);
  for (long i = 0; i < M; ++i) {
    double* q = &pts[8 * i];
    q[0] = pts3d[3 * i]; q[1] = pts3d[3 * i + 1]; q[2] = pts3d[3 * i + 2]; q[3] = kpts[2 * i]; q[4] = kpts[2 * i + 1];
    bearing(cam, q[3], q[4], q + 5);
  }
  const double thr2 = (double)thresh_px * (double)thresh_px;
  const PolarTable& tab = table();
  Rng rng(seed);
  double bestR[9] = {0}, bestT[3] = {0};
  long best = 0;
  int iters = kIters;
  for (int it = 0; it < iters; ++it) {
    int idx[kSample];
    draw_sample(rng, M, kSample, idx);
    double X[9], f[9], poses[kPose * kSol];
    for (int k = 0; k < 3; ++k) for (int c = 0; c < 3; ++c) { X[3 * k + c] = pts[8 * (size_t)idx[k] + c]; f[3 * k + c] = pts[8 * (size_t)idx[k] + 5 + c]; }
    const int ns = p3p(X, f, poses, tab);
    for (int sol = 0; sol < ns; ++sol) {
      const double *Rs = poses + kPose * sol, *ts = Rs + 9;
      const long cnt = score(cam, Rs, ts, pts.data(), M, thr2, nullptr);
      if (cnt > best) {
        best = cnt;
        memcpy(bestR, Rs, sizeof(bestR));
        memcpy(bestT, ts, sizeof(bestT));
        iters = adaptive_iters(cnt, M, kSample, conf, it, iters);
      }
    }
  }
  if (best < 3) return LOFTR_OK;
  std::vector<uint8_t> in(M), in2(M);
  score(cam, bestR, bestT, pts.data(), M, thr2, in.data());
  // Gauss-Newton refit on the current model's inliers, adopted when it keeps at least as many; repeated while it strictly gains some
  for (int round = 0; round < kRefitRounds; ++round) {
    double fR[9], fT[3];
    memcpy(fR, bestR, sizeof(fR));
    memcpy(fT, bestT, sizeof(fT));
    if (best < 4 || !refit(cam, pts.data(), M, in.data(), fR, fT)) break;
    const long cnt = score(cam, fR, fT, pts.data(), M, thr2, in2.data());
    if (cnt < best) break;
    const bool grew = cnt > best;
    best = cnt;
    memcpy(bestR, fR, sizeof(bestR));
    memcpy(bestT, fT, sizeof(bestT));
    in.swap(in2);
    if (!grew) break;
  }
  for (int i = 0; i < 9; ++i) R_out[i] = (float)bestR[i];
  for (int i = 0; i < 3; ++i) t_out[i] = (float)bestT[i];
  memcpy(inliers_out, in.data(), (size_t)M);
  *n_inliers = best;
  return LOFTR_OK;
}
