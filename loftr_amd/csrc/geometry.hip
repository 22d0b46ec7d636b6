// Homography and fundamental matrix from matches: minimal solvers inside RANSAC + a least-squares refit (host code, double
// precision).  The uncalibrated counterparts of loftr_estimate_pose (pose.hip): what cv2.findHomography(RANSAC) /
// cv2.findFundamentalMat(FM_RANSAC) are used for on planar pairs (HPatches) and on retrieval pairs without intrinsics.  OpenCV is
// not in this image, so this is a restatement of the published algorithms, NOT of OpenCV's source:
//   * Hartley normalisation (centroid 0, mean distance sqrt 2) of the sample / of the inliers, per image;
//   * homography: 4-point DLT, null vector of the 8 x 9 design matrix (smallest eigenvector of A^T A by cyclic Jacobi); samples with
//     three (nearly) collinear points or with flipped orientation are rejected;
//   * fundamental matrix: 7-point, the two null vectors and the cubic det(a F1 + (1 - a) F2) = 0, its real roots by the Aberth-
//     Ehrlich finder of the five-point solver;
//   * RANSAC with loftr_estimate_pose's sampler (xorshift64*, duplicate rejection), cap (1000) and adaptive stop (exponent = sample
//     size); residuals in pixels: squared forward transfer error (H), squared Sampson distance (F);
//   * a normalised least-squares refit on the inliers of the best hypothesis (rank 2 enforced for F), adopted when it keeps at
//     least as many inliers, and repeated on the adopted model's inliers while the set strictly grows (at most 4 fits): the adaptive
//     stop can end the loop on a hypothesis that holds only part of the inliers, and one fit over that part is not the fit over all.
// This function DEFINES the result: loftr_estimate_geometry_batched (geometry_gpu.hip) reproduces it bit for bit, which is why all
// the arithmetic lives in geometry_core.h and why the refit's sums have a fixed order (256 strided partials, then a pairwise tree).
// PARITY UNPINNED against OpenCV: own sampling sequence, own degeneracy tests.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/loftr_hip.h"
#include "geometry_core.h"

#pragma clang fp contract(off)

namespace {

using namespace geo;

const PolarTable& table() { static const PolarTable t = polar_table<3>(); return t; }

long score(int model, const double* m, const double* pts, long n, double thr2, uint8_t* mask) {
  long cnt = 0;
  for (long i = 0; i < n; ++i) {
    const bool in = is_inlier(model, m, pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], pts[4 * i + 3], thr2);
    if (mask) mask[i] = in;
    cnt += in;
  }
  return cnt;
}

// least-squares fit on the matches with in[i] != 0 (cnt of them)
bool refit(int model, const double* pts, long n, const uint8_t* in, long cnt, double* out) {
  std::vector<double> part((size_t)kLanes * 45);
  double col[kLanes];
  auto reduce = [&](int q, int stride) { for (int k = 0; k < kLanes; ++k) col[k] = part[(size_t)k * stride + q]; return tree(col); };
  // centroids
  std::fill(part.begin(), part.end(), 0.0);
  for (long i = 0; i < n; ++i) if (in[i]) { double* a = &part[(size_t)(i % kLanes) * 4]; for (int q = 0; q < 4; ++q) a[q] += pts[4 * i + q]; }
  double c[4];
  for (int q = 0; q < 4; ++q) c[q] = reduce(q, 4) / (double)cnt;
  // mean distances to them
  std::fill(part.begin(), part.end(), 0.0);
  for (long i = 0; i < n; ++i) if (in[i]) {
    double* a = &part[(size_t)(i % kLanes) * 2];
    const double dx0 = pts[4 * i] - c[0], dy0 = pts[4 * i + 1] - c[1], dx1 = pts[4 * i + 2] - c[2], dy1 = pts[4 * i + 3] - c[3];
    a[0] += sqrt(dx0 * dx0 + dy0 * dy0);
    a[1] += sqrt(dx1 * dx1 + dy1 * dy1);
  }
  Norm n0, n1;
  const double sd0 = reduce(0, 2), sd1 = reduce(1, 2);
  if (!make_norm(c[0], c[1], sd0, (double)cnt, &n0) || !make_norm(c[2], c[3], sd1, (double)cnt, &n1)) return false;
  // normal matrix
  std::fill(part.begin(), part.end(), 0.0);
  for (long i = 0; i < n; ++i) if (in[i])
    accum45(model, (pts[4 * i] - n0.cx) * n0.s, (pts[4 * i + 1] - n0.cy) * n0.s, (pts[4 * i + 2] - n1.cx) * n1.s, (pts[4 * i + 3] - n1.cy) * n1.s,
            &part[(size_t)(i % kLanes) * 45]);
  double acc[45];
  for (int q = 0; q < 45; ++q) acc[q] = reduce(q, 45);
  return refit_solve(model, acc, n0, n1, out);
}

}  // namespace

extern "C" int loftr_geometry_minimal(const double* p0, const double* p1, int model, double* mats_out, int* n_solutions) {
  if (!p0 || !p1 || !mats_out || !n_solutions || (model != 0 && model != 1)) return LOFTR_ERR_BAD_ARG;
  const int s = sample_size(model);
  double x0[7], y0[7], x1[7], y1[7];
  for (int i = 0; i < s; ++i) { x0[i] = p0[2 * i]; y0[i] = p0[2 * i + 1]; x1[i] = p1[2 * i]; y1[i] = p1[2 * i + 1]; }
  double mats[27];
  const int ns = solve_minimal(model, x0, y0, x1, y1, mats, table());
  for (int k = 0; k < ns; ++k) output_sign(model, mats + 9 * k);
  memcpy(mats_out, mats, sizeof(double) * 9 * ns);
  *n_solutions = ns;
  return LOFTR_OK;
}

extern "C" int loftr_estimate_geometry(const float* kpts0, const float* kpts1, long M, int model, float thresh_px, float conf,
                                       unsigned seed, float* mat_out, uint8_t* inliers_out, long* n_inliers) {
  if (!kpts0 || !kpts1 || !mat_out || !inliers_out || !n_inliers || M < 0 || (model != 0 && model != 1)) return LOFTR_ERR_BAD_ARG;
  *n_inliers = -1;
  const int s = sample_size(model);
  if (M < s) return LOFTR_OK;
  std::vector<double> pts(4 * (size_t)M);
  for (long i = 0; i < M; ++i) { pts[4 * i] = kpts0[2 * i]; pts[4 * i + 1] = kpts0[2 * i + 1]; pts[4 * i + 2] = kpts1[2 * i]; pts[4 * i + 3] = kpts1[2 * i + 1]; }
  const double thr2 = (double)thresh_px * (double)thresh_px;
  const PolarTable& tab = table();
  Rng rng(seed);
  double bestM[9] = {0};
  long best = 0;
  int iters = kIters;
  for (int it = 0; it < iters; ++it) {
    int idx[kMaxSample];
    draw_sample(rng, M, s, idx);
    double x0[7], y0[7], x1[7], y1[7], mats[27];
    for (int k = 0; k < s; ++k) { x0[k] = pts[4 * idx[k]]; y0[k] = pts[4 * idx[k] + 1]; x1[k] = pts[4 * idx[k] + 2]; y1[k] = pts[4 * idx[k] + 3]; }
    const int ns = solve_minimal(model, x0, y0, x1, y1, mats, tab);
    for (int sol = 0; sol < ns; ++sol) {
      const long cnt = score(model, mats + 9 * sol, pts.data(), M, thr2, nullptr);
      if (cnt > best) {
        best = cnt;
        memcpy(bestM, mats + 9 * sol, sizeof(bestM));
        iters = adaptive_iters(cnt, M, s, conf, it, iters);
      }
    }
  }
  if (best < s) return LOFTR_OK;
  std::vector<uint8_t> in(M), in2(M);
  score(model, bestM, pts.data(), M, thr2, in.data());
  // least-squares refit on the current model's inliers, adopted when it keeps at least as many; repeated while it strictly gains some
  for (int round = 0; round < kRefitRounds; ++round) {
    double fit[9];
    if ((model == 1 && best < 8) || !refit(model, pts.data(), M, in.data(), best, fit)) break;
    const long cnt = score(model, fit, pts.data(), M, thr2, in2.data());
    if (cnt < best) break;
    const bool grew = cnt > best;
    best = cnt;
    memcpy(bestM, fit, sizeof(bestM));
    in.swap(in2);
    if (!grew) break;
  }
  output_sign(model, bestM);
  for (int i = 0; i < 9; ++i) mat_out[i] = (float)bestM[i];
  memcpy(inliers_out, in.data(), (size_t)M);
  *n_inliers = best;
  return LOFTR_OK;
}
