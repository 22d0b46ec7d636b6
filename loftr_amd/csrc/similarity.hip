// 3D similarity / rigid transform between two point sets, dst = s R src + t: the closed form of Kabsch / Umeyama inside RANSAC and as
// the refit (host code, double precision).  What georegistration of a reconstruction against surveyed camera centres and 3D-3D
// registration of two depth-lifted point sets need (Open3D's registration_ransac_based_on_correspondence, COLMAP's model_aligner;
// neither library is in this image, so this is a restatement of the published algorithm, NOT of their source):
//   * minimal sample: 3 correspondences, one model (similarity_core.h: minimal); collinear or coincident triples on either side, and
//     a scale that is not finite or not positive, give none;
//   * RANSAC with loftr_estimate_pose's sampler (xorshift64*, duplicate rejection), cap (1000), strict `>` adoption and adaptive stop
//     (exponent 3); residual: |s R src + t - dst|^2 in the units of dst;
//   * refit: the same closed form over the inliers of the best hypothesis, adopted when it keeps at least as many inliers and
//     repeated on the adopted model's inliers while the set strictly grows (at most 4 fits), exactly as loftr_estimate_absolute_pose.
// This function DEFINES the result: loftr_estimate_similarity_batched (similarity_gpu.hip) reproduces it bit for bit, which is why all
// the arithmetic lives in similarity_core.h and why the refit's sums have a fixed order (256 strided partials, then a pairwise tree).
// loftr_transform_model_host, which moves a model by such a transform, is at the end.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/loftr_hip.h"
#include "similarity_core.h"

#pragma clang fp contract(off)

namespace {

using namespace simt;

// pts [n,6]: src (3), dst (3)
long score(const double* m, const double* pts, long n, double thr2, uint8_t* mask) {
  long cnt = 0;
  for (long i = 0; i < n; ++i) {
    const bool in = is_inlier(m, pts + kPt * i, thr2);
    if (mask) mask[i] = in;
    cnt += in;
  }
  return cnt;
}

// the nq sums of one refit pass over the correspondences with in[i] != 0: strided partials, then the tree
template <class Accum>
void pass_sums(const double* pts, long n, const uint8_t* in, int nq, double* sums, Accum accum) {
  std::vector<double> part((size_t)kLanes * nq, 0.0);
  double col[kLanes];
  for (long i = 0; i < n; ++i) if (in[i]) accum(pts + kPt * i, &part[(size_t)(i % kLanes) * nq]);
  for (int q = 0; q < nq; ++q) {
    for (int k = 0; k < kLanes; ++k) col[k] = part[(size_t)k * nq + q];
    sums[q] = tree(col);
  }
}

// closed-form fit on the cnt correspondences with in[i] != 0
bool refit(const double* pts, long n, const uint8_t* in, long cnt, int with_scale, double* m) {
  double s1[kSums1], s2[kSums2], mu[6];
  pass_sums(pts, n, in, kSums1, s1, [](const double* q, double* a) { for (int c = 0; c < kSums1; ++c) a[c] = a[c] + q[c]; });
  for (int c = 0; c < 6; ++c) mu[c] = s1[c] / (double)cnt;
  pass_sums(pts, n, in, kSums2, s2, [&](const double* q, double* a) { accum10(mu, mu + 3, q, a); });
  return model_from_moments(s2, s2[9], mu, mu + 3, with_scale, m);
}

}  // namespace

extern "C" int loftr_similarity_minimal(const double* src3, const double* dst3, int with_scale, double* s, double* R, double* t,
                                        int* n_solutions) {
  if (!src3 || !dst3 || !s || !R || !t || !n_solutions) return LOFTR_ERR_BAD_ARG;
  double m[kModel];
  const int ns = minimal(src3, dst3, with_scale != 0, m);
  *s = 0.0;
  for (int i = 0; i < 9; ++i) R[i] = 0.0;
  for (int i = 0; i < 3; ++i) t[i] = 0.0;
  if (ns) {
    *s = m[0];
    memcpy(R, m + 1, sizeof(double) * 9);
    memcpy(t, m + 10, sizeof(double) * 3);
  }
  *n_solutions = ns;
  return LOFTR_OK;
}

extern "C" int loftr_estimate_similarity(const double* src, const double* dst, long M, int with_scale, double thresh, float conf,
                                         unsigned seed, double* s_out, double* R_out, double* t_out, uint8_t* inliers_out, long* n_inliers) {
  if (!s_out || !R_out || !t_out || !n_inliers || M < 0 || (M > 0 && (!src || !dst || !inliers_out))) return LOFTR_ERR_BAD_ARG;
  *n_inliers = -1;
  *s_out = 0.0;
  for (int i = 0; i < 9; ++i) R_out[i] = 0.0;
  for (int i = 0; i < 3; ++i) t_out[i] = 0.0;
  if (M > 0) memset(inliers_out, 0, (size_t)M);
  if (M < 3) return LOFTR_OK;
  with_scale = with_scale != 0;
  std::vector<double> pts(kPt * (size_t)M);
  for (long i = 0; i < M; ++i)
    for (int c = 0; c < 3; ++c) { pts[kPt * i + c] = src[3 * i + c]; pts[kPt * i + 3 + c] = dst[3 * i + c]; }
  const double thr2 = thresh * thresh;
  Rng rng(seed);
  double bestM[kModel] = {0};
  long best = 0;
  int iters = kIters;
  for (int it = 0; it < iters; ++it) {
    int idx[kSample];
    draw_sample(rng, M, kSample, idx);
    double a[9], b[9], m[kModel];
    for (int k = 0; k < 3; ++k) for (int c = 0; c < 3; ++c) { a[3 * k + c] = pts[kPt * (size_t)idx[k] + c]; b[3 * k + c] = pts[kPt * (size_t)idx[k] + 3 + c]; }
    if (!minimal(a, b, with_scale, m)) continue;
    const long cnt = score(m, pts.data(), M, thr2, nullptr);
    if (cnt > best) {
      best = cnt;
      memcpy(bestM, m, sizeof(bestM));
      iters = adaptive_iters(cnt, M, kSample, conf, it, iters);
    }
  }
  if (best < 3) return LOFTR_OK;
  std::vector<uint8_t> in(M), in2(M);
  score(bestM, pts.data(), M, thr2, in.data());
  // refit on the current model's inliers, adopted when it keeps at least as many; repeated while it strictly gains some
  for (int round = 0; round < kRefitRounds; ++round) {
    double fit[kModel];
    if (best < 3 || !refit(pts.data(), M, in.data(), best, with_scale, fit)) break;
    const long cnt = score(fit, pts.data(), M, thr2, in2.data());
    if (cnt < best) break;
    const bool grew = cnt > best;
    best = cnt;
    memcpy(bestM, fit, sizeof(bestM));
    in.swap(in2);
    if (!grew) break;
  }
  *s_out = bestM[0];
  memcpy(R_out, bestM + 1, sizeof(double) * 9);
  memcpy(t_out, bestM + 10, sizeof(double) * 3);
  memcpy(inliers_out, in.data(), (size_t)M);
  *n_inliers = best;
  return LOFTR_OK;
}

extern "C" int loftr_transform_model_host(const float* xyz, long N, const double* T_cam_from_world, const uint8_t* posed, int n_images,
                                          const double* s, const double* R, const double* t, float* xyz_out, double* T_out) {
  if (N < 0 || n_images < 0 || !s || !R || !t) return LOFTR_ERR_BAD_ARG;
  if ((N > 0 && (!xyz || !xyz_out)) || (n_images > 0 && (!T_cam_from_world || !posed || !T_out))) return LOFTR_ERR_BAD_ARG;
  double m[kModel];
  m[0] = *s;
  memcpy(m + 1, R, sizeof(double) * 9);
  memcpy(m + 10, t, sizeof(double) * 3);
  for (long i = 0; i < N; ++i) transform_point(m, xyz + 3 * i, xyz_out + 3 * i);
  for (int i = 0; i < n_images; ++i) {
    if (posed[i]) transform_pose(m, T_cam_from_world + 16 * (size_t)i, T_out + 16 * (size_t)i);
    else if (T_out != T_cam_from_world) memcpy(T_out + 16 * (size_t)i, T_cam_from_world + 16 * (size_t)i, sizeof(double) * 16);   // the input's bits
  }
  return LOFTR_OK;
}
