// Batched homography / fundamental-matrix RANSAC on the GPU: loftr_estimate_geometry (geometry.hip, host code) for every pair of a
// batch, with the same result -- same inlier count, same inlier mask, the matrix equal after the float32 rounding -- for the same
// seed.  The sequence is ransac_gpu.h's (all 1000 minimal samples of a pair drawn up front, solved and scored in parallel, the sequential
// decision replayed on the host over the counts); this file holds the model's kernels:
//   geo_prep_kernel    (thread per match)    fp64 copies of the points pts [M,4] = (x0, y0, x1, y1), m_bids checked;
//   geo_solve_kernel   (thread per sample)   per-sample Hartley normalisation, 9 x 9 Jacobi, for F the cubic: up to 1 (H) / 3 (F)
//                                            unit-norm matrices per sample;
//   GeoScore           the model's inlier test for the shared scorer;
//   geo_refit_kernel   (workgroup per pair)  mask of the best hypothesis, then the host's refit loop: the sums in the host's order
//                                            (thread k = strided partial k, then the pairwise tree in LDS), Jacobi / svd3 in
//                                            thread 0, the refit scored, the adoption rule, again while the inlier set grows;
//                                            mask / matrix / count written.
// Identical decisions need identical arithmetic: every formula is geometry_core.h's, compiled from the same text as the host
// estimator's, fp64 without FMA contraction.  Plain C++ throughout; all stores are ordinary vector stores.
#include <math.h>
#include "geometry_core.h"
#include "ransac_gpu.h"

#pragma clang fp contract(off)

namespace {

using namespace geo;

constexpr Problem problem(int model) { return {model == 0 ? 4 : 7, model == 0 ? 1 : 3, 9, 4}; }

// grid ceil(M / 256) x 256: pts [M,4] = (x0, y0, x1, y1) in fp64, m_bids checked
__global__ void geo_prep_kernel(const float* __restrict__ k0, const float* __restrict__ k1, const long* __restrict__ m_bids, long M, int P,
                                double* __restrict__ pts, int* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  if (checked_bid(m_bids, i, P, status) < 0) return;
  pts[4 * i] = k0[2 * i]; pts[4 * i + 1] = k0[2 * i + 1]; pts[4 * i + 2] = k1[2 * i]; pts[4 * i + 3] = k1[2 * i + 1];
}

// one minimal sample per thread -> mats [P, kIters * kSol, 9] (ransac_gpu.h: sample_slots, append_hypotheses)
template <int kModel>
__global__ void __launch_bounds__(64) geo_solve_kernel(const double* __restrict__ pts, const long* __restrict__ start,
                                                       const int* __restrict__ idx, int P, PolarTable tab, double* __restrict__ mats,
                                                       int* __restrict__ counts, int* __restrict__ hyp, int* __restrict__ n_hyp,
                                                       const int* __restrict__ status) {
  constexpr int s = problem(kModel).s, kSol = problem(kModel).sol, kHyp = kIters * kSol;
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int p, it;
  if (!sample_slots<kSol>(g, P, s, start, status, counts, &p, &it)) return;
  const double* q = pts + 4 * start[p];
  double x0[7], y0[7], x1[7], y1[7];
  for (int k = 0; k < s; ++k) {
    const long i = idx[g * s + k];
    x0[k] = q[4 * i]; y0[k] = q[4 * i + 1]; x1[k] = q[4 * i + 2]; y1[k] = q[4 * i + 3];
  }
  double m[9 * kSol];
  const int ns = solve_minimal(kModel, x0, y0, x1, y1, m, tab);
  double* out = mats + ((long)p * kHyp + it * kSol) * 9;
  for (int k = 0; k < 9 * ns; ++k) out[k] = m[k];
  append_hypotheses<kSol>(p, it, ns, hyp, n_hyp);
}

template <int kModel>
struct GeoScore {                            // ransac_score_kernel's model
  static constexpr int kSol = problem(kModel).sol, kModelSize = 9, kPt = 4, kTilePt = 4;
  typedef double Params;                     // the squared threshold
  typedef double Ctx;
  static __device__ Ctx context(Params thr2, int) { return thr2; }
  static __device__ bool is_inlier(Ctx thr2, const double* m, const double* q) { return geo::is_inlier(kModel, m, q[0], q[1], q[2], q[3], thr2); }
};

// grid P x kLanes: refit + final.  Pairs without a model (best[p] < 0): n_inliers = -1, matrix and mask 0.
template <int kModel>
__global__ void __launch_bounds__(kLanes) geo_refit_kernel(const double* __restrict__ pts, const long* __restrict__ start, double thr2,
                                                          const double* __restrict__ mats, const int* __restrict__ best,
                                                          uint8_t* __restrict__ bits, float* __restrict__ mat_out,
                                                          uint8_t* __restrict__ mask, long* __restrict__ n_inliers) {
  constexpr int kHyp = kIters * (kModel == 0 ? 1 : 3);
  __shared__ double red[kRefitChunk][kLanes];
  __shared__ double sBest[9], sFit[9], sums[45];
  __shared__ int cnt[2], fitted;
  const int p = blockIdx.x, tid = threadIdx.x;
  const long s0 = start[p], n = pair_count(start, p);
  const int b = best[p];
  if (b < 0) {                                                            // (uniform over the block)
    if (tid == 0) n_inliers[p] = -1;
    if (tid < 9) mat_out[9 * (long)p + tid] = 0.f;
    for (long j = tid; j < n; j += kLanes) mask[s0 + j] = 0;
    return;
  }
  if (tid < 9) sBest[tid] = mats[((long)p * kHyp + b) * 9 + tid];
  if (tid < 2) cnt[tid] = 0;
  if (tid == 0) fitted = 0;
  __syncthreads();
  const double* q = pts + 4 * s0;
  // bit 0: inlier of the current model, first the best hypothesis (thread k owns the matches j = k (mod kLanes) in every pass below)
  int c = 0;
  for (long j = tid; j < n; j += kLanes) {
    const bool in = is_inlier(kModel, sBest, q[4 * j], q[4 * j + 1], q[4 * j + 2], q[4 * j + 3], thr2);
    bits[s0 + j] = (uint8_t)in;
    c += in;
  }
  if (c) atomicAdd(&cnt[0], c);
  __syncthreads();
  int cur = cnt[0];                                                       // inliers of the current model sBest (bit 0 of bits)
  for (int round = 0; round < kRefitRounds; ++round) {                    // geometry.hip's refit loop, sum for sum; every exit is uniform
    if (kModel == 1 && cur < 8) break;
    double a[kRefitChunk];
    for (int k = 0; k < 4; ++k) a[k] = 0.0;
    for (long j = tid; j < n; j += kLanes) if (bits[s0 + j] & 1) for (int k = 0; k < 4; ++k) a[k] += q[4 * j + k];
    block_tree<4>(red, a, sums);
    double cen[4];
    for (int k = 0; k < 4; ++k) cen[k] = sums[k] / (double)cur;
    a[0] = 0.0; a[1] = 0.0;
    for (long j = tid; j < n; j += kLanes) if (bits[s0 + j] & 1) {
      const double dx0 = q[4 * j] - cen[0], dy0 = q[4 * j + 1] - cen[1], dx1 = q[4 * j + 2] - cen[2], dy1 = q[4 * j + 3] - cen[3];
      a[0] += sqrt(dx0 * dx0 + dy0 * dy0);
      a[1] += sqrt(dx1 * dx1 + dy1 * dy1);
    }
    block_tree<2>(red, a, sums);
    Norm n0, n1;
    const bool ok0 = make_norm(cen[0], cen[1], sums[0], (double)cur, &n0), ok1 = make_norm(cen[2], cen[3], sums[1], (double)cur, &n1);
    if (!(ok0 && ok1)) break;
    double acc[45];
    for (int k = 0; k < 45; ++k) acc[k] = 0.0;
    for (long j = tid; j < n; j += kLanes) if (bits[s0 + j] & 1)
      accum45(kModel, (q[4 * j] - n0.cx) * n0.s, (q[4 * j + 1] - n0.cy) * n0.s, (q[4 * j + 2] - n1.cx) * n1.s, (q[4 * j + 3] - n1.cy) * n1.s, acc);
    for (int ch = 0; ch < 45; ch += kRefitChunk) block_tree<kRefitChunk>(red, acc + ch, sums + ch);
    if (tid == 0) {
      double fit[9], total[45];
      for (int k = 0; k < 45; ++k) total[k] = sums[k];
      const bool ok = refit_solve(kModel, total, n0, n1, fit);
      fitted = ok;
      cnt[1] = 0;
      if (ok) for (int k = 0; k < 9; ++k) sFit[k] = fit[k];
    }
    __syncthreads();
    if (!fitted) break;
    c = 0;                                                                // bit 1: inlier of the refit
    for (long j = tid; j < n; j += kLanes) {
      const bool in = is_inlier(kModel, sFit, q[4 * j], q[4 * j + 1], q[4 * j + 2], q[4 * j + 3], thr2);
      bits[s0 + j] = (uint8_t)((bits[s0 + j] & 1) | (in << 1));
      c += in;
    }
    if (c) atomicAdd(&cnt[1], c);
    __syncthreads();
    const int nc = cnt[1];
    if (nc < cur) break;                                                  // the adoption rule: a refit that loses inliers is dropped
    if (tid < 9) sBest[tid] = sFit[tid];
    for (long j = tid; j < n; j += kLanes) bits[s0 + j] >>= 1;
    const bool grew = nc > cur;
    cur = nc;
    __syncthreads();
    if (!grew) break;                                                     // another fit only over a strictly larger inlier set
  }
  if (tid == 0) {
    double m[9];
    for (int k = 0; k < 9; ++k) m[k] = sBest[k];
    output_sign(kModel, m);
    for (int k = 0; k < 9; ++k) mat_out[9 * (long)p + k] = (float)m[k];
    n_inliers[p] = cur;
  }
  for (long j = tid; j < n; j += kLanes) mask[s0 + j] = bits[s0 + j] & 1;
}

template <int kModel>
int run_model(const float* k0, const float* k1, const long* m_bids, long M, int P, float thresh_px, float conf, unsigned seed, float* mat_out,
              uint8_t* inliers_out, long* n_inliers, const Layout& L, const Workspace& W, hipStream_t s) {
  const double thr2 = (double)thresh_px * (double)thresh_px;
  static const PolarTable tab = polar_table<3>();
  return run<problem(kModel).s>(
      m_bids, M, P, problem(kModel), conf, seed, L, W, s,
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(geo_prep_kernel, g, b, 0, s, k0, k1, m_bids, M, P, W.pts, W.status); },
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(geo_solve_kernel<kModel>, g, b, 0, s, W.pts, W.start, W.idx, P, tab, W.models, W.counts, W.hyp, W.n_hyp, W.status); },
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(ransac_score_kernel<GeoScore<kModel>>, g, b, 0, s, W.pts, W.start, thr2, W.models, W.hyp, W.n_hyp, W.counts, W.status); },
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(geo_refit_kernel<kModel>, g, b, 0, s, W.pts, W.start, thr2, W.models, W.best, W.bits, mat_out, inliers_out, n_inliers); });
}

}  // namespace

extern "C" size_t loftr_estimate_geometry_batched_workspace_bytes(long M, int P, int model) {
  if (M < 0 || P < 0 || (model != 0 && model != 1)) return 0;
  return layout(M, P, problem(model)).total;
}

extern "C" int loftr_estimate_geometry_batched(const float* mkpts0_f, const float* mkpts1_f, const long* m_bids, long M, int P, int model,
                                               float thresh_px, float conf, unsigned seed, float* mat_out, uint8_t* inliers_out,
                                               long* n_inliers, void* ws, size_t ws_bytes, void* stream) {
  LOFTR_CHECK_ARG(M >= 0 && P >= 0 && (model == 0 || model == 1));
  if (P == 0) return M == 0 ? LOFTR_OK : LOFTR_ERR_BAD_ARG;             // every pair id would be out of range
  LOFTR_CHECK_ARG(mat_out && n_inliers && ws);
  LOFTR_CHECK_ARG(M == 0 || (mkpts0_f && mkpts1_f && m_bids && inliers_out));
  if (too_large(M, P)) return LOFTR_ERR_UNSUPPORTED;
  const Layout L = layout(M, P, problem(model));
  if (ws_bytes < L.total) return LOFTR_ERR_WORKSPACE;
  const Workspace W = workspace(ws, L);
  return model == 0 ? run_model<0>(mkpts0_f, mkpts1_f, m_bids, M, P, thresh_px, conf, seed, mat_out, inliers_out, n_inliers, L, W, (hipStream_t)stream)
                    : run_model<1>(mkpts0_f, mkpts1_f, m_bids, M, P, thresh_px, conf, seed, mat_out, inliers_out, n_inliers, L, W, (hipStream_t)stream);
}
