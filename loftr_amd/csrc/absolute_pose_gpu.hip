// Batched absolute pose (P3P RANSAC + Gauss-Newton refit) on the GPU: loftr_estimate_absolute_pose (absolute_pose.hip, host code) for
// every pair of a batch, with the same result -- same inlier count, same inlier mask, R and t equal after the float32 rounding -- for
// the same seed.  The sequence is ransac_gpu.h's (all 1000 minimal samples of a pair drawn up front, solved and scored in parallel, the
// sequential decision replayed on the host over the counts); this file holds the model's kernels:
//   abs_prep_kernel    (thread per match)    fp64 world point, pixel and unit bearing of every match, m_bids checked;
//   abs_solve_kernel   (thread per sample)   P3P: up to 4 poses per sample;
//   AbsScore           the model's inlier test for the shared scorer;
//   abs_refit_kernel   (workgroup per pair)  mask of the best hypothesis, then the host's refit loop: the Gauss-Newton sums in the
//                                            host's order (thread k = strided partial k, then the pairwise tree in LDS), the 6 x 6
//                                            solve in thread 0, the fit scored, the adoption rule, again while the inlier set grows;
//                                            mask / pose / count written.
// Identical decisions need identical arithmetic: every formula is absolute_pose_core.h's, compiled from the same text as the host
// estimator's, fp64 without FMA contraction.  loftr_lift_keypoints (the first half of the reference's warp_kpts, fp32) is at the end.
// Plain C++ throughout; all stores are ordinary vector stores.
#include <math.h>
#include "absolute_pose_core.h"
#include "ransac_gpu.h"

#pragma clang fp contract(off)

namespace {

using namespace absp;

constexpr int kHyp = kIters * kSol;          // hypothesis slots per pair
constexpr int kPt = 8;                       // doubles per match: world point (3), pixel (2), unit bearing (3)
constexpr Problem kProblem = {kSample, kSol, kPose, kPt};

// grid ceil(M / 256) x 256: pts [M,8] in fp64, m_bids checked
__global__ void abs_prep_kernel(const float* __restrict__ pts3d, const float* __restrict__ kpts, const long* __restrict__ m_bids, long M,
                                const float* __restrict__ K, int P, double* __restrict__ pts, int* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const long b = checked_bid(m_bids, i, P, status);
  if (b < 0) return;
  const Cam cam = cam_from_K(K + 9 * b);
  double* q = pts + kPt * i;
  double f[3];
  const double u = kpts[2 * i], v = kpts[2 * i + 1];
  bearing(cam, u, v, f);
  q[0] = pts3d[3 * i]; q[1] = pts3d[3 * i + 1]; q[2] = pts3d[3 * i + 2]; q[3] = u; q[4] = v; q[5] = f[0]; q[6] = f[1]; q[7] = f[2];
}

// one minimal sample per thread -> poses [P, kHyp, 12] (ransac_gpu.h: sample_slots, append_hypotheses)
__global__ void __launch_bounds__(64) abs_solve_kernel(const double* __restrict__ pts, const long* __restrict__ start,
                                                       const int* __restrict__ idx, int P, PolarTable tab, double* __restrict__ poses,
                                                       int* __restrict__ counts, int* __restrict__ hyp, int* __restrict__ n_hyp,
                                                       const int* __restrict__ status) {
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int p, it;
  if (!sample_slots<kSol>(g, P, kSample, start, status, counts, &p, &it)) return;
  const double* q = pts + kPt * start[p];
  double X[9], f[9];
  for (int k = 0; k < 3; ++k) {
    const long i = idx[g * 3 + k];
    for (int c = 0; c < 3; ++c) { X[3 * k + c] = q[kPt * i + c]; f[3 * k + c] = q[kPt * i + 5 + c]; }
  }
  const int ns = p3p(X, f, poses + ((long)p * kHyp + it * kSol) * kPose, tab);   // the sample's kSol slots, filled in solver order
  append_hypotheses<kSol>(p, it, ns, hyp, n_hyp);
}

struct AbsScore {                            // ransac_score_kernel's model; the tile holds world point and pixel
  static constexpr int kSol = absp::kSol, kModelSize = kPose, kPt = ::kPt, kTilePt = 5;
  struct Params { const float* K; double thr2; };
  struct Ctx { Cam cam; double thr2; };
  static __device__ Ctx context(const Params& a, int p) { return {cam_from_K(a.K + 9 * (long)p), a.thr2}; }
  static __device__ bool is_inlier(const Ctx& c, const double* m, const double* q) { return absp::is_inlier(c.cam, m, m + 9, q, q[3], q[4], c.thr2); }
};

// grid P x kLanes: refit + final.  Pairs without a model (best[p] < 0): n_inliers = -1, pose and mask 0.
__global__ void __launch_bounds__(kLanes) abs_refit_kernel(const double* __restrict__ pts, const long* __restrict__ start,
                                                          const float* __restrict__ K, double thr2, const double* __restrict__ poses,
                                                          const int* __restrict__ best, uint8_t* __restrict__ bits, float* __restrict__ R_out,
                                                          float* __restrict__ t_out, uint8_t* __restrict__ mask, long* __restrict__ n_inliers) {
  __shared__ double red[kRefitChunk][kLanes];
  __shared__ double sBest[kPose], sFit[kPose], sums[kSums];
  __shared__ int cnt[2], fitted;
  const int p = blockIdx.x, tid = threadIdx.x;
  const long s0 = start[p], n = pair_count(start, p);
  const int b = best[p];
  if (b < 0) {                                                            // (uniform over the block)
    if (tid == 0) n_inliers[p] = -1;
    if (tid < 9) R_out[9 * (long)p + tid] = 0.f;
    if (tid < 3) t_out[3 * (long)p + tid] = 0.f;
    for (long j = tid; j < n; j += kLanes) mask[s0 + j] = 0;
    return;
  }
  const Cam cam = cam_from_K(K + 9 * (long)p);
  if (tid < kPose) sBest[tid] = poses[((long)p * kHyp + b) * kPose + tid];
  if (tid < 2) cnt[tid] = 0;
  if (tid == 0) fitted = 0;
  __syncthreads();
  const double* q = pts + kPt * s0;
  // bit 0: inlier of the current model, first the best hypothesis (thread k owns the matches j = k (mod kLanes) in every pass below)
  int c = 0;
  for (long j = tid; j < n; j += kLanes) {
    const bool in = is_inlier(cam, sBest, sBest + 9, q + kPt * j, q[kPt * j + 3], q[kPt * j + 4], thr2);
    bits[s0 + j] = (uint8_t)in;
    c += in;
  }
  if (c) atomicAdd(&cnt[0], c);
  __syncthreads();
  int cur = cnt[0];                                                       // inliers of the current model sBest (bit 0 of bits)
  for (int round = 0; round < kRefitRounds; ++round) {                    // absolute_pose.hip's refit loop, sum for sum; every exit is uniform
    if (cur < 4) break;
    if (tid < kPose) sFit[tid] = sBest[tid];
    if (tid == 0) { fitted = 1; cnt[1] = 0; }
    __syncthreads();
    for (int it = 0; it < kGnIters; ++it) {
      double a[kSums];
      for (int k = 0; k < kSums; ++k) a[k] = 0.0;
      for (long j = tid; j < n; j += kLanes) if (bits[s0 + j] & 1) accum27(cam, sFit, sFit + 9, q + kPt * j, q[kPt * j + 3], q[kPt * j + 4], a);
      for (int ch = 0; ch < kSums; ch += kRefitChunk) block_tree<kRefitChunk>(red, a + ch, sums + ch);
      if (tid == 0) {
        double total[kSums], R[9], t[3];
        for (int k = 0; k < kSums; ++k) total[k] = sums[k];
        for (int k = 0; k < 9; ++k) R[k] = sFit[k];
        for (int k = 0; k < 3; ++k) t[k] = sFit[9 + k];
        const bool ok = gn_step(total, R, t);
        fitted = ok;
        if (ok) { for (int k = 0; k < 9; ++k) sFit[k] = R[k]; for (int k = 0; k < 3; ++k) sFit[9 + k] = t[k]; }
      }
      __syncthreads();
      if (!fitted) break;
    }
    if (!fitted) break;
    c = 0;                                                                // bit 1: inlier of the refit
    for (long j = tid; j < n; j += kLanes) {
      const bool in = is_inlier(cam, sFit, sFit + 9, q + kPt * j, q[kPt * j + 3], q[kPt * j + 4], thr2);
      bits[s0 + j] = (uint8_t)((bits[s0 + j] & 1) | (in << 1));
      c += in;
    }
    if (c) atomicAdd(&cnt[1], c);
    __syncthreads();
    const int nc = cnt[1];
    if (nc < cur) break;                                                  // the adoption rule: a refit that loses inliers is dropped
    __syncthreads();                                                      // (every thread has read sBest / cnt[1] before they change)
    if (tid < kPose) sBest[tid] = sFit[tid];
    for (long j = tid; j < n; j += kLanes) bits[s0 + j] >>= 1;
    const bool grew = nc > cur;
    cur = nc;
    __syncthreads();
    if (!grew) break;                                                     // another fit only over a strictly larger inlier set
  }
  if (tid < 9) R_out[9 * (long)p + tid] = (float)sBest[tid];
  if (tid < 3) t_out[3 * (long)p + tid] = (float)sBest[9 + tid];
  if (tid == 0) n_inliers[p] = cur;
  for (long j = tid; j < n; j += kLanes) mask[s0 + j] = bits[s0 + j] & 1;
}

// grid ceil(M / 256) x 256.  fp32 as the reference's warp_kpts; no FMA contraction, so that a float32 restatement of the same
// operations in the same order gives the same bits.
__global__ void LOFTR_NO_PACKED_FP32 lift_keypoints_kernel(const float* __restrict__ kpts, const long* __restrict__ m_bids,
                                                            const float* __restrict__ depth, int dh, int dw, const float* __restrict__ K,
                                                            const float* __restrict__ T, int P, long M, float* __restrict__ out,
                                                            uint8_t* __restrict__ valid) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const long b = m_bids[i];
  const float x = kpts[2 * i], y = kpts[2 * i + 1];
  const float xr = rintf(x), yr = rintf(y);                               // half to even, = torch.round
  float d = 0.f;
  // an out-of-map keypoint (NaN included) or an out-of-range pair id is invalid and reads no depth
  if (b >= 0 && b < P && xr >= 0.f && xr < (float)dw && yr >= 0.f && yr < (float)dh) d = depth[((size_t)b * dh + (size_t)(int)yr) * dw + (size_t)(int)xr];
  float X = 0.f, Y = 0.f, Z = 0.f;
  const bool ok = d != 0.f;                                               // (a NaN depth counts as non-zero, as in the reference)
  if (ok) {
    const float* k = K + 9 * b;
    const float hx = x * d, hy = y * d;
    Y = (hy - k[5] * d) / k[4];
    X = (hx - k[1] * Y - k[2] * d) / k[0];
    Z = d;
    if (T) {
      const float* t = T + 16 * b;
      const float wx = t[0] * X + t[1] * Y + t[2] * Z + t[3], wy = t[4] * X + t[5] * Y + t[6] * Z + t[7], wz = t[8] * X + t[9] * Y + t[10] * Z + t[11];
      X = wx; Y = wy; Z = wz;
    }
  }
  out[3 * i] = X; out[3 * i + 1] = Y; out[3 * i + 2] = Z;
  valid[i] = (uint8_t)ok;
}

}  // namespace

extern "C" size_t loftr_estimate_absolute_pose_batched_workspace_bytes(long M, int P) {
  if (M < 0 || P < 0) return 0;
  return layout(M, P, kProblem).total;
}

extern "C" int loftr_estimate_absolute_pose_batched(const float* pts3d, const float* kpts, const long* m_bids, long M, const float* K, int P,
                                                    float thresh_px, float conf, unsigned seed, float* R_out, float* t_out,
                                                    uint8_t* inliers_out, long* n_inliers, void* ws, size_t ws_bytes, void* stream) {
  LOFTR_CHECK_ARG(M >= 0 && P >= 0);
  if (P == 0) return M == 0 ? LOFTR_OK : LOFTR_ERR_BAD_ARG;             // every pair id would be out of range
  LOFTR_CHECK_ARG(K && R_out && t_out && n_inliers && ws);
  LOFTR_CHECK_ARG(M == 0 || (pts3d && kpts && m_bids && inliers_out));
  if (too_large(M, P)) return LOFTR_ERR_UNSUPPORTED;
  const Layout L = layout(M, P, kProblem);
  if (ws_bytes < L.total) return LOFTR_ERR_WORKSPACE;
  const Workspace W = workspace(ws, L);
  hipStream_t s = (hipStream_t)stream;
  static const PolarTable tab = polar_table<4>();
  const double thr2 = (double)thresh_px * (double)thresh_px;
  const AbsScore::Params prm = {K, thr2};
  return run<kProblem.s>(
      m_bids, M, P, kProblem, conf, seed, L, W, s,
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(abs_prep_kernel, g, b, 0, s, pts3d, kpts, m_bids, M, K, P, W.pts, W.status); },
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(abs_solve_kernel, g, b, 0, s, W.pts, W.start, W.idx, P, tab, W.models, W.counts, W.hyp, W.n_hyp, W.status); },
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(ransac_score_kernel<AbsScore>, g, b, 0, s, W.pts, W.start, prm, W.models, W.hyp, W.n_hyp, W.counts, W.status); },
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(abs_refit_kernel, g, b, 0, s, W.pts, W.start, K, thr2, W.models, W.best, W.bits, R_out, t_out, inliers_out, n_inliers); });
}

extern "C" int loftr_lift_keypoints(const float* kpts, const long* m_bids, long M, const float* depth, int dh, int dw, const float* K,
                                    const float* T, int P, float* pts3d_out, uint8_t* valid_out, void* stream) {
  LOFTR_CHECK_ARG(M >= 0 && P >= 0 && dh >= 0 && dw >= 0);
  if (M == 0) return LOFTR_OK;
  LOFTR_CHECK_ARG(kpts && m_bids && K && pts3d_out && valid_out && P > 0 && (depth || dh == 0 || dw == 0));
  if ((M + 255) / 256 >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(lift_keypoints_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, kpts, m_bids, depth, dh, dw, K, T,
                     P, M, pts3d_out, valid_out);
  LOFTR_CHECK_LAUNCH();
  return LOFTR_OK;
}
