// Batched relative pose on the GPU: loftr_estimate_pose (pose.hip, host code) for every pair of a batch, with the same result -- same
// inlier count, same inlier mask, R and t equal after the float32 rounding -- for the same seed.
//
// The sequence is ransac_gpu.h's (all 1000 minimal samples of a pair drawn up front, solved and scored in parallel, the sequential
// decision replayed on the host over the counts); this file holds the model's kernels:
//   pose_prep_kernel    (thread per match)  pixels -> normalised points pts [M,4] = (x0, y0, x1, y1) in fp64, m_bids checked;
//   pose_solve_kernel   (thread per sample) Nister's five-point solver -> up to 10 unit-norm E per sample;
//   PoseScore           Sampson inlier counts with the host's expression and the pair's threshold;
//   pose_recover_kernel (block per pair)    RANSAC mask of the best E, svd3 + sign fixes + four (R, t) candidates, cheirality (4x4 Jacobi
//                                           triangulation per inlier), first maximum wins.
// Identical decisions need identical arithmetic: every formula is pose_core.h's, compiled from the same text as the host estimator's,
// fp64 without FMA contraction (the x86 host path has no FMA), IEEE division / sqrt (correctly rounded on both sides).
#include <math.h>
#include "pose_core.h"
#include "ransac_gpu.h"

#pragma clang fp contract(off)

namespace {

using namespace pose;

constexpr int kHyp = kIters * kSol;          // hypothesis slots per pair
constexpr Problem kProblem = {kSample, kSol, 9, 4};

// grid ceil(M / 256) x 256: normalised points q = (kpts - [cx, cy]) / [fx, fy] in fp64, m_bids checked
__global__ void pose_prep_kernel(const float* __restrict__ k0, const float* __restrict__ k1, const long* __restrict__ m_bids, long M,
                                 const float* __restrict__ K0, const float* __restrict__ K1, int P, double* __restrict__ pts,
                                 int* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const long b = checked_bid(m_bids, i, P, status);
  if (b < 0) return;
  const float* A = K0 + 9 * b;
  const float* B = K1 + 9 * b;
  pts[4 * i] = ((double)k0[2 * i] - A[2]) / A[0]; pts[4 * i + 1] = ((double)k0[2 * i + 1] - A[5]) / A[4];
  pts[4 * i + 2] = ((double)k1[2 * i] - B[2]) / B[0]; pts[4 * i + 3] = ((double)k1[2 * i + 1] - B[5]) / B[4];
}

// one minimal sample per thread -> Es [P, kHyp, 9] (ransac_gpu.h: sample_slots, append_hypotheses)
__global__ void __launch_bounds__(64) pose_solve_kernel(const double* __restrict__ pts, const long* __restrict__ start,
                                                        const int* __restrict__ idx, int P, PolarTable tab, double* __restrict__ Es,
                                                        int* __restrict__ counts, int* __restrict__ hyp, int* __restrict__ n_hyp,
                                                        const int* __restrict__ status) {
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int p, it;
  if (!sample_slots<kSol>(g, P, kSample, start, status, counts, &p, &it)) return;
  const double* q = pts + 4 * start[p];
  int d[kSample];
  for (int k = 0; k < kSample; ++k) d[k] = idx[g * kSample + k];
  const int ns = five_point(q, q + 2, 4, d, kSample, Es + ((long)p * kHyp + it * kSol) * 9, tab);
  append_hypotheses<kSol>(p, it, ns, hyp, n_hyp);
}

struct PoseScore {                           // ransac_score_kernel's model
  static constexpr int kSol = pose::kSol, kModelSize = 9, kPt = 4, kTilePt = 4;
  struct Params { const float *K0, *K1; float thresh_px; };
  typedef double Ctx;                        // the pair's squared threshold
  static __device__ Ctx context(const Params& a, int p) { return sampson_thr2(a.thresh_px, a.K0 + 9 * (long)p, a.K1 + 9 * (long)p); }
  static __device__ bool is_inlier(Ctx thr2, const double* E, const double* q) { return sampson_in(E, q[0], q[1], q[2], q[3], thr2); }
};

// grid P x 256: the RANSAC mask of the selected hypothesis, the four (R, t) of its E and the cheirality vote.  Outputs of a
// pair without a pose (best[p] < 0, or no point in front of both cameras): n_inliers = -1, R = t = 0, mask 0.
__global__ void __launch_bounds__(kLanes) pose_recover_kernel(const double* __restrict__ pts, const long* __restrict__ start,
                                                             PoseScore::Params prm, const double* __restrict__ Es,
                                                             const int* __restrict__ best, uint8_t* __restrict__ bits,
                                                             float* __restrict__ R_out, float* __restrict__ t_out,
                                                             uint8_t* __restrict__ mask, long* __restrict__ n_inliers) {
  __shared__ double sR[4][9], st[4][3], sE[9];
  __shared__ int votes[4], pick[2];
  const int p = blockIdx.x, tid = threadIdx.x;
  const long s0 = start[p], n = pair_count(start, p);
  const int b = best[p];
  if (tid < 4) votes[tid] = 0;
  if (b >= 0 && tid < 9) sE[tid] = Es[((long)p * kHyp + b) * 9 + tid];
  __syncthreads();
  if (b >= 0 && tid == 0) pose_candidates(sE, sR, st);
  __syncthreads();
  if (b >= 0) {
    const double t2 = PoseScore::context(prm, p);
    int v[4] = {0, 0, 0, 0};
    for (long j = tid; j < n; j += kLanes) {
      const long i = s0 + j;
      const double x0 = pts[4 * i], y0 = pts[4 * i + 1], x1 = pts[4 * i + 2], y1 = pts[4 * i + 3];
      unsigned f = 0;
      if (sampson_in(sE, x0, y0, x1, y1, t2))
        for (int c = 0; c < 4; ++c) if (in_front(sR[c], st[c], x0, y0, x1, y1, 1e9)) { f |= 1u << c; ++v[c]; }
      bits[i] = (uint8_t)f;
    }
    for (int c = 0; c < 4; ++c) if (v[c]) atomicAdd(&votes[c], v[c]);
  }
  __syncthreads();
  if (tid == 0) {
    long bestc = -1;
    int bi = 0;
    if (b >= 0) for (int c = 0; c < 4; ++c) if (votes[c] > bestc) { bestc = votes[c]; bi = c; }
    pick[0] = bestc > 0 ? bi : -1;
    n_inliers[p] = bestc > 0 ? bestc : -1;
    for (int i = 0; i < 9; ++i) R_out[9 * (long)p + i] = bestc > 0 ? (float)sR[bi][i] : 0.f;
    for (int i = 0; i < 3; ++i) t_out[3 * (long)p + i] = bestc > 0 ? (float)st[bi][i] : 0.f;
  }
  __syncthreads();
  const int bi = pick[0];
  for (long j = tid; j < n; j += kLanes) mask[s0 + j] = bi >= 0 ? (bits[s0 + j] >> bi) & 1 : 0;
}

}  // namespace

extern "C" size_t loftr_estimate_pose_batched_workspace_bytes(long M, int P) {
  if (M < 0 || P < 0) return 0;
  return layout(M, P, kProblem).total;
}

extern "C" int loftr_estimate_pose_batched(const float* mkpts0_f, const float* mkpts1_f, const long* m_bids, long M,
                                           const float* K0, const float* K1, int P, float thresh_px, float conf, unsigned seed,
                                           float* R_out, float* t_out, uint8_t* inliers_out, long* n_inliers, void* ws,
                                           size_t ws_bytes, void* stream) {
  LOFTR_CHECK_ARG(M >= 0 && P >= 0);
  if (P == 0) return M == 0 ? LOFTR_OK : LOFTR_ERR_BAD_ARG;             // every pair id would be out of range
  LOFTR_CHECK_ARG(K0 && K1 && R_out && t_out && n_inliers && ws);
  LOFTR_CHECK_ARG(M == 0 || (mkpts0_f && mkpts1_f && m_bids && inliers_out));
  if (too_large(M, P)) return LOFTR_ERR_UNSUPPORTED;
  const Layout L = layout(M, P, kProblem);
  if (ws_bytes < L.total) return LOFTR_ERR_WORKSPACE;
  const Workspace W = workspace(ws, L);
  hipStream_t s = (hipStream_t)stream;
  static const PolarTable tab = polar_table<10>();
  const PoseScore::Params prm = {K0, K1, thresh_px};
  return run<kProblem.s>(
      m_bids, M, P, kProblem, conf, seed, L, W, s,
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(pose_prep_kernel, g, b, 0, s, mkpts0_f, mkpts1_f, m_bids, M, K0, K1, P, W.pts, W.status); },
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(pose_solve_kernel, g, b, 0, s, W.pts, W.start, W.idx, P, tab, W.models, W.counts, W.hyp, W.n_hyp, W.status); },
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(ransac_score_kernel<PoseScore>, g, b, 0, s, W.pts, W.start, prm, W.models, W.hyp, W.n_hyp, W.counts, W.status); },
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(pose_recover_kernel, g, b, 0, s, W.pts, W.start, prm, W.models, W.best, W.bits, R_out, t_out, inliers_out, n_inliers); });
}
