// Batched 3D similarity / rigid RANSAC on the GPU: loftr_estimate_similarity (similarity.hip, host code) for every problem of a batch,
// with the same result -- same inlier count, same inlier mask, s, R and t equal bit for bit (fp64 outputs) -- for the same seed.  The
// sequence is ransac_gpu.h's (all 1000 minimal samples of a problem drawn up front, solved and scored in parallel, the sequential
// decision replayed on the host over the counts); this file holds the model's kernels:
//   sim_prep_kernel    (thread per correspondence)  src and dst side by side, 6 doubles per correspondence, m_bids checked;
//   sim_solve_kernel   (thread per sample)          the closed form on 3 correspondences: one model per sample;
//   SimScore           the model's inlier test for the shared scorer;
//   sim_refit_kernel   (workgroup per problem)      mask of the best hypothesis, then the host's refit loop: the two passes of sums
//                                                   in the host's order (thread k = strided partial k, then the pairwise tree in
//                                                   LDS), the 3 x 3 algebra in thread 0, the fit scored, the adoption rule, again
//                                                   while the inlier set grows; mask / model / count written.
// Identical results need identical arithmetic: every formula is similarity_core.h's, compiled from the same text as the host
// estimator's, fp64 without FMA contraction.  loftr_transform_model (a thread per point and a thread per image) is at the end.
// Plain C++ throughout; all stores are ordinary vector stores.
#include <math.h>
#include "similarity_core.h"
#include "ransac_gpu.h"

#pragma clang fp contract(off)

namespace {

using namespace simt;

constexpr int kHyp = kIters * kSol;          // hypothesis slots per problem
constexpr Problem kProblem = {kSample, kSol, kModel, kPt};

// grid ceil(M / 256) x 256: pts [M,6], m_bids checked
__global__ void sim_prep_kernel(const double* __restrict__ src, const double* __restrict__ dst, const long* __restrict__ m_bids, long M, int P,
                                double* __restrict__ pts, int* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  if (checked_bid(m_bids, i, P, status) < 0) return;
  double* q = pts + kPt * i;
  for (int c = 0; c < 3; ++c) { q[c] = src[3 * i + c]; q[3 + c] = dst[3 * i + c]; }
}

// one minimal sample per thread -> models [P, kHyp, 13] (ransac_gpu.h: sample_slots, append_hypotheses)
__global__ void __launch_bounds__(64) sim_solve_kernel(const double* __restrict__ pts, const long* __restrict__ start,
                                                       const int* __restrict__ idx, int P, int with_scale, double* __restrict__ models,
                                                       int* __restrict__ counts, int* __restrict__ hyp, int* __restrict__ n_hyp,
                                                       const int* __restrict__ status) {
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int p, it;
  if (!sample_slots<kSol>(g, P, kSample, start, status, counts, &p, &it)) return;
  const double* q = pts + kPt * start[p];
  double a[9], b[9], m[kModel];
  for (int k = 0; k < 3; ++k) {
    const long i = idx[g * 3 + k];
    for (int c = 0; c < 3; ++c) { a[3 * k + c] = q[kPt * i + c]; b[3 * k + c] = q[kPt * i + 3 + c]; }
  }
  const int ns = minimal(a, b, with_scale, m);
  if (ns) for (int k = 0; k < kModel; ++k) models[((long)p * kHyp + it) * kModel + k] = m[k];
  append_hypotheses<kSol>(p, it, ns, hyp, n_hyp);
}

struct SimScore {                            // ransac_score_kernel's model; the tile holds the whole correspondence
  static constexpr int kSol = simt::kSol, kModelSize = kModel, kPt = simt::kPt, kTilePt = 6;
  struct Params { double thr2; };
  struct Ctx { double thr2; };
  static __device__ Ctx context(const Params& a, int) { return {a.thr2}; }
  static __device__ bool is_inlier(const Ctx& c, const double* m, const double* q) { return simt::is_inlier(m, q, c.thr2); }
};

// grid P x kLanes: refit + final.  Problems without a model (best[p] < 0): n_inliers = -1, model and mask 0.
__global__ void __launch_bounds__(kLanes) sim_refit_kernel(const double* __restrict__ pts, const long* __restrict__ start, int with_scale,
                                                          double thr2, const double* __restrict__ models, const int* __restrict__ best,
                                                          uint8_t* __restrict__ bits, double* __restrict__ s_out, double* __restrict__ R_out,
                                                          double* __restrict__ t_out, uint8_t* __restrict__ mask, long* __restrict__ n_inliers) {
  __shared__ double red[kRefitChunk][kLanes];
  __shared__ double sBest[kModel], sFit[kModel], sums[kSums2], sMu[6];
  __shared__ int cnt[2], fitted;
  const int p = blockIdx.x, tid = threadIdx.x;
  const long s0 = start[p], n = pair_count(start, p);
  const int b = best[p];
  if (b < 0) {                                                            // (uniform over the block)
    if (tid == 0) { n_inliers[p] = -1; s_out[p] = 0.0; }
    if (tid < 9) R_out[9 * (long)p + tid] = 0.0;
    if (tid < 3) t_out[3 * (long)p + tid] = 0.0;
    for (long j = tid; j < n; j += kLanes) mask[s0 + j] = 0;
    return;
  }
  if (tid < kModel) sBest[tid] = models[((long)p * kHyp + b) * kModel + tid];
  if (tid < 2) cnt[tid] = 0;
  if (tid == 0) fitted = 0;
  __syncthreads();
  const double* q = pts + kPt * s0;
  // bit 0: inlier of the current model, first the best hypothesis (thread k owns the correspondences j = k (mod kLanes) in every pass)
  int c = 0;
  for (long j = tid; j < n; j += kLanes) {
    const bool in = is_inlier(sBest, q + kPt * j, thr2);
    bits[s0 + j] = (uint8_t)in;
    c += in;
  }
  if (c) atomicAdd(&cnt[0], c);
  __syncthreads();
  int cur = cnt[0];                                                       // inliers of the current model sBest (bit 0 of bits)
  for (int round = 0; round < kRefitRounds; ++round) {                    // similarity.hip's refit loop, sum for sum; every exit is uniform
    if (cur < 3) break;
    if (tid == 0) cnt[1] = 0;
    double a[kSums2];
    for (int k = 0; k < kSums1; ++k) a[k] = 0.0;                          // pass 1: the centroids
    for (long j = tid; j < n; j += kLanes) if (bits[s0 + j] & 1) for (int k = 0; k < kSums1; ++k) a[k] = a[k] + q[kPt * j + k];
    block_tree<kSums1>(red, a, sums);
    if (tid < 6) sMu[tid] = sums[tid] / (double)cur;
    __syncthreads();
    double mu[6];
    for (int k = 0; k < 6; ++k) mu[k] = sMu[k];
    for (int k = 0; k < kSums2; ++k) a[k] = 0.0;                          // pass 2: H about the centroids and the source's spread
    for (long j = tid; j < n; j += kLanes) if (bits[s0 + j] & 1) accum10(mu, mu + 3, q + kPt * j, a);
    block_tree<kRefitChunk>(red, a, sums);
    block_tree<kSums2 - kRefitChunk>(red, a + kRefitChunk, sums + kRefitChunk);
    if (tid == 0) {
      double H[kSums2], m[kModel];
      for (int k = 0; k < kSums2; ++k) H[k] = sums[k];
      const bool ok = model_from_moments(H, H[9], mu, mu + 3, with_scale, m);
      fitted = ok;
      if (ok) for (int k = 0; k < kModel; ++k) sFit[k] = m[k];
    }
    __syncthreads();
    if (!fitted) break;
    c = 0;                                                                // bit 1: inlier of the refit
    for (long j = tid; j < n; j += kLanes) {
      const bool in = is_inlier(sFit, q + kPt * j, thr2);
      bits[s0 + j] = (uint8_t)((bits[s0 + j] & 1) | (in << 1));
      c += in;
    }
    if (c) atomicAdd(&cnt[1], c);
    __syncthreads();
    const int nc = cnt[1];
    if (nc < cur) break;                                                  // the adoption rule: a refit that loses inliers is dropped
    __syncthreads();                                                      // (every thread has read sBest / cnt[1] before they change)
    if (tid < kModel) sBest[tid] = sFit[tid];
    for (long j = tid; j < n; j += kLanes) bits[s0 + j] >>= 1;
    const bool grew = nc > cur;
    cur = nc;
    __syncthreads();
    if (!grew) break;                                                     // another fit only over a strictly larger inlier set
  }
  if (tid == 0) { s_out[p] = sBest[0]; n_inliers[p] = cur; }
  if (tid < 9) R_out[9 * (long)p + tid] = sBest[1 + tid];
  if (tid < 3) t_out[3 * (long)p + tid] = sBest[10 + tid];
  for (long j = tid; j < n; j += kLanes) mask[s0 + j] = bits[s0 + j] & 1;
}

// grid ceil(max(N, n) / 256) x 256: thread i moves point i and image i (in place: every thread reads its row before it writes it)
__global__ void transform_model_kernel(const float* xyz, long N, const double* T, const uint8_t* __restrict__ posed, int n_images,
                                       const double* __restrict__ s, const double* __restrict__ R, const double* __restrict__ t,
                                       float* xyz_out, double* T_out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N && i >= n_images) return;
  double m[kModel];
  m[0] = *s;
  for (int k = 0; k < 9; ++k) m[1 + k] = R[k];
  for (int k = 0; k < 3; ++k) m[10 + k] = t[k];
  if (i < N) {
    const float x[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    float y[3];
    transform_point(m, x, y);
    xyz_out[3 * i] = y[0]; xyz_out[3 * i + 1] = y[1]; xyz_out[3 * i + 2] = y[2];
  }
  if (i < n_images) {
    double Ti[16], To[16];
    for (int k = 0; k < 16; ++k) Ti[k] = T[16 * i + k];
    if (posed[i]) transform_pose(m, Ti, To);
    else for (int k = 0; k < 16; ++k) To[k] = Ti[k];                      // the input's bits (a move, no arithmetic)
    for (int k = 0; k < 16; ++k) T_out[16 * i + k] = To[k];
  }
}

}  // namespace

extern "C" size_t loftr_estimate_similarity_batched_workspace_bytes(long M, int P) {
  if (M < 0 || P < 0) return 0;
  return layout(M, P, kProblem).total;
}

extern "C" int loftr_estimate_similarity_batched(const double* src, const double* dst, const long* m_bids, long M, int P, int with_scale,
                                                 double thresh, float conf, unsigned seed, double* s_out, double* R_out, double* t_out,
                                                 uint8_t* inliers_out, long* n_inliers, void* ws, size_t ws_bytes, void* stream) {
  LOFTR_CHECK_ARG(M >= 0 && P >= 0);
  if (P == 0) return M == 0 ? LOFTR_OK : LOFTR_ERR_BAD_ARG;             // every problem id would be out of range
  LOFTR_CHECK_ARG(s_out && R_out && t_out && n_inliers && ws);
  LOFTR_CHECK_ARG(M == 0 || (src && dst && m_bids && inliers_out));
  if (too_large(M, P)) return LOFTR_ERR_UNSUPPORTED;
  const Layout L = layout(M, P, kProblem);
  if (ws_bytes < L.total) return LOFTR_ERR_WORKSPACE;
  const Workspace W = workspace(ws, L);
  hipStream_t s = (hipStream_t)stream;
  with_scale = with_scale != 0;
  const double thr2 = thresh * thresh;
  const SimScore::Params prm = {thr2};
  return run<kProblem.s>(
      m_bids, M, P, kProblem, conf, seed, L, W, s,
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(sim_prep_kernel, g, b, 0, s, src, dst, m_bids, M, P, W.pts, W.status); },
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(sim_solve_kernel, g, b, 0, s, W.pts, W.start, W.idx, P, with_scale, W.models, W.counts, W.hyp, W.n_hyp, W.status); },
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(ransac_score_kernel<SimScore>, g, b, 0, s, W.pts, W.start, prm, W.models, W.hyp, W.n_hyp, W.counts, W.status); },
      [&](dim3 g, dim3 b) { hipLaunchKernelGGL(sim_refit_kernel, g, b, 0, s, W.pts, W.start, with_scale, thr2, W.models, W.best, W.bits, s_out, R_out, t_out, inliers_out, n_inliers); });
}

extern "C" int loftr_transform_model(const float* xyz, long N, const double* T_cam_from_world, const uint8_t* posed, int n_images,
                                     const double* s, const double* R, const double* t, float* xyz_out, double* T_out, void* stream) {
  LOFTR_CHECK_ARG(N >= 0 && n_images >= 0 && s && R && t);
  LOFTR_CHECK_ARG((N == 0 || (xyz && xyz_out)) && (n_images == 0 || (T_cam_from_world && posed && T_out)));
  const long n = N > n_images ? N : (long)n_images;
  if (n == 0) return LOFTR_OK;
  if ((n + 255) / 256 >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(transform_model_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, xyz, N, T_cam_from_world, posed,
                     n_images, s, R, t, xyz_out, T_out);
  LOFTR_CHECK_LAUNCH();
  return LOFTR_OK;
}
