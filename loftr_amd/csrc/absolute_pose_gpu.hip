// Batched absolute pose (P3P RANSAC + Gauss-Newton refit) on the GPU: loftr_estimate_absolute_pose (absolute_pose.hip, host code) for
// every pair of a batch, with the same result -- same inlier count, same inlier mask, R and t equal after the float32 rounding -- for
// the same seed.  The layout follows geometry_gpu.hip: the host loop's random stream does not depend on the scores, so all
// 1000 minimal samples of a pair are drawn up front, solved and scored in parallel, and the sequential decision is replayed afterwards:
//   1. abs_prep_kernel    (thread per match)    fp64 world point, pixel and unit bearing of every match, m_bids checked (range, grouping);
//   2. abs_sample_kernel  (thread per pair)     pair offsets, the 1000 samples of Rng(seed) with the host's duplicate rejection;
//   3. abs_solve_kernel   (thread per sample)   P3P: up to 4 poses per sample, appended to a per-pair work list of hypotheses;
//   4. abs_score_kernel   (thread per hypothesis, 512-match tiles of the pair in LDS)  inlier counts;
//   5. host replay of the RANSAC loop over the copied counts (strict `>`, the adaptive count with the host's own pow / log);
//   6. abs_refit_kernel   (workgroup per pair)  mask of the best hypothesis, then the host's refit loop: the Gauss-Newton sums in the
//                                               host's order (thread k = strided partial k, then the pairwise tree in LDS), the 6 x 6
//                                               solve in thread 0, the fit scored, the adoption rule, again while the inlier set grows;
//                                               mask / pose / count written.
// Identical decisions need identical arithmetic: every formula is absolute_pose_core.h's, compiled from the same text as the host
// estimator's, fp64 without FMA contraction.  loftr_lift_keypoints (the first half of the reference's warp_kpts, fp32) is at the end.
// Plain C++ throughout; all stores are ordinary vector stores.
#include <math.h>
#include <string.h>
#include <vector>
#include "common.h"
#include "absolute_pose_core.h"

#pragma clang fp contract(off)

namespace {

using namespace absp;

constexpr int kHyp = kIters * kSol;          // hypothesis slots per pair
constexpr int kPt = 8;                       // doubles per match: world point (3), pixel (2), unit bearing (3)
constexpr int kScoreThreads = 256;
constexpr int kScoreTile = 512;              // matches per LDS tile of the scorer (20 KiB)
constexpr int kRefitChunk = 9;               // sums reduced per pass through the LDS tree (18 KiB)

enum : int { kBadBid = 1, kUngrouped = 2 };  // status word bits (device-side findings)

__device__ long lower_bound(const long* a, long n, long key) {
  long lo = 0, hi = n;
  while (lo < hi) { const long mid = lo + (hi - lo) / 2; if (a[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}
// pair p's matches [start[p], start[p] + count) (a negative difference -- only with ungrouped m_bids -- counts as none)
__device__ __forceinline__ long pair_count(const long* start, int p) { const long n = start[p + 1] - start[p]; return n > 0 ? n : 0; }

// grid ceil(M / 256) x 256: pts [M,8] in fp64, m_bids checked
__global__ void abs_prep_kernel(const float* __restrict__ pts3d, const float* __restrict__ kpts, const long* __restrict__ m_bids, long M,
                                const float* __restrict__ K, int P, double* __restrict__ pts, int* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const long b = m_bids[i];
  if (b < 0 || b >= P) { atomicOr(status, (int)kBadBid); return; }
  if (i > 0 && m_bids[i - 1] > b) atomicOr(status, (int)kUngrouped);
  const Cam cam = cam_from_K(K + 9 * b);
  double* q = pts + kPt * i;
  double f[3];
  const double u = kpts[2 * i], v = kpts[2 * i + 1];
  bearing(cam, u, v, f);
  q[0] = pts3d[3 * i]; q[1] = pts3d[3 * i + 1]; q[2] = pts3d[3 * i + 2]; q[3] = u; q[4] = v; q[5] = f[0]; q[6] = f[1]; q[7] = f[2];
}

// grid ceil((P + 1) / 64) x 64: pair offsets, the kIters minimal samples (3 indices each) of every pair with >= 3 matches
__global__ void abs_sample_kernel(const long* __restrict__ m_bids, long M, int P, unsigned seed, long* __restrict__ start,
                                  int* __restrict__ idx, int* __restrict__ n_hyp) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > P) return;
  const long s0 = lower_bound(m_bids, M, p);
  start[p] = s0;
  if (p == P) return;
  n_hyp[p] = 0;
  const long n = lower_bound(m_bids, M, p + 1) - s0;
  if (n < 3) return;
  Rng rng(seed);
  int* out = idx + (long)p * kIters * 3;
  for (int it = 0; it < kIters; ++it) {
    int d[3];
    draw_sample(rng, n, d);
    out[it * 3] = d[0]; out[it * 3 + 1] = d[1]; out[it * 3 + 2] = d[2];
  }
}

// grid ceil(P * kIters / 64) x 64: one minimal sample per thread -> poses [P, kHyp, 12], counts [P, kHyp] = -1 (filled by the scorer
// for the solutions), work list hyp [P, kHyp] of slot ids it * kSol + sol (any order), n_hyp [P]
__global__ void __launch_bounds__(64) abs_solve_kernel(const double* __restrict__ pts, const long* __restrict__ start,
                                                       const int* __restrict__ idx, int P, PolarTable tab, double* __restrict__ poses,
                                                       int* __restrict__ counts, int* __restrict__ hyp, int* __restrict__ n_hyp,
                                                       const int* __restrict__ status) {
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long)P * kIters || *status) return;
  const int p = (int)(g / kIters), it = (int)(g % kIters);
  int* cnt = counts + (long)p * kHyp + it * kSol;
  for (int k = 0; k < kSol; ++k) cnt[k] = -1;
  if (pair_count(start, p) < 3) return;
  const double* q = pts + kPt * start[p];
  double X[9], f[9];
  for (int k = 0; k < 3; ++k) {
    const long i = idx[g * 3 + k];
    for (int c = 0; c < 3; ++c) { X[3 * k + c] = q[kPt * i + c]; f[3 * k + c] = q[kPt * i + 5 + c]; }
  }
  const int ns = p3p(X, f, poses + ((long)p * kHyp + it * kSol) * kPose, tab);   // the sample's kSol slots, filled in solver order
  if (ns == 0) return;
  const int base = atomicAdd(n_hyp + p, ns);
  for (int k = 0; k < ns; ++k) hyp[(long)p * kHyp + base + k] = it * kSol + k;
}

// grid (P, ceil(kHyp / 256)) x 256: thread = hypothesis of the pair's work list; the pair's matches stream through LDS
__global__ void __launch_bounds__(kScoreThreads) abs_score_kernel(const double* __restrict__ pts, const long* __restrict__ start,
                                                                 const float* __restrict__ K, double thr2, const double* __restrict__ poses,
                                                                 const int* __restrict__ hyp, const int* __restrict__ n_hyp,
                                                                 int* __restrict__ counts, const int* __restrict__ status) {
  __shared__ double tile[kScoreTile][5];
  const int p = blockIdx.x;
  const int nh = n_hyp[p];
  const int h = blockIdx.y * kScoreThreads + threadIdx.x;
  if (*status || (int)blockIdx.y * kScoreThreads >= nh) return;           // (uniform over the block)
  const bool valid = h < nh;
  const int slot = valid ? hyp[(long)p * kHyp + h] : 0;
  const Cam cam = cam_from_K(K + 9 * (long)p);
  double m[kPose];
  for (int i = 0; i < kPose; ++i) m[i] = valid ? poses[((long)p * kHyp + slot) * kPose + i] : 0.0;
  const long s0 = start[p], n = pair_count(start, p);
  int cnt = 0;
  for (long b = 0; b < n; b += kScoreTile) {
    const int nt = (int)(n - b < kScoreTile ? n - b : kScoreTile);
    __syncthreads();
    for (int j = threadIdx.x; j < nt; j += kScoreThreads) {
      const double* q = pts + kPt * (s0 + b + j);
      for (int c = 0; c < 5; ++c) tile[j][c] = q[c];
    }
    __syncthreads();
    for (int j = 0; j < nt; ++j) cnt += is_inlier(cam, m, m + 9, tile[j], tile[j][3], tile[j][4], thr2);
  }
  if (valid) counts[(long)p * kHyp + slot] = cnt;
}

// the host's tree() over kLanes partials, N sums at a time: a[q] of thread k is partial k of sum q; out[0..N) in LDS
template <int N>
__device__ void block_tree(double (*red)[kLanes], const double* a, double* out) {
  const int tid = threadIdx.x;
  __syncthreads();
  for (int q = 0; q < N; ++q) red[q][tid] = a[q];
  __syncthreads();
  for (int st = kLanes / 2; st >= 1; st >>= 1) {
    if (tid < st) for (int q = 0; q < N; ++q) red[q][tid] = red[q][tid] + red[q][tid + st];
    __syncthreads();
  }
  if (tid < N) out[tid] = red[tid][0];
  __syncthreads();
}

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

// workspace layout (byte offsets, 256-aligned)
struct Layout { size_t status, start, counts, pts, idx, poses, hyp, n_hyp, best, bits, total; };
Layout layout(long M, int P) {
  Layout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
  // status, start and counts are contiguous: the one device -> host copy of the replay
  L.status = take(8);
  L.start = L.status + 8;
  o = align_up(L.start + sizeof(long) * ((size_t)P + 1), 8);
  L.counts = o;
  o = align_up(o + sizeof(int) * (size_t)P * kHyp, 256);
  L.pts = take(sizeof(double) * kPt * (size_t)M);
  L.idx = take(sizeof(int) * 3 * (size_t)P * kIters);
  L.poses = take(sizeof(double) * kPose * (size_t)P * kHyp);
  L.hyp = take(sizeof(int) * (size_t)P * kHyp);
  L.n_hyp = take(sizeof(int) * (size_t)P);
  L.best = take(sizeof(int) * (size_t)P);
  L.bits = take((size_t)M);
  L.total = o;
  return L;
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
  return layout(M, P).total;
}

extern "C" int loftr_estimate_absolute_pose_batched(const float* pts3d, const float* kpts, const long* m_bids, long M, const float* K, int P,
                                                    float thresh_px, float conf, unsigned seed, float* R_out, float* t_out,
                                                    uint8_t* inliers_out, long* n_inliers, void* ws, size_t ws_bytes, void* stream) {
  LOFTR_CHECK_ARG(M >= 0 && P >= 0);
  if (P == 0) return M == 0 ? LOFTR_OK : LOFTR_ERR_BAD_ARG;             // every pair id would be out of range
  LOFTR_CHECK_ARG(K && R_out && t_out && n_inliers && ws);
  LOFTR_CHECK_ARG(M == 0 || (pts3d && kpts && m_bids && inliers_out));
  if ((M + 255) / 256 >= (1L << 31) || M >= (1L << 31) || (long)P * kIters >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  const Layout L = layout(M, P);
  if (ws_bytes < L.total) return LOFTR_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  int* status = (int*)(w + L.status);
  long* start = (long*)(w + L.start);
  int* counts = (int*)(w + L.counts);
  double *pts = (double*)(w + L.pts), *poses = (double*)(w + L.poses);
  int *idx = (int*)(w + L.idx), *hyp = (int*)(w + L.hyp), *n_hyp = (int*)(w + L.n_hyp), *best = (int*)(w + L.best);
  uint8_t* bits = (uint8_t*)(w + L.bits);
  const double thr2 = (double)thresh_px * (double)thresh_px;
  if (hipMemsetAsync(status, 0, sizeof(int), s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  if (M > 0) {
    hipLaunchKernelGGL(abs_prep_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, pts3d, kpts, m_bids, M, K, P, pts, status);
    LOFTR_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(abs_sample_kernel, dim3((unsigned)((P + 1 + 63) / 64)), dim3(64), 0, s, m_bids, M, P, seed, start, idx, n_hyp);
  LOFTR_CHECK_LAUNCH();
  static const PolarTable tab = polar_table();
  hipLaunchKernelGGL(abs_solve_kernel, dim3((unsigned)(((long)P * kIters + 63) / 64)), dim3(64), 0, s, pts, start, idx, P, tab, poses, counts, hyp,
                     n_hyp, status);
  LOFTR_CHECK_LAUNCH();
  hipLaunchKernelGGL(abs_score_kernel, dim3((unsigned)P, (unsigned)((kHyp + kScoreThreads - 1) / kScoreThreads)), dim3(kScoreThreads), 0, s, pts,
                     start, K, thr2, poses, hyp, n_hyp, counts, status);
  LOFTR_CHECK_LAUNCH();
  // ---- replay of the host loop (absolute_pose.hip loftr_estimate_absolute_pose) over the counts: one copy down, one copy up ----
  const size_t down = L.counts + sizeof(int) * (size_t)P * kHyp - L.status;
  std::vector<char> host(down);
  if (hipMemcpyAsync(host.data(), w + L.status, down, hipMemcpyDeviceToHost, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  if (hipStreamSynchronize(s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  int st;
  memcpy(&st, host.data(), sizeof(int));
  if (st) return LOFTR_ERR_BAD_ARG;                                     // m_bids out of [0, P) or not grouped by ascending pair
  const long* h_start = (const long*)(host.data() + (L.start - L.status));
  const int* h_counts = (const int*)(host.data() + (L.counts - L.status));
  std::vector<int> h_best(P);
  for (int p = 0; p < P; ++p) {
    const long Mp = h_start[p + 1] - h_start[p];
    h_best[p] = -1;
    if (Mp < 3) continue;
    const int* c = h_counts + (size_t)p * kHyp;
    long bestn = 0;
    int max_iters = kIters, iters = max_iters;
    for (int it = 0; it < iters; ++it) {
      for (int sol = 0; sol < kSol && c[it * kSol + sol] >= 0; ++sol) {
        const long cnt = c[it * kSol + sol];
        if (cnt > bestn) {
          bestn = cnt;
          h_best[p] = it * kSol + sol;
          const double wr = (double)cnt / (double)Mp;
          const double p_all = pow(wr, 3.0);
          if (p_all > 1 - 1e-12) iters = it + 1;
          else if (p_all > 1e-12) {
            const double need = log(1.0 - (double)conf) / log(1.0 - p_all);
            if (need < iters) iters = need < it + 1 ? it + 1 : (int)ceil(need);
          }
        }
      }
    }
    if (bestn < 3) h_best[p] = -1;
  }
  if (hipMemcpyAsync(best, h_best.data(), sizeof(int) * P, hipMemcpyHostToDevice, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  hipLaunchKernelGGL(abs_refit_kernel, dim3((unsigned)P), dim3(kLanes), 0, s, pts, start, K, thr2, poses, best, bits, R_out, t_out, inliers_out,
                     n_inliers);
  LOFTR_CHECK_LAUNCH();
  // h_best is pageable host memory that goes out of scope on return: wait for the stream rather than rely on the copy staging it
  if (hipStreamSynchronize(s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  return LOFTR_OK;
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
