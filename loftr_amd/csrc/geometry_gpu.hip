// Batched homography / fundamental-matrix RANSAC on the GPU: loftr_estimate_geometry (geometry.hip, host code) for every pair of a
// batch, with the same result -- same inlier count, same inlier mask, the matrix equal after the float32 rounding -- for the same
// seed.  The layout follows pose_gpu.hip: the host loop's random stream does not depend on the scores, so all 1000
// minimal samples of a pair are drawn up front, solved and scored in parallel, and the sequential decision is replayed afterwards:
//   1. geo_prep_kernel    (thread per match)    fp64 copies of the points, m_bids checked (range, grouping);
//   2. geo_sample_kernel  (thread per pair)     pair offsets, the 1000 samples of Rng(seed) with the host's duplicate rejection;
//   3. geo_solve_kernel   (thread per sample)   per-sample Hartley normalisation, 9 x 9 Jacobi, for F the cubic: up to 1 (H) / 3 (F)
//                                               unit-norm matrices per sample, appended to a per-pair work list of hypotheses;
//   4. geo_score_kernel   (thread per hypothesis, 512-match tiles of the pair in LDS)  inlier counts;
//   5. host replay of the RANSAC loop over the copied counts (strict `>`, the adaptive count with the host's own pow / log);
//   6. geo_refit_kernel   (workgroup per pair)  mask of the best hypothesis, then the host's refit loop: the sums in the host's order
//                                               (thread k = strided partial k, then the pairwise tree in LDS), Jacobi / svd3 in
//                                               thread 0, the refit scored, the adoption rule, again while the inlier set grows;
//                                               mask / matrix / count written.
// Identical decisions need identical arithmetic: every formula is geometry_core.h's, compiled from the same text as the host
// estimator's, fp64 without FMA contraction.  Plain C++ throughout; all stores are ordinary vector stores.
#include <math.h>
#include <string.h>
#include <vector>
#include "common.h"
#include "geometry_core.h"

#pragma clang fp contract(off)

namespace {

using namespace geo;

constexpr int kScoreThreads = 256;
constexpr int kScoreTile = 512;              // matches per LDS tile of the scorer (16 KiB)
constexpr int kRefitChunk = 9;               // sums reduced per pass through the LDS tree (18 KiB)

enum : int { kBadBid = 1, kUngrouped = 2 };  // status word bits (device-side findings)

struct Rng {                                 // xorshift64* (pose.hip)
  uint64_t s;
  __device__ explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) { if (!s) s = 1; }
  __device__ uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
  __device__ long below(long n) { return (long)(next() % (uint64_t)n); }
};

__device__ long lower_bound(const long* a, long n, long key) {
  long lo = 0, hi = n;
  while (lo < hi) { const long mid = lo + (hi - lo) / 2; if (a[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}
// pair p's matches [start[p], start[p] + count) (a negative difference -- only with ungrouped m_bids -- counts as none)
__device__ __forceinline__ long pair_count(const long* start, int p) { const long n = start[p + 1] - start[p]; return n > 0 ? n : 0; }

// grid ceil(M / 256) x 256: pts [M,4] = (x0, y0, x1, y1) in fp64, m_bids checked
__global__ void geo_prep_kernel(const float* __restrict__ k0, const float* __restrict__ k1, const long* __restrict__ m_bids, long M, int P,
                                double* __restrict__ pts, int* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const long b = m_bids[i];
  if (b < 0 || b >= P) { atomicOr(status, (int)kBadBid); return; }
  if (i > 0 && m_bids[i - 1] > b) atomicOr(status, (int)kUngrouped);
  pts[4 * i] = k0[2 * i]; pts[4 * i + 1] = k0[2 * i + 1]; pts[4 * i + 2] = k1[2 * i]; pts[4 * i + 3] = k1[2 * i + 1];
}

// grid ceil((P + 1) / 64) x 64: pair offsets, the kIters minimal samples (s indices each) of every pair with >= s matches
__global__ void geo_sample_kernel(const long* __restrict__ m_bids, long M, int P, int s, unsigned seed, long* __restrict__ start,
                                  int* __restrict__ idx, int* __restrict__ n_hyp) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > P) return;
  const long s0 = lower_bound(m_bids, M, p);
  start[p] = s0;
  if (p == P) return;
  n_hyp[p] = 0;
  const long n = lower_bound(m_bids, M, p + 1) - s0;
  if (n < s) return;
  Rng rng(seed);
  int* out = idx + (long)p * kIters * s;
  for (int it = 0; it < kIters; ++it) {
    int d[7];
    for (int k = 0; k < s;) {
      const int c = (int)rng.below(n);
      bool dup = false;
      for (int j = 0; j < k; ++j) dup = dup || d[j] == c;
      if (!dup) d[k++] = c;
    }
    for (int k = 0; k < s; ++k) out[it * s + k] = d[k];
  }
}

// grid ceil(P * kIters / 64) x 64: one minimal sample per thread -> mats [P, kIters * kSol, 9], counts [P, kIters * kSol] = -1 (filled
// by the scorer for the solutions), work list hyp [P, kIters * kSol] of slot ids it * kSol + sol (any order), n_hyp [P]
template <int kModel>
__global__ void __launch_bounds__(64) geo_solve_kernel(const double* __restrict__ pts, const long* __restrict__ start,
                                                       const int* __restrict__ idx, int P, PolarTable tab, double* __restrict__ mats,
                                                       int* __restrict__ counts, int* __restrict__ hyp, int* __restrict__ n_hyp,
                                                       const int* __restrict__ status) {
  constexpr int s = kModel == 0 ? 4 : 7, kSol = kModel == 0 ? 1 : 3, kHyp = kIters * kSol;
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long)P * kIters || *status) return;
  const int p = (int)(g / kIters), it = (int)(g % kIters);
  int* cnt = counts + (long)p * kHyp + it * kSol;
  for (int k = 0; k < kSol; ++k) cnt[k] = -1;
  if (pair_count(start, p) < s) return;
  const double* q = pts + 4 * start[p];
  double x0[7], y0[7], x1[7], y1[7];
  for (int k = 0; k < s; ++k) {
    const long i = idx[g * s + k];
    x0[k] = q[4 * i]; y0[k] = q[4 * i + 1]; x1[k] = q[4 * i + 2]; y1[k] = q[4 * i + 3];
  }
  double m[9 * kSol];
  const int ns = solve_minimal(kModel, x0, y0, x1, y1, m, tab);
  if (ns == 0) return;
  double* out = mats + ((long)p * kHyp + it * kSol) * 9;
  for (int k = 0; k < 9 * ns; ++k) out[k] = m[k];
  const int base = atomicAdd(n_hyp + p, ns);
  for (int k = 0; k < ns; ++k) hyp[(long)p * kHyp + base + k] = it * kSol + k;
}

// grid (P, ceil(kHyp / 256)) x 256: thread = hypothesis of the pair's work list; the pair's matches stream through LDS
template <int kModel>
__global__ void __launch_bounds__(kScoreThreads) geo_score_kernel(const double* __restrict__ pts, const long* __restrict__ start, double thr2,
                                                                 const double* __restrict__ mats, const int* __restrict__ hyp,
                                                                 const int* __restrict__ n_hyp, int* __restrict__ counts,
                                                                 const int* __restrict__ status) {
  constexpr int kHyp = kIters * (kModel == 0 ? 1 : 3);
  __shared__ double tile[kScoreTile][4];
  const int p = blockIdx.x;
  const int nh = n_hyp[p];
  const int h = blockIdx.y * kScoreThreads + threadIdx.x;
  if (*status || (int)blockIdx.y * kScoreThreads >= nh) return;           // (uniform over the block)
  const bool valid = h < nh;
  const int slot = valid ? hyp[(long)p * kHyp + h] : 0;
  double m[9];
  for (int i = 0; i < 9; ++i) m[i] = valid ? mats[((long)p * kHyp + slot) * 9 + i] : 0.0;
  const long s0 = start[p], n = pair_count(start, p);
  int cnt = 0;
  for (long b = 0; b < n; b += kScoreTile) {
    const int nt = (int)(n - b < kScoreTile ? n - b : kScoreTile);
    __syncthreads();
    for (int j = threadIdx.x; j < nt; j += kScoreThreads) {
      const long i = s0 + b + j;
      tile[j][0] = pts[4 * i]; tile[j][1] = pts[4 * i + 1]; tile[j][2] = pts[4 * i + 2]; tile[j][3] = pts[4 * i + 3];
    }
    __syncthreads();
    for (int j = 0; j < nt; ++j) cnt += is_inlier(kModel, m, tile[j][0], tile[j][1], tile[j][2], tile[j][3], thr2);
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

// workspace layout (byte offsets, 256-aligned)
struct Layout { size_t status, start, counts, pts, idx, mats, hyp, n_hyp, best, bits, total; };
Layout layout(long M, int P, int model) {
  const size_t kHyp = (size_t)kIters * max_solutions(model);
  Layout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
  // status, start and counts are contiguous: the one device -> host copy of the replay
  L.status = take(8);
  L.start = L.status + 8;
  o = align_up(L.start + sizeof(long) * ((size_t)P + 1), 8);
  L.counts = o;
  o = align_up(o + sizeof(int) * (size_t)P * kHyp, 256);
  L.pts = take(sizeof(double) * 4 * (size_t)M);
  L.idx = take(sizeof(int) * sample_size(model) * (size_t)P * kIters);
  L.mats = take(sizeof(double) * 9 * (size_t)P * kHyp);
  L.hyp = take(sizeof(int) * (size_t)P * kHyp);
  L.n_hyp = take(sizeof(int) * (size_t)P);
  L.best = take(sizeof(int) * (size_t)P);
  L.bits = take((size_t)M);
  L.total = o;
  return L;
}

template <int kModel>
int run(const float* k0, const float* k1, const long* m_bids, long M, int P, float thresh_px, float conf, unsigned seed, float* mat_out,
        uint8_t* inliers_out, long* n_inliers, char* w, const Layout& L, hipStream_t s) {
  constexpr int sz = kModel == 0 ? 4 : 7, kSol = kModel == 0 ? 1 : 3, kHyp = kIters * kSol;
  int* status = (int*)(w + L.status);
  long* start = (long*)(w + L.start);
  int* counts = (int*)(w + L.counts);
  double *pts = (double*)(w + L.pts), *mats = (double*)(w + L.mats);
  int *idx = (int*)(w + L.idx), *hyp = (int*)(w + L.hyp), *n_hyp = (int*)(w + L.n_hyp), *best = (int*)(w + L.best);
  uint8_t* bits = (uint8_t*)(w + L.bits);
  const double thr2 = (double)thresh_px * (double)thresh_px;
  if (hipMemsetAsync(status, 0, sizeof(int), s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  if (M > 0) {
    hipLaunchKernelGGL(geo_prep_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, k0, k1, m_bids, M, P, pts, status);
    LOFTR_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(geo_sample_kernel, dim3((unsigned)((P + 1 + 63) / 64)), dim3(64), 0, s, m_bids, M, P, sz, seed, start, idx, n_hyp);
  LOFTR_CHECK_LAUNCH();
  static const PolarTable tab = polar_table();
  hipLaunchKernelGGL(geo_solve_kernel<kModel>, dim3((unsigned)(((long)P * kIters + 63) / 64)), dim3(64), 0, s, pts, start, idx, P, tab, mats,
                     counts, hyp, n_hyp, status);
  LOFTR_CHECK_LAUNCH();
  hipLaunchKernelGGL(geo_score_kernel<kModel>, dim3((unsigned)P, (unsigned)((kHyp + kScoreThreads - 1) / kScoreThreads)), dim3(kScoreThreads), 0,
                     s, pts, start, thr2, mats, hyp, n_hyp, counts, status);
  LOFTR_CHECK_LAUNCH();
  // ---- replay of the host loop (geometry.hip loftr_estimate_geometry) over the counts: one copy down, one copy up ----
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
    if (Mp < sz) continue;
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
          const double p_all = pow(wr, (double)sz);
          if (p_all > 1 - 1e-12) iters = it + 1;
          else if (p_all > 1e-12) {
            const double need = log(1.0 - (double)conf) / log(1.0 - p_all);
            if (need < iters) iters = need < it + 1 ? it + 1 : (int)ceil(need);
          }
        }
      }
    }
    if (bestn < sz) h_best[p] = -1;
  }
  if (hipMemcpyAsync(best, h_best.data(), sizeof(int) * P, hipMemcpyHostToDevice, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  hipLaunchKernelGGL(geo_refit_kernel<kModel>, dim3((unsigned)P), dim3(kLanes), 0, s, pts, start, thr2, mats, best, bits, mat_out, inliers_out,
                     n_inliers);
  LOFTR_CHECK_LAUNCH();
  // h_best is pageable host memory that goes out of scope on return: wait for the stream rather than rely on the copy staging it
  if (hipStreamSynchronize(s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  return LOFTR_OK;
}

}  // namespace

extern "C" size_t loftr_estimate_geometry_batched_workspace_bytes(long M, int P, int model) {
  if (M < 0 || P < 0 || (model != 0 && model != 1)) return 0;
  return layout(M, P, model).total;
}

extern "C" int loftr_estimate_geometry_batched(const float* mkpts0_f, const float* mkpts1_f, const long* m_bids, long M, int P, int model,
                                               float thresh_px, float conf, unsigned seed, float* mat_out, uint8_t* inliers_out,
                                               long* n_inliers, void* ws, size_t ws_bytes, void* stream) {
  LOFTR_CHECK_ARG(M >= 0 && P >= 0 && (model == 0 || model == 1));
  if (P == 0) return M == 0 ? LOFTR_OK : LOFTR_ERR_BAD_ARG;             // every pair id would be out of range
  LOFTR_CHECK_ARG(mat_out && n_inliers && ws);
  LOFTR_CHECK_ARG(M == 0 || (mkpts0_f && mkpts1_f && m_bids && inliers_out));
  if ((M + 255) / 256 >= (1L << 31) || M >= (1L << 31) || (long)P * kIters >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  const Layout L = layout(M, P, model);
  if (ws_bytes < L.total) return LOFTR_ERR_WORKSPACE;
  return model == 0 ? run<0>(mkpts0_f, mkpts1_f, m_bids, M, P, thresh_px, conf, seed, mat_out, inliers_out, n_inliers, (char*)ws, L, (hipStream_t)stream)
                    : run<1>(mkpts0_f, mkpts1_f, m_bids, M, P, thresh_px, conf, seed, mat_out, inliers_out, n_inliers, (char*)ws, L, (hipStream_t)stream);
}
