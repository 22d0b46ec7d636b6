// The device scaffold of the batched RANSAC estimators (pose_gpu.hip, geometry_gpu.hip, absolute_pose_gpu.hip), written once.
//
// A host estimator's random stream does not depend on the scores: iteration `it` always draws its sample from the same xorshift64*
// state sequence, and the adaptive iteration count only truncates that sequence.  So all kIters minimal samples of a pair are drawn up
// front, solved and scored in parallel, and the sequential decision is replayed afterwards over the counts:
//   1. the model's prep kernel (thread per match)    fp64 form of every match, m_bids checked (range, grouping: checked_bid);
//   2. ransac_sample_kernel<s> (thread per pair)     pair offsets, the kIters samples of Rng(seed) with the host's duplicate rejection
//                                                    (integer arithmetic only: exact by construction);
//   3. the model's solve kernel (thread per sample)  up to kSol models per sample in the sample's slots, appended to a per-pair work
//                                                    list of hypotheses (sample_slots / append_hypotheses);
//   4. ransac_score_kernel<Model> (thread per hypothesis, 512-match tiles of the pair in LDS)  inlier counts;
//   5. host replay of the RANSAC loop over the copied counts (replay_best: strict `>`, ransac_core.h's adaptive count with the host's
//      own pow / log): one device -> host copy and one host -> device copy per batch;
//   6. the model's final kernel (workgroup per pair) mask of the best hypothesis, recovery or refit (block_tree), outputs.
// run() is that sequence; a model hands it its four launches.  Plain C++ throughout; all stores are ordinary vector stores.
#pragma once
#include <string.h>
#include <vector>
#include "common.h"
#include "ransac_core.h"

#pragma clang fp contract(off)

namespace ransac {

constexpr int kScoreThreads = 256;
constexpr int kScoreTile = 512;              // matches per LDS tile of the scorer
constexpr int kRefitChunk = 9;               // sums reduced per pass through the LDS tree (18 KiB)

enum : int { kBadBid = 1, kUngrouped = 2 };  // status word bits (device-side findings)

// m_bids[i], or -1 when it is outside [0, P); that, and a predecessor above it (not grouped by ascending pair), go to the status word
__device__ __forceinline__ long checked_bid(const long* m_bids, long i, int P, int* status) {
  const long b = m_bids[i];
  if (b < 0 || b >= P) { atomicOr(status, (int)kBadBid); return -1; }
  if (i > 0 && m_bids[i - 1] > b) atomicOr(status, (int)kUngrouped);
  return b;
}

__device__ inline long lower_bound(const long* a, long n, long key) {
  long lo = 0, hi = n;
  while (lo < hi) { const long mid = lo + (hi - lo) / 2; if (a[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}
// pair p's matches [start[p], start[p] + count) (a negative difference -- only with ungrouped m_bids -- counts as none)
__device__ __forceinline__ long pair_count(const long* start, int p) { const long n = start[p + 1] - start[p]; return n > 0 ? n : 0; }

// grid ceil((P + 1) / 64) x 64: pair offsets, the kIters minimal samples (s indices each) of every pair with >= s matches.  The sample
// size is a template argument: the thread draws its pair's samples one after the other, and only with a constant s do the draw's loops
// unroll and the sample stay in registers.
template <int s>
__global__ void ransac_sample_kernel(const long* __restrict__ m_bids, long M, int P, unsigned seed, long* __restrict__ start,
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
    int d[s];
    draw_sample(rng, n, s, d);
    for (int k = 0; k < s; ++k) out[it * s + k] = d[k];
  }
}

// Solve kernels: grid ceil(P * kIters / 64) x 64, thread g = sample g % kIters of pair g / kIters.  Its kSol slots of counts [P, kIters *
// kSol] are set to -1 (the scorer fills those of the solutions); false when there is nothing to solve (g out of range, a finding in the
// status word, a pair with fewer than s matches).
template <int kSol>
__device__ __forceinline__ bool sample_slots(long g, int P, int s, const long* start, const int* status, int* counts, int* p, int* it) {
  if (g >= (long)P * kIters || *status) return false;
  *p = (int)(g / kIters); *it = (int)(g % kIters);
  int* cnt = counts + ((long)*p * kIters + *it) * kSol;
  for (int k = 0; k < kSol; ++k) cnt[k] = -1;
  return pair_count(start, *p) >= s;
}
// the sample's ns solutions (slots it * kSol + 0 .. ns) join the pair's work list hyp [P, kIters * kSol] (any order), n_hyp [P]
template <int kSol>
__device__ __forceinline__ void append_hypotheses(int p, int it, int ns, int* hyp, int* n_hyp) {
  if (ns == 0) return;
  const int base = atomicAdd(n_hyp + p, ns);
  for (int k = 0; k < ns; ++k) hyp[(long)p * kIters * kSol + base + k] = it * kSol + k;
}

// grid (P, ceil(kIters * kSol / 256)) x 256: thread = hypothesis of the pair's work list; the pair's matches stream through LDS.
// Model: kSol, kModelSize (doubles per hypothesis), kPt (doubles per match), kTilePt (the first of them, which the test reads), Params,
// Ctx context(Params, pair) and bool is_inlier(Ctx, model, tile point).
template <class Model>
__global__ void __launch_bounds__(kScoreThreads) ransac_score_kernel(const double* __restrict__ pts, const long* __restrict__ start,
                                                                    typename Model::Params prm, const double* __restrict__ models,
                                                                    const int* __restrict__ hyp, const int* __restrict__ n_hyp,
                                                                    int* __restrict__ counts, const int* __restrict__ status) {
  constexpr int kHyp = kIters * Model::kSol;
  __shared__ double tile[kScoreTile][Model::kTilePt];
  const int p = blockIdx.x;
  const int nh = n_hyp[p];
  const int h = blockIdx.y * kScoreThreads + threadIdx.x;
  if (*status || (int)blockIdx.y * kScoreThreads >= nh) return;           // (uniform over the block)
  const bool valid = h < nh;
  const int slot = valid ? hyp[(long)p * kHyp + h] : 0;
  const typename Model::Ctx ctx = Model::context(prm, p);
  double m[Model::kModelSize];
  for (int i = 0; i < Model::kModelSize; ++i) m[i] = valid ? models[((long)p * kHyp + slot) * Model::kModelSize + i] : 0.0;
  const long s0 = start[p], n = pair_count(start, p);
  int cnt = 0;
  for (long b = 0; b < n; b += kScoreTile) {
    const int nt = (int)(n - b < kScoreTile ? n - b : kScoreTile);
    __syncthreads();
    for (int j = threadIdx.x; j < nt; j += kScoreThreads) {
      const double* q = pts + Model::kPt * (s0 + b + j);
      for (int c = 0; c < Model::kTilePt; ++c) tile[j][c] = q[c];
    }
    __syncthreads();
    for (int j = 0; j < nt; ++j) cnt += Model::is_inlier(ctx, m, tile[j]);
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

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct Problem { int s, sol, model, pt; };   // sample size, solutions per sample, doubles per hypothesis, doubles per match

// the workspace (byte offsets): status word at 0, start [P + 1] and counts [P, kIters * sol] right behind it (the three are the one
// device -> host copy of the replay, `down` bytes), the rest 256-aligned
struct Layout { size_t start, counts, down, pts, idx, models, hyp, n_hyp, best, bits, total; };
inline Layout layout(long M, int P, const Problem& pr) {
  const size_t hyp = (size_t)P * kIters * pr.sol;
  Layout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
  L.start = 8;
  L.counts = L.start + sizeof(long) * ((size_t)P + 1);
  L.down = L.counts + sizeof(int) * hyp;
  o = align_up(L.down, 256);
  L.pts = take(sizeof(double) * pr.pt * (size_t)M);
  L.idx = take(sizeof(int) * pr.s * (size_t)P * kIters);
  L.models = take(sizeof(double) * pr.model * hyp);
  L.hyp = take(sizeof(int) * hyp);
  L.n_hyp = take(sizeof(int) * (size_t)P);
  L.best = take(sizeof(int) * (size_t)P);
  L.bits = take((size_t)M);
  L.total = o;
  return L;
}
struct Workspace { int* status; long* start; int* counts; double* pts; int* idx; double* models; int *hyp, *n_hyp, *best; uint8_t* bits; };
inline Workspace workspace(void* ws, const Layout& L) {
  char* w = (char*)ws;
  return {(int*)w, (long*)(w + L.start), (int*)(w + L.counts), (double*)(w + L.pts), (int*)(w + L.idx), (double*)(w + L.models),
          (int*)(w + L.hyp), (int*)(w + L.n_hyp), (int*)(w + L.best), (uint8_t*)(w + L.bits)};
}

// grids are ceil(M / 256) and ceil(P * kIters / 64) blocks; sample indices and hypothesis slots are ints
inline bool too_large(long M, int P) { return (M + 255) / 256 >= (1L << 31) || M >= (1L << 31) || (long)P * kIters >= (1L << 31); }

// the host loop over one pair's counts [kIters, sol] (-1: no such solution): the slot it adopted last, -1 for no model
inline int replay_best(const int* c, long Mp, const Problem& pr, float conf) {
  if (Mp < pr.s) return -1;
  int best = -1;
  long bestn = 0;
  int iters = kIters;
  for (int it = 0; it < iters; ++it)
    for (int sol = 0; sol < pr.sol && c[it * pr.sol + sol] >= 0; ++sol) {
      const long cnt = c[it * pr.sol + sol];
      if (cnt > bestn) {
        bestn = cnt;
        best = it * pr.sol + sol;
        iters = adaptive_iters(cnt, Mp, pr.s, conf, it, iters);
      }
    }
  return bestn < pr.s ? -1 : best;
}

// One batch, P > 0: prep (only with matches), sample, solve and score launched on `s`, the replay on the host, then final.  The four
// callables launch the model's kernels on the workspace and the stream; a failed launch is found by the check after each.
// kSampleSize is pr.s as a constant, for the sample kernel.
template <int kSampleSize, class Prep, class Solve, class Score, class Final>
int run(const long* m_bids, long M, int P, const Problem& pr, float conf, unsigned seed, const Layout& L, const Workspace& W, hipStream_t s,
        Prep prep, Solve solve, Score score, Final final) {
  if (hipMemsetAsync(W.status, 0, sizeof(int), s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  if (M > 0) { prep(dim3((unsigned)((M + 255) / 256)), dim3(256)); LOFTR_CHECK_LAUNCH(); }
  hipLaunchKernelGGL(ransac_sample_kernel<kSampleSize>, dim3((unsigned)((P + 1 + 63) / 64)), dim3(64), 0, s, m_bids, M, P, seed, W.start, W.idx, W.n_hyp);
  LOFTR_CHECK_LAUNCH();
  solve(dim3((unsigned)(((long)P * kIters + 63) / 64)), dim3(64));
  LOFTR_CHECK_LAUNCH();
  score(dim3((unsigned)P, (unsigned)((kIters * pr.sol + kScoreThreads - 1) / kScoreThreads)), dim3(kScoreThreads));
  LOFTR_CHECK_LAUNCH();
  // ---- replay of the host loop over the counts: one copy down, one copy up ----
  std::vector<char> host(L.down);
  if (hipMemcpyAsync(host.data(), W.status, L.down, hipMemcpyDeviceToHost, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  if (hipStreamSynchronize(s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  int st;
  memcpy(&st, host.data(), sizeof(int));
  if (st) return LOFTR_ERR_BAD_ARG;                                     // m_bids out of [0, P) or not grouped by ascending pair
  const long* h_start = (const long*)(host.data() + L.start);
  const int* h_counts = (const int*)(host.data() + L.counts);
  std::vector<int> h_best(P);
  for (int p = 0; p < P; ++p) h_best[p] = replay_best(h_counts + (size_t)p * kIters * pr.sol, h_start[p + 1] - h_start[p], pr, conf);
  if (hipMemcpyAsync(W.best, h_best.data(), sizeof(int) * P, hipMemcpyHostToDevice, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  final(dim3((unsigned)P), dim3(kLanes));
  LOFTR_CHECK_LAUNCH();
  // h_best is pageable host memory that goes out of scope on return: wait for the stream rather than rely on the copy staging it
  if (hipStreamSynchronize(s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  return LOFTR_OK;
}

}  // namespace ransac
