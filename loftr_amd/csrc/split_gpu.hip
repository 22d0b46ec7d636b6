// Track splitting on the GPU (gfx950, wave64, 256 threads per block): loftr_split_tracks_host (split.hip) with the same result bit for
// bit.  Every per-item step is split_core.h's, compiled from the same text; what this file adds is only how the work is
// spread over threads.  A fixed schedule on the caller's stream, nothing read back:
//   memsets                the counts, the round counters and the component lengths to 0, the per-track minimum to all ones;
//   split_check_kernel     (thread per edge / keypoint) the checks, which OR a failed check's bit into counts[1]; the smallest keypoint
//                          of every track by an unsigned atomicMin; next <- -1;
//   split_init_kernel      (thread per edge / keypoint) label (frozen: the track's minimum; free: the keypoint; loose: -1); the state
//                          of every edge (open or ignored);
//   per round r            a memset of best, then
//     split_propose_kernel (thread per edge)  internal / conflict / candidate; a candidate does two unsigned 64-bit atomicMax into best;
//     split_accept_kernel  (thread per edge)  a candidate whose word is best at both components takes a slot of the round's list
//                          (one atomicAdd per wave on the round's counter);
//     split_merge_kernel   (thread per accepted edge)  the splice and the relabelling of its two components, which no other thread
//                          touches: a component is in at most one accepted edge;
//   split_length_kernel    (thread per keypoint)  members per label by integer atomicAdd;
//   split_flag_kernel      roots long enough to be tracks per block; the largest component by a 64-bit atomicMax; scan (scan.hip);
//   split_number_kernel    number and track_len_new of every root;
//   split_write_kernel     (thread per edge / keypoint / track / round)  track_id_new, edge_state, round_accepted, the counts.
// A launch reads only what an earlier launch wrote (the merge kernel reads and writes the labels and links of its own two components
// only).  Every launch after the check returns at once when counts[1] is set, so nothing is read through a bad value and no output
// but the counts is written; a round's launches also return when the round before accepted nothing.  No persistent or waiting
// kernel, no graph, no grid-wide barrier.  Integer atomics only.  Plain C++, ordinary vector stores.
#include <algorithm>
#include "compact_gpu.h"
#include "split_core.h"
#include "stage_timer.h"
#include "tracks_core.h"

namespace {

using namespace split;
using namespace compact;

struct In {
  const int* edge_kp;
  const float* edge_conf;
  long E;
  const int* kp_image;
  const int* track_id;
  long K;
  const uint8_t* track_ok;
  long T;
  int n_images;
};

__device__ __forceinline__ unsigned votes(bool p) { return (unsigned)__popcll(__ballot(p)); }
__device__ __forceinline__ void add_votes(u64* counts, int slot, bool p) {
  const unsigned n = votes(p);
  if (threadIdx.x % 64 == 0 && n) atomicAdd(counts + slot, (u64)n);
}
// the rounds' gate: a bad table, or a round before this one that accepted nothing (the same in every thread)
__device__ __forceinline__ bool round_idle(const u64* counts, const int* accepted_n, int r) {
  return counts[kErrors] != 0 || (r > 0 && accepted_n[r - 1] == 0);
}

// grid ceil(max(E, K) / 256) x 256
__global__ void __launch_bounds__(kBlock) split_check_kernel(In a, unsigned* __restrict__ track_min, int* __restrict__ next, u64* counts) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  int err = 0;
  if (i < a.E) err |= check_edge(a.edge_kp, a.edge_conf, a.K, i);
  if (i < a.K) {
    const int bad = check_keypoint(a.kp_image, a.track_id, a.T, a.n_images, i);
    err |= bad;
    if (!(bad & kBadKeypoint) && a.track_id[i] >= 0) atomicMin(track_min + a.track_id[i], (unsigned)i);
    next[i] = -1;
  }
  if (err) atomicOr(counts + kErrors, (u64)err);
}

// grid ceil(max(E, K) / 256) x 256
__global__ void __launch_bounds__(kBlock) split_init_kernel(In a, const unsigned* __restrict__ track_min, int* __restrict__ label,
                                                            uint8_t* __restrict__ state, const u64* counts) {
  if (counts[kErrors] != 0) return;                                              // uniform: a bad table is not read
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i < a.K) {
    const int t = a.track_id[i];
    label[i] = t < 0 ? -1 : (a.track_ok[t] ? (int)track_min[t] : (int)i);
  }
  if (i < a.E) state[i] = edge_open(a.edge_kp, a.track_id, a.track_ok, i) ? kOpen : kIgnored;
}

// grid ceil(E / 256) x 256
__global__ void __launch_bounds__(kBlock) split_propose_kernel(In a, const int* __restrict__ label, const int* __restrict__ next,
                                                               uint8_t* __restrict__ state, u64* __restrict__ best,
                                                               const int* __restrict__ accepted_n, int r, u64* counts) {
  if (round_idle(counts, accepted_n, r)) return;
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= a.E || state[e] != kOpen) return;
  const int la = label[a.edge_kp[2 * e]], lb = label[a.edge_kp[2 * e + 1]];
  if (la == lb) { state[e] = kInternal; return; }
  const int shared = shared_image(next, a.kp_image, a.n_images, la, lb);
  if (shared < 0) { atomicOr(counts + kErrors, (u64)kTooLong); return; }
  if (shared) { state[e] = kConflict; return; }
  const u64 w = (u64)atlas::pack(a.edge_conf[e], (uint32_t)e);
  atomicMax(best + la, w);
  atomicMax(best + lb, w);
}

// grid ceil(E / 256) x 256
__global__ void __launch_bounds__(kBlock) split_accept_kernel(In a, const int* __restrict__ label, const uint8_t* __restrict__ state,
                                                              const u64* __restrict__ best, int* __restrict__ accepted_n, int r,
                                                              int* __restrict__ accepted, const u64* counts) {
  if (round_idle(counts, accepted_n, r)) return;
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  bool won = false;
  if (e < a.E && state[e] == kOpen) {
    const u64 w = (u64)atlas::pack(a.edge_conf[e], (uint32_t)e);
    won = best[label[a.edge_kp[2 * e]]] == w && best[label[a.edge_kp[2 * e + 1]]] == w;
  }
  const u64 b = __ballot(won);                                                   // one atomicAdd per wave claims its slots
  if (b == 0ull) return;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0) base = atomicAdd(accepted_n + r, (int)__popcll(b));
  base = __shfl(base, 0, 64);
  if (won) accepted[base + (int)__popcll(b & ((1ull << lane) - 1ull))] = (int)e;
}

// grid ceil(min(E, K / 2 + 1) / 256) x 256: at most one accepted edge per two components
__global__ void __launch_bounds__(kBlock) split_merge_kernel(In a, int* __restrict__ label, int* __restrict__ next, uint8_t* __restrict__ state,
                                                             const int* __restrict__ accepted_n, int r, const int* __restrict__ accepted,
                                                             u64* counts) {
  if (round_idle(counts, accepted_n, r)) return;
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= accepted_n[r]) return;
  const long e = accepted[i];
  const int la = label[a.edge_kp[2 * e]], lb = label[a.edge_kp[2 * e + 1]];
  if (splice(next, label, a.n_images, la < lb ? la : lb, la < lb ? lb : la) < 0) atomicOr(counts + kErrors, (u64)kTooLong);
  state[e] = kInternal;
}

// grid ceil(K / 256) x 256
__global__ void __launch_bounds__(kBlock) split_length_kernel(long K, const int* __restrict__ label, int* __restrict__ len, const u64* counts) {
  if (counts[kErrors] != 0) return;
  const long k = (long)blockIdx.x * kBlock + threadIdx.x;
  if (k < K && label[k] >= 0) atomicAdd(len + label[k], 1);
}

// grid ceil(K / 256) x 256.  On a bad table every block counts 0, so the scan leaves counts[0] = 0.
__global__ void __launch_bounds__(kBlock) split_flag_kernel(In a, const int* __restrict__ label, const int* __restrict__ len, int min_track_len,
                                                            unsigned* __restrict__ block_counts, u64* counts) {
  const bool bad = counts[kErrors] != 0;
  const long k = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool root = !bad && k < a.K && label[k] == (int)k;
  unsigned tot;
  block_rank(root && len[k] >= min_track_len, &tot);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = tot;
  int most = root && is_free(a.track_id, a.track_ok, k) ? len[k] : 0;            // the largest grown component: a maximum per wave first
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) most = max(most, __shfl_xor(most, o, 64));
  if (threadIdx.x % 64 == 0 && most > 0) atomicMax(counts + kLargest, (u64)most);
}

// grid ceil(K / 256) x 256
__global__ void __launch_bounds__(kBlock) split_number_kernel(long K, const int* __restrict__ label, const int* __restrict__ len,
                                                              int min_track_len, const unsigned* __restrict__ block_offsets,
                                                              int* __restrict__ number, int* __restrict__ track_len_new, const u64* counts) {
  if (counts[kErrors] != 0) return;                                              // uniform
  const long k = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool root = k < K && label[k] == (int)k && len[k] >= min_track_len;
  unsigned tot;
  const long t = (long)block_offsets[blockIdx.x] + block_rank(root, &tot);
  if (!root) return;
  number[k] = (int)t;
  track_len_new[t] = len[k];
}

// grid ceil(max(E, K, T, max_rounds) / 256) x 256
__global__ void __launch_bounds__(kBlock) split_write_kernel(In a, const int* __restrict__ label, const int* __restrict__ len,
                                                             const int* __restrict__ number, const uint8_t* __restrict__ state,
                                                             const int* __restrict__ accepted_n, int min_track_len, int max_rounds,
                                                             int* __restrict__ track_id_new, uint8_t* __restrict__ edge_state,
                                                             int* __restrict__ round_accepted, u64* counts) {
  if (counts[kErrors] != 0) return;                                              // uniform: no output but the counts
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  bool free_kp = false, rescued = false;
  if (i < a.K) {
    const int l = label[i];
    const int id = l >= 0 && len[l] >= min_track_len ? number[l] : -1;
    track_id_new[i] = id;
    free_kp = is_free(a.track_id, a.track_ok, i);
    rescued = free_kp && id >= 0;
  }
  const int st = i < a.E ? (int)state[i] : -1;
  if (i < a.E) edge_state[i] = (uint8_t)st;
  const int acc = i < max_rounds ? accepted_n[i] : 0;
  if (i < max_rounds) round_accepted[i] = acc;
  add_votes(counts, kBadKeypoints, free_kp);
  add_votes(counts, kRescued, rescued);
  for (int s = kIgnored; s <= kOpen; ++s) add_votes(counts, kIgnoredEdges + s, st == s);
  add_votes(counts, kBadTracks, i < a.T && a.track_ok[i] == 0);
  add_votes(counts, kRounds, acc > 0);
}

struct Layout {
  size_t block_counts, partials, track_min, label, next, len, number, state, best, accepted_n, accepted, total;
};
long merge_items(long E, long K) { return std::min(E, K / 2 + 1); }
Layout layout(long E, long K, long T, int max_rounds) {
  Layout L;
  const long nb = std::max(blocks_of(K), 1L);
  size_t o = 0;
  auto take = [&o](size_t bytes) { return tracks::carve(&o, bytes); };
  L.block_counts = take(sizeof(unsigned) * (size_t)nb);
  L.partials = take(sizeof(unsigned) * (size_t)std::max(scan_blocks(nb), 1L));
  L.track_min = take(sizeof(unsigned) * (size_t)std::max(T, 1L));
  L.label = take(sizeof(int) * (size_t)std::max(K, 1L));
  L.next = take(sizeof(int) * (size_t)std::max(K, 1L));
  L.len = take(sizeof(int) * (size_t)std::max(K, 1L));
  L.number = take(sizeof(int) * (size_t)std::max(K, 1L));
  L.state = take((size_t)std::max(E, 1L));
  L.best = take(sizeof(u64) * (size_t)std::max(K, 1L));
  L.accepted_n = take(sizeof(int) * (size_t)std::max(max_rounds, 1));
  L.accepted = take(sizeof(int) * (size_t)std::max(merge_items(E, K), 1L));
  L.total = o;
  return L;
}

}  // namespace

extern "C" size_t loftr_split_tracks_workspace_bytes(long E, long K, long T, int max_rounds) {
  if (!sizes_ok(E, K, T, 0, max_rounds)) return 0;
  return layout(E, K, T, max_rounds).total;
}

extern "C" int loftr_split_tracks(const int* edge_kp, const float* edge_conf, long E, const int* kp_image, const int* track_id, long K,
                                  const uint8_t* track_ok, long T, int n_images, int min_track_len, int max_rounds, int* track_id_new,
                                  int* track_len_new, uint8_t* edge_state, int* round_accepted, long* counts, void* ws, size_t ws_bytes,
                                  float* stage_ms, void* stream) {
  LOFTR_CHECK_ARG(counts && ws && E >= 0 && K >= 0 && T >= 0 && n_images >= 0 && min_track_len >= 1 && max_rounds >= 0);
  LOFTR_CHECK_ARG(E == 0 || (edge_kp && edge_conf && edge_state));
  LOFTR_CHECK_ARG(K == 0 || (kp_image && track_id && track_id_new && track_len_new));
  LOFTR_CHECK_ARG((T == 0 || track_ok) && (max_rounds == 0 || round_accepted));
  if (!sizes_ok(E, K, T, n_images, max_rounds)) return LOFTR_ERR_UNSUPPORTED;
  const Layout L = layout(E, K, T, max_rounds);
  if (ws_bytes < L.total) return LOFTR_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  unsigned *block_counts = (unsigned*)(w + L.block_counts), *partials = (unsigned*)(w + L.partials), *track_min = (unsigned*)(w + L.track_min);
  int *label = (int*)(w + L.label), *next = (int*)(w + L.next), *len = (int*)(w + L.len), *number = (int*)(w + L.number);
  int *accepted_n = (int*)(w + L.accepted_n), *accepted = (int*)(w + L.accepted);
  uint8_t* state = (uint8_t*)(w + L.state);
  u64 *best = (u64*)(w + L.best), *cnt = (u64*)counts;
  const In a{edge_kp, edge_conf, E, kp_image, track_id, K, track_ok, T, n_images};
  StageTimer timer(stage_ms, LOFTR_SPLIT_STAGES(max_rounds), s);
  auto fill = [s](void* p, int v, size_t bytes) { return hipMemsetAsync(p, v, bytes, s) == hipSuccess; };
  const unsigned nbe = (unsigned)std::max(blocks_of(E), 1L), nbk = (unsigned)std::max(blocks_of(K), 1L);
  const unsigned nbm = (unsigned)std::max(blocks_of(merge_items(E, K)), 1L);

  if (!fill(counts, 0, sizeof(long) * kCounts) || !fill(accepted_n, 0, sizeof(int) * (size_t)std::max(max_rounds, 1)) ||
      !fill(len, 0, sizeof(int) * (size_t)std::max(K, 1L)) || !fill(track_min, 0xFF, sizeof(unsigned) * (size_t)std::max(T, 1L)))
    return LOFTR_ERR_LAUNCH;
  timer.mark();
  hipLaunchKernelGGL(split_check_kernel, dim3(std::max(nbe, nbk)), dim3(kBlock), 0, s, a, track_min, next, cnt);
  LOFTR_CHECK_LAUNCH();
  hipLaunchKernelGGL(split_init_kernel, dim3(std::max(nbe, nbk)), dim3(kBlock), 0, s, a, track_min, label, state, cnt);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  const bool rounds = E > 0 && K > 0;                                              // (the marks do not depend on it: a stage keeps its slot)
  for (int r = 0; r < max_rounds; ++r) {
    if (rounds && !fill(best, 0, sizeof(u64) * (size_t)K)) return LOFTR_ERR_LAUNCH;
    timer.mark();
    if (rounds) hipLaunchKernelGGL(split_propose_kernel, dim3(nbe), dim3(kBlock), 0, s, a, label, next, state, best, accepted_n, r, cnt);
    LOFTR_CHECK_LAUNCH();
    timer.mark();
    if (rounds) hipLaunchKernelGGL(split_accept_kernel, dim3(nbe), dim3(kBlock), 0, s, a, label, state, best, accepted_n, r, accepted, cnt);
    LOFTR_CHECK_LAUNCH();
    timer.mark();
    if (rounds) hipLaunchKernelGGL(split_merge_kernel, dim3(nbm), dim3(kBlock), 0, s, a, label, next, state, accepted_n, r, accepted, cnt);
    LOFTR_CHECK_LAUNCH();
    timer.mark();
  }
  if (K > 0) {
    hipLaunchKernelGGL(split_length_kernel, dim3(nbk), dim3(kBlock), 0, s, K, label, len, cnt);
    LOFTR_CHECK_LAUNCH();
    hipLaunchKernelGGL(split_flag_kernel, dim3(nbk), dim3(kBlock), 0, s, a, label, len, min_track_len, block_counts, cnt);
    LOFTR_CHECK_LAUNCH();
    if (scan_u32(block_counts, nbk, partials, counts + kTracks, s) != LOFTR_OK) return LOFTR_ERR_LAUNCH;
    hipLaunchKernelGGL(split_number_kernel, dim3(nbk), dim3(kBlock), 0, s, K, label, len, min_track_len, block_counts, number, track_len_new,
                       cnt);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  const long most = std::max(std::max(E, K), std::max(T, (long)max_rounds));
  hipLaunchKernelGGL(split_write_kernel, dim3((unsigned)std::max(blocks_of(most), 1L)), dim3(kBlock), 0, s, a, label, len, number, state,
                     accepted_n, min_track_len, max_rounds, track_id_new, edge_state, round_accepted, cnt);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  return timer.finish();
}
