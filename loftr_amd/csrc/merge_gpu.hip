// Track merging on the GPU: loftr_merge_tracks_host (merge.hip) with the same result bit for bit.  Every per-item step is
// merge_core.h's, compiled from the same text, fp64 without FMA contraction; what this file adds is only how the work is spread over
// threads.  A fixed schedule on the caller's stream, nothing read back:
//   memsets                                        best [T] to all ones (the empty entry), counts to 0;
//   complete_camera_kernel, complete_check_kernel  completion's (complete_kernels.h): the camera table; the checks, which OR a failed
//                                                  check's bit into counts[1];
//   merge_meet_kernel     (thread per row x a chunk of kChunk images per blockIdx.y)  the image loop and the cursor of
//                         complete_link_kernel; a meeting runs the disjoint walk and the agreement test inline and, accepted, does two
//                         unsigned 64-bit atomicMins of (f32 bits of the score) << 32 | partner, into best[row] and best[partner];
//                         the counts are summed per wave (ballot + popcount) and added once per wave;
//   merge_pair_kernel     (thread per row)         the mutual test; row_into, merge_r2, counts[0] (a pair counts where j < m);
//   merge_relabel_kernel  (thread per keypoint)    kp_row_new, counts[7].
// No value that a kernel writes is read in the same kernel: best is only written (atomics) by the meet kernel and only read by the pair
// kernel; row_into is written by the pair kernel and read by the relabel kernel; counts[1] is raised by the check kernel and read by the
// meet and relabel kernels: the first returns at once on a bad table, so every entry of best stays empty and the pair kernel writes the
// identity, the second then copies kp_row; nothing is read through a bad value.  No persistent or waiting kernel, no graph, no grid-wide
// barrier.  Integer atomics only.  Plain C++, ordinary vector stores.
#include "complete_kernels.h"
#include "merge_core.h"
#include "stage_timer.h"

#pragma clang fp contract(off)

namespace {

using namespace merge;

constexpr int kChunk = LOFTR_MERGE_IMAGE_CHUNK;                                  // images per blockIdx.y (a tuning constant: no result depends on it)

// grid ceil(T / 256) x max(1, ceil(n / kChunk)), 256 threads
__global__ void __launch_bounds__(kThreads) merge_meet_kernel(In a, u64* __restrict__ best, u64* counts) {
  if (counts[kErrors] != 0) return;                                              // uniform: a bad table is not read
  const complete::In& c = a.c;
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  const int i0 = (int)blockIdx.y * kChunk, i1 = i0 + kChunk < c.n ? i0 + kChunk : c.n;
  double X[3] = {0.0, 0.0, 0.0};
  const bool src = j < c.T && complete::source(c, j, X);
  long cur = 0, end = 0;
  if (src) {
    end = c.offsets[j + 1];
    cur = complete::lower_bound(c.image, c.offsets[j], end, i0);
  }
  const unsigned n_src = blockIdx.y == 0 ? votes(src) : 0u;
  unsigned n_pairs = 0, n_meet = 0, n_disjoint = 0, n_accepted = 0;
  if (__ballot(src) != 0) {
    for (int i = i0; i < i1; ++i) {
      if (!complete::target_image(c, i)) continue;                               // the same in every lane
      bool pair = false;
      if (src) {
        while (cur < end && c.image[cur] < i) ++cur;
        pair = !(cur < end && c.image[cur] == i);
      }
      long m = -1;
      int verdict = 0;
      if (pair) {
        m = meet(a, i, j, X);
        if (m >= 0) {
          uint32_t bits = 0;
          verdict = judge(a, j, m, &bits);
          if (verdict & 2) {
            atomicMin(best + j, (u64)key(bits, m));
            atomicMin(best + m, (u64)key(bits, j));
          }
        }
      }
      n_pairs += votes(pair);
      n_meet += votes(m >= 0);
      n_disjoint += votes((verdict & 1) != 0);
      n_accepted += votes((verdict & 2) != 0);
    }
  }
  if (threadIdx.x % 64 == 0) {
    if (n_src) atomicAdd(counts + kSources, (u64)n_src);
    if (n_pairs) atomicAdd(counts + kPairs, (u64)n_pairs);
    if (n_meet) atomicAdd(counts + kMeetings, (u64)n_meet);
    if (n_disjoint) atomicAdd(counts + kDisjoint, (u64)n_disjoint);
    if (n_accepted) atomicAdd(counts + kAccepted, (u64)n_accepted);
  }
}

// grid ceil(T / 256) x 256
__global__ void __launch_bounds__(kThreads) merge_pair_kernel(const u64* __restrict__ best, long T, int* __restrict__ row_into,
                                                             float* __restrict__ merge_r2, u64* counts) {
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  bool lower = false;
  if (j < T) {
    bool merged;
    float r2 = __builtin_nanf("");
    const long into = survivor((const uint64_t*)best, j, &merged, &r2);
    row_into[j] = (int)into;
    merge_r2[j] = merged ? r2 : __builtin_nanf("");
    lower = merged && into == j;
  }
  const unsigned n = votes(lower);
  if (threadIdx.x % 64 == 0 && n) atomicAdd(counts + kMerged, (u64)n);
}

// grid ceil(K / 256) x 256
__global__ void __launch_bounds__(kThreads) merge_relabel_kernel(const int* __restrict__ row_into, const int* __restrict__ kp_row, long K,
                                                                int* __restrict__ kp_row_new, u64* counts) {
  const bool bad = counts[kErrors] != 0;                                         // uniform: a bad kp_row indexes nothing
  const long k = (long)blockIdx.x * kThreads + threadIdx.x;
  bool changed = false;
  if (k < K) {
    const int row = kp_row[k];
    const int into = (bad || row < 0) ? row : row_into[row];
    kp_row_new[k] = into;
    changed = into != row;
  }
  const unsigned n = votes(changed);
  if (threadIdx.x % 64 == 0 && n) atomicAdd(counts + kRelabelled, (u64)n);
}

size_t layout(long T, int n_images, size_t* best_at) {
  size_t off = 0;
  tracks::carve(&off, sizeof(double) * tri::kCam * (size_t)(n_images > 0 ? n_images : 1));
  const size_t at = tracks::carve(&off, sizeof(u64) * (size_t)(T > 0 ? T : 1));
  if (best_at) *best_at = at;
  return off;
}

}  // namespace

extern "C" size_t loftr_merge_tracks_workspace_bytes(long T, long N, long K, int n_images) {
  if (!complete::sizes_ok(T, N, K, n_images)) return 0;
  return layout(T, n_images, nullptr);
}

extern "C" int loftr_merge_tracks(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                                  const float* xyz, const uint8_t* status, const long* kp_offsets, const float* keypoints, const int* kp_cell,
                                  const int* kp_row, long K, const double* Kmat, const double* T_cam_from_world, const uint8_t* posed,
                                  int n_images, float inv, int gh, int gw, double thresh_px, int reach, int* row_into, float* merge_r2,
                                  int* kp_row_new, long* counts, void* ws, size_t ws_bytes, float* stage_ms, void* stream) {
  LOFTR_CHECK_ARG(offsets && kp_offsets && counts && ws && T >= 0 && N >= 0 && K >= 0 && n_images >= 0 && gh >= 0 && gw >= 0);
  LOFTR_CHECK_ARG(T == 0 || (xyz && status && row_into && merge_r2));
  LOFTR_CHECK_ARG(N == 0 || (obs_image && obs_xy && obs_mask));
  LOFTR_CHECK_ARG(K == 0 || (keypoints && kp_cell && kp_row && kp_row_new));
  LOFTR_CHECK_ARG(n_images == 0 || (Kmat && T_cam_from_world && posed));
  LOFTR_CHECK_ARG(thresh_px >= 0.0 && tri::fin(thresh_px) && reach >= 0 && reach <= complete::kMaxReach);
  LOFTR_CHECK_ARG((T > 0 || N == 0) && (n_images > 0 || K == 0));                 // observations / keypoints outside every row / image
  if (!complete::sizes_ok(T, N, K, n_images) || !complete::grid_ok(gh, gw)) return LOFTR_ERR_UNSUPPORTED;
  const long chunks = n_images > 0 ? ((long)n_images + kChunk - 1) / kChunk : 1;
  if (chunks > 65535) return LOFTR_ERR_UNSUPPORTED;
  size_t best_at;
  if (ws_bytes < layout(T, n_images, &best_at)) return LOFTR_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  double* tab = (double*)ws;
  u64* best = (u64*)((char*)ws + best_at);
  u64* cnt = (u64*)counts;
  const In a{{offsets, T, obs_image, N, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, tab, posed, n_images, inv, gh, gw,
              thresh_px * thresh_px, reach}, obs_xy, obs_mask};
  StageTimer timer(stage_ms, LOFTR_MERGE_STAGES, s);
  auto blocks = [](long items, long per) { return (unsigned)(items > 0 ? (items + per - 1) / per : 1); };
  if (hipMemsetAsync(best, 0xFF, sizeof(u64) * (size_t)(T > 0 ? T : 1), s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  if (hipMemsetAsync(counts, 0, sizeof(long) * kCounts, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  timer.mark();
  if (n_images > 0) {
    hipLaunchKernelGGL(complete_camera_kernel, dim3(blocks(n_images, 64)), dim3(64), 0, s, Kmat, T_cam_from_world, n_images, tab);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  const long most = T > K ? (T > n_images ? T : n_images) : (K > n_images ? K : n_images);
  hipLaunchKernelGGL(complete_check_kernel, dim3(blocks(most, kThreads)), dim3(kThreads), 0, s, a.c, cnt);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  if (T > 0) {
    hipLaunchKernelGGL(merge_meet_kernel, dim3(blocks(T, kThreads), (unsigned)chunks), dim3(kThreads), 0, s, a, best, cnt);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  if (T > 0) {
    hipLaunchKernelGGL(merge_pair_kernel, dim3(blocks(T, kThreads)), dim3(kThreads), 0, s, best, T, row_into, merge_r2, cnt);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  if (K > 0) {
    hipLaunchKernelGGL(merge_relabel_kernel, dim3(blocks(K, kThreads)), dim3(kThreads), 0, s, row_into, kp_row, K, kp_row_new, cnt);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  return timer.finish();
}
