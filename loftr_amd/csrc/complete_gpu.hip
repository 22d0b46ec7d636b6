// Track completion on the GPU: loftr_complete_tracks_host (complete.hip) with the same result bit for bit.  Every
// per-item step is complete_core.h's, compiled from the same text, fp64 without FMA contraction; what this file adds is only how the
// work is spread over threads.  A fixed schedule on the caller's stream, nothing read back:
//   memsets                                        claim [K] to all ones (the empty claim), counts to 0;
//   complete_camera_kernel   (thread per image)    the camera table of tri::cam_table; an invalid camera is all NaN;
//   complete_check_kernel    (thread per row, keypoint and image)  offsets, image ids, their order within a row, kp_offsets, the range
//                                                  of kp_row; a failed check ORs its bit into counts[1];
//   complete_link_kernel     (thread per row x a chunk of kChunk images per blockIdx.y)  the lane's row is projected into the images
//                            of the chunk in ascending order; the image index, posed[i] and the camera are the same in every lane of a
//                            wave; the lane's cursor into its own ascending observation list starts by a lower bound at the chunk's
//                            first image and advances with the loop (the merge walk of the host routine); a proposal is ONE unsigned
//                            64-bit atomicMin of (f32 bits of r2) << 32 | row into claim[keypoint]; the counts are summed per wave
//                            (ballot + popcount) and added once per wave;
//   complete_resolve_kernel  (thread per keypoint)  kp_row_new, link_r2, counts[0]; counts[6] = proposals - links.
// No value that a kernel writes is read in the same kernel: claim is only written (atomics) by the link kernel and only read by the
// resolve kernel; counts[1] is raised by the check kernel and read by the link kernel, which returns at once on a bad table and so
// reads nothing through a bad value; every claim is then empty and the resolve kernel copies kp_row.  No persistent or waiting kernel,
// no graph, no grid-wide barrier.  Integer atomics only.  Plain C++, ordinary vector stores.
#include "complete_kernels.h"                                                        // the camera table and the table check, shared with merge_gpu.hip
#include "stage_timer.h"

#pragma clang fp contract(off)

namespace {

using namespace complete;

constexpr int kChunk = LOFTR_COMPLETE_IMAGE_CHUNK;                               // images per blockIdx.y (a tuning constant: no result depends on it)

// grid ceil(T / 256) x max(1, ceil(n / kChunk)), 256 threads
__global__ void __launch_bounds__(kThreads) complete_link_kernel(In a, u64* __restrict__ claim, u64* counts) {
  if (counts[kErrors] != 0) return;                                              // uniform: a bad table is not read
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  const int i0 = (int)blockIdx.y * kChunk, i1 = i0 + kChunk < a.n ? i0 + kChunk : a.n;
  double X[3] = {0.0, 0.0, 0.0};
  const bool src = j < a.T && source(a, j, X);
  long cur = 0, end = 0;
  if (src) {
    end = a.offsets[j + 1];
    cur = lower_bound(a.image, a.offsets[j], end, i0);
  }
  const unsigned n_src = blockIdx.y == 0 ? votes(src) : 0u;
  unsigned n_pairs = 0, n_inside = 0, n_prop = 0, n_blocked = 0;
  if (__ballot(src) != 0) {
    for (int i = i0; i < i1; ++i) {
      if (!target_image(a, i)) continue;                                         // the same in every lane
      bool pair = false;
      if (src) {
        while (cur < end && a.image[cur] < i) ++cur;
        pair = !(cur < end && a.image[cur] == i);
      }
      uint32_t bits = 0;
      int flags = 0;
      long k = -1;
      if (pair) {
        k = propose(a, i, X, &bits, &flags);
        if (k >= 0) atomicMin(claim + k, (u64)key(bits, j));
      }
      n_pairs += votes(pair);
      n_inside += votes((flags & kFlagInside) != 0);
      n_prop += votes(k >= 0);
      n_blocked += votes((flags & kFlagBlocked) != 0);
    }
  }
  if (threadIdx.x % 64 == 0) {
    if (n_src) atomicAdd(counts + kSources, (u64)n_src);
    if (n_pairs) atomicAdd(counts + kPairs, (u64)n_pairs);
    if (n_inside) atomicAdd(counts + kInside, (u64)n_inside);
    if (n_prop) { atomicAdd(counts + kProposals, (u64)n_prop); atomicAdd(counts + kLost, (u64)n_prop); }
    if (n_blocked) atomicAdd(counts + kBlocked, (u64)n_blocked);
  }
}

// grid ceil(K / 256) x 256
__global__ void __launch_bounds__(kThreads) complete_resolve_kernel(const u64* __restrict__ claim, const int* __restrict__ kp_row, long K,
                                                                   int* __restrict__ kp_row_new, float* __restrict__ link_r2, u64* counts) {
  const long k = (long)blockIdx.x * kThreads + threadIdx.x;
  bool won = false;
  if (k < K) {
    const u64 w = claim[k];
    won = w != kNoClaim;
    kp_row_new[k] = won ? key_row(w) : kp_row[k];
    link_r2[k] = won ? key_r2(w) : __builtin_nanf("");
  }
  const unsigned n = votes(won);
  if (threadIdx.x % 64 == 0 && n) {
    atomicAdd(counts + kLinks, (u64)n);
    atomicAdd(counts + kLost, (u64)0 - (u64)n);                                  // proposals - links (the link kernel added the proposals)
  }
}

size_t layout(long K, int n_images, size_t* claim_at) {
  size_t off = 0;
  tracks::carve(&off, sizeof(double) * tri::kCam * (size_t)(n_images > 0 ? n_images : 1));
  const size_t at = tracks::carve(&off, sizeof(u64) * (size_t)(K > 0 ? K : 1));
  if (claim_at) *claim_at = at;
  return off;
}

}  // namespace

extern "C" size_t loftr_complete_tracks_workspace_bytes(long T, long N, long K, int n_images) {
  if (!sizes_ok(T, N, K, n_images)) return 0;
  return layout(K, n_images, nullptr);
}

extern "C" int loftr_complete_tracks(const long* offsets, long T, const int* obs_image, long N, const float* xyz, const uint8_t* status,
                                     const long* kp_offsets, const float* keypoints, const int* kp_cell, const int* kp_row, long K,
                                     const double* Kmat, const double* T_cam_from_world, const uint8_t* posed, int n_images, float inv, int gh,
                                     int gw, double thresh_px, int reach, int* kp_row_new, float* link_r2, long* counts, void* ws,
                                     size_t ws_bytes, float* stage_ms, void* stream) {
  LOFTR_CHECK_ARG(offsets && kp_offsets && counts && ws && T >= 0 && N >= 0 && K >= 0 && n_images >= 0 && gh >= 0 && gw >= 0);
  LOFTR_CHECK_ARG(T == 0 || (xyz && status));
  LOFTR_CHECK_ARG(N == 0 || obs_image);
  LOFTR_CHECK_ARG(K == 0 || (keypoints && kp_cell && kp_row && kp_row_new && link_r2));
  LOFTR_CHECK_ARG(n_images == 0 || (Kmat && T_cam_from_world && posed));
  LOFTR_CHECK_ARG(thresh_px >= 0.0 && tri::fin(thresh_px) && reach >= 0 && reach <= kMaxReach);
  LOFTR_CHECK_ARG((T > 0 || N == 0) && (n_images > 0 || K == 0));                 // observations / keypoints outside every row / image
  if (!sizes_ok(T, N, K, n_images) || !grid_ok(gh, gw)) return LOFTR_ERR_UNSUPPORTED;
  const long chunks = n_images > 0 ? ((long)n_images + kChunk - 1) / kChunk : 1;
  if (chunks > 65535) return LOFTR_ERR_UNSUPPORTED;
  size_t claim_at;
  if (ws_bytes < layout(K, n_images, &claim_at)) return LOFTR_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  double* tab = (double*)ws;
  u64* claim = (u64*)((char*)ws + claim_at);
  u64* cnt = (u64*)counts;
  const In a{offsets, T, obs_image, N, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, tab, posed, n_images, inv, gh, gw,
             thresh_px * thresh_px, reach};
  StageTimer timer(stage_ms, LOFTR_COMPLETE_STAGES, s);
  auto blocks = [](long items, long per) { return (unsigned)(items > 0 ? (items + per - 1) / per : 1); };
  if (hipMemsetAsync(claim, 0xFF, sizeof(u64) * (size_t)(K > 0 ? K : 1), s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  if (hipMemsetAsync(counts, 0, sizeof(long) * kCounts, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  timer.mark();
  if (n_images > 0) {
    hipLaunchKernelGGL(complete_camera_kernel, dim3(blocks(n_images, 64)), dim3(64), 0, s, Kmat, T_cam_from_world, n_images, tab);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  const long most = T > K ? (T > n_images ? T : n_images) : (K > n_images ? K : n_images);
  hipLaunchKernelGGL(complete_check_kernel, dim3(blocks(most, kThreads)), dim3(kThreads), 0, s, a, cnt);
  LOFTR_CHECK_LAUNCH();
  timer.mark();
  if (T > 0) {
    hipLaunchKernelGGL(complete_link_kernel, dim3(blocks(T, kThreads), (unsigned)chunks), dim3(kThreads), 0, s, a, claim, cnt);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  if (K > 0) {
    hipLaunchKernelGGL(complete_resolve_kernel, dim3(blocks(K, kThreads)), dim3(kThreads), 0, s, claim, kp_row, K, kp_row_new, link_r2, cnt);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  return timer.finish();
}
