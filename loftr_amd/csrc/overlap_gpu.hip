// View overlap on the GPU: loftr_view_overlap_host (overlap.hip) with the same integers.  Every per-entry step is
// overlap_core.h's, compiled from the same text, fp64 without FMA contraction; what this file adds is only how the work is spread over
// threads.  A fixed schedule on the caller's stream, nothing read back:
//   memsets                                      overlap [n, m], n_vis [n] and counts to 0;
//   overlap_check_kernel  (thread per source and per entry)  vis_offsets, the range of vis_point; a failed check ORs its bit into counts[1];
//   overlap_setup_kernel  (a wave per source, then a thread per target)  the view tables (an invalid view is all NaN); the wave of a
//                         valid source walks its list 64 entries at a time and sums the usable ones (ballot + popcount) into n_vis[i];
//   overlap_count_kernel  (block = source i x a tile of kTile targets)  each lane owns ONE target, its table in registers; the block stages
//                         the source's entries kTile at a time into LDS as X, a = c_i - X, aa (computed once per point, not once per
//                         target; an unusable entry is staged as NaN, which fails the predicate's first comparison); every lane walks the
//                         chunk through broadcast LDS reads and keeps its own integer count; the lane writes one overlap[i, j].
// No value that a kernel writes is read in the same kernel: counts[1] is raised by the check kernel and read by the two others, which
// return at once on a bad list and so read nothing through a bad value; the outputs then stay as the memsets left them.  n_vis and the
// tables are written by the setup kernel and read by the count kernel.  No persistent or waiting kernel, no graph, no float atomics:
// integer atomics only for the error word and the counts.  Plain C++, ordinary vector stores.
#include "common.h"
#include "overlap_core.h"
#include "stage_timer.h"

#pragma clang fp contract(off)

namespace {

using namespace overlap;

typedef unsigned long long u64;
constexpr int kThreads = 256;
constexpr int kTile = LOFTR_OVERLAP_TILE;                                        // targets per block = entries per staged chunk
constexpr int kSlot = 8;                                                         // doubles per staged entry (kPoint, padded to 64 bytes)
static_assert(kTile == kThreads && kPoint <= kSlot, "one lane per target and per staged entry");

struct In {
  const long* vis_offsets; const int* vis_point; long V;
  const float* xyz; const uint8_t* point_ok; long T;
  const double* K_src; const double* T_src; const uint8_t* src_ok; int n;
  const double* K_tgt; const double* T_tgt; const uint8_t* tgt_ok; const double* tgt_hw; int m;
  double border, cos_min, max_scale2;
};

__device__ __forceinline__ unsigned votes(bool p) { return (unsigned)__popcll(__ballot(p)); }

// grid ceil(max(n, V) / 256) x 256
__global__ void __launch_bounds__(kThreads) overlap_check_kernel(In a, u64* counts) {
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  int err = 0;
  if (t < a.n) err |= check_source(a.vis_offsets, a.n, a.V, (int)t);
  if (t < a.V) err |= check_entry(a.vis_point, a.T, t);
  if (err) atomicOr(counts + kErrors, (u64)err);
}

// grid (n + ceil(m / 64)) x 64: block b < n is source b, the blocks after them hold 64 targets each
__global__ void __launch_bounds__(64) overlap_setup_kernel(In a, double* __restrict__ src_tab, double* __restrict__ tgt_tab,
                                                           int* __restrict__ n_vis, u64* counts) {
  if (counts[kErrors] != 0) return;                                              // uniform: a bad list is not read
  const int lane = threadIdx.x;
  double t[kView];
  if ((long)blockIdx.x < a.n) {
    const long i = blockIdx.x;
    view_table(a.K_src + 9 * i, a.T_src + 16 * i, a.src_ok[i] != 0, nullptr, a.border, t);        // the same in every lane
    if (lane == 0) for (int k = 0; k < kView; ++k) src_tab[kView * i + k] = t[k];
    if (!view_valid(t)) return;                                                  // n_vis[i] stays 0
    const long b = a.vis_offsets[i], e = a.vis_offsets[i + 1];
    unsigned vis = 0;
    for (long k0 = b; k0 < e; k0 += 64) {
      const long k = k0 + lane;
      double X[3];
      vis += votes(k < e && usable(a.xyz, a.point_ok, a.vis_point[k], X));       // (vis_point[k] is read only when k < e)
    }
    if (lane == 0) {
      n_vis[i] = (int)vis;
      atomicAdd(counts + kSources, (u64)1);
      if (vis) atomicAdd(counts + kVisible, (u64)vis);
    }
    return;
  }
  const long j = ((long)blockIdx.x - a.n) * 64 + lane;
  bool valid = false;
  if (j < a.m) {
    view_table(a.K_tgt + 9 * j, a.T_tgt + 16 * j, a.tgt_ok[j] != 0, a.tgt_hw + 2 * j, a.border, t);
    for (int k = 0; k < kView; ++k) tgt_tab[kView * j + k] = t[k];
    valid = view_valid(t);
  }
  const unsigned nv = votes(valid);
  if (lane == 0 && nv) atomicAdd(counts + kTargets, (u64)nv);
}

// grid n x ceil(m / kTile), kTile threads
__global__ void __launch_bounds__(kThreads) overlap_count_kernel(In a, const double* __restrict__ src_tab, const double* __restrict__ tgt_tab,
                                                                 const int* __restrict__ n_vis, int* __restrict__ overlap_out, u64* counts) {
  __shared__ double sh[kTile * kSlot];
  if (counts[kErrors] != 0) return;                                              // uniform
  const long i = blockIdx.x;
  if (n_vis[i] == 0) return;                                                     // uniform: an invalid source, or nothing usable
  const int tid = threadIdx.x;
  const long j = (long)blockIdx.y * kTile + tid;
  double tab[kView];
  for (int k = 0; k < kView; ++k) tab[k] = j < a.m ? tgt_tab[kView * j + k] : __builtin_nan("");
  const bool active = view_valid(tab);
  const double* src = src_tab + kView * i;
  const double f2i = src[tri::kCam];
  const long b = a.vis_offsets[i], e = a.vis_offsets[i + 1];
  int count = 0;
  for (long k0 = b; k0 < e; k0 += kTile) {
    __syncthreads();                                                             // the chunk before this one has been walked
    double pt[kSlot], X[3];
    for (int c = 0; c < kSlot; ++c) pt[c] = __builtin_nan("");
    const long k = k0 + tid;
    if (k < e && usable(a.xyz, a.point_ok, a.vis_point[k], X)) point_terms(src, X, pt);
    for (int c = 0; c < kSlot; ++c) sh[tid * kSlot + c] = pt[c];
    __syncthreads();
    const int len = e - k0 < kTile ? (int)(e - k0) : kTile;
    if (active)
      for (int s = 0; s < len; ++s) count += counts_for(tab, sh + s * kSlot, f2i, a.border, a.cos_min, a.max_scale2);
  }
  if (active) overlap_out[i * a.m + j] = count;
  const unsigned nz = votes(active && count != 0);
  if (tid % 64 == 0 && nz) atomicAdd(counts + kNonZero, (u64)nz);
}

size_t layout(int n, int m, size_t* tgt_at) {
  size_t off = 0;
  tracks::carve(&off, sizeof(double) * kView * (size_t)(n > 0 ? n : 1));
  const size_t at = tracks::carve(&off, sizeof(double) * kView * (size_t)(m > 0 ? m : 1));
  if (tgt_at) *tgt_at = at;
  return off;
}

}  // namespace

extern "C" size_t loftr_view_overlap_workspace_bytes(int n, int m) {
  if (n < 0 || m < 0 || (long)n * (long)m > (1L << 31)) return 0;
  return layout(n, m, nullptr);
}

extern "C" int loftr_view_overlap(const long* vis_offsets, const int* vis_point, long V, const float* xyz, const uint8_t* point_ok, long T,
                                  const double* K_src, const double* T_src, const uint8_t* src_ok, int n, const double* K_tgt,
                                  const double* T_tgt, const uint8_t* tgt_ok, const double* tgt_hw, int m, double border_px, double cos_min,
                                  double max_scale2, int* overlap_out, int* n_vis, long* counts, void* ws, size_t ws_bytes, float* stage_ms,
                                  void* stream) {
  LOFTR_CHECK_ARG(counts && ws && V >= 0 && T >= 0 && n >= 0 && m >= 0);
  LOFTR_CHECK_ARG(n == 0 || (vis_offsets && K_src && T_src && src_ok && n_vis));
  LOFTR_CHECK_ARG(m == 0 || (K_tgt && T_tgt && tgt_ok && tgt_hw));
  LOFTR_CHECK_ARG(V == 0 || vis_point);
  LOFTR_CHECK_ARG(T == 0 || (xyz && point_ok));
  LOFTR_CHECK_ARG(n == 0 || m == 0 || overlap_out);
  LOFTR_CHECK_ARG(params_ok(border_px, cos_min, max_scale2));
  LOFTR_CHECK_ARG(n > 0 || V == 0);                                              // entries outside every list
  if (!sizes_ok(V, T, n, m)) return LOFTR_ERR_UNSUPPORTED;
  const long tiles = ((long)m + kTile - 1) / kTile;
  if (tiles > 65535) return LOFTR_ERR_UNSUPPORTED;
  size_t tgt_at;
  if (ws_bytes < layout(n, m, &tgt_at)) return LOFTR_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  double* src_tab = (double*)ws;
  double* tgt_tab = (double*)((char*)ws + tgt_at);
  u64* cnt = (u64*)counts;
  const In a{vis_offsets, vis_point, V, xyz, point_ok, T, K_src, T_src, src_ok, n, K_tgt, T_tgt, tgt_ok, tgt_hw, m, border_px, cos_min, max_scale2};
  StageTimer timer(stage_ms, LOFTR_OVERLAP_STAGES, s);
  auto blocks = [](long items, long per) { return (unsigned)(items > 0 ? (items + per - 1) / per : 1); };
  if (n > 0 && m > 0 && hipMemsetAsync(overlap_out, 0, sizeof(int) * (size_t)n * (size_t)m, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  if (n > 0 && hipMemsetAsync(n_vis, 0, sizeof(int) * (size_t)n, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  if (hipMemsetAsync(counts, 0, sizeof(long) * kCounts, s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  timer.mark();
  if (n > 0) {
    hipLaunchKernelGGL(overlap_check_kernel, dim3(blocks(V > n ? V : n, kThreads)), dim3(kThreads), 0, s, a, cnt);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  if (n > 0 || m > 0) {
    hipLaunchKernelGGL(overlap_setup_kernel, dim3((unsigned)n + (m > 0 ? blocks(m, 64) : 0u)), dim3(64), 0, s, a, src_tab, tgt_tab, n_vis, cnt);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  if (n > 0 && m > 0) {
    hipLaunchKernelGGL(overlap_count_kernel, dim3((unsigned)n, (unsigned)tiles), dim3(kThreads), 0, s, a, src_tab, tgt_tab, n_vis, overlap_out, cnt);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  return timer.finish();
}
