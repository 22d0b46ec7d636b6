// Keypoint atlas on the GPU (gfx950, wave64): loftr_atlas_observe + loftr_atlas_finalize reproduce loftr_atlas_host (atlas.hip) bit for bit.
// No MFMA, no float atomic: every reduction is a 64-bit unsigned max (the packed word of atlas_core.h), an integer add or a compare-and-swap,
// so the result does not depend on the order in which the atomics arrive.  A slot's POSITION in the hash table may vary from run to run;
// its key -> value mapping may not.  Every atomically written value is read only by a later kernel, with one exception: the union-find
// parents, which are read with relaxed agent-scope atomic loads (a plain load may be served from another XCD's stale L2 line).
//
//   observe   (per add)  a thread per match: record + one atomicMax per side into the dense per-image cell grid (8 bytes per cell)
//   compact              occupied cells per block (ballot + popcount) -> exclusive scan -> keypoints; grid word <- keypoint index
//   resolve              (k_a, k_b) per match, n_obs by integer atomicAdd, table[(row, side, keypoint)] <- max packed (conf, match)
//   mutual best          a match is kept when it is the table's winner on both sides; count -> scan -> write matches and row offsets
//   tracks               union-find over the kept matches (larger root hooked under the smaller by atomicCAS, path halving),
//                        flatten + lengths + table[(label, image)] counts, same-image flags, flag -> scan -> number
// The one u32 scan (scan.hip: reduce / scan / downsweep over per-block counts) serves the cells, the keep flags and the track flags;
// it, the block helpers and the table are compact_gpu.h's.
#include <algorithm>
#include "compact_gpu.h"
#include "stage_timer.h"
#include "tracks_core.h"

namespace {

using namespace atlas;
using namespace compact;

// ---- observe ---------------------------------------------------------------------------------------------------------------------
__global__ void atlas_observe_kernel(const float* __restrict__ kpts0, const float* __restrict__ kpts1, const float* __restrict__ conf,
                                     const long* __restrict__ m_bids, const uint8_t* __restrict__ mask, long n, int n_rows, long match_base,
                                     long row_base, const int* __restrict__ row_images, int n_images, int gh, int gw, float inv,
                                     u64* __restrict__ grid, float* __restrict__ obs_xy, int* __restrict__ obs_cell, float* __restrict__ m_conf,
                                     int* __restrict__ m_row, uint8_t* __restrict__ m_reason, int* __restrict__ status) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const long m = match_base + i, bid = m_bids[i];
  const bool row_ok = bid >= 0 && bid < n_rows;
  int bad = row_ok ? 0 : kStatusBadRow;
  if (i > 0 && m_bids[i - 1] > bid) bad |= kStatusUnsorted;
  if (bad) atomicOr(status, bad);
  const long row = row_base + (row_ok ? bid : (bid < 0 ? 0 : n_rows - 1));      // kept in range and ascending for the later kernels
  const float x0 = kpts0[2 * i], y0 = kpts0[2 * i + 1], x1 = kpts1[2 * i], y1 = kpts1[2 * i + 1], c = conf[i];
  int c0, c1;
  int why = classify(x0, y0, x1, y1, c, row_ok, mask && !mask[i], inv, gw, gh, &c0, &c1);
  int ia = 0, ib = 0;
  if (why == kValid) {
    ia = row_images[2 * row];
    ib = row_images[2 * row + 1];
    if (ia < 0 || ia >= n_images || ib < 0 || ib >= n_images) why = kBadRow;  // (the caller checks the ids; never index the grid with a bad one)
  }
  const long cpi = (long)gh * gw;
  const int g0 = why == kValid ? (int)(ia * cpi + c0) : -1, g1 = why == kValid ? (int)(ib * cpi + c1) : -1;
  obs_xy[4 * m] = x0; obs_xy[4 * m + 1] = y0; obs_xy[4 * m + 2] = x1; obs_xy[4 * m + 3] = y1;
  obs_cell[2 * m] = g0;
  obs_cell[2 * m + 1] = g1;
  m_conf[m] = c;
  m_row[m] = (int)row;
  m_reason[m] = (uint8_t)why;
  if (why == kValid) {
    atomicMax(&grid[g0], (u64)pack(c, (uint32_t)(2 * m)));
    atomicMax(&grid[g1], (u64)pack(c, (uint32_t)(2 * m + 1)));
  }
}

// ---- compact ---------------------------------------------------------------------------------------------------------------------
__global__ void atlas_count_cells_kernel(const u64* __restrict__ grid, long G, unsigned* __restrict__ block_counts) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  unsigned tot;
  block_rank(i < G && grid[i] != 0ull, &tot);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = tot;
}

// keypoint k of an occupied cell = cells occupied before it; the word of the cell becomes k.  Also the per-keypoint state of the later
// stages (n_obs, union-find parent, length, same-image flag) and kp_offsets (the rank of every image's first cell).
__global__ void atlas_write_keypoints_kernel(u64* __restrict__ grid, long G, const unsigned* __restrict__ block_offsets, long cpi, int n_images,
                                             const float* __restrict__ obs_xy, const float* __restrict__ m_conf, float* __restrict__ keypoints,
                                             float* __restrict__ score, int* __restrict__ n_obs, long* __restrict__ kp_offsets,
                                             int* __restrict__ kp_image, int* __restrict__ parent, int* __restrict__ len,
                                             uint8_t* __restrict__ bad) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  const u64 w = i < G ? grid[i] : 0ull;
  unsigned tot;
  const long k = (long)block_offsets[blockIdx.x] + block_rank(w != 0ull, &tot);
  if (i >= G) return;
  if (i % cpi == 0) kp_offsets[i / cpi] = k;
  if (i == G - 1) kp_offsets[n_images] = k + (w != 0ull);
  if (w == 0ull) return;
  const uint32_t o = packed_index(w);
  keypoints[2 * k] = obs_xy[2 * (size_t)o];
  keypoints[2 * k + 1] = obs_xy[2 * (size_t)o + 1];
  score[k] = m_conf[o >> 1];
  n_obs[k] = 0;
  kp_image[k] = (int)(i / cpi);
  parent[k] = (int)k;
  len[k] = 0;
  bad[k] = 0;
  grid[i] = (u64)k;
}

// ---- resolve + mutual best -------------------------------------------------------------------------------------------------------
__global__ void atlas_resolve_kernel(long M, const int* __restrict__ obs_cell, const float* __restrict__ m_conf, const int* __restrict__ m_row,
                                     const uint8_t* __restrict__ m_reason, const u64* __restrict__ grid, int* __restrict__ mk,
                                     int* __restrict__ n_obs, u64* __restrict__ keys, u64* __restrict__ vals, u64 mask,
                                     u64* __restrict__ counts) {
  const long m = (long)blockIdx.x * kBlock + threadIdx.x;
  const int why = m < M ? (int)m_reason[m] : -1;
  for (int r = 0; r < kReasons; ++r) {                                   // one integer atomicAdd per wave and reason
    const u64 b = __ballot(why == r);
    if (b != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&counts[kCountReason + r], (u64)__popcll(b));
  }
  if (m >= M) return;
  int ka = -1, kb = -1;
  if (why == kValid) {
    ka = (int)grid[obs_cell[2 * m]];
    kb = (int)grid[obs_cell[2 * m + 1]];
    atomicAdd(&n_obs[ka], 1);
    atomicAdd(&n_obs[kb], 1);
    const u64 w = pack(m_conf[m], (uint32_t)m);
    atomicMax(&vals[table_claim(keys, mask, key_match(m_row[m], 0, ka))], w);
    atomicMax(&vals[table_claim(keys, mask, key_match(m_row[m], 1, kb))], w);
  }
  mk[2 * m] = ka;
  mk[2 * m + 1] = kb;
}

__global__ void atlas_keep_kernel(long M, const int* __restrict__ mk, const float* __restrict__ m_conf, const int* __restrict__ m_row,
                                  const u64* __restrict__ keys, const u64* __restrict__ vals, u64 mask, uint8_t* __restrict__ keep,
                                  unsigned* __restrict__ block_counts) {
  const long m = (long)blockIdx.x * kBlock + threadIdx.x;
  bool k = false;
  if (m < M && mk[2 * m] >= 0) {
    const u64 w = pack(m_conf[m], (uint32_t)m);
    k = table_find(keys, vals, mask, key_match(m_row[m], 0, mk[2 * m])) == w &&
        table_find(keys, vals, mask, key_match(m_row[m], 1, mk[2 * m + 1])) == w;
  }
  if (m < M) keep[m] = (uint8_t)k;
  unsigned tot;
  block_rank(k, &tot);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = tot;
}

// kept matches in input order with local keypoint indices; row_offsets[r] = kept matches of the rows before r (m_row ascends, so the
// thread of the first match of a row -- and of the last match, for the rows after it -- knows them from its own rank)
__global__ void atlas_write_matches_kernel(long M, long R, const uint8_t* __restrict__ keep, const unsigned* __restrict__ block_offsets,
                                           const int* __restrict__ mk, const float* __restrict__ m_conf, const int* __restrict__ m_row,
                                           const int* __restrict__ kp_image, const long* __restrict__ kp_offsets, int* __restrict__ matches,
                                           float* __restrict__ match_conf, long* __restrict__ row_offsets) {
  const long m = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool k = m < M && keep[m];
  unsigned tot;
  const long e = (long)block_offsets[blockIdx.x] + block_rank(k, &tot);
  if (m >= M) return;
  const long cur = m_row[m], prev = m > 0 ? (long)m_row[m - 1] : -1;
  for (long r = prev + 1; r <= cur; ++r) row_offsets[r] = e;
  if (m == M - 1) for (long r = cur + 1; r <= R; ++r) row_offsets[r] = e + k;
  if (!k) return;
  const int ka = mk[2 * m], kb = mk[2 * m + 1];
  matches[2 * e] = (int)(ka - kp_offsets[kp_image[ka]]);
  matches[2 * e + 1] = (int)(kb - kp_offsets[kp_image[kb]]);
  match_conf[e] = m_conf[m];
}

// ---- tracks ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// root of x with path halving.  parent[x] <= x always and only ever moves to an ancestor, so a halving store that loses a race is harmless.
__device__ __forceinline__ int uf_find(int* __restrict__ parent, int x) {
  for (;;) {
    const int p = uf_load(parent + x);
    if (p == x) return x;
    const int g = uf_load(parent + p);
    if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
  }
}
__global__ void atlas_union_kernel(long M, const uint8_t* __restrict__ keep, const int* __restrict__ mk, int* __restrict__ parent) {
  const long m = (long)blockIdx.x * kBlock + threadIdx.x;
  if (m >= M || !keep[m]) return;
  int a = mk[2 * m], b = mk[2 * m + 1];
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(&parent[hi], hi, lo) == hi) return;               // hi was still a root: hooked under the smaller one
    a = hi; b = lo;                                                 // somebody hooked hi meanwhile: find again
  }
}
// label = root (no more unions run: a read-only walk), component lengths, keypoints per (label, image)
__global__ void atlas_label_kernel(const long* __restrict__ Kp, const int* __restrict__ parent, const int* __restrict__ kp_image,
                                   int* __restrict__ label, int* __restrict__ len, u64* __restrict__ keys, u64* __restrict__ vals, u64 mask) {
  const long k = (long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= *Kp) return;
  int x = (int)k;
  for (int p = uf_load(parent + x); p != x; p = uf_load(parent + x)) x = p;
  label[k] = x;
  atomicAdd(&len[x], 1);
  atomicAdd(&vals[table_claim(keys, mask, key_track(x, kp_image[k]))], 1ull);
}
// same-image flags of the components, and the number of components long enough to be tracks per block
__global__ void atlas_flag_tracks_kernel(const long* __restrict__ Kp, const int* __restrict__ label, const int* __restrict__ len,
                                         const int* __restrict__ kp_image, const u64* __restrict__ keys, const u64* __restrict__ vals, u64 mask,
                                         int min_track_len, uint8_t* __restrict__ bad, unsigned* __restrict__ block_counts) {
  const long k = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool in = k < *Kp;
  if (in && table_find(keys, vals, mask, key_track(label[k], kp_image[k])) > 1ull) bad[label[k]] = 1;
  unsigned tot;
  block_rank(in && label[k] == (int)k && len[k] >= min_track_len, &tot);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = tot;
}
__global__ void atlas_number_tracks_kernel(const long* __restrict__ Kp, const int* __restrict__ label, const int* __restrict__ len,
                                           const uint8_t* __restrict__ bad, const unsigned* __restrict__ block_offsets, int min_track_len,
                                           int* __restrict__ number, int* __restrict__ track_len, uint8_t* __restrict__ track_ok) {
  const long k = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool root = k < *Kp && label[k] == (int)k && len[k] >= min_track_len;
  unsigned tot;
  const long t = (long)block_offsets[blockIdx.x] + block_rank(root, &tot);
  if (!root) return;
  number[k] = (int)t;
  track_len[t] = len[k];
  track_ok[t] = (uint8_t)!bad[k];
}
__global__ void atlas_track_id_kernel(const long* __restrict__ Kp, const int* __restrict__ label, const int* __restrict__ len,
                                      const int* __restrict__ number, int min_track_len, int* __restrict__ track_id) {
  const long k = (long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= *Kp) return;
  const int l = label[k];
  track_id[k] = len[l] >= min_track_len ? number[l] : -1;
}

struct Layout {
  size_t block_counts, partials, mk, keep, kp_image, parent, label, len, number, bad, keys, vals, total;
  u64 cap;
};
Layout layout(long M, long G) {
  Layout L;
  const long Kb = keypoint_bound(M, G);
  const long nb = std::max(blocks_of(G), std::max(blocks_of(M), blocks_of(Kb)));
  size_t o = 0;
  auto take = [&o](size_t bytes) { return tracks::carve(&o, bytes); };
  L.block_counts = take(sizeof(unsigned) * (size_t)nb);
  L.partials = take(sizeof(unsigned) * (size_t)scan_blocks(nb));
  L.mk = take(sizeof(int) * 2 * (size_t)M);
  L.keep = take((size_t)M);
  L.kp_image = take(sizeof(int) * (size_t)Kb);
  L.parent = take(sizeof(int) * (size_t)Kb);
  L.label = take(sizeof(int) * (size_t)Kb);
  L.len = take(sizeof(int) * (size_t)Kb);
  L.number = take(sizeof(int) * (size_t)Kb);
  L.bad = take((size_t)Kb);
  L.cap = table_capacity(2 * (u64)M);                                   // <= 2 M keys in either use: (row, side, keypoint), (label, image)
  L.keys = take(sizeof(u64) * L.cap);
  L.vals = take(sizeof(u64) * L.cap);
  L.total = o;
  return L;
}

bool supported(long M, long R, int n_images, int gh, int gw) {
  if (gw > kMaxGridSide || gh > kMaxGridSide || M > kMaxMatches || R > kMaxRows) return false;
  return n_images == 0 || (long)gh * gw <= kMaxCells / n_images;
}

}  // namespace

extern "C" int loftr_atlas_observe(const float* kpts0, const float* kpts1, const float* conf, const long* m_bids, const uint8_t* mask, long n,
                                   int n_rows, long match_base, long row_base, const int* row_images, int n_images, int gh, int gw, float inv,
                                   u64* grid, float* obs_xy, int* obs_cell, float* m_conf, int* m_row, uint8_t* m_reason, int* status,
                                   void* stream) {
  LOFTR_CHECK_ARG(n >= 0 && n_rows >= 0 && match_base >= 0 && row_base >= 0 && n_images >= 0 && gh >= 0 && gw >= 0);
  if (n == 0) return LOFTR_OK;
  LOFTR_CHECK_ARG(kpts0 && kpts1 && conf && m_bids && row_images && grid && obs_xy && obs_cell && m_conf && m_row && m_reason && status);
  LOFTR_CHECK_ARG(n_rows > 0 && n_images > 0 && gh > 0 && gw > 0);
  if (!supported(match_base + n, row_base + n_rows, n_images, gh, gw)) return LOFTR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(atlas_observe_kernel, dim3((unsigned)blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, kpts0, kpts1, conf, m_bids, mask, n,
                     n_rows, match_base, row_base, row_images, n_images, gh, gw, inv, grid, obs_xy, obs_cell, m_conf, m_row, m_reason, status);
  LOFTR_CHECK_LAUNCH();
  return LOFTR_OK;
}

extern "C" size_t loftr_atlas_finalize_workspace_bytes(long M, int n_images, int gh, int gw) {
  if (M < 0 || n_images < 0 || gh < 0 || gw < 0 || !supported(M, 0, n_images, gh, gw)) return 0;
  return layout(M, (long)n_images * gh * gw).total;
}

extern "C" int loftr_atlas_finalize(u64* grid, const float* obs_xy, const int* obs_cell, const float* m_conf, const int* m_row,
                                    const uint8_t* m_reason, long M, long R, int n_images, int gh, int gw, int min_track_len, const int* status,
                                    const LoftrAtlasOut* out, void* ws, size_t ws_bytes, float* stage_ms, void* stream) {
  LOFTR_CHECK_ARG(out && M >= 0 && R >= 0 && n_images >= 0 && gh >= 0 && gw >= 0 && min_track_len >= 1);
  LOFTR_CHECK_ARG(out->kp_offsets && out->row_offsets && out->counts && ws);
  if (!supported(M, R, n_images, gh, gw)) return LOFTR_ERR_UNSUPPORTED;
  const long cpi = (long)gh * gw, G = cpi * n_images, Kb = keypoint_bound(M, G);
  LOFTR_CHECK_ARG(G == 0 || grid);
  LOFTR_CHECK_ARG(M == 0 || (G > 0 && R > 0 && obs_xy && obs_cell && m_conf && m_row && m_reason && out->keypoints && out->score && out->n_obs &&
                             out->matches && out->match_conf && out->track_id && out->track_len && out->track_ok));
  const Layout L = layout(M, G);
  if (ws_bytes < L.total) return LOFTR_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  unsigned *block_counts = (unsigned*)(w + L.block_counts), *partials = (unsigned*)(w + L.partials);
  int *mk = (int*)(w + L.mk), *kp_image = (int*)(w + L.kp_image), *parent = (int*)(w + L.parent), *label = (int*)(w + L.label);
  int *len = (int*)(w + L.len), *number = (int*)(w + L.number);
  uint8_t *keep = (uint8_t*)(w + L.keep), *bad = (uint8_t*)(w + L.bad);
  u64 *keys = (u64*)(w + L.keys), *vals = (u64*)(w + L.vals);
  const u64 mask = L.cap - 1;
  long* counts = out->counts;

  StageTimer timer(stage_ms, LOFTR_ATLAS_STAGES, s);                    // stage boundaries, only when the caller asked for timings
  auto zero = [s](void* p, size_t bytes) { return hipMemsetAsync(p, 0, bytes, s) == hipSuccess; };

  if (!zero(counts, sizeof(long) * kCounts) || !zero(out->kp_offsets, sizeof(long) * ((size_t)n_images + 1)) ||
      !zero(out->row_offsets, sizeof(long) * ((size_t)R + 1)))
    return LOFTR_ERR_LAUNCH;
  if (status && hipMemcpyAsync(counts + kCountStatus, status, sizeof(int), hipMemcpyDeviceToDevice, s) != hipSuccess)   // the low half of the zeroed slot
    return LOFTR_ERR_LAUNCH;
  timer.mark();
  // ---- compact
  if (G > 0 && M > 0) {
    const long nb = blocks_of(G);
    hipLaunchKernelGGL(atlas_count_cells_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, grid, G, block_counts);
    LOFTR_CHECK_LAUNCH();
    if (scan_u32(block_counts, nb, partials, counts + kCountK, s) != LOFTR_OK) return LOFTR_ERR_LAUNCH;
    hipLaunchKernelGGL(atlas_write_keypoints_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, grid, G, block_counts, cpi, n_images, obs_xy, m_conf,
                       out->keypoints, out->score, out->n_obs, out->kp_offsets, kp_image, parent, len, bad);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  if (M > 0) {
    const unsigned nbm = (unsigned)blocks_of(M), nbk = (unsigned)blocks_of(Kb);
    // ---- resolve
    if (!zero(keys, sizeof(u64) * L.cap) || !zero(vals, sizeof(u64) * L.cap)) return LOFTR_ERR_LAUNCH;
    hipLaunchKernelGGL(atlas_resolve_kernel, dim3(nbm), dim3(kBlock), 0, s, M, obs_cell, m_conf, m_row, m_reason, grid, mk, out->n_obs, keys, vals,
                       mask, (u64*)counts);
    LOFTR_CHECK_LAUNCH();
    timer.mark();
    // ---- mutual best
    hipLaunchKernelGGL(atlas_keep_kernel, dim3(nbm), dim3(kBlock), 0, s, M, mk, m_conf, m_row, keys, vals, mask, keep, block_counts);
    LOFTR_CHECK_LAUNCH();
    if (scan_u32(block_counts, nbm, partials, counts + kCountMk, s) != LOFTR_OK) return LOFTR_ERR_LAUNCH;
    timer.mark();
    hipLaunchKernelGGL(atlas_write_matches_kernel, dim3(nbm), dim3(kBlock), 0, s, M, R, keep, block_counts, mk, m_conf, m_row, kp_image,
                       out->kp_offsets, out->matches, out->match_conf, out->row_offsets);
    LOFTR_CHECK_LAUNCH();
    timer.mark();
    // ---- tracks
    hipLaunchKernelGGL(atlas_union_kernel, dim3(nbm), dim3(kBlock), 0, s, M, keep, mk, parent);
    LOFTR_CHECK_LAUNCH();
    timer.mark();
    if (!zero(keys, sizeof(u64) * L.cap) || !zero(vals, sizeof(u64) * L.cap)) return LOFTR_ERR_LAUNCH;
    const long* Kp = counts + kCountK;
    hipLaunchKernelGGL(atlas_label_kernel, dim3(nbk), dim3(kBlock), 0, s, Kp, parent, kp_image, label, len, keys, vals, mask);
    LOFTR_CHECK_LAUNCH();
    timer.mark();
    hipLaunchKernelGGL(atlas_flag_tracks_kernel, dim3(nbk), dim3(kBlock), 0, s, Kp, label, len, kp_image, keys, vals, mask, min_track_len, bad,
                       block_counts);
    LOFTR_CHECK_LAUNCH();
    if (scan_u32(block_counts, nbk, partials, counts + kCountT, s) != LOFTR_OK) return LOFTR_ERR_LAUNCH;
    hipLaunchKernelGGL(atlas_number_tracks_kernel, dim3(nbk), dim3(kBlock), 0, s, Kp, label, len, bad, block_counts, min_track_len, number,
                       out->track_len, out->track_ok);
    LOFTR_CHECK_LAUNCH();
    hipLaunchKernelGGL(atlas_track_id_kernel, dim3(nbk), dim3(kBlock), 0, s, Kp, label, len, number, min_track_len, out->track_id);
    LOFTR_CHECK_LAUNCH();
    timer.mark();
  }
  return timer.finish();
}
