// Localisation against a triangulated model on the GPU (gfx950, wave64): loftr_model_lookup reproduces loftr_model_lookup_host
// (model_lookup.hip) bit for bit.  No MFMA, no float atomic: the fusion is a 64-bit unsigned max of the packed word of atlas_core.h into an
// open-addressing table claimed by compare-and-swap, every count an integer add, so the result does not depend on the order in which
// the atomics arrive.  A slot's POSITION in the table may vary from run to run; its key -> value mapping may not.  Every atomically
// written value (table, counts, status) is read only by a later kernel.
//
//   lookup   a thread per match: reason (model_lookup_core.h), binary search of the cell among the image's keypoints, the 3D point,
//            table[(query, point)] <- max packed (conf, match); a thread per row: the checks of row_db / row_query
//   keep     a match is kept when it is the table's winner; kept per block (ballot + popcount) and per query (one atomicAdd per wave
//            and query: the queries of a wave's matches ascend)
//   scans    block counts -> offsets and C; query counts -> q_offsets
//   write    the compacted correspondences in match order, q_offsets widened to int64
// The u32 scan (scan.hip), the block helpers and the table are compact_gpu.h's, shared with atlas_gpu.hip.
#include <algorithm>
#include "compact_gpu.h"
#include "stage_timer.h"
#include "tracks_core.h"
#include "model_lookup_core.h"

namespace {

using namespace model_lookup;
using namespace compact;
using atlas::pack;

// one integer atomicAdd per wave for the lanes with flag set (every lane of the wave must call it)
__device__ __forceinline__ void wave_count(bool flag, u64* __restrict__ slot) {
  const u64 b = __ballot(flag);
  if (b != 0ull && (threadIdx.x & 63) == 0) atomicAdd(slot, (u64)__popcll(b));
}

// ---- model cells -----------------------------------------------------------------------------------------------------------------
// is k the first keypoint of an image (a value of kp_offsets [n_images + 1], ascending)?
__device__ __forceinline__ bool image_start(const long* __restrict__ kp_offsets, int n_images, long k) {
  int lo = 0, hi = n_images + 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (kp_offsets[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo <= n_images && kp_offsets[lo] == k;
}
__global__ void model_cells_kernel(const long* __restrict__ kp_offsets, int n_images, const float* __restrict__ keypoints,
                                   const int* __restrict__ kp_point, long K, long P, int gh, int gw, float inv, int* __restrict__ kp_cell,
                                   int* __restrict__ status) {
  const long k = (long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= K) return;
  const int cell = cell_of(keypoints[2 * k], keypoints[2 * k + 1], inv, gw, gh);
  kp_cell[k] = cell;
  int bad = cell < 0 ? kStatusBadCells : 0;
  if (k > 0 && !image_start(kp_offsets, n_images, k) && cell_of(keypoints[2 * k - 2], keypoints[2 * k - 1], inv, gw, gh) >= cell)
    bad |= kStatusBadCells;
  const int p = kp_point[k];
  if (p < -1 || p >= P) bad |= kStatusBadPoint;
  if (bad) atomicOr(status, bad);
}

// ---- lookup ----------------------------------------------------------------------------------------------------------------------
__global__ void model_lookup_kernel(const long* __restrict__ kp_offsets, const int* __restrict__ kp_cell, const int* __restrict__ kp_point, long K,
                                    long P, int n_images, int gh, int gw, float inv, const float* __restrict__ kpts_db,
                                    const float* __restrict__ kpts_q, const float* __restrict__ conf, const int* __restrict__ rows,
                                    const uint8_t* __restrict__ mask, long M, const int* __restrict__ row_db, const int* __restrict__ row_query,
                                    long R, long Q, int* __restrict__ m_point, int* __restrict__ m_query, uint8_t* __restrict__ match_reason,
                                    u64* __restrict__ keys, u64* __restrict__ vals, u64 tmask, u64* __restrict__ counts) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  int bad = 0;
  if (i < R) {                                                           // a thread per row: rows without a match are checked too
    const int d = row_db[i], q = row_query[i];
    if (d < 0 || d >= n_images) bad |= kStatusBadImage;
    if (q < 0 || q >= Q || (i > 0 && row_query[i - 1] > q)) bad |= kStatusBadQuery;
  }
  int why = -1;
  if (i < M) {
    const long r = rows[i];
    const bool row_ok = r >= 0 && r < R;
    if (!row_ok) bad |= kStatusBadRow;
    if (i > 0 && rows[i - 1] > r) bad |= kStatusUnsorted;
    why = kBadRow;
    int point = -1, q = 0;
    if (row_ok) {                                                        // nothing is read through a bad row, image or query
      const int d = row_db[r];
      q = row_query[r];
      if (d >= 0 && d < n_images && q >= 0 && q < Q) {
        int cell;
        why = classify(kpts_db[2 * i], kpts_db[2 * i + 1], kpts_q[2 * i], kpts_q[2 * i + 1], conf[i], mask && !mask[i], inv, gw, gh, &cell);
        if (why == kKept) {
          long lo = kp_offsets[d], hi = kp_offsets[d + 1];
          lo = lo < 0 ? 0 : (lo > K ? K : lo);                            // (a checked model has them in range: never index past kp_cell)
          hi = hi < lo ? lo : (hi > K ? K : hi);
          const long k = find_cell(kp_cell, lo, hi, cell);
          if (k < 0) why = kNoKeypoint;
          else {
            const int p = kp_point[k];
            if (p < 0 || p >= P) why = kNoPoint;
            else {
              point = p;
              why = kFused;                                              // until the keep kernel finds it to be the winner
              atomicMax(&vals[table_claim(keys, tmask, key_point(q, p))], (u64)pack(conf[i], (uint32_t)i));
            }
          }
        }
      } else {
        q = 0;
      }
    }
    m_point[i] = point;
    m_query[i] = q;
    match_reason[i] = (uint8_t)why;
  }
  if (bad) atomicOr(&counts[kCountStatus], (u64)bad);
  for (int r = kBadRow; r < kFused; ++r) wave_count(why == r, &counts[kCountReason + r]);
}

// ---- keep ------------------------------------------------------------------------------------------------------------------------
__global__ void model_keep_kernel(long M, const int* __restrict__ m_point, const int* __restrict__ m_query, const float* __restrict__ conf,
                                  const u64* __restrict__ keys, const u64* __restrict__ vals, u64 tmask, uint8_t* __restrict__ match_reason,
                                  unsigned* __restrict__ block_counts, unsigned* __restrict__ q_counts, u64* __restrict__ counts) {
  const long m = (long)blockIdx.x * kBlock + threadIdx.x;
  const int p = m < M ? m_point[m] : -1, q = m < M ? m_query[m] : 0;
  const bool kept = p >= 0 && table_find(keys, vals, tmask, key_point(q, p)) == pack(conf[m], (uint32_t)m);
  if (kept) match_reason[m] = (uint8_t)kKept;
  wave_count(kept, &counts[kCountReason + kKept]);
  wave_count(p >= 0 && !kept, &counts[kCountReason + kFused]);
  unsigned tot;
  block_rank(kept, &tot);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = tot;
  // kept matches per query: one add per wave and query
  const int lane = threadIdx.x & 63;
  u64 pending = __ballot(kept);
  while (pending != 0ull) {
    const int first = __ffsll((long long)pending) - 1;
    const int qq = __shfl(q, first, 64);
    const u64 same = __ballot(kept && q == qq) & pending;
    if (lane == first) atomicAdd(&q_counts[qq], (unsigned)__popcll(same));
    pending &= ~same;
  }
}

// ---- write -----------------------------------------------------------------------------------------------------------------------
// the blocks of the first M threads carry the matches; threads [0, Q] of the grid also widen the scanned query counts into q_offsets
__global__ void model_write_kernel(long M, long Q, const uint8_t* __restrict__ match_reason, const unsigned* __restrict__ block_offsets,
                                   const unsigned* __restrict__ q_counts, const long* __restrict__ counts, const int* __restrict__ m_point,
                                   const int* __restrict__ m_query, const float* __restrict__ xyz, const float* __restrict__ kpts_q,
                                   const float* __restrict__ conf, float* __restrict__ pts3d, float* __restrict__ kpts, long* __restrict__ q_ids,
                                   int* __restrict__ match, int* __restrict__ point, float* __restrict__ out_conf, long* __restrict__ q_offsets) {
  const long m = (long)blockIdx.x * kBlock + threadIdx.x;
  if (m < Q) q_offsets[m] = (long)q_counts[m];
  if (m == Q) q_offsets[m] = counts[kCountC];
  const bool kept = m < M && match_reason[m] == kKept;
  unsigned tot;
  const unsigned rank = block_rank(kept, &tot);
  if (!kept) return;
  const long e = (long)block_offsets[blockIdx.x] + rank;                 // (a kept match sits in a block that the keep kernel counted)
  const long p = m_point[m];
  pts3d[3 * e] = xyz[3 * p];
  pts3d[3 * e + 1] = xyz[3 * p + 1];
  pts3d[3 * e + 2] = xyz[3 * p + 2];
  kpts[2 * e] = kpts_q[2 * m];
  kpts[2 * e + 1] = kpts_q[2 * m + 1];
  q_ids[e] = (long)m_query[m];
  match[e] = (int)m;
  point[e] = (int)p;
  out_conf[e] = conf[m];
}

struct Layout {
  size_t block_counts, partials, q_counts, q_partials, q_total, m_point, m_query, keys, vals, total;
  u64 cap;
};
Layout layout(long M, long Q) {
  Layout L;
  size_t o = 0;
  auto take = [&o](size_t bytes) { return tracks::carve(&o, bytes); };
  L.block_counts = take(sizeof(unsigned) * (size_t)blocks_of(M));
  L.partials = take(sizeof(unsigned) * (size_t)scan_blocks(blocks_of(M)));
  L.q_counts = take(sizeof(unsigned) * (size_t)Q);
  L.q_partials = take(sizeof(unsigned) * (size_t)scan_blocks(Q));
  L.q_total = take(sizeof(long));
  L.m_point = take(sizeof(int) * (size_t)M);
  L.m_query = take(sizeof(int) * (size_t)M);
  L.cap = atlas::table_capacity((u64)M);                                // at most M keys (query, point)
  L.keys = take(sizeof(u64) * L.cap);
  L.vals = take(sizeof(u64) * L.cap);
  L.total = o;
  return L;
}

bool supported(long M, long R, long Q) { return M <= atlas::kMaxMatches && R <= kMaxIds && Q <= kMaxIds; }
bool grid_supported(long K, long P, int gh, int gw) {
  return K <= atlas::kMaxCells && P <= kMaxIds && gw <= atlas::kMaxGridSide && gh <= atlas::kMaxGridSide && (long)gh * gw <= atlas::kMaxCells;
}

}  // namespace

extern "C" int loftr_model_cells(const long* kp_offsets, int n_images, const float* keypoints, const int* kp_point, long K, long P, int gh, int gw,
                                 float inv, int* kp_cell, int* status, void* stream) {
  LOFTR_CHECK_ARG(n_images >= 0 && K >= 0 && P >= 0 && gh >= 0 && gw >= 0);
  if (!grid_supported(K, P, gh, gw)) return LOFTR_ERR_UNSUPPORTED;
  LOFTR_CHECK_ARG(kp_offsets && status && (K == 0 || (keypoints && kp_point && kp_cell)));
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, sizeof(int), s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  if (K == 0) return LOFTR_OK;
  hipLaunchKernelGGL(model_cells_kernel, dim3((unsigned)blocks_of(K)), dim3(kBlock), 0, s, kp_offsets, n_images, keypoints, kp_point, K, P, gh, gw,
                     inv, kp_cell, status);
  LOFTR_CHECK_LAUNCH();
  return LOFTR_OK;
}

extern "C" size_t loftr_model_lookup_workspace_bytes(long M, long Q) {
  if (M < 0 || Q < 0 || !supported(M, 0, Q)) return 0;
  return layout(M, Q).total;
}

extern "C" int loftr_model_lookup(const LoftrModel* model, const float* kpts_db, const float* kpts_q, const float* conf, const int* rows,
                                  const uint8_t* mask, long M, const int* row_db, const int* row_query, long R, long Q,
                                  const LoftrModelLookupOut* out, void* ws, size_t ws_bytes, float* stage_ms, void* stream) {
  LOFTR_CHECK_ARG(M >= 0 && R >= 0 && Q >= 0);
  if (!supported(M, R, Q)) return LOFTR_ERR_UNSUPPORTED;
  LOFTR_CHECK_ARG(model && out && ws);
  const int n_images = model->n_images, gh = model->gh, gw = model->gw;
  const long K = model->K, P = model->P;
  LOFTR_CHECK_ARG(n_images >= 0 && K >= 0 && P >= 0 && gh >= 0 && gw >= 0);
  if (!grid_supported(K, P, gh, gw)) return LOFTR_ERR_UNSUPPORTED;
  LOFTR_CHECK_ARG(model->kp_offsets && (K == 0 || (model->kp_cell && model->kp_point)) && (P == 0 || model->xyz));
  LOFTR_CHECK_ARG(out->q_offsets && out->counts);
  LOFTR_CHECK_ARG(M == 0 || (kpts_db && kpts_q && conf && rows && out->pts3d && out->kpts && out->q_ids && out->match && out->point && out->conf &&
                             out->match_reason));
  LOFTR_CHECK_ARG(R == 0 || (row_db && row_query));
  const Layout L = layout(M, Q);
  if (ws_bytes < L.total) return LOFTR_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  unsigned *block_counts = (unsigned*)(w + L.block_counts), *partials = (unsigned*)(w + L.partials);
  unsigned *q_counts = (unsigned*)(w + L.q_counts), *q_partials = (unsigned*)(w + L.q_partials);
  long* q_total = (long*)(w + L.q_total);
  int *m_point = (int*)(w + L.m_point), *m_query = (int*)(w + L.m_query);
  u64 *keys = (u64*)(w + L.keys), *vals = (u64*)(w + L.vals);
  const u64 tmask = L.cap - 1;
  long* counts = out->counts;

  StageTimer timer(stage_ms, LOFTR_MODEL_LOOKUP_STAGES, s);             // stage boundaries, only when the caller asked for timings
  auto zero = [s](void* p, size_t bytes) { return hipMemsetAsync(p, 0, bytes, s) == hipSuccess; };

  if (!zero(counts, sizeof(long) * kCounts) || !zero(out->q_offsets, sizeof(long) * ((size_t)Q + 1))) return LOFTR_ERR_LAUNCH;
  timer.mark();
  const long nbm = blocks_of(M);
  // ---- lookup (the row checks run even without a match)
  if (M > 0 && (!zero(keys, sizeof(u64) * L.cap) || !zero(vals, sizeof(u64) * L.cap))) return LOFTR_ERR_LAUNCH;
  if (Q > 0 && !zero(q_counts, sizeof(unsigned) * (size_t)Q)) return LOFTR_ERR_LAUNCH;
  if (std::max(M, R) > 0) {
    hipLaunchKernelGGL(model_lookup_kernel, dim3((unsigned)blocks_of(std::max(M, R))), dim3(kBlock), 0, s, model->kp_offsets, model->kp_cell,
                       model->kp_point, K, P, n_images, gh, gw, model->inv, kpts_db, kpts_q, conf, rows, mask, M, row_db, row_query, R, Q, m_point,
                       m_query, out->match_reason, keys, vals, tmask, (u64*)counts);
    LOFTR_CHECK_LAUNCH();
  }
  timer.mark();
  if (M > 0) {
    // ---- keep
    hipLaunchKernelGGL(model_keep_kernel, dim3((unsigned)nbm), dim3(kBlock), 0, s, M, m_point, m_query, conf, keys, vals, tmask, out->match_reason,
                       block_counts, q_counts, (u64*)counts);
    LOFTR_CHECK_LAUNCH();
    if (scan_u32(block_counts, nbm, partials, counts + kCountC, s) != LOFTR_OK) return LOFTR_ERR_LAUNCH;
    if (Q > 0 && scan_u32(q_counts, Q, q_partials, q_total, s) != LOFTR_OK) return LOFTR_ERR_LAUNCH;
    timer.mark();
    // ---- write
    hipLaunchKernelGGL(model_write_kernel, dim3((unsigned)blocks_of(std::max(M, Q + 1))), dim3(kBlock), 0, s, M, Q, out->match_reason,
                       block_counts, q_counts, counts, m_point, m_query, model->xyz, kpts_q, conf, out->pts3d, out->kpts, out->q_ids, out->match,
                       out->point, out->conf, out->q_offsets);
    LOFTR_CHECK_LAUNCH();
    timer.mark();
  }
  return timer.finish();
}
