// Localisation against a triangulated model, host routines: plain C++ on host arrays.  loftr_model_lookup_host DEFINES the result of
// rules 1-3 (include/loftr_hip.h); loftr_model_lookup (model_lookup_gpu.hip) reproduces it bit for bit.  It is written the
// way a careful user would write it on the host (one pass in match order, an ordered map per fusion key), not the way the kernels work
// (a hash table, atomics, scans): the two share only model_lookup_core.h -- the cell function, the reasons, the search of a cell among
// an image's keypoints and the packed "greatest confidence, then smallest index" word.
#include <stdint.h>
#include <map>
#include <utility>
#include <vector>
#include "../../include/loftr_hip.h"
#include "model_lookup_core.h"

using namespace model_lookup;

namespace {

bool offsets_ok(const long* kp_offsets, int n_images, long K) {
  if (kp_offsets[0] != 0 || kp_offsets[n_images] != K) return false;
  for (int i = 0; i < n_images; ++i)
    if (kp_offsets[i] > kp_offsets[i + 1]) return false;
  return true;
}

}  // namespace

extern "C" int loftr_model_cells_host(const long* kp_offsets, int n_images, const float* keypoints, const int* kp_point, long K, long P, int gh,
                                      int gw, float inv, int* kp_cell, int* status) {
  if (n_images < 0 || K < 0 || P < 0 || gh < 0 || gw < 0) return LOFTR_ERR_BAD_ARG;
  if (K > atlas::kMaxCells || P > kMaxIds || gw > atlas::kMaxGridSide || gh > atlas::kMaxGridSide) return LOFTR_ERR_UNSUPPORTED;
  if (!kp_offsets || !status || (K > 0 && (!keypoints || !kp_point || !kp_cell))) return LOFTR_ERR_BAD_ARG;
  if ((long)gh * gw > atlas::kMaxCells) return LOFTR_ERR_UNSUPPORTED;
  if (!offsets_ok(kp_offsets, n_images, K)) return LOFTR_ERR_BAD_ARG;
  int bad = 0;
  for (int i = 0; i < n_images; ++i) {
    for (long k = kp_offsets[i]; k < kp_offsets[i + 1]; ++k) {
      kp_cell[k] = cell_of(keypoints[2 * k], keypoints[2 * k + 1], inv, gw, gh);
      if (kp_cell[k] < 0 || (k > kp_offsets[i] && kp_cell[k - 1] >= kp_cell[k])) bad |= kStatusBadCells;
      if (kp_point[k] < -1 || kp_point[k] >= P) bad |= kStatusBadPoint;
    }
  }
  *status = bad;
  return LOFTR_OK;
}

extern "C" int loftr_model_lookup_host(const LoftrModel* model, const float* kpts_db, const float* kpts_q, const float* conf, const int* rows,
                                       const uint8_t* mask, long M, const int* row_db, const int* row_query, long R, long Q,
                                       const LoftrModelLookupOut* out) {
  if (M < 0 || R < 0 || Q < 0) return LOFTR_ERR_BAD_ARG;
  if (M > atlas::kMaxMatches || R > kMaxIds || Q > kMaxIds) return LOFTR_ERR_UNSUPPORTED;
  if (!model || !out) return LOFTR_ERR_BAD_ARG;
  const int n_images = model->n_images, gh = model->gh, gw = model->gw;
  const long K = model->K, P = model->P;
  if (n_images < 0 || K < 0 || P < 0 || gh < 0 || gw < 0) return LOFTR_ERR_BAD_ARG;
  if (K > atlas::kMaxCells || P > kMaxIds || gw > atlas::kMaxGridSide || gh > atlas::kMaxGridSide || (long)gh * gw > atlas::kMaxCells)
    return LOFTR_ERR_UNSUPPORTED;
  if (!model->kp_offsets || (K > 0 && (!model->kp_cell || !model->kp_point)) || (P > 0 && !model->xyz)) return LOFTR_ERR_BAD_ARG;
  if (!out->q_offsets || !out->counts) return LOFTR_ERR_BAD_ARG;
  if (M > 0 && (!kpts_db || !kpts_q || !conf || !rows || !out->pts3d || !out->kpts || !out->q_ids || !out->match || !out->point || !out->conf ||
                !out->match_reason)) return LOFTR_ERR_BAD_ARG;
  if (R > 0 && (!row_db || !row_query)) return LOFTR_ERR_BAD_ARG;
  if (!offsets_ok(model->kp_offsets, n_images, K)) return LOFTR_ERR_BAD_ARG;
  // rule 4: the errors
  for (long r = 0; r < R; ++r) {
    if (row_db[r] < 0 || row_db[r] >= n_images) return LOFTR_ERR_BAD_ARG;
    if (row_query[r] < 0 || row_query[r] >= Q || (r > 0 && row_query[r] < row_query[r - 1])) return LOFTR_ERR_BAD_ARG;
  }
  for (long m = 0; m < M; ++m)
    if (rows[m] < 0 || rows[m] >= R || (m > 0 && rows[m] < rows[m - 1])) return LOFTR_ERR_BAD_ARG;
  long* counts = out->counts;
  for (int i = 0; i < kCounts; ++i) counts[i] = 0;
  for (long q = 0; q <= Q; ++q) out->q_offsets[q] = 0;

  // rule 1: the reason of every match and the 3D point of the candidates; rule 2: the best candidate of every (query, point)
  std::vector<int> point((size_t)M, -1);
  std::map<std::pair<int, int>, uint64_t> best;
  for (long m = 0; m < M; ++m) {
    int cell;
    int why = classify(kpts_db[2 * m], kpts_db[2 * m + 1], kpts_q[2 * m], kpts_q[2 * m + 1], conf[m], mask && !mask[m], model->inv, gw, gh, &cell);
    if (why == kKept) {
      const int d = row_db[rows[m]];
      const long k = find_cell(model->kp_cell, model->kp_offsets[d], model->kp_offsets[d + 1], cell);
      if (k < 0) why = kNoKeypoint;
      else if (model->kp_point[k] < 0 || model->kp_point[k] >= P) why = kNoPoint;
      else {
        point[m] = model->kp_point[k];
        uint64_t& w = best[{row_query[rows[m]], point[m]}];
        const uint64_t mine = atlas::pack(conf[m], (uint32_t)m);
        if (mine > w) w = mine;
      }
    }
    out->match_reason[m] = (uint8_t)why;
  }
  // rules 2 and 3: the winners in ascending match order
  long C = 0;
  for (long m = 0; m < M; ++m) {
    if (point[m] >= 0) {
      const int q = row_query[rows[m]];
      if (best[{q, point[m]}] != atlas::pack(conf[m], (uint32_t)m)) out->match_reason[m] = (uint8_t)kFused;
      else {
        for (int j = 0; j < 3; ++j) out->pts3d[3 * C + j] = model->xyz[3 * (long)point[m] + j];
        out->kpts[2 * C] = kpts_q[2 * m];
        out->kpts[2 * C + 1] = kpts_q[2 * m + 1];
        out->q_ids[C] = q;
        out->match[C] = (int)m;
        out->point[C] = point[m];
        out->conf[C] = conf[m];
        ++out->q_offsets[q + 1];
        ++C;
      }
    }
    ++counts[kCountReason + out->match_reason[m]];
  }
  for (long q = 0; q < Q; ++q) out->q_offsets[q + 1] += out->q_offsets[q];
  counts[kCountC] = C;
  return LOFTR_OK;
}
