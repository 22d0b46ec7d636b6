// Keypoint atlas, host routine: plain C++ on host arrays.  This function DEFINES the result of rules 1-4 (include/loftr_hip.h);
// loftr_atlas_observe + loftr_atlas_finalize (atlas_gpu.hip) reproduce it bit for bit.  It is written the way a careful user would write it
// on the host (ordered maps, a sequential union-find), not the way the kernels work (dense grid, atomics, a hash table): the two share only
// atlas_core.h -- the cell function, the drop reasons and the packed "greatest conf, then smallest index" word.
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <unordered_map>
#include <vector>
#include "../../include/loftr_hip.h"
#include "atlas_core.h"

namespace {

using namespace atlas;

int find_root(std::vector<int>& parent, int x) {
  while (parent[x] != x) {
    parent[x] = parent[parent[x]];
    x = parent[x];
  }
  return x;
}

}  // namespace

extern "C" int loftr_atlas_host(const float* kpts0, const float* kpts1, const float* conf, const int* rows, const uint8_t* mask, long M,
                                const int* row_images, long R, int n_images, int gh, int gw, float inv, int min_track_len,
                                const LoftrAtlasOut* out) {
  if (!out || M < 0 || R < 0 || n_images < 0 || gh < 0 || gw < 0 || min_track_len < 1) return LOFTR_ERR_BAD_ARG;
  if (!out->kp_offsets || !out->row_offsets || !out->counts) return LOFTR_ERR_BAD_ARG;
  if (M > 0 && (!kpts0 || !kpts1 || !conf || !rows || !out->keypoints || !out->score || !out->n_obs || !out->matches || !out->match_conf ||
                !out->track_id || !out->track_len || !out->track_ok)) return LOFTR_ERR_BAD_ARG;
  if (R > 0 && !row_images) return LOFTR_ERR_BAD_ARG;
  if (gw > kMaxGridSide || gh > kMaxGridSide) return LOFTR_ERR_UNSUPPORTED;
  const long cells_per_image = (long)gh * gw;
  if (M > kMaxMatches || R > kMaxRows || (n_images > 0 && cells_per_image > kMaxCells / n_images)) return LOFTR_ERR_UNSUPPORTED;
  for (long r = 0; r < R; ++r) {
    const int a = row_images[2 * r], b = row_images[2 * r + 1];
    if (a == b || a < 0 || b < 0 || a >= n_images || b >= n_images) return LOFTR_ERR_BAD_ARG;
  }
  for (long m = 0; m < M; ++m)
    if (rows[m] < 0 || rows[m] >= R || (m > 0 && rows[m] < rows[m - 1])) return LOFTR_ERR_BAD_ARG;
  long* counts = out->counts;
  for (int i = 0; i < kCounts; ++i) counts[i] = 0;

  // rule 1: cells and reasons; rule 2: the best observation and the number of observations of every occupied cell, ordered by cell
  std::vector<int> cell(2 * (size_t)M, -1);
  std::map<int, std::pair<uint64_t, int>> occupied;              // global cell -> (packed best, n_obs)
  for (long m = 0; m < M; ++m) {
    int c0, c1;
    const int why = classify(kpts0[2 * m], kpts0[2 * m + 1], kpts1[2 * m], kpts1[2 * m + 1], conf[m], true, mask && !mask[m], inv, gw, gh,
                             &c0, &c1);
    ++counts[kCountReason + why];
    if (why != kValid) continue;
    const int* im = row_images + 2 * (long)rows[m];
    cell[2 * m] = (int)(im[0] * cells_per_image + c0);
    cell[2 * m + 1] = (int)(im[1] * cells_per_image + c1);
    for (int side = 0; side < 2; ++side) {
      auto& slot = occupied[cell[2 * m + side]];
      slot.first = std::max(slot.first, pack(conf[m], (uint32_t)(2 * m + side)));
      ++slot.second;
    }
  }
  const long K = (long)occupied.size();
  std::unordered_map<int, int> kp_of_cell;
  kp_of_cell.reserve((size_t)K);
  std::vector<int> kp_image((size_t)K);
  for (int i = 0; i <= n_images; ++i) out->kp_offsets[i] = 0;
  long k = 0;
  for (const auto& it : occupied) {
    const uint32_t o = packed_index(it.second.first);
    const float* xy = (o & 1u) ? kpts1 + 2 * (size_t)(o >> 1) : kpts0 + 2 * (size_t)(o >> 1);
    out->keypoints[2 * k] = xy[0];
    out->keypoints[2 * k + 1] = xy[1];
    out->score[k] = conf[o >> 1];
    out->n_obs[k] = it.second.second;
    kp_image[k] = (int)(it.first / cells_per_image);
    ++out->kp_offsets[kp_image[k] + 1];
    kp_of_cell[it.first] = (int)k;
    ++k;
  }
  for (int i = 0; i < n_images; ++i) out->kp_offsets[i + 1] += out->kp_offsets[i];
  counts[kCountK] = K;

  // rule 3: per row and side, the best match of every keypoint; a match is kept when it is that best on both sides
  std::vector<int> parent((size_t)K);
  for (long i = 0; i < K; ++i) parent[i] = (int)i;
  long Mk = 0, m = 0;
  for (long r = 0; r < R; ++r) {
    out->row_offsets[r] = Mk;
    const long first = m;
    std::unordered_map<int, uint64_t> best[2];
    for (; m < M && rows[m] == r; ++m) {
      if (cell[2 * m] < 0) continue;
      for (int side = 0; side < 2; ++side) {
        uint64_t& w = best[side][kp_of_cell[cell[2 * m + side]]];
        w = std::max(w, pack(conf[m], (uint32_t)m));
      }
    }
    for (long q = first; q < m; ++q) {
      if (cell[2 * q] < 0) continue;
      const int ka = kp_of_cell[cell[2 * q]], kb = kp_of_cell[cell[2 * q + 1]];
      const uint64_t w = pack(conf[q], (uint32_t)q);
      if (best[0][ka] != w || best[1][kb] != w) continue;
      out->matches[2 * Mk] = (int)(ka - out->kp_offsets[kp_image[ka]]);
      out->matches[2 * Mk + 1] = (int)(kb - out->kp_offsets[kp_image[kb]]);
      out->match_conf[Mk] = conf[q];
      ++Mk;
      // rule 4: union, the smaller root stays the root
      const int ra = find_root(parent, ka), rb = find_root(parent, kb);
      if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
    }
  }
  out->row_offsets[R] = Mk;
  counts[kCountMk] = Mk;

  // rule 4: labels, lengths, same-image test, numbering by ascending label
  std::vector<int> label((size_t)K), len((size_t)K, 0), number((size_t)K, -1);
  std::vector<uint8_t> bad((size_t)K, 0);
  std::map<std::pair<int, int>, int> seen;                          // (label, image) -> keypoints
  for (long i = 0; i < K; ++i) {
    label[i] = find_root(parent, (int)i);
    ++len[label[i]];
    if (++seen[{label[i], kp_image[i]}] > 1) bad[label[i]] = 1;
  }
  long T = 0;
  for (long i = 0; i < K; ++i) {
    if (label[i] != i || len[i] < min_track_len) continue;
    number[i] = (int)T;
    out->track_len[T] = len[i];
    out->track_ok[T] = !bad[i];
    ++T;
  }
  for (long i = 0; i < K; ++i) out->track_id[i] = number[label[i]];
  counts[kCountT] = T;
  return LOFTR_OK;
}
