// Localisation against a triangulated model (matches of query images -> fused 2D-3D correspondences): what the host routine
// (model_lookup.hip) and the kernels (model_lookup_gpu.hip) share, on top of atlas_core.h, which is included unchanged.  Everything
// here is integer or the atlas's single fp32 multiply, so host and device agree bit for bit:
//   * the cell of the database-side point (atlas::cell_coord) and the reason a match yields no correspondence (rule 1 of DESIGN §17);
//   * the search for that cell among the ascending cells of one image's keypoints;
//   * the key (query << 32 | point) + 1 of the fusion table; its value is atlas::pack(conf, match): ONE unsigned 64-bit max picks
//     "greatest confidence, then smallest match index" (rule 2).
#pragma once
#include "atlas_core.h"

namespace model_lookup {

constexpr long kMaxIds = 0x7FFFFFFFL;            // Q, P, R < 2^31: (query << 32 | point) + 1 fits 64 bits, row ids are int32

// what became of a match; the first that applies, in this order (kKept / kFused are decided by the fusion)
enum Reason { kKept = 0, kBadRow = 1, kMasked = 2, kNonFinite = 3, kNegConf = 4, kOutside = 5, kNoKeypoint = 6, kNoPoint = 7, kFused = 8,
              kReasons = 9 };

// slots of the counts array (int64 each)
enum Count { kCountC = 0, kCountStatus = 3, kCountReason = 4, kCounts = 16 };
// status bits
constexpr int kStatusBadRow = 1;                 // a rows entry outside [0, R)
constexpr int kStatusUnsorted = 2;               // rows not in ascending order
constexpr int kStatusBadQuery = 4;               // a row_query entry outside [0, Q), or row_query descending
constexpr int kStatusBadImage = 8;               // a row_db entry outside [0, n_images)
constexpr int kStatusBadCells = 16;              // (loftr_model_cells) a keypoint outside the grid, or cells not strictly ascending in an image
constexpr int kStatusBadPoint = 32;              // (loftr_model_cells) a kp_point entry outside [-1, P)

// cell (cy * gw + cx) of a position, -1 outside the grid or not finite
ATLAS_HD int cell_of(float x, float y, float inv, int gw, int gh) {
  if (!atlas::is_finite(x) || !atlas::is_finite(y)) return -1;
  const int cx = atlas::cell_coord(x, inv, gw), cy = atlas::cell_coord(y, inv, gh);
  return (cx | cy) < 0 ? -1 : cy * gw + cx;
}

// Reasons 2 .. 5 of a match whose row is good; kKept stands for "none of them", and *cell is then the database point's cell.
ATLAS_HD int classify(float xd, float yd, float xq, float yq, float conf, bool masked_out, float inv, int gw, int gh, int* cell) {
  *cell = -1;
  if (masked_out) return kMasked;
  if (!atlas::is_finite(xd) || !atlas::is_finite(yd) || !atlas::is_finite(xq) || !atlas::is_finite(yq) || !atlas::is_finite(conf))
    return kNonFinite;
  if (!(conf >= 0.f)) return kNegConf;
  const int cx = atlas::cell_coord(xd, inv, gw), cy = atlas::cell_coord(yd, inv, gh);
  if ((cx | cy) < 0) return kOutside;
  *cell = cy * gw + cx;
  return kKept;
}

// keypoint in [lo, hi) whose cell is `cell`, or -1; kp_cell ascends strictly in [lo, hi)
ATLAS_HD long find_cell(const int* kp_cell, long lo, long hi, int cell) {
  const long end = hi;
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (kp_cell[mid] < cell) lo = mid + 1; else hi = mid;
  }
  return (lo < end && kp_cell[lo] == cell) ? lo : -1;
}

ATLAS_HD uint64_t key_point(int query, int point) { return (((uint64_t)(uint32_t)query << 32) | (uint64_t)(uint32_t)point) + 1u; }

}  // namespace model_lookup
