// Keypoint atlas (pair lists -> consolidated keypoints, index matches, tracks): what the host routine (atlas.hip) and the kernels
// (atlas_gpu.hip) share, as geometry_core.h is shared by the estimators.  Everything here is integer or a single fp32 multiply, so
// host and device agree bit for bit:
//   * the cell of an observation and the reason a match is dropped (rule 1 of DESIGN §15);
//   * the 64-bit word `conf_bits << 32 | (0xFFFFFFFF - index)`: non-negative finite fp32 bit patterns order like the floats, so ONE
//     unsigned 64-bit max picks "greatest conf, then smallest index" (rules 2 and 3); 0 is the empty word, which no observation packs to
//     because indices stop short of 0xFFFFFFFF (kMaxMatches);
//   * the keys and the hash of the open-addressing table (rule 3: (row, side, keypoint); rule 4: (label, image)); key 0 is the empty slot.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATLAS_HD __host__ __device__ inline
#else
#define ATLAS_HD inline
#endif

namespace atlas {

constexpr long kMaxMatches = 0x7FFFFFFEL;        // observation index 2 m + side <= 0xFFFFFFFD: the packed word is never 0
constexpr long kMaxCells = 0x7FFFFFFFL;          // n_images * gh * gw (a cell id and a keypoint index are int32)
constexpr long kMaxRows = 1L << 30;              // (row << 33 | side << 32 | keypoint) + 1 fits 64 bits
constexpr int kMaxGridSide = 1 << 24;            // (float)gw is exact

// why a match is not used; the first that applies, in this order
enum Reason { kValid = 0, kBadRow = 1, kMasked = 2, kNonFinite = 3, kNegConf = 4, kOutside = 5, kReasons = 6 };

// slots of the counts array that finalize leaves (int64 each)
enum Count { kCountK = 0, kCountMk = 1, kCountT = 2, kCountStatus = 3, kCountReason = 4, kCounts = 16 };
// status bits raised by the observe step
constexpr int kStatusBadRow = 1;                 // an m_bids entry outside [0, n)
constexpr int kStatusUnsorted = 2;               // m_bids of one add not in ascending order

ATLAS_HD uint32_t f32_bits(float v) {
  uint32_t b;
  memcpy(&b, &v, sizeof(b));
  return b;
}
ATLAS_HD bool is_finite(float v) { return (f32_bits(v) & 0x7F800000u) != 0x7F800000u; }

// cell coordinate of x on a side of g cells: floorf(x * inv), one fp32 multiply; -1 outside [0, g)
ATLAS_HD int cell_coord(float x, float inv, int g) {
  const float f = floorf(x * inv);
  return (f >= 0.f && f < (float)g) ? (int)f : -1;
}

// Reason of one match and, when valid, the cells (cy * gw + cx) of its two observations.
ATLAS_HD int classify(float x0, float y0, float x1, float y1, float conf, bool row_ok, bool masked_out, float inv, int gw, int gh,
                      int* cell0, int* cell1) {
  *cell0 = *cell1 = -1;
  if (!row_ok) return kBadRow;
  if (masked_out) return kMasked;
  if (!is_finite(x0) || !is_finite(y0) || !is_finite(x1) || !is_finite(y1) || !is_finite(conf)) return kNonFinite;
  if (!(conf >= 0.f)) return kNegConf;
  const int cx0 = cell_coord(x0, inv, gw), cy0 = cell_coord(y0, inv, gh), cx1 = cell_coord(x1, inv, gw), cy1 = cell_coord(y1, inv, gh);
  if ((cx0 | cy0 | cx1 | cy1) < 0) return kOutside;
  *cell0 = cy0 * gw + cx0;
  *cell1 = cy1 * gw + cx1;
  return kValid;
}

// conf >= 0 and finite.  -0.0 packs as +0.0 (its bit pattern would order above every positive float).
ATLAS_HD uint64_t pack(float conf, uint32_t index) {
  const uint32_t c = conf == 0.f ? 0u : f32_bits(conf);
  return ((uint64_t)c << 32) | (uint64_t)(0xFFFFFFFFu - index);
}
ATLAS_HD uint32_t packed_index(uint64_t w) { return 0xFFFFFFFFu - (uint32_t)w; }

ATLAS_HD uint64_t key_match(int row, int side, int keypoint) {
  return (((uint64_t)(uint32_t)row << 33) | ((uint64_t)(uint32_t)side << 32) | (uint64_t)(uint32_t)keypoint) + 1u;
}
ATLAS_HD uint64_t key_track(int label, int image) { return (((uint64_t)(uint32_t)label << 32) | (uint64_t)(uint32_t)image) + 1u; }

// splitmix64 finaliser
ATLAS_HD uint64_t hash64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// power of two, load <= 0.5 for `entries` keys: a probe always meets an empty slot
inline uint64_t table_capacity(uint64_t entries) {
  uint64_t cap = 64;
  while (cap < 2 * entries) cap <<= 1;
  return cap;
}

inline long keypoint_bound(long M, long cells) { return 2 * M < cells ? 2 * M : cells; }

}  // namespace atlas
