// Track completion (points claim the atlas keypoints they project onto): what the host routine (complete.hip) and the kernels
// (complete_gpu.hip) share.  triangulate_core.h (the camera table, the projection arithmetic of residual2) and model_lookup_core.h (the
// cell arithmetic of the atlas) are included unchanged; like them this is one text compiled for both sides, fp64 without FMA
// contraction, + - * / only, so host and device take identical decisions and produce identical bits.  The rule is stated in
// include/loftr_hip.h and DESIGN §20:
//   * the source test of a row and the target test of an image (the merge walk over the row's ascending images is the caller's);
//   * the projection of a point to a cell of the atlas grid;
//   * the lower bound among the ascending cells of one image's keypoints and the order in which the candidates are visited;
//   * the proposal of a (row, image) pair: the free keypoint within the threshold with the smallest (f32 bits of r2, index);
//   * the key (f32 bits of r2) << 32 | row: ONE unsigned 64-bit min picks "nearest, then lowest row"; all ones is the empty claim,
//     which no key equals because the bits of a finite float never are 0xFFFFFFFF.
#pragma once
#include "triangulate_core.h"
#include "model_lookup_core.h"

#pragma clang fp contract(off)

namespace complete {

constexpr int kCounts = 8;
constexpr int kMaxReach = 8;
using tracks::kBadImage;                         // error bits (counts[1]): 1 an obs_image outside [0, n)
using tracks::kBadOffsets;                       // 2 offsets / kp_offsets that do not start at 0, end at N / K and ascend
enum : int { kBadOrder = 4, kBadRow = 8 };       // 4 obs_image descends within a row; 8 a kp_row outside [-1, T)
enum Count { kLinks = 0, kErrors = 1, kSources = 2, kPairs = 3, kInside = 4, kProposals = 5, kLost = 6, kBlocked = 7 };
enum : int { kFlagInside = 1, kFlagBlocked = 2 };
constexpr uint64_t kNoClaim = ~(uint64_t)0;

struct In {
  const long* offsets; long T;                   // rows: [T + 1] over the N observations
  const int* image; long N;
  const float* xyz; const uint8_t* status;       // [T,3], [T]
  const long* kp_offsets; const float* keypoints; const int* kp_cell; const int* kp_row; long K;
  const double* tab; const uint8_t* posed; int n;
  float inv; int gh, gw;
  double thr2; int reach;
};

TRI_HD bool sizes_ok(long T, long N, long K, int n) { return tracks::sizes_ok(T, N, n) && K >= 0 && K <= atlas::kMaxCells; }
TRI_HD bool grid_ok(int gh, int gw) {
  return gh >= 0 && gw >= 0 && gh <= atlas::kMaxGridSide && gw <= atlas::kMaxGridSide && (long)gh * gw <= atlas::kMaxCells;
}

// step 1: row j is a source; X = its point in fp64
TRI_HD bool source(const In& a, long j, double* X) {
  if (a.status[j] != 0) return false;
  const float* p = a.xyz + 3 * j;
  if (!atlas::is_finite(p[0]) || !atlas::is_finite(p[1]) || !atlas::is_finite(p[2])) return false;
  X[0] = (double)p[0]; X[1] = (double)p[1]; X[2] = (double)p[2];
  return true;
}

// step 2, the part that does not depend on the row: image i has a pose and a valid camera
TRI_HD bool target_image(const In& a, int i) { return a.posed[i] != 0 && tri::cam_valid(a.tab + (long)tri::kCam * i); }

// first index in [lo, hi) whose value is not below v (hi when there is none); a [lo, hi) ascends
TRI_HD long lower_bound(const int* a, long lo, long hi, int v) {
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// step 3: the cell of X in camera P (the x, y, z of tri::residual2, in its operation order); false behind the camera or outside the grid
TRI_HD bool project(const double* P, const double* X, float inv, int gw, int gh, bool* front, int* cx, int* cy) {
  const double x = (tri::dot3(P, X)) + P[3], y = (tri::dot3(P + 4, X)) + P[7], z = (tri::dot3(P + 8, X)) + P[11];
  *front = z > 0.0;
  if (!*front) return false;
  const double u = x / z, v = y / z;
  *cx = atlas::cell_coord((float)u, inv, gw);
  *cy = atlas::cell_coord((float)v, inv, gh);
  return (*cx | *cy) >= 0;
}

// the keypoint is free: it belongs to no row, or to a row without a point
TRI_HD bool is_free(const In& a, long k) {
  const int row = a.kp_row[k];
  return row == -1 || a.status[row] != 0;
}

// steps 3-5: the proposal of (X, target image i) -> keypoint index, -1 for none; *bits = f32 bits of its (float) r2;
// *flags: kFlagInside (in front and inside the grid), kFlagBlocked (no proposal, but a keypoint within the threshold that is not free).
// Candidates are visited by cell row, then by ascending index: "smallest (bits, index)" is a strict < on the bits.
TRI_HD long propose(const In& a, int i, const double* X, uint32_t* bits, int* flags) {
  const double* P = a.tab + (long)tri::kCam * i;
  bool front;
  int cx, cy;
  *flags = 0;
  *bits = 0;
  if (!project(P, X, a.inv, a.gw, a.gh, &front, &cx, &cy)) return -1;
  *flags = kFlagInside;
  const long lo = a.kp_offsets[i], hi = a.kp_offsets[i + 1];
  const int y0 = cy - a.reach < 0 ? 0 : cy - a.reach, y1 = cy + a.reach > a.gh - 1 ? a.gh - 1 : cy + a.reach;
  const int x0 = cx - a.reach < 0 ? 0 : cx - a.reach, x1 = cx + a.reach > a.gw - 1 ? a.gw - 1 : cx + a.reach;
  long best = -1;
  uint32_t best_bits = 0;
  bool blocked = false;
  for (int y = y0; y <= y1; ++y) {
    const int first = y * a.gw + x0, last = y * a.gw + x1;
    for (long k = lower_bound(a.kp_cell, lo, hi, first); k < hi && a.kp_cell[k] <= last; ++k) {
      double r2;
      if (!tri::residual2(P, X, (double)a.keypoints[2 * k], (double)a.keypoints[2 * k + 1], &r2) || !(r2 <= a.thr2)) continue;
      if (!is_free(a, k)) { blocked = true; continue; }
      const uint32_t b = atlas::f32_bits((float)r2);
      if (best < 0 || b < best_bits) { best = k; best_bits = b; }
    }
  }
  if (best < 0 && blocked) *flags |= kFlagBlocked;
  *bits = best_bits;
  return best;
}

// step 6: the key of row j's proposal and what a winning key holds
TRI_HD uint64_t key(uint32_t bits, long j) { return ((uint64_t)bits << 32) | (uint64_t)(uint32_t)j; }
TRI_HD int key_row(uint64_t w) { return (int)(uint32_t)w; }
TRI_HD float key_r2(uint64_t w) {
  const uint32_t b = (uint32_t)(w >> 32);
  float f;
  memcpy(&f, &b, sizeof(f));
  return f;
}

// the checks of the tables (error bits); each reads nothing through a bad value
TRI_HD int check_row(const In& a, long t) {
  long b, e;
  if (!tracks::span(a.offsets, a.T, a.N, t, &b, &e)) return kBadOffsets;
  int err = 0;
  for (long o = b; o < e; ++o) {
    if (a.image[o] < 0 || a.image[o] >= a.n) err |= kBadImage;
    if (o > b && a.image[o] < a.image[o - 1]) err |= kBadOrder;
  }
  return err;
}
TRI_HD int check_keypoint(const In& a, long k) { return (a.kp_row[k] < -1 || a.kp_row[k] >= a.T) ? kBadRow : 0; }
TRI_HD int check_image(const In& a, int i) {
  const long b = a.kp_offsets[i], e = a.kp_offsets[i + 1];
  return (b < 0 || e < b || e > a.K || (i == 0 && b != 0) || (i == a.n - 1 && e != a.K)) ? kBadOffsets : 0;
}

}  // namespace complete
