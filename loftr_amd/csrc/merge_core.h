// Track merging (rows whose points meet and agree become one track): what the host routine (merge.hip) and the kernels (merge_gpu.hip)
// share.  complete_core.h (the source and target tests, the projection to a cell, the lower bound, the table checks) and
// triangulate_core.h (the camera table, residual2) are included unchanged; like them this is one text compiled for both sides, fp64
// without FMA contraction, + - * / only, so host and device take identical decisions and produce identical bits.  The rule is stated
// in include/loftr_hip.h and DESIGN §21:
//   * the candidate of a (row, image) pair: the keypoint within the threshold with the smallest (f32 bits of r2, index) among those
//     held by ANOTHER source row (the cells and the visiting order are completion's);
//   * the disjoint test: a merge walk over the two rows' ascending images;
//   * the weighted point of a pair and its agreement test: every masked observation of both rows within the threshold of that point;
//   * the key (f32 bits of the score) << 32 | partner: ONE unsigned 64-bit min per row picks "best score, then lowest partner"; all
//     ones is the empty entry, which no key equals because the bits of a finite float never are 0xFFFFFFFF.
#pragma once
#include "complete_core.h"

#pragma clang fp contract(off)

namespace merge {

constexpr int kCounts = 8;
using complete::kErrors;                         // counts[1]: completion's four error bits
enum Count { kMerged = 0, kSources = 2, kPairs = 3, kMeetings = 4, kDisjoint = 5, kAccepted = 6, kRelabelled = 7 };
constexpr uint64_t kNoPartner = ~(uint64_t)0;

struct In {
  complete::In c;                                // the tables of completion
  const float* xy;                               // [N,2] the pixel of every observation
  const uint8_t* mask;                           // [N] the observations that define the row's point
};

// step 2: the meeting of (source row j with point X, target image i) -> the other source row, -1 for none.  Candidates are visited by
// cell row, then by ascending index: "smallest (bits, index)" is a strict < on the bits.
TRI_HD long meet(const In& a, int i, long j, const double* X) {
  const complete::In& c = a.c;
  const double* P = c.tab + (long)tri::kCam * i;
  bool front;
  int cx, cy;
  if (!complete::project(P, X, c.inv, c.gw, c.gh, &front, &cx, &cy)) return -1;
  const long lo = c.kp_offsets[i], hi = c.kp_offsets[i + 1];
  const int y0 = cy - c.reach < 0 ? 0 : cy - c.reach, y1 = cy + c.reach > c.gh - 1 ? c.gh - 1 : cy + c.reach;
  const int x0 = cx - c.reach < 0 ? 0 : cx - c.reach, x1 = cx + c.reach > c.gw - 1 ? c.gw - 1 : cx + c.reach;
  long best = -1;
  uint32_t best_bits = 0;
  for (int y = y0; y <= y1; ++y) {
    const int first = y * c.gw + x0, last = y * c.gw + x1;
    for (long k = complete::lower_bound(c.kp_cell, lo, hi, first); k < hi && c.kp_cell[k] <= last; ++k) {
      const long m = c.kp_row[k];
      if (m < 0 || m == j) continue;                                               // free keypoints are completion's business
      double r2, Xm[3];
      if (!tri::residual2(P, X, (double)c.keypoints[2 * k], (double)c.keypoints[2 * k + 1], &r2) || !(r2 <= c.thr2)) continue;
      if (!complete::source(c, m, Xm)) continue;
      const uint32_t b = atlas::f32_bits((float)r2);
      if (best < 0 || b < best_bits) { best = m; best_bits = b; }
    }
  }
  return best;
}

// step 3: rows j and m share no image (all observations, masked or not)
TRI_HD bool disjoint(const complete::In& c, long j, long m) {
  long p = c.offsets[j], q = c.offsets[m];
  const long pe = c.offsets[j + 1], qe = c.offsets[m + 1];
  while (p < pe && q < qe) {
    const int ip = c.image[p], iq = c.image[q];
    if (ip == iq) return false;
    if (ip < iq) ++p; else ++q;
  }
  return true;
}

// step 4: the number of masked observations of row t
TRI_HD long weight(const In& a, long t) {
  long w = 0;
  for (long o = a.c.offsets[t]; o < a.c.offsets[t + 1]; ++o) w += a.mask[o] != 0;
  return w;
}
// every masked observation of row t lies in a target image within the threshold of X; *worst ends as the largest r2 seen
TRI_HD bool row_agrees(const In& a, long t, const double* X, double* worst) {
  for (long o = a.c.offsets[t]; o < a.c.offsets[t + 1]; ++o) {
    if (a.mask[o] == 0) continue;
    const int i = a.c.image[o];
    double r2;
    if (!complete::target_image(a.c, i)) return false;
    if (!tri::residual2(a.c.tab + (long)tri::kCam * i, X, (double)a.xy[2 * o], (double)a.xy[2 * o + 1], &r2) || !(r2 <= a.c.thr2)) return false;
    if (r2 > *worst) *worst = r2;
  }
  return true;
}
// the agreement of the source rows lo < hi (a function of the pair alone: both sides of a meeting compute the same bits)
TRI_HD bool agree(const In& a, long lo, long hi, uint32_t* bits) {
  const long wa = weight(a, lo), wb = weight(a, hi);
  if (wa == 0 || wb == 0) return false;
  double Xa[3], Xb[3], X[3];
  if (!complete::source(a.c, lo, Xa) || !complete::source(a.c, hi, Xb)) return false;
  for (int k = 0; k < 3; ++k) X[k] = ((double)wa * Xa[k] + (double)wb * Xb[k]) / (double)(wa + wb);
  double worst = 0.0;
  if (!row_agrees(a, lo, X, &worst) || !row_agrees(a, hi, X, &worst)) return false;
  *bits = atlas::f32_bits((float)worst);
  return true;
}

// steps 3-4 of a meeting (j, m): bit 0 disjoint, bit 1 accepted
TRI_HD int judge(const In& a, long j, long m, uint32_t* bits) {
  if (!disjoint(a.c, j, m)) return 0;
  return agree(a, j < m ? j : m, j < m ? m : j, bits) ? 3 : 1;
}

// step 5: the key a row holds for a partner, and what it unpacks to
TRI_HD uint64_t key(uint32_t bits, long partner) { return ((uint64_t)bits << 32) | (uint64_t)(uint32_t)partner; }
TRI_HD long key_partner(uint64_t w) { return (long)(uint32_t)w; }
using complete::key_r2;

// step 6: row j's survivor given the table of best keys (j itself when it does not merge); *r2 the pair's score when it merges
TRI_HD long survivor(const uint64_t* best, long j, bool* merged, float* r2) {
  const uint64_t w = best[j];
  *merged = false;
  if (w == kNoPartner) return j;
  const long m = key_partner(w);
  const uint64_t v = best[m];
  if (v == kNoPartner || key_partner(v) != j) return j;
  *merged = true;
  *r2 = key_r2(w);
  return j < m ? j : m;
}

}  // namespace merge
