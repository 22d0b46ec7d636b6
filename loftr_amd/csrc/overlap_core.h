// View overlap (which image pairs are worth matching, from the model): what the host routine (overlap.hip) and the kernels
// (overlap_gpu.hip) share.  triangulate_core.h (the camera table, the projection order of residual2) and atlas_core.h (the exponent-bit
// finiteness test of a float) are included unchanged; like them this is one text compiled for both sides, fp64 without FMA contraction,
// + - * / and sqrt only, so host and device take identical decisions.  The rule is stated in include/loftr_hip.h and DESIGN §23:
//   * the table of a source and of a target view (all NaN when the view is not valid);
//   * the usable entry of a visibility list and the terms of a point that do not depend on the target: X, a = c_i - X, aa = a . a;
//   * the predicate "entry counts for target j": in front, inside the image less the border, viewing angle, ratio of apparent sizes;
//   * the checks of the lists (error bits); each reads nothing through a bad value.
// Every rejection is written as "unless (x > y)": a NaN rejects.
#pragma once
#include "triangulate_core.h"
#include "atlas_core.h"

#pragma clang fp contract(off)

namespace overlap {

constexpr int kCounts = 8;
enum Count { kVisible = 0, kErrors = 1, kSources = 2, kTargets = 3, kNonZero = 4 };
enum : int { kBadPoint = 1 };                    // error bits (counts[1]): 1 a vis_point outside [0, T)
using tracks::kBadOffsets;                       // 2 vis_offsets that do not start at 0, end at V and ascend
constexpr int kView = tri::kCam + 4;             // doubles per view of a table: tri::cam_table [24], fx^2, H - border, W - border, 0

TRI_HD bool sizes_ok(long V, long T, int n, int m) {
  return V >= 0 && T >= 0 && n >= 0 && m >= 0 && V < (1L << 31) && T < (1L << 31) && (long)n * (long)m <= (1L << 31);
}
TRI_HD bool params_ok(double border, double cos_min, double max_scale2) {
  return border >= 0.0 && tri::fin(border) && cos_min >= -1.0 && cos_min <= 1.0 && max_scale2 >= 1.0;          // (NaN fails each)
}

// step 1: the table of a view; hw == nullptr for a source.  An invalid view is all NaN, so tri::cam_valid answers for the whole of step 1.
TRI_HD void view_table(const double* K, const double* T, bool ok, const double* hw, double border, double* tab) {
  tri::cam_table(K, T, tab);
  tab[tri::kCam] = K[0] * K[0];
  tab[tri::kCam + 1] = hw ? hw[0] - border : 0.0;
  tab[tri::kCam + 2] = hw ? hw[1] - border : 0.0;
  tab[tri::kCam + 3] = 0.0;
  if (hw) ok = ok && tri::fin(hw[0]) && tri::fin(hw[1]) && hw[0] > 0.0 && hw[1] > 0.0;
  if (!ok || !tri::cam_valid(tab)) for (int i = 0; i < kView; ++i) tab[i] = __builtin_nan("");
}
TRI_HD bool view_valid(const double* tab) { return tri::cam_valid(tab); }

// step 2: entry p (already known to lie in [0, T)) is usable; X = its point in fp64
TRI_HD bool usable(const float* xyz, const uint8_t* point_ok, long p, double* X) {
  if (point_ok[p] == 0) return false;
  const float* q = xyz + 3 * p;
  if (!atlas::is_finite(q[0]) || !atlas::is_finite(q[1]) || !atlas::is_finite(q[2])) return false;
  X[0] = (double)q[0]; X[1] = (double)q[1]; X[2] = (double)q[2];
  return true;
}

// the terms of a usable entry of source i that every target shares: pt = X [3], a = c_i - X [3], aa
constexpr int kPoint = 7;
TRI_HD void point_terms(const double* src_tab, const double* X, double* pt) {
  const double* c = src_tab + 12;
  pt[0] = X[0]; pt[1] = X[1]; pt[2] = X[2];
  pt[3] = c[0] - X[0]; pt[4] = c[1] - X[1]; pt[5] = c[2] - X[2];
  pt[6] = tri::dot3(pt + 3, pt + 3);
}

// step 3: the entry with terms pt of a source with fx^2 = f2i counts for the valid target tab
TRI_HD bool counts_for(const double* tab, const double* pt, double f2i, double border, double cos_min, double max_scale2) {
  const double* P = tab;
  const double x = (tri::dot3(P, pt)) + P[3], y = (tri::dot3(P + 4, pt)) + P[7], z = (tri::dot3(P + 8, pt)) + P[11];
  if (!(z > 0.0)) return false;
  const double u = x / z, v = y / z;
  if (!(u >= border) || !(u < tab[tri::kCam + 2]) || !(v >= border) || !(v < tab[tri::kCam + 1])) return false;
  const double b[3] = {tab[12] - pt[0], tab[13] - pt[1], tab[14] - pt[2]};
  const double aa = pt[6], bb = tri::dot3(b, b), d = tri::dot3(pt + 3, b);
  if (!(d >= cos_min * sqrt(aa * bb))) return false;
  const double sj = tab[tri::kCam] * aa, si = f2i * bb;
  return (sj <= max_scale2 * si) && (si <= max_scale2 * sj);
}

// the checks of the lists (error bits)
TRI_HD int check_source(const long* vis_offsets, int n, long V, int i) {
  long b, e;
  return tracks::span(vis_offsets, n, V, i, &b, &e) ? 0 : kBadOffsets;
}
TRI_HD int check_entry(const int* vis_point, long T, long k) { return (vis_point[k] < 0 || vis_point[k] >= T) ? kBadPoint : 0; }

}  // namespace overlap
