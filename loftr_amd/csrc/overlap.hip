// View overlap, host routine (plain C++ on host arrays, double precision): overlap[i, j] = how many of the points that source image i
// observes project into target view j inside the image, within a viewing-angle change and a change of apparent size that the matcher can
// bridge (the contract is in include/loftr_hip.h).  The idea is the one hloc ships as pairs_from_covisibility /
// pairs_from_poses; hloc is not in this image, so this is a statement of the idea, NOT of its source.  PARITY UNPINNED against it.
// This function DEFINES the result: loftr_view_overlap (overlap_gpu.hip) reproduces it exactly, which is why the per-entry predicate
// lives in overlap_core.h.  It is written as sources x entries x targets in order.
#include <stdint.h>
#include <vector>
#include "../../include/loftr_hip.h"
#include "overlap_core.h"

#pragma clang fp contract(off)

using namespace overlap;

extern "C" int loftr_view_overlap_host(const long* vis_offsets, const int* vis_point, long V, const float* xyz, const uint8_t* point_ok, long T,
                                       const double* K_src, const double* T_src, const uint8_t* src_ok, int n, const double* K_tgt,
                                       const double* T_tgt, const uint8_t* tgt_ok, const double* tgt_hw, int m, double border_px,
                                       double cos_min, double max_scale2, int* overlap_out, int* n_vis, long* counts) {
  if (!counts || V < 0 || T < 0 || n < 0 || m < 0) return LOFTR_ERR_BAD_ARG;
  if (n > 0 && (!vis_offsets || !K_src || !T_src || !src_ok || !n_vis)) return LOFTR_ERR_BAD_ARG;
  if (m > 0 && (!K_tgt || !T_tgt || !tgt_ok || !tgt_hw)) return LOFTR_ERR_BAD_ARG;
  if (V > 0 && !vis_point) return LOFTR_ERR_BAD_ARG;
  if (T > 0 && (!xyz || !point_ok)) return LOFTR_ERR_BAD_ARG;
  if (n > 0 && m > 0 && !overlap_out) return LOFTR_ERR_BAD_ARG;
  if (!params_ok(border_px, cos_min, max_scale2)) return LOFTR_ERR_BAD_ARG;
  if (n == 0 && V != 0) return LOFTR_ERR_BAD_ARG;                                        // entries outside every list
  if (!sizes_ok(V, T, n, m)) return LOFTR_ERR_UNSUPPORTED;
  int err = 0;
  for (int i = 0; i < n; ++i) err |= check_source(vis_offsets, n, V, i);
  for (long k = 0; k < V; ++k) err |= check_entry(vis_point, T, k);
  for (int c = 0; c < kCounts; ++c) counts[c] = 0;
  counts[kErrors] = err;
  if (err) return LOFTR_ERR_BAD_ARG;
  std::vector<double> tgt((size_t)kView * (size_t)m);
  for (int j = 0; j < m; ++j) {
    view_table(K_tgt + 9 * (size_t)j, T_tgt + 16 * (size_t)j, tgt_ok[j] != 0, tgt_hw + 2 * (size_t)j, border_px, &tgt[(size_t)kView * j]);
    counts[kTargets] += view_valid(&tgt[(size_t)kView * j]);
  }
  std::vector<int> row((size_t)m);
  for (int i = 0; i < n; ++i) {
    double src[kView];
    view_table(K_src + 9 * (size_t)i, T_src + 16 * (size_t)i, src_ok[i] != 0, nullptr, border_px, src);
    for (int j = 0; j < m; ++j) row[(size_t)j] = 0;
    int vis = 0;
    if (view_valid(src)) {
      ++counts[kSources];
      for (long k = vis_offsets[i]; k < vis_offsets[i + 1]; ++k) {
        double X[3], pt[kPoint];
        if (!usable(xyz, point_ok, vis_point[k], X)) continue;
        ++vis;
        point_terms(src, X, pt);
        for (int j = 0; j < m; ++j) {
          const double* t = &tgt[(size_t)kView * j];
          if (view_valid(t) && counts_for(t, pt, src[tri::kCam], border_px, cos_min, max_scale2)) ++row[(size_t)j];
        }
      }
    }
    n_vis[i] = vis;
    counts[kVisible] += vis;
    for (int j = 0; j < m; ++j) {
      overlap_out[(size_t)i * (size_t)m + (size_t)j] = row[(size_t)j];
      counts[kNonZero] += row[(size_t)j] != 0;
    }
  }
  return LOFTR_OK;
}
