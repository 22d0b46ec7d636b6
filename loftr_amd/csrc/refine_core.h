// Track refinement: where the fine windows of a point pair sit (the contract is in include/loftr_hip.h).  One text for the
// host routine (refine.hip) and the kernel (refine_gpu.hip): fp32 divisions, one addition, floorf and integer work only, nothing a
// compiler could contract, so both sides give the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#define RF_HD __host__ __device__ inline

#pragma clang fp contract(off)

namespace refine {

struct Geometry {
  int hf0, wf0, hf1, wf1;          // extents of the fine maps
  int h0c, w0c, h1c, w1c;          // extents of the coarse maps
  int stride;                      // fine pixels per coarse cell
  float s;                         // image pixels per fine pixel
};

RF_HD bool fin(float x) { return fabsf(x) <= 3.4028234663852886e38f; }         // false for NaN and the infinities

RF_HD bool geometry_ok(const Geometry& g) {
  return g.hf0 > 0 && g.wf0 > 0 && g.hf1 > 0 && g.wf1 > 0 && g.h0c > 0 && g.w0c > 0 && g.h1c > 0 && g.w1c > 0 && g.stride > 0 && fin(g.s) &&
         g.s > 0.f;
}

// clamp((int)floorf(p / scale / s + 0.5f), 0, extent - 1), the clamp taken in fp32 so that no value outside int is ever converted;
// scale == nullptr: the division by it is left out
RF_HD int centre(float p, const float* scale, float s, int extent) {
  float q = p;
  if (scale) q = q / *scale;
  q = floorf(q / s + 0.5f);
  if (!(q > 0.f)) return 0;
  if (q >= (float)(extent - 1)) return extent - 1;
  return (int)q;
}

RF_HD int coarse_cell(int c, int stride, int extent_c) {
  const int cell = (c + stride / 2) / stride;
  return cell < extent_c - 1 ? cell : extent_c - 1;
}

RF_HD float snapped(int c, float s, const float* scale) {
  float v = (float)c * s;
  if (scale) v = v * *scale;
  return v;
}

// One side of one row: centre (x, y), coarse cell and snapped point.  `p` = the point, `scale` = the pair's (w, h) scale or nullptr.
RF_HD void side(const float* p, const float* scale, bool ok, int hf, int wf, int hc, int wc, int stride, float s, int* c, int64_t* cell,
                float* p_s) {
  const float* sx = scale, *sy = scale ? scale + 1 : nullptr;
  const int cx = ok ? centre(p[0], sx, s, wf) : 0, cy = ok ? centre(p[1], sy, s, hf) : 0;
  c[0] = cx; c[1] = cy;
  *cell = ok ? (int64_t)coarse_cell(cy, stride, hc) * wc + coarse_cell(cx, stride, wc) : 0;
  p_s[0] = snapped(cx, s, sx); p_s[1] = snapped(cy, s, sy);
}

// Row m.  ok = every coordinate finite and the pair inside [0, n_pairs) (no scale is read for a pair outside it).  A row that is not ok
// has centre 0, cell 0 and the snapped point (0, 0) on both sides.
RF_HD void row(long m, const float* pts0, const float* pts1, const int64_t* b_ids, const float* scale0, const float* scale1, int n_pairs,
               const Geometry& g, int* c0, int* c1, int64_t* i_ids, int64_t* j_ids, float* pts0_s, float* pts1_s, uint8_t* ok) {
  const int64_t b = b_ids[m];
  const bool good = b >= 0 && b < n_pairs && fin(pts0[2 * m]) && fin(pts0[2 * m + 1]) && fin(pts1[2 * m]) && fin(pts1[2 * m + 1]);
  const float* sc0 = good && scale0 ? scale0 + 2 * b : nullptr;
  const float* sc1 = good && scale1 ? scale1 + 2 * b : nullptr;
  side(pts0 + 2 * m, sc0, good, g.hf0, g.wf0, g.h0c, g.w0c, g.stride, g.s, c0 + 2 * m, i_ids + m, pts0_s + 2 * m);
  side(pts1 + 2 * m, sc1, good, g.hf1, g.wf1, g.h1c, g.w1c, g.stride, g.s, c1 + 2 * m, j_ids + m, pts1_s + 2 * m);
  ok[m] = (uint8_t)good;
}

inline int check_args(const float* pts0, const float* pts1, const int64_t* b_ids, long M, int n_pairs, const Geometry& g, const int* c0,
                      const int* c1, const int64_t* i_ids, const int64_t* j_ids, const float* pts0_s, const float* pts1_s, const uint8_t* ok) {
  if (M < 0 || n_pairs < 0 || !geometry_ok(g)) return LOFTR_ERR_BAD_ARG;
  if (M > 0 && (!pts0 || !pts1 || !b_ids || !c0 || !c1 || !i_ids || !j_ids || !pts0_s || !pts1_s || !ok)) return LOFTR_ERR_BAD_ARG;
  return LOFTR_OK;
}

}  // namespace refine
