// The correspondence table of the images that have no pose yet (include/loftr_hip.h repeats the rule): every per-item step of
// loftr_register_corr_host (register.hip) and of the kernels of loftr_register_corr (register_gpu.hip), compiled from this one text for
// both sides.  Everything here is integer work and bit copies, so the two sides can differ only in the order of their writes, and the
// rule fixes that order: candidates by ascending image id, a candidate's rows in the order of its list.
//   1. Observation o of track j is a CORRESPONDENCE iff posed[obs_image[o]] == 0, status[j] == 0, the three floats of xyz[j] are finite
//      and the two floats of obs_xy[o] are finite (a NaN fails the test: it is made on the exponent bits).
//   2. n_corr[i]: the correspondences in image i's list (0 for a posed image).
//   3. Image i is a CANDIDATE iff it is not posed and n_corr[i] >= min_corr; candidates are numbered in ascending image id.
//   4. The table holds the correspondences of the candidates only, candidates in ascending rank, rows in the order of cam_obs.
// Self-contained: it includes none of the other *_core.h.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define REG_HD __host__ __device__ static inline
#else
#define REG_HD static inline
#endif

namespace reg {

constexpr int kCounts = 8;
constexpr int kMinCorr = 4;                                                      // a P3P sample and the point that picks its root
enum : int { kBadImage = 1, kBadOffsets = 2, kBadGroups = 4 };                   // error bits (counts[2]); §18's meanings

struct Ctx {
  // the problem
  const long* offsets; long T;
  const int* image; const float* xy; long N;
  const float* xyz; const uint8_t* status; const uint8_t* posed; int n;
  const long* cam_offsets; const int* cam_obs;
  int min_corr;
  // the result
  int* n_corr; int* cand_rank; int* cand_image; long* cand_offsets;
  float* corr_xyz; float* corr_xy; long* corr_bid; int* corr_obs; long* counts;
  // the workspace (layout(): the same on both sides)
  int* obs_track; uint8_t* obs_corr; int* img_corr; int* err;
};

// carves the workspace out of base (nullptr: sizes only) -> bytes
REG_HD size_t layout(Ctx& c, char* base) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return p;
  };
  c.err = (int*)take(sizeof(int));
  c.obs_track = (int*)take((size_t)c.N * sizeof(int));
  c.obs_corr = (uint8_t*)take((size_t)c.N);
  c.img_corr = (int*)take((size_t)c.n * sizeof(int));
  return off;
}

REG_HD bool finite_bits(const float* p) {                                        // false for NaN and the infinities
  return ((*(const uint32_t*)p) & 0x7f800000u) != 0x7f800000u;
}

// rule 1 for the observations of track t: obs_track, obs_corr -> error bits.  Reads nothing through a bad value.
REG_HD int track_flags(const Ctx& c, long t) {
  const long b = c.offsets[t], e = c.offsets[t + 1];
  if (b < 0 || e < b || e > c.N || (t == 0 && b != 0) || (t == c.T - 1 && e != c.N)) return kBadOffsets;
  for (long o = b; o < e; ++o) if (c.image[o] < 0 || c.image[o] >= c.n) return kBadImage;
  const float* X = c.xyz + 3 * t;
  const bool pt = c.status[t] == 0 && finite_bits(X) && finite_bits(X + 1) && finite_bits(X + 2);
  for (long o = b; o < e; ++o) {
    c.obs_track[o] = (int)t;
    c.obs_corr[o] = (uint8_t)(pt && c.posed[c.image[o]] == 0 && finite_bits(c.xy + 2 * o) && finite_bits(c.xy + 2 * o + 1));
  }
  return 0;
}

REG_HD bool group_range(const Ctx& c, long i, long* b, long* e) {
  *b = c.cam_offsets[i]; *e = c.cam_offsets[i + 1];
  return !(*b < 0 || *e < *b || *e > c.N || (i == 0 && *b != 0) || (i == c.n - 1 && *e != c.N));
}
// slot k of image i's list -> error bits, *corr = the observation is a correspondence.  Reads nothing through a bad value.
REG_HD int group_check(const Ctx& c, long i, long b, long k, bool* corr) {
  *corr = false;
  const int o = c.cam_obs[k];
  if (o < 0 || o >= c.N) return kBadGroups;
  if (c.image[o] != i) return kBadGroups;
  if (k > b && !(c.cam_obs[k - 1] < o)) return kBadGroups;
  *corr = c.obs_corr[o] != 0;
  return 0;
}

REG_HD bool candidate(const Ctx& c, long i, int cnt) { return c.posed[i] == 0 && cnt >= c.min_corr; }

// row `row` of the table: observation o of the candidate of rank r (bit copies)
REG_HD void write_row(const Ctx& c, long row, int r, int o) {
  const uint32_t* X = (const uint32_t*)(c.xyz + 3 * (long)c.obs_track[o]);
  const uint32_t* x = (const uint32_t*)(c.xy + 2 * (long)o);
  uint32_t* dX = (uint32_t*)(c.corr_xyz + 3 * row);
  uint32_t* dx = (uint32_t*)(c.corr_xy + 2 * row);
  dX[0] = X[0]; dX[1] = X[1]; dX[2] = X[2];
  dx[0] = x[0]; dx[1] = x[1];
  c.corr_bid[row] = r;
  c.corr_obs[row] = o;
}

// what an error leaves: the bits, C = P = 0
REG_HD void write_error(const Ctx& c, int err) {
  for (int k = 0; k < kCounts; ++k) c.counts[k] = 0;
  c.counts[2] = err;
}

}  // namespace reg
