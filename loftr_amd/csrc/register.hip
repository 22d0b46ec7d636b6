// loftr_register_corr_host: the host routine that DEFINES the correspondence table of the unposed images (the rule is in
// register_core.h and include/loftr_hip.h).  Sequential, in the order the rule names; register_gpu.hip reproduces it bit for bit.
#include <vector>
#include "common.h"
#include "register_core.h"

using namespace reg;

extern "C" int loftr_register_corr_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, long N, const float* xyz,
                                        const uint8_t* status, const uint8_t* posed, int n_images, const long* cam_offsets,
                                        const int* cam_obs, int min_corr, int* n_corr, int* cand_rank, int* cand_image, long* cand_offsets,
                                        float* corr_xyz, float* corr_xy, long* corr_bid, int* corr_obs, long* counts) {
  if (!offsets || !cam_offsets || !cand_offsets || !counts || T < 0 || N < 0 || n_images < 0) return LOFTR_ERR_BAD_ARG;
  if (T > 0 && (!xyz || !status)) return LOFTR_ERR_BAD_ARG;
  if (N > 0 && (!obs_image || !obs_xy || !cam_obs || !corr_xyz || !corr_xy || !corr_bid || !corr_obs)) return LOFTR_ERR_BAD_ARG;
  if (n_images > 0 && (!posed || !n_corr || !cand_rank || !cand_image)) return LOFTR_ERR_BAD_ARG;
  if (min_corr < kMinCorr) return LOFTR_ERR_BAD_ARG;
  if (T >= (1L << 31) || N >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  for (int k = 0; k < kCounts; ++k) counts[k] = 0;
  if ((T == 0 || n_images == 0) && N > 0) return LOFTR_ERR_BAD_ARG;              // observations outside every track or image
  Ctx c{};
  c.offsets = offsets; c.T = T; c.image = obs_image; c.xy = obs_xy; c.N = N; c.xyz = xyz; c.status = status; c.posed = posed; c.n = n_images;
  c.cam_offsets = cam_offsets; c.cam_obs = cam_obs; c.min_corr = min_corr;
  c.n_corr = n_corr; c.cand_rank = cand_rank; c.cand_image = cand_image; c.cand_offsets = cand_offsets;
  c.corr_xyz = corr_xyz; c.corr_xy = corr_xy; c.corr_bid = corr_bid; c.corr_obs = corr_obs; c.counts = counts;
  std::vector<char> ws(layout(c, nullptr), 0);
  layout(c, ws.data());
  const long n = n_images;
  int err = 0;
  for (long t = 0; t < T; ++t) err |= track_flags(c, t);
  if (err) { write_error(c, err); return LOFTR_ERR_BAD_ARG; }
  for (long i = 0; i < n; ++i) {
    long b, e;
    int cnt = 0;
    if (!group_range(c, i, &b, &e)) { err |= kBadGroups; continue; }
    for (long k = b; k < e; ++k) {
      bool corr;
      err |= group_check(c, i, b, k, &corr);
      cnt += corr;
    }
    c.img_corr[i] = posed[i] ? 0 : cnt;
  }
  if (err) { write_error(c, err); return LOFTR_ERR_BAD_ARG; }
  long C = 0, P = 0, unposed = 0, seen = 0, all = 0, largest = 0;
  for (long i = 0; i < n; ++i) {
    const int cnt = c.img_corr[i];
    n_corr[i] = cnt;
    unposed += posed[i] == 0;
    seen += posed[i] == 0 && cnt >= 1;
    all += cnt;
    if (cnt > largest) largest = cnt;
    if (!candidate(c, i, cnt)) { cand_rank[i] = -1; continue; }
    cand_rank[i] = (int)P;
    cand_image[P] = (int)i;
    cand_offsets[P] = C;
    long row = C;
    for (long k = cam_offsets[i]; k < cam_offsets[i + 1]; ++k) {
      const int o = cam_obs[k];
      if (c.obs_corr[o]) write_row(c, row++, (int)P, o);
    }
    C += cnt;
    P += 1;
  }
  cand_offsets[P] = C;
  counts[0] = C; counts[1] = P; counts[2] = 0; counts[3] = unposed; counts[4] = seen; counts[5] = all; counts[6] = largest; counts[7] = 0;
  return LOFTR_OK;
}
