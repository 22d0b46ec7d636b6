// Stand-alone driver of the host routine of the bundle adjustment with focal refinement (csrc/bundle.hip) for a sanitizer
// pass on the CPU: a hand-written problem (a camera with fx = 0, one without observations, a NaN point, a masked observation, a mixed
// refine mask), a start at the optimum, a start whose first trials leave the focal bounds, and the empty problems.  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/bundle_focal_host_driver.cpp loftr_amd/csrc/bundle.hip -o driver
//   ./driver
// It uses no GPU.  Inputs and outputs live in exactly-sized heap blocks, so that a read or write past an end is caught.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../include/loftr_hip.h"

struct Problem {
  std::vector<long> offsets{0};
  std::vector<int> image;
  std::vector<float> xy, xyz;
  std::vector<uint8_t> mask, fixed, refine;
  std::vector<double> K, K_true, T;
  std::vector<long> cam_offsets;
  std::vector<int> cam_obs;
  int n() const { return (int)fixed.size(); }
  // a camera at centre (cx, cy, 0) looking along +z; f_true makes the observations, f is what the adjustment is given
  void camera(double cx, double cy, double f_true, double f, bool fix, bool ref) {
    const double Kt[9] = {f_true, 0, 320, 0, f_true, 240, 0, 0, 1}, Kg[9] = {f, 0, 320, 0, f, 240, 0, 0, 1};
    const double Tc[16] = {1, 0, 0, -cx, 0, 1, 0, -cy, 0, 0, 1, 0, 0, 0, 0, 1};
    K_true.insert(K_true.end(), Kt, Kt + 9);
    K.insert(K.end(), Kg, Kg + 9);
    T.insert(T.end(), Tc, Tc + 16);
    fixed.push_back(fix);
    refine.push_back(ref);
  }
  // a point seen by the cameras listed, projected with the true intrinsics; the start is moved by (dx, 0, 0)
  void track(double X, double Y, double Z, const std::vector<int>& cams, double dx) {
    for (int c : cams) {
      const double* k = &K_true[9 * c];
      const double* t = &T[16 * c];
      const double y0 = X + t[3], y1 = Y + t[7], y2 = Z + t[11];
      image.push_back(c);
      xy.push_back((float)(k[0] * y0 / y2 + k[2]));
      xy.push_back((float)(k[4] * y1 / y2 + k[5]));
      mask.push_back(1);
    }
    offsets.push_back((long)image.size());
    xyz.push_back((float)(X + dx)); xyz.push_back((float)Y); xyz.push_back((float)Z);
  }
  void group() {
    cam_obs.resize(image.size());
    std::iota(cam_obs.begin(), cam_obs.end(), 0);
    std::stable_sort(cam_obs.begin(), cam_obs.end(), [&](int a, int b) { return image[a] < image[b]; });
    cam_offsets.assign(n() + 1, 0);
    for (int im : image) cam_offsets[im + 1] += 1;
    for (int i = 0; i < n(); ++i) cam_offsets[i + 1] += cam_offsets[i];
  }
};

struct Result {
  int status;
  std::vector<double> T, K;
  std::vector<float> xyz;
  std::vector<uint8_t> obs_active, cam_free, point_active, cam_focal;
  std::vector<long> counts;
  double real(int k) const { double d; memcpy(&d, &counts[k], 8); return d; }
};

template <class T> static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

static Result run(Problem& p, int max_iters, int min_focal_obs, double lo, double hi) {
  const long T = (long)p.offsets.size() - 1, N = (long)p.image.size();
  const int n = p.n();
  Result r;
  r.T.assign(16 * n, -1.0); r.K.assign(9 * n, -1.0); r.xyz.assign(3 * T, -1.f);
  r.obs_active.assign(N, 9); r.cam_free.assign(n, 9); r.point_active.assign(T, 9); r.cam_focal.assign(n, 9);
  r.counts.assign(16, 7);
  r.status = loftr_bundle_adjust_focal_host(p.offsets.data(), T, ptr(p.image), ptr(p.xy), ptr(p.mask), N, ptr(p.xyz), ptr(p.K), ptr(p.T), ptr(p.fixed),
                                            ptr(p.refine), n, p.cam_offsets.data(), ptr(p.cam_obs), 0.0, max_iters, 30, 1e-2, 1e-9, min_focal_obs,
                                            lo, hi, ptr(r.T), ptr(r.xyz), ptr(r.obs_active), ptr(r.cam_free), ptr(r.point_active), ptr(r.K),
                                            ptr(r.cam_focal), r.counts.data());
  return r;
}

// cameras 0 and 1 fixed, `free_cams` further ones whose focal is off by the factor `off`; a 4 x 4 grid of points at two depths seen by all
static Problem scene(int free_cams, double off, double dx) {
  Problem p;
  p.camera(-1.0, 0.0, 500.0, 500.0, true, true);
  p.camera(1.0, 0.1, 520.0, 520.0, true, true);
  for (int i = 0; i < free_cams; ++i) p.camera(-0.5 + 0.5 * i, 0.25 * (i % 3) - 0.25, 480.0 + 15.0 * i, (480.0 + 15.0 * i) * off, false, true);
  std::vector<int> all(p.n());
  std::iota(all.begin(), all.end(), 0);
  for (int z = 0; z < 2; ++z)
    for (int x = 0; x < 4; ++x)
      for (int y = 0; y < 4; ++y) p.track(-0.75 + 0.5 * x, -0.6 + 0.4 * y, 4.0 + 3.0 * z + 0.1 * x, all, dx);
  return p;
}

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b, size_t at, size_t len) {
  return memcmp(a.data() + at, b.data() + at, 8 * len) == 0;
}

int main() {
  // ---- the hand-written problem: cameras 0, 1 fixed; 2, 3, 4 free (4 left out of the mask); 5 with fx = 0; 6 without an observation
  Problem h = scene(3, 1.06, 0.02);
  h.camera(0.3, 0.3, 500.0, 500.0, false, true);                       // 5
  h.K[9 * 5] = 0.0;
  h.camera(2.0, 2.0, 500.0, 500.0, false, true);                       // 6
  h.refine[4] = 0;
  h.track(0.1, 0.1, 5.0, {0, 1, 5}, 0.0);                               // 32: its observation in camera 5 cannot be active
  h.track(0.2, -0.1, 5.0, {0, 1, 2}, 0.0);                              // 33: a NaN point
  h.xyz[3 * 33 + 1] = NAN;
  h.track(-0.2, 0.2, 6.0, {0, 2, 3}, 0.0);                              // 34: the observation in camera 0 is masked out
  h.mask[h.offsets[34]] = 0;
  h.group();
  Result r = run(h, 30, 1, 0.5, 2.0);
  EXPECT(r.status == LOFTR_OK && r.counts[0] == 0 && r.counts[1] == 0);
  EXPECT((r.cam_free == std::vector<uint8_t>{0, 0, 1, 1, 1, 0, 0}) && (r.cam_focal == std::vector<uint8_t>{0, 0, 1, 1, 0, 0, 0}));
  EXPECT(r.counts[7] == 3 && r.counts[13] == 2 && r.counts[6] == 34);
  EXPECT(!r.obs_active[h.offsets[32] + 2] && r.point_active[32] && !r.point_active[33] && !r.obs_active[h.offsets[34]] && r.point_active[34]);
  for (int i : {0, 1, 4, 5, 6}) EXPECT(same_bits(r.K, h.K, 9 * i, 9));
  for (int i : {0, 1, 5, 6}) EXPECT(same_bits(r.T, h.T, 16 * i, 16));
  for (int i : {2, 3}) {
    EXPECT(fabs(r.K[9 * i] / h.K_true[9 * i] - 1.0) < 0.5 * 0.06 && fabs(r.K[9 * i + 4] / h.K_true[9 * i + 4] - 1.0) < 0.5 * 0.06);
    EXPECT(r.K[9 * i + 2] == 320.0 && r.K[9 * i + 5] == 240.0 && r.K[9 * i + 8] == 1.0 && r.K[9 * i + 3] == 0.0);
  }
  EXPECT(r.real(9) < r.real(8) && isnan(r.xyz[3 * 33 + 1]));
  // min_focal_obs above every list: nobody refines, every K comes back
  r = run(h, 30, 1000, 0.5, 2.0);
  EXPECT(r.status == LOFTR_OK && r.counts[13] == 0 && same_bits(r.K, h.K, 0, h.K.size()) && r.counts[7] == 3);

  // ---- a start at the optimum: no trial, every bit back
  Problem e = scene(2, 1.0, 0.0);
  e.group();
  r = run(e, 30, 1, 0.5, 2.0);
  EXPECT(r.status == LOFTR_OK && r.counts[13] == 2);
  if (r.real(8) == 0.0) EXPECT(r.counts[0] == 0 && r.counts[2] == 0 && same_bits(r.K, e.K, 0, e.K.size()));
  EXPECT(r.real(9) <= r.real(8));

  // ---- bounds: the focal is 8 % off, (0.97, 1.03) rejects the first trial; nothing moves in one trial, and no result leaves the bounds
  Problem b = scene(3, 1.08, 0.02);
  b.group();
  r = run(b, 1, 1, 0.97, 1.03);
  EXPECT(r.status == LOFTR_OK && r.counts[2] == 1 && r.counts[3] == 0 && r.counts[0] == 1 && r.real(12) == 10.0 * 1e-4);
  EXPECT(same_bits(r.K, b.K, 0, b.K.size()) && r.real(9) == r.real(8));
  r = run(b, 40, 1, 0.97, 1.03);
  EXPECT(r.status == LOFTR_OK && r.counts[3] < r.counts[2]);
  for (int i = 2; i < 5; ++i) EXPECT(r.K[9 * i] / b.K[9 * i] > 0.97 && r.K[9 * i] / b.K[9 * i] < 1.03);
  r = run(b, 40, 1, 0.5, 2.0);
  EXPECT(r.status == LOFTR_OK && r.counts[0] == 0 && r.counts[13] == 3);
  for (int i = 2; i < 5; ++i) EXPECT(fabs(r.K[9 * i] / b.K_true[9 * i] - 1.0) < 0.01);
  EXPECT(run(b, 40, 0, 0.5, 2.0).status == LOFTR_ERR_BAD_ARG && run(b, 40, 1, 1.0, 2.0).status == LOFTR_ERR_BAD_ARG);
  EXPECT(run(b, 40, 1, 0.5, NAN).status == LOFTR_ERR_BAD_ARG && run(b, 40, 1, 0.5, 1.0).status == LOFTR_ERR_BAD_ARG);

  // ---- the empty problems: no image at all; images and points without an observation
  Problem z;
  z.group();
  r = run(z, 30, 1, 0.5, 2.0);
  EXPECT(r.status == LOFTR_OK && r.counts[0] == 3 && r.counts[13] == 0);
  Problem o = scene(2, 1.05, 0.0);
  o.offsets.assign(o.offsets.size(), 0);
  o.image.clear(); o.xy.clear(); o.mask.clear();
  o.group();
  r = run(o, 30, 1, 0.5, 2.0);
  EXPECT(r.status == LOFTR_OK && r.counts[0] == 3 && r.counts[7] == 0 && r.counts[13] == 0 && same_bits(r.K, o.K, 0, o.K.size()));
  EXPECT(same_bits(r.T, o.T, 0, o.T.size()) && (r.cam_focal == std::vector<uint8_t>(4, 0)));
  // an image id out of range is answered before anything is read through it
  Problem bad = scene(2, 1.05, 0.0);
  bad.group();
  bad.image[5] = 9;
  EXPECT(run(bad, 30, 1, 0.5, 2.0).status == LOFTR_ERR_BAD_ARG);
  printf("bundle_focal_host_driver: all cases passed\n");
  return 0;
}
