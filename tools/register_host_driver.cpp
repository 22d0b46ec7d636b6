// Stand-alone driver of the host routine of the correspondence table (csrc/register.hip) for a sanitizer pass on the CPU: the
// hand-written cases of tests/_registration_cases.py (hand(), all posed, none posed, T = 0, N = 0, n = 0, the error bits).  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/register_host_driver.cpp loftr_amd/csrc/register.hip -o driver
//   ./driver
// It uses no GPU.  Inputs and outputs live in exactly-sized heap blocks, so that a read or write past an end is caught.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../include/loftr_hip.h"

struct Case {
  std::vector<long> offsets;
  std::vector<int> image;
  std::vector<float> xy, xyz;
  std::vector<uint8_t> status, posed;
  std::vector<long> cam_offsets;
  std::vector<int> cam_obs;
  void group() {
    const int n = (int)posed.size();
    cam_obs.resize(image.size());
    std::iota(cam_obs.begin(), cam_obs.end(), 0);
    std::stable_sort(cam_obs.begin(), cam_obs.end(), [&](int a, int b) { return image[a] < image[b]; });
    cam_offsets.assign(n + 1, 0);
    for (int im : image) if (im >= 0 && im < n) cam_offsets[im + 1] += 1;
    for (int i = 0; i < n; ++i) cam_offsets[i + 1] += cam_offsets[i];
  }
};

template <class T> static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

static int run(Case& c, int min_corr, std::vector<int>* n_corr_out, std::vector<long>* counts_out) {
  const long T = (long)c.offsets.size() - 1, N = (long)c.image.size();
  const int n = (int)c.posed.size();
  std::vector<int> n_corr(n), cand_rank(n), cand_image(n), corr_obs(N);
  std::vector<long> cand_offsets(n + 1), corr_bid(N), counts(8);
  std::vector<float> corr_xyz(3 * N), corr_xy(2 * N);
  const int st = loftr_register_corr_host(c.offsets.data(), T, ptr(c.image), ptr(c.xy), N, ptr(c.xyz), ptr(c.status), ptr(c.posed), n,
                                          c.cam_offsets.data(), ptr(c.cam_obs), min_corr, ptr(n_corr), ptr(cand_rank), ptr(cand_image),
                                          cand_offsets.data(), ptr(corr_xyz), ptr(corr_xy), ptr(corr_bid), ptr(corr_obs), counts.data());
  if (n_corr_out) *n_corr_out = n_corr;
  if (counts_out) *counts_out = counts;
  return st;
}

static Case hand() {
  const float nan = NAN, inf = INFINITY;
  struct Obs { int im; float x, y; };
  struct Track { int status; float X[3]; std::vector<Obs> obs; };
  const std::vector<Track> tracks = {
      {0, {0, 0, 4}, {{0, 1, 1}, {1, 2, 2}, {2, 3, 3}, {3, 4, 4}}},
      {0, {1, 0, 4}, {{0, 1, 2}, {1, 2, 3}, {2, 3, 4}, {3, 4, 5}, {3, 4.5f, 5.5f}}},
      {0, {2, 0, 4}, {{1, 5, 5}, {2, 6, 6}, {5, 7, 7}}},
      {0, {3, 0, 4}, {{1, 8, 8}, {3, 9, 9}, {0, 9, 1}}},
      {3, {4, 0, 4}, {{1, 1, 9}, {2, 2, 9}, {3, 3, 9}}},
      {0, {5, nan, 4}, {{1, 1, 8}, {2, 2, 8}, {3, 3, 8}}},
      {0, {6, 0, inf}, {{1, 1, 7}, {2, 2, 7}}},
      {0, {7, 0, 4}, {{1, nan, 7}, {2, 2, nan}, {3, 3, 6}, {4, inf, 1}}},
      {0, {8, 0, 4}, {}},
      {1, {nan, nan, nan}, {{4, 5, 5}, {0, 5, 6}}}};
  Case c;
  c.offsets.push_back(0);
  for (const Track& t : tracks) {
    for (const Obs& o : t.obs) { c.image.push_back(o.im); c.xy.push_back(o.x); c.xy.push_back(o.y); }
    c.offsets.push_back((long)c.image.size());
    c.status.push_back((uint8_t)t.status);
    c.xyz.insert(c.xyz.end(), t.X, t.X + 3);
  }
  c.posed = {1, 0, 0, 0, 0, 1};
  c.group();
  return c;
}

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  std::vector<int> n_corr;
  std::vector<long> counts;
  Case h = hand();
  EXPECT(run(h, 4, &n_corr, &counts) == LOFTR_OK);
  EXPECT((n_corr == std::vector<int>{0, 4, 3, 5, 0, 0}));
  EXPECT((counts == std::vector<long>{9, 2, 0, 4, 3, 12, 5, 0}));
  EXPECT(run(h, 5, &n_corr, &counts) == LOFTR_OK && counts[0] == 5 && counts[1] == 1);
  EXPECT(run(h, 6, &n_corr, &counts) == LOFTR_OK && counts[0] == 0 && counts[1] == 0);
  EXPECT(run(h, 3, nullptr, nullptr) == LOFTR_ERR_BAD_ARG);
  Case all = hand(), none = hand();
  all.posed.assign(6, 1);
  none.posed.assign(6, 0);
  EXPECT(run(all, 4, &n_corr, &counts) == LOFTR_OK && counts[0] == 0 && counts[3] == 0);
  EXPECT(run(none, 4, &n_corr, &counts) == LOFTR_OK && counts[3] == 6);
  Case t0, n0, e0;
  t0.offsets = {0}; t0.posed = {0, 1, 0}; t0.group();
  n0.offsets = {0, 0, 0}; n0.xyz.assign(6, 1.f); n0.status = {0, 0}; n0.posed = {0, 1, 0}; n0.group();
  e0.offsets = {0}; e0.group();
  EXPECT(run(t0, 4, &n_corr, &counts) == LOFTR_OK && counts[3] == 2 && counts[1] == 0);
  EXPECT(run(n0, 4, &n_corr, &counts) == LOFTR_OK && counts[3] == 2 && counts[1] == 0);
  EXPECT(run(e0, 4, &n_corr, &counts) == LOFTR_OK && counts[3] == 0);
  // the error bits
  Case b = hand();
  b.image[7] = 6;
  EXPECT(run(b, 4, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[2] == 1 && counts[0] == 0);
  b = hand(); b.image[7] = -1;
  EXPECT(run(b, 4, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[2] == 1);
  b = hand(); b.offsets[2] = 3;
  EXPECT(run(b, 4, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[2] == 2);
  b = hand(); b.offsets.back() = 99;
  EXPECT(run(b, 4, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[2] == 2);
  b = hand(); std::swap(b.cam_obs[0], b.cam_obs[1]);
  EXPECT(run(b, 4, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[2] == 4);
  b = hand(); b.cam_obs[3] = 999;
  EXPECT(run(b, 4, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[2] == 4);
  b = hand(); b.cam_obs[3] = -2;
  EXPECT(run(b, 4, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[2] == 4);
  b = hand(); b.cam_offsets[2] = 9;
  EXPECT(run(b, 4, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[2] == 4);
  b = hand(); b.cam_offsets.back() = 5;
  EXPECT(run(b, 4, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[2] == 4);
  printf("register_host_driver: all cases passed\n");
  return 0;
}
