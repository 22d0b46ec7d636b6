// Stand-alone driver of the host routine of track completion (csrc/complete.hip) for a sanitizer pass on the CPU: hand-written cases in
// the manner of tests/_completion_cases.py (a point behind a camera, outside the grid, in the last cell with reach 0 / 1 / 2, an image
// already in the row, an unposed image, fx = 0, a NaN point, a row without a point, a blocked and a taken keypoint, two free keypoints,
// an exact tie, an image without keypoints, T = 0, K = 0, n = 0, the four error bits).  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/complete_host_driver.cpp loftr_amd/csrc/complete.hip -o driver
//   ./driver
// It uses no GPU.  Inputs and outputs live in exactly-sized heap blocks, so that a read or write past an end is caught.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../include/loftr_hip.h"

static const int kGh = 240, kGw = 320;                                    // 640 x 480 at 2 px cells
static const float kInv = 0.5f;

struct Kp { int image; float x, y; int row; };
struct Case {
  std::vector<long> offsets{0};
  std::vector<int> image;
  std::vector<float> xyz;
  std::vector<uint8_t> status, posed;
  std::vector<double> K, T;
  std::vector<Kp> kps;
  // the pool, ordered by image, then by cell
  std::vector<long> kp_offsets;
  std::vector<float> keypoints;
  std::vector<int> kp_cell, kp_row;
  void camera(double f, double cx, double cy, double cz, bool posed_) {  // identity rotation, principal point (320, 240)
    const double k[9] = {f, 0, 320, 0, f, 240, 0, 0, 1}, t[16] = {1, 0, 0, -cx, 0, 1, 0, -cy, 0, 0, 1, -cz, 0, 0, 0, 1};
    K.insert(K.end(), k, k + 9);
    T.insert(T.end(), t, t + 16);
    posed.push_back(posed_);
  }
  int row(int st, float x, float y, float z, std::vector<int> images) {
    image.insert(image.end(), images.begin(), images.end());
    offsets.push_back((long)image.size());
    status.push_back((uint8_t)st);
    const float X[3] = {x, y, z};
    xyz.insert(xyz.end(), X, X + 3);
    return (int)status.size() - 1;
  }
  static int cell(const Kp& k) { return (int)floorf(k.y * kInv) * kGw + (int)floorf(k.x * kInv); }
  void pool() {
    std::stable_sort(kps.begin(), kps.end(), [](const Kp& a, const Kp& b) { return a.image != b.image ? a.image < b.image : cell(a) < cell(b); });
    kp_offsets.assign(posed.size() + 1, 0);
    keypoints.clear(); kp_cell.clear(); kp_row.clear();
    for (const Kp& k : kps) {
      kp_offsets[k.image + 1] += 1;
      keypoints.push_back(k.x); keypoints.push_back(k.y);
      kp_cell.push_back(cell(k));
      kp_row.push_back(k.row);
    }
    for (size_t i = 0; i < posed.size(); ++i) kp_offsets[i + 1] += kp_offsets[i];
  }
  int find(float x, float y) const {
    for (size_t k = 0; k < kp_row.size(); ++k) if (keypoints[2 * k] == x && keypoints[2 * k + 1] == y) return (int)k;
    return -1;
  }
};

template <class T> static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

static int run(Case& c, int reach, std::vector<int>* rows, std::vector<float>* r2, std::vector<long>* counts_out) {
  const long T = (long)c.offsets.size() - 1, N = (long)c.image.size(), K = (long)c.kp_row.size();
  const int n = (int)c.posed.size();
  std::vector<int> kp_row_new(K, -7);
  std::vector<float> link_r2(K, -7.f);
  std::vector<long> counts(8, -7);
  const int st = loftr_complete_tracks_host(c.offsets.data(), T, ptr(c.image), N, ptr(c.xyz), ptr(c.status), c.kp_offsets.data(), ptr(c.keypoints),
                                            ptr(c.kp_cell), ptr(c.kp_row), K, ptr(c.K), ptr(c.T), ptr(c.posed), n, kInv, kGh, kGw, 4.0, reach,
                                            ptr(kp_row_new), ptr(link_r2), counts.data());
  if (rows) *rows = kp_row_new;
  if (r2) *r2 = link_r2;
  if (counts_out) *counts_out = counts;
  return st;
}

// images: 0 A (0,0,0), 1 B (1,0,0), 2 behind the points, 3 D (0.5,0,0), 4 unposed, 5 fx = 0, 6 without keypoints, 7 H (1,0.5,0).
// The projection of (x, y, 4) in a camera at (cx, cy, 0) is (125 (x - cx) + 320, 125 (y - cy) + 240).
static Case hand() {
  Case c;
  c.camera(500, 0, 0, 0, true); c.camera(500, 1, 0, 0, true); c.camera(500, 0, 0, 10, true); c.camera(500, 0.5, 0, 0, true);
  c.camera(500, 0.5, 0.5, 0, false); c.camera(0, 0.5, -0.5, 0, true); c.camera(500, 0, 0.5, 0, true); c.camera(500, 1, 0.5, 0, true);
  auto all_but = [](std::vector<int> targets) {
    std::vector<int> v;
    for (int i = 0; i < 8; ++i) if (std::find(targets.begin(), targets.end(), i) == targets.end()) v.push_back(i);
    return v;
  };
  const int owner_ok = c.row(0, -1.2f, 1.5f, 4, all_but({})), owner_pointless = c.row(2, -0.9f, 1.5f, 4, all_but({}));
  c.row(0, -1.0f, -0.6f, 4, all_but({2}));                                                   // 2 behind
  c.row(0, 4.0f, -0.6f, 4, all_but({3}));                                                    // 3 outside the grid
  c.row(0, 0.5f + 318.1f / 125, 238.1f / 125, 4, all_but({3}));                              // 4 the last cell: (638.1, 478.1)
  c.kps.push_back({3, 635.9f, 478.1f, -1}); c.kps.push_back({3, 636.1f, 476.1f, -1}); c.kps.push_back({3, 1.0f, 479.0f, -1});
  c.row(0, -0.7f, -0.6f, 4, all_but({}));                                                    // 5 visits D already
  c.kps.push_back({3, 170.5f, 165.0f, -1});
  c.row(0, -0.4f, -0.6f, 4, all_but({4}));                                                   // 6 unposed
  c.kps.push_back({4, 208.0f, 102.5f, -1});
  c.row(0, -0.1f, -0.6f, 4, all_but({5}));                                                   // 7 fx = 0
  c.kps.push_back({5, 300.0f, 200.0f, -1});
  c.row(0, NAN, -0.3f, 4, all_but({3}));                                                     // 8 NaN
  c.row(3, -1.0f, -0.3f, 4, all_but({3}));                                                   // 9 no point
  c.kps.push_back({3, 133.0f, 202.5f, -1});
  c.row(0, -0.7f, -0.3f, 4, all_but({3}));                                                   // 10 blocked: (170, 202.5)
  c.kps.push_back({3, 171.0f, 202.5f, owner_ok});
  c.row(0, -0.4f, -0.3f, 4, all_but({3}));                                                   // 11 takes: (207.5, 202.5)
  c.kps.push_back({3, 206.5f, 202.5f, owner_pointless});
  c.row(0, -0.1f, -0.3f, 4, all_but({3}));                                                   // 12 two free: (245, 202.5)
  c.kps.push_back({3, 245.8f, 202.75f, -1}); c.kps.push_back({3, 242.5f, 202.75f, -1});
  c.row(0, 0.2f, -0.3f, 4, all_but({7})); c.row(0, 0.2f, -0.3f, 4, all_but({7}));            // 13, 14 the tie: (220, 140) in H
  c.kps.push_back({7, 220.5f, 140.25f, -1});
  c.row(0, 0.8f, -0.3f, 4, all_but({6}));                                                    // 15 an image without keypoints
  c.pool();
  return c;
}

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  std::vector<int> rows;
  std::vector<float> r2;
  std::vector<long> counts;
  Case h = hand();
  const int corner2 = h.find(635.9f, 478.1f), corner1 = h.find(636.1f, 476.1f), taken = h.find(206.5f, 202.5f), blocked = h.find(171.0f, 202.5f);
  const int near_ = h.find(245.8f, 202.75f), far_ = h.find(242.5f, 202.75f), tie = h.find(220.5f, 140.25f);
  EXPECT(corner2 >= 0 && corner1 >= 0 && taken >= 0 && blocked >= 0 && near_ >= 0 && far_ >= 0 && tie >= 0);
  for (int reach = 0; reach <= 2; ++reach) {
    EXPECT(run(h, reach, &rows, &r2, &counts) == LOFTR_OK);
    EXPECT(rows[corner2] == (reach == 2 ? 4 : -1) && rows[corner1] == (reach == 1 ? 4 : -1));
    EXPECT(rows[taken] == 11 && rows[blocked] == 0 && rows[near_] == 12 && rows[far_] == -1 && rows[tie] == 13);
    EXPECT(!isnan(r2[taken]) && isnan(r2[blocked]) && isnan(r2[far_]) && fabsf(r2[tie] - 0.3125f) < 1e-4f);
    EXPECT((counts == std::vector<long>{reach == 0 ? 3 : 4, 0, 13, 9, 7, reach == 0 ? 4 : 5, 1, 1}));
  }
  for (int reach : {-1, 9}) EXPECT(run(h, reach, nullptr, nullptr, nullptr) == LOFTR_ERR_BAD_ARG);
  EXPECT(run(h, 8, &rows, &r2, &counts) == LOFTR_OK && counts[0] == 4);
  // T = 0, K = 0, n = 0
  Case t0 = hand();
  t0.offsets = {0}; t0.image.clear(); t0.xyz.clear(); t0.status.clear();
  for (Kp& k : t0.kps) k.row = -1;
  t0.pool();
  EXPECT(run(t0, 2, &rows, &r2, &counts) == LOFTR_OK && counts[0] == 0 && counts[2] == 0);
  Case k0 = hand();
  k0.kps.clear(); k0.pool();
  EXPECT(run(k0, 2, &rows, &r2, &counts) == LOFTR_OK && counts[0] == 0 && counts[2] == 13 && counts[3] == 9);
  Case n0;
  n0.pool();
  EXPECT(run(n0, 2, &rows, &r2, &counts) == LOFTR_OK && counts[2] == 0);
  // the error bits
  Case b = hand();
  b.image[b.offsets[3] - 1] = 8;
  EXPECT(run(b, 2, nullptr, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[1] == 1);
  b = hand(); b.offsets.back() -= 1;
  EXPECT(run(b, 2, nullptr, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[1] == 2);
  b = hand(); b.kp_offsets[1] = 1;
  EXPECT(run(b, 2, nullptr, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[1] == 2);
  b = hand(); std::swap(b.image[b.offsets[5]], b.image[b.offsets[5] + 1]);
  EXPECT(run(b, 2, nullptr, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[1] == 4);
  b = hand(); b.kp_row[0] = (int)b.status.size();
  EXPECT(run(b, 2, nullptr, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[1] == 8);
  b = hand(); b.kp_row[0] = -2;
  EXPECT(run(b, 2, nullptr, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[1] == 8);
  printf("complete_host_driver: all cases passed\n");
  return 0;
}
