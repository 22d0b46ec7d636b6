// Stand-alone driver of the host routine of track merging (csrc/merge.hip) for a sanitizer pass on the CPU: hand-written cases in the
// manner of tests/_merge_cases.py (two points on one ray that disagree, two rows that share an image, a meeting found from one side only,
// a chain A - B - C, equal scores among three rows, a partner with a NaN point, a row with w = 0, a masked observation in an unposed
// image, a nearer free keypoint, an image without keypoints, T = 0, K = 0, n = 0, the four error bits).  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/merge_host_driver.cpp loftr_amd/csrc/merge.hip -o driver
//   ./driver
// It uses no GPU.  Inputs and outputs live in exactly-sized heap blocks, so that a read or write past an end is caught.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>
#include "../include/loftr_hip.h"

static const int kGh = 240, kGw = 320;                                    // 640 x 480 at 2 px cells
static const float kInv = 0.5f;
static const int kImages = 10, kUnposed = 8;
static const double kCentre[kImages][2] = {{0, 0}, {1, 0}, {0.5, 0}, {0.5, 0.5}, {0, 0.5}, {1, 0.5}, {-0.5, 0}, {-0.5, 0.5}, {0.5, -0.5}, {0, -0.5}};

struct Kp { int image; float x, y; int row; };
struct Case {
  std::vector<long> offsets{0};
  std::vector<int> image;
  std::vector<float> xy, xyz;
  std::vector<uint8_t> mask, status, posed;
  std::vector<double> K, T;
  std::vector<Kp> kps;
  std::map<std::string, int> id;
  // the pool, ordered by image, then by cell
  std::vector<long> kp_offsets;
  std::vector<float> keypoints;
  std::vector<int> kp_cell, kp_row;
  void cameras() {                                                        // identity rotations, f = 500, principal point (320, 240)
    for (int i = 0; i < kImages; ++i) {
      const double k[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1}, t[16] = {1, 0, 0, -kCentre[i][0], 0, 1, 0, -kCentre[i][1], 0, 0, 1, 0, 0, 0, 0, 1};
      K.insert(K.end(), k, k + 9);
      T.insert(T.end(), t, t + 16);
      posed.push_back(i != kUnposed);
    }
  }
  // a row at X that visits `images` (ascending); its keypoints sit at the projections, moved by (dx, dy) in image `moved`
  int row(const char* name, double x, double y, double z, std::vector<int> images, int st = 0, int moved = -1, float dx = 0, float dy = 0,
          int masked_out = -1, bool nan_point = false) {
    const int r = (int)status.size();
    for (int i : images) {
      const float u = (float)(500 * (x - kCentre[i][0]) / z + 320) + (i == moved ? dx : 0), v = (float)(500 * (y - kCentre[i][1]) / z + 240) + (i == moved ? dy : 0);
      image.push_back(i);
      xy.push_back(u); xy.push_back(v);
      mask.push_back(i != masked_out);
      kps.push_back({i, u, v, r});
    }
    offsets.push_back((long)image.size());
    status.push_back((uint8_t)st);
    const float X[3] = {nan_point ? NAN : (float)x, (float)y, (float)z};
    xyz.insert(xyz.end(), X, X + 3);
    return id[name] = r;
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
};

template <class T> static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

struct Result { std::vector<int> row_into, kp_row_new; std::vector<float> r2; std::vector<long> counts; };

static int run(Case& c, int reach, Result* out) {
  const long T = (long)c.offsets.size() - 1, N = (long)c.image.size(), K = (long)c.kp_row.size();
  const int n = (int)c.posed.size();
  Result r{std::vector<int>(T, -7), std::vector<int>(K, -7), std::vector<float>(T, -7.f), std::vector<long>(8, -7)};
  const int st = loftr_merge_tracks_host(c.offsets.data(), T, ptr(c.image), ptr(c.xy), ptr(c.mask), N, ptr(c.xyz), ptr(c.status), c.kp_offsets.data(),
                                         ptr(c.keypoints), ptr(c.kp_cell), ptr(c.kp_row), K, ptr(c.K), ptr(c.T), ptr(c.posed), n, kInv, kGh, kGw, 4.0,
                                         reach, ptr(r.row_into), ptr(r.r2), ptr(r.kp_row_new), r.counts.data());
  if (out) *out = r;
  return st;
}

// the cases of tests/_merge_cases.py hand(); nobody visits image 9
static Case hand() {
  Case c;
  c.cameras();
  c.row("ray_near", -1.0, -0.9, 4, {1, 2});
  c.row("ray_far", -1.5, -1.35, 6, {0, 3});
  c.row("shared_a", -0.4, -0.9, 4, {0, 2});
  c.row("shared_b", -0.4, -0.9, 4, {1, 2}, 0, 2, 3.0f, 0);
  c.row("one_sided_in", -319.0 / 125, 0.3, 4, {0, 4});
  c.row("one_sided_out", -321.0 / 125, 0.3, 4, {6, 7});
  c.row("chain_a", 0.2 - 0.016, -0.9, 4, {0});
  c.row("chain_b", 0.2, -0.9, 4, {1});
  c.row("chain_c", 0.2 + 0.004, -0.9, 4, {2});
  c.row("equal_a", 0.8, -0.9, 4, {0}, 0, 0, 3.0f, 0);
  c.row("equal_b", 0.8 + 0.004, -0.9, 4, {1});
  c.row("equal_c", 0.8 + 0.004, -0.9, 4, {1}, 0, 1, 0, 2.2f);
  c.row("nan_meets", -1.0, -0.3, 4, {0});
  c.row("nan_point", -1.0, -0.3, 4, {1}, 0, -1, 0, 0, -1, true);
  c.row("weight_a", -0.4, -0.3, 4, {0});
  c.row("weight_0", -0.4, -0.3, 4, {1}, 0, -1, 0, 0, 1);
  c.row("unposed_a", 0.2, -0.3, 4, {0, kUnposed});
  c.row("unposed_b", 0.2, -0.3, 4, {1});
  c.row("free_a", 0.8, -0.3, 4, {0});
  c.row("free_b", 0.8, -0.3, 4, {1}, 0, 1, 2.5f, 0);
  c.kps.push_back({1, (float)(125 * (0.8 - 1) + 320) + 0.5f, (float)(125 * -0.3 + 240), -1});
  c.row("pointless", -1.0, 0.9, 4, {0}, 2);
  c.row("pointless_meets", -1.0, 0.9, 4, {1});
  c.pool();
  return c;
}

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  Result r;
  Case h = hand();
  for (int reach : {2, 8}) {
    EXPECT(run(h, reach, &r) == LOFTR_OK);
    for (const auto& kv : h.id) {
      const std::string& name = kv.first;
      const int want = name == "one_sided_out" ? h.id["one_sided_in"] : name == "chain_c" ? h.id["chain_b"] : name == "equal_b" ? h.id["equal_a"]
                     : name == "free_b" ? h.id["free_a"] : kv.second;
      if (r.row_into[kv.second] != want) { fprintf(stderr, "%s: into %d, expected %d\n", name.c_str(), r.row_into[kv.second], want); return 1; }
    }
    EXPECT(r.counts[0] == 4 && r.counts[1] == 0 && r.counts[4] == 20 && r.counts[5] == 18 && r.counts[6] == 13 && r.counts[7] == 5);
    EXPECT(fabsf(r.r2[h.id["free_a"]] - 6.25f) < 1e-3f && r.r2[h.id["free_a"]] == r.r2[h.id["free_b"]] && isnan(r.r2[h.id["chain_a"]]));
    for (size_t k = 0; k < h.kp_row.size(); ++k) EXPECT(r.kp_row_new[k] == (h.kp_row[k] < 0 ? h.kp_row[k] : r.row_into[h.kp_row[k]]));
  }
  EXPECT(run(h, 0, &r) == LOFTR_OK && r.counts[1] == 0);
  for (int reach : {-1, 9}) EXPECT(run(h, reach, nullptr) == LOFTR_ERR_BAD_ARG);
  // T = 0, K = 0, n = 0
  Case t0 = hand();
  t0.offsets = {0}; t0.image.clear(); t0.xy.clear(); t0.mask.clear(); t0.xyz.clear(); t0.status.clear();
  for (Kp& k : t0.kps) k.row = -1;
  t0.pool();
  EXPECT(run(t0, 2, &r) == LOFTR_OK && r.counts[0] == 0 && r.counts[2] == 0 && r.counts[7] == 0);
  Case k0 = hand();
  k0.kps.clear(); k0.pool();
  EXPECT(run(k0, 2, &r) == LOFTR_OK && r.counts[0] == 0 && r.counts[2] == 20 && r.counts[4] == 0);
  Case n0;
  n0.pool();
  EXPECT(run(n0, 2, &r) == LOFTR_OK && r.counts[2] == 0);
  // the error bits
  Case b = hand();
  b.image[b.offsets[3] - 1] = kImages;
  EXPECT(run(b, 2, &r) == LOFTR_ERR_BAD_ARG && r.counts[1] == 1);
  b = hand(); b.offsets.back() -= 1;
  EXPECT(run(b, 2, &r) == LOFTR_ERR_BAD_ARG && r.counts[1] == 2);
  b = hand(); b.kp_offsets.back() -= 1;
  EXPECT(run(b, 2, &r) == LOFTR_ERR_BAD_ARG && r.counts[1] == 2);
  b = hand(); std::swap(b.image[0], b.image[1]);
  EXPECT(run(b, 2, &r) == LOFTR_ERR_BAD_ARG && r.counts[1] == 4);
  b = hand(); b.kp_row[0] = (int)b.status.size();
  EXPECT(run(b, 2, &r) == LOFTR_ERR_BAD_ARG && r.counts[1] == 8);
  b = hand(); b.kp_row[0] = -2;
  EXPECT(run(b, 2, &r) == LOFTR_ERR_BAD_ARG && r.counts[1] == 8);
  printf("merge_host_driver: all cases passed\n");
  return 0;
}
