// Stand-alone driver of the two host routines of the radial camera model (csrc/bundle.hip, csrc/undistort.hip) for a
// sanitizer pass on the CPU: a hand-written problem (a camera with fx = 0, one without observations, a NaN point, a masked observation, a
// mixed radial mask inside a group, a start value that is not finite, fixed-pose members that carry the lens), a start whose first trial
// leaves the radial bounds, a group whose members all keep their pose, every pose known, bad groupings, the empty problems, and a small
// undistortion batch with failing points and a bad image id.  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/bundle_radial_host_driver.cpp loftr_amd/csrc/bundle.hip loftr_amd/csrc/undistort.hip -o driver
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
  std::vector<uint8_t> mask, fixed, refine, refine_radial;
  std::vector<double> K, K_true, T, k_true, k_start;
  std::vector<long> cam_offsets, group_offsets;
  std::vector<int> cam_obs, body, cam_group, group_cams;
  int n() const { return (int)fixed.size(); }
  int G() const { return (int)group_offsets.size() - 1; }
  // a camera of body `b` at centre (cx, cy, 0) looking along +z; f_true and k make the observations, f and k = 0 is what the adjustment starts from
  void camera(int b, double cx, double cy, double f_true, double f, double k, bool fix, bool ref) {
    const double Kt[9] = {f_true, 0, 320, 0, f_true, 240, 0, 0, 1}, Kg[9] = {f, 0, 320, 0, f, 240, 0, 0, 1};
    const double Tc[16] = {1, 0, 0, -cx, 0, 1, 0, -cy, 0, 0, 1, 0, 0, 0, 0, 1};
    K_true.insert(K_true.end(), Kt, Kt + 9);
    K.insert(K.end(), Kg, Kg + 9);
    T.insert(T.end(), Tc, Tc + 16);
    fixed.push_back(fix);
    refine.push_back(ref);
    refine_radial.push_back(ref);
    k_true.push_back(k);
    k_start.push_back(0.0);
    body.push_back(b);
  }
  // a point seen by the cameras listed through their true lens; the start is moved by (dx, 0, 0)
  void track(double X, double Y, double Z, const std::vector<int>& cams, double dx) {
    for (int c : cams) {
      const double* k = &K_true[9 * c];
      const double* t = &T[16 * c];
      const double a = (X + t[3]) / (Z + t[11]), b = (Y + t[7]) / (Z + t[11]), m = 1.0 + k_true[c] * (a * a + b * b);
      image.push_back(c);
      xy.push_back((float)(k[0] * (a * m) + k[2]));
      xy.push_back((float)(k[4] * (b * m) + k[5]));
      mask.push_back(1);
    }
    offsets.push_back((long)image.size());
    xyz.push_back((float)(X + dx)); xyz.push_back((float)Y); xyz.push_back((float)Z);
  }
  // the observations grouped by image, the images grouped by body (bodies relabelled in the order of their first images)
  void group() {
    cam_obs.resize(image.size());
    std::iota(cam_obs.begin(), cam_obs.end(), 0);
    std::stable_sort(cam_obs.begin(), cam_obs.end(), [&](int a, int b) { return image[a] < image[b]; });
    cam_offsets.assign(n() + 1, 0);
    for (int im : image) cam_offsets[im + 1] += 1;
    for (int i = 0; i < n(); ++i) cam_offsets[i + 1] += cam_offsets[i];
    std::vector<int> seen;
    cam_group.assign(n(), 0);
    for (int i = 0; i < n(); ++i) {
      auto at = std::find(seen.begin(), seen.end(), body[i]);
      cam_group[i] = (int)(at - seen.begin());
      if (at == seen.end()) seen.push_back(body[i]);
    }
    group_cams.resize(n());
    std::iota(group_cams.begin(), group_cams.end(), 0);
    std::stable_sort(group_cams.begin(), group_cams.end(), [&](int a, int b) { return cam_group[a] < cam_group[b]; });
    group_offsets.assign(seen.size() + 1, 0);
    for (int g : cam_group) group_offsets[g + 1] += 1;
    for (size_t g = 0; g < seen.size(); ++g) group_offsets[g + 1] += group_offsets[g];
  }
};

struct Result {
  int status;
  std::vector<double> T, K, k;
  std::vector<float> xyz;
  std::vector<uint8_t> obs_active, cam_free, point_active, cam_focal, group_focal, cam_radial, group_radial;
  std::vector<long> counts;
  double real(int i) const { double d; memcpy(&d, &counts[i], 8); return d; }
};

template <class T> static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

static Result run(Problem& p, int max_iters, int min_focal_obs, double lo, double hi) {
  const long T = (long)p.offsets.size() - 1, N = (long)p.image.size();
  const int n = p.n(), G = p.G();
  Result r;
  r.T.assign(16 * n, -1.0); r.K.assign(9 * n, -1.0); r.k.assign(n, -9.0); r.xyz.assign(3 * T, -1.f);
  r.obs_active.assign(N, 9); r.cam_free.assign(n, 9); r.point_active.assign(T, 9); r.cam_focal.assign(n, 9); r.group_focal.assign(G, 9);
  r.cam_radial.assign(n, 9); r.group_radial.assign(G, 9);
  r.counts.assign(16, 7);
  r.status = loftr_bundle_adjust_radial_host(p.offsets.data(), T, ptr(p.image), ptr(p.xy), ptr(p.mask), N, ptr(p.xyz), ptr(p.K), ptr(p.T),
                                             ptr(p.fixed), ptr(p.refine), n, p.cam_offsets.data(), ptr(p.cam_obs), ptr(p.cam_group),
                                             p.group_offsets.data(), ptr(p.group_cams), G, ptr(p.k_start), ptr(p.refine_radial), 0.0, max_iters,
                                             30, 1e-2, 1e-9, min_focal_obs, 0.5, 2.0, lo, hi, ptr(r.T), ptr(r.xyz), ptr(r.obs_active),
                                             ptr(r.cam_free), ptr(r.point_active), ptr(r.K), ptr(r.cam_focal), ptr(r.group_focal), ptr(r.k),
                                             ptr(r.cam_radial), ptr(r.group_radial), r.counts.data());
  return r;
}

// cameras 0 (body 7) and 1 (body 3) keep their pose, `free_cams` further ones alternate between the two bodies; body 7's focal is off by
// the factor `off7` and its lens is k7, body 3's off3 and k3; the last camera (body 11) has the true K, no lens and does not refine: every
// camera here looks along +z from the plane z = 0, so one common factor on all focals and all depths would change no pixel, and this camera
// is what holds it.  A 6 x 6 grid of points at two depths seen by all, wide enough (r up to 0.6) for the lens to show
static Problem scene(int free_cams, double off7, double off3, double k7, double k3, double dx) {
  Problem p;
  p.camera(7, -1.0, 0.0, 500.0, 500.0 * off7, k7, true, true);
  p.camera(3, 1.0, 0.1, 520.0, 520.0 * off3, k3, true, true);
  for (int i = 0; i < free_cams; ++i) {
    const double f = 480.0 + 15.0 * i;
    p.camera(i % 2 ? 3 : 7, -0.5 + 0.5 * i, 0.25 * (i % 3) - 0.25, f, f * (i % 2 ? off3 : off7), i % 2 ? k3 : k7, false, true);
  }
  p.camera(11, 0.2, -0.4, 510.0, 510.0, 0.0, false, false);
  std::vector<int> all(p.n());
  std::iota(all.begin(), all.end(), 0);
  for (int z = 0; z < 2; ++z)
    for (int x = 0; x < 6; ++x)
      for (int y = 0; y < 6; ++y) p.track(-2.0 + 0.8 * x, -1.5 + 0.6 * y, 4.0 + 3.0 * z + 0.1 * x, all, dx);
  return p;
}

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b, size_t at, size_t len) {
  return memcmp(a.data() + at, b.data() + at, 8 * len) == 0;
}

int main() {
  // ---- the hand-written problem: cameras 0, 1 keep their pose and carry; 2, 3, 4 free (4, of body 7, left out of the RADIAL mask); 5 the
  // camera that holds the scale; 6 (body 9) with fx = 0; 7 (body 9) without an observation; 8 (body 3) with a start value that is NaN
  Problem h = scene(3, 1.06, 0.95, -0.10, 0.06, 0.02);
  h.camera(9, 0.3, 0.3, 500.0, 500.0, 0.0, false, true);               // 6
  h.K[9 * 6] = 0.0;
  h.camera(9, 2.0, 2.0, 500.0, 500.0, 0.0, false, true);               // 7
  h.camera(3, 0.6, -0.2, 505.0, 505.0 * 0.95, 0.06, false, true);      // 8
  h.k_start[8] = NAN;
  h.refine_radial[4] = 0;
  h.k_start[4] = -0.10;                                                 // (its lens is known; its focal still refines with its body)
  const long T0 = (long)h.offsets.size() - 1;
  h.track(0.1, 0.1, 5.0, {0, 1, 6}, 0.0);                               // T0: its observation in camera 6 cannot be active
  h.track(0.2, -0.1, 5.0, {0, 1, 2, 8}, 0.0);                           // T0 + 1: a NaN point; camera 8 is not valid either
  h.xyz[3 * (T0 + 1) + 1] = NAN;
  h.track(-0.2, 0.2, 6.0, {0, 2, 3, 8}, 0.0);                           // T0 + 2: the observation in camera 0 is masked out
  h.mask[h.offsets[T0 + 2]] = 0;
  h.group();
  EXPECT((h.cam_group == std::vector<int>{0, 1, 0, 1, 0, 2, 3, 3, 1}) && h.G() == 4);
  Result r = run(h, 40, 1, -1.0, 1.0);
  EXPECT(r.status == LOFTR_OK && r.counts[0] == 0 && r.counts[1] == 0);
  EXPECT((r.cam_free == std::vector<uint8_t>{0, 0, 1, 1, 1, 1, 0, 0, 0}) && (r.cam_focal == std::vector<uint8_t>{1, 1, 1, 1, 1, 0, 0, 0, 0}));
  EXPECT((r.cam_radial == std::vector<uint8_t>{1, 1, 1, 1, 0, 0, 0, 0, 0}) && (r.group_radial == std::vector<uint8_t>{1, 1, 0, 0}));
  EXPECT((r.group_focal == std::vector<uint8_t>{1, 1, 0, 0}) && r.counts[13] == 5 && r.counts[14] == 2 && r.counts[15] == 4);
  EXPECT(!r.obs_active[h.offsets[T0] + 2] && !r.point_active[T0 + 1] && !r.obs_active[h.offsets[T0 + 2]] && !r.obs_active[h.offsets[T0 + 2] + 3]);
  for (int i : {4, 5, 6, 7, 8}) EXPECT(same_bits(r.k, h.k_start, i, 1));                // the input's bits, the NaN's too
  for (int i : {0, 2}) EXPECT(fabs(r.k[i] + 0.10) < 0.01);
  for (int i : {1, 3}) EXPECT(fabs(r.k[i] - 0.06) < 0.01);
  EXPECT(r.k[0] == r.k[2] && r.k[1] == r.k[3]);                                          // one step per body on equal starts
  for (int i : {0, 1, 6, 7, 8}) EXPECT(same_bits(r.T, h.T, 16 * i, 16));
  for (int i : {0, 1, 2, 3, 4}) EXPECT(fabs(r.K[9 * i] / h.K_true[9 * i] - 1.0) < 0.01);
  EXPECT(r.real(9) < 1e-3 * r.real(8));
  // min_focal_obs above every group: nobody refines, every K and k comes back
  r = run(h, 30, 100000, -1.0, 1.0);
  EXPECT(r.status == LOFTR_OK && r.counts[13] == 0 && r.counts[15] == 0 && same_bits(r.K, h.K, 0, h.K.size()) && same_bits(r.k, h.k_start, 0, 9));

  // ---- bounds: the lenses are -0.10 and 0.06, [-0.01, 0.01] rejects the first trial; nothing moves in one trial, and no result leaves
  Problem b = scene(3, 1.04, 0.97, -0.10, 0.06, 0.02);
  b.group();
  r = run(b, 1, 1, -0.01, 0.01);
  EXPECT(r.status == LOFTR_OK && r.counts[2] == 1 && r.counts[3] == 0 && r.counts[0] == 1 && r.real(12) == 10.0 * 1e-4);
  EXPECT(same_bits(r.K, b.K, 0, b.K.size()) && same_bits(r.k, b.k_start, 0, b.k_start.size()) && r.real(9) == r.real(8));
  r = run(b, 40, 1, -0.01, 0.01);
  EXPECT(r.status == LOFTR_OK && r.counts[3] < r.counts[2]);
  for (int i = 0; i < 6; ++i) EXPECT(r.k[i] >= -0.01 && r.k[i] <= 0.01);
  r = run(b, 40, 1, -1.0, 1.0);
  EXPECT(r.status == LOFTR_OK && r.counts[0] == 0 && r.counts[15] == 5 && fabs(r.k[0] + 0.10) < 0.005 && fabs(r.k[1] - 0.06) < 0.005);
  EXPECT(run(b, 40, 1, NAN, 1.0).status == LOFTR_ERR_BAD_ARG && run(b, 40, 1, -1.0, INFINITY).status == LOFTR_ERR_BAD_ARG);
  EXPECT(run(b, 40, 1, 0.5, -0.5).status == LOFTR_ERR_BAD_ARG && run(b, 40, 0, -1.0, 1.0).status == LOFTR_ERR_BAD_ARG);

  // ---- a group whose members all keep their pose (body 3), and every pose known: the lenses move, the poses come back bit for bit
  Problem a = scene(3, 1.05, 0.93, -0.08, 0.05, 0.02);
  a.fixed[3] = 1;
  a.group();
  r = run(a, 40, 1, -1.0, 1.0);
  EXPECT(r.status == LOFTR_OK && (r.cam_free == std::vector<uint8_t>{0, 0, 1, 0, 1, 1}) && (r.cam_radial == std::vector<uint8_t>{1, 1, 1, 1, 1, 0}));
  EXPECT(same_bits(r.T, a.T, 16 * 1, 16) && same_bits(r.T, a.T, 16 * 3, 16) && fabs(r.k[1] - 0.05) < 0.005 && fabs(r.k[3] - 0.05) < 0.005);
  std::fill(a.fixed.begin(), a.fixed.end(), 1);
  r = run(a, 40, 1, -1.0, 1.0);
  EXPECT(r.status == LOFTR_OK && r.counts[7] == 0 && r.counts[15] == 5 && r.counts[14] == 2 && r.counts[4] > 0 && same_bits(r.T, a.T, 0, a.T.size()));
  EXPECT(fabs(r.k[0] + 0.08) < 0.005 && fabs(r.k[1] - 0.05) < 0.005);

  // ---- bad groupings are answered before anything is read through them
  Problem g = scene(3, 1.05, 0.95, -0.05, 0.05, 0.0);
  g.group();
  { Problem w = g; w.cam_group[2] = 1; EXPECT(run(w, 5, 1, -1.0, 1.0).status == LOFTR_ERR_BAD_ARG); }
  { Problem w = g; w.cam_group[2] = 3; EXPECT(run(w, 5, 1, -1.0, 1.0).status == LOFTR_ERR_BAD_ARG); }
  { Problem w = g; std::swap(w.group_cams[0], w.group_cams[1]); EXPECT(run(w, 5, 1, -1.0, 1.0).status == LOFTR_ERR_BAD_ARG); }
  { Problem w = g; w.group_cams[4] = 6; EXPECT(run(w, 5, 1, -1.0, 1.0).status == LOFTR_ERR_BAD_ARG); }
  { Problem w = g; w.group_cams[4] = -3; EXPECT(run(w, 5, 1, -1.0, 1.0).status == LOFTR_ERR_BAD_ARG); }
  { Problem w = g; w.group_offsets[1] = 1L << 40; EXPECT(run(w, 5, 1, -1.0, 1.0).status == LOFTR_ERR_BAD_ARG); }
  { Problem w = g; w.group_offsets[1] = 0; EXPECT(run(w, 5, 1, -1.0, 1.0).status == LOFTR_ERR_BAD_ARG); }
  EXPECT(run(g, 5, 1, -1.0, 1.0).status == LOFTR_OK);

  // ---- the empty problems: no image at all; images and points without an observation; an image id out of range
  Problem z;
  z.group();
  r = run(z, 30, 1, -1.0, 1.0);
  EXPECT(r.status == LOFTR_OK && r.counts[0] == 3 && r.counts[13] == 0 && r.counts[15] == 0);
  Problem o = scene(2, 1.05, 0.95, -0.05, 0.05, 0.0);
  o.offsets.assign(o.offsets.size(), 0);
  o.image.clear(); o.xy.clear(); o.mask.clear();
  o.group();
  r = run(o, 30, 1, -1.0, 1.0);
  EXPECT(r.status == LOFTR_OK && r.counts[0] == 3 && r.counts[7] == 0 && r.counts[15] == 0 && same_bits(r.K, o.K, 0, o.K.size()));
  EXPECT(same_bits(r.k, o.k_start, 0, o.k_start.size()) && (r.cam_radial == std::vector<uint8_t>(5, 0)) && (r.group_radial == std::vector<uint8_t>(3, 0)));
  Problem bad = scene(2, 1.05, 0.95, -0.05, 0.05, 0.0);
  bad.group();
  bad.image[5] = 9;
  EXPECT(run(bad, 30, 1, -1.0, 1.0).status == LOFTR_ERR_BAD_ARG);

  // ---- a small undistortion batch: the round trip, a point beyond the fold, a NaN pixel, a camera with fx = 0, a bad image, no point
  std::vector<double> K = {500, 1, 320, 0, 510, 240, 0, 0, 1, 0, 0, 320, 0, 500, 240, 0, 0, 1}, kk = {-0.3, 0.1};
  std::vector<float> px = {330.f, 250.f, 600.f, 100.f, 320.f, 240.f, 5000.f, 240.f, NAN, 240.f, 330.f, 250.f}, d(12, -1.f), u(12, -1.f);
  std::vector<int> im = {0, 0, 0, 0, 0, 1};
  std::vector<uint8_t> okd(6, 9), oku(6, 9);
  std::vector<long> cnt(8, 7);
  EXPECT(loftr_distort_points_host(px.data(), im.data(), 6, K.data(), kk.data(), 2, d.data(), okd.data(), cnt.data()) == LOFTR_OK);
  EXPECT((okd == std::vector<uint8_t>{1, 1, 1, 1, 0, 0}) && cnt[0] == 4 && cnt[1] == 0 && cnt[2] == 2);
  d[6] = 5000.f; d[7] = 240.f;                                           // r_d = 9.4: far beyond the fold of k = -0.3
  EXPECT(loftr_undistort_points_host(d.data(), im.data(), 6, K.data(), kk.data(), 2, u.data(), oku.data(), cnt.data()) == LOFTR_OK);
  EXPECT((oku == std::vector<uint8_t>{1, 1, 1, 0, 0, 0}) && cnt[0] == 3 && cnt[2] == 3);
  for (int i = 0; i < 6; ++i) EXPECT(fabsf(u[i] - px[i]) < 1e-3f);
  for (int i = 6; i < 12; ++i) EXPECT(isnan(u[i]));
  EXPECT(u[4] == 320.f && u[5] == 240.f);
  im[3] = 2;
  std::vector<float> keep = u;
  EXPECT(loftr_undistort_points_host(d.data(), im.data(), 6, K.data(), kk.data(), 2, u.data(), oku.data(), cnt.data()) == LOFTR_ERR_BAD_ARG);
  EXPECT(cnt[1] == 1 && cnt[0] == 0 && memcmp(keep.data(), u.data(), 48) == 0);        // the bit, and nothing written
  EXPECT(loftr_undistort_points_host(nullptr, nullptr, 0, K.data(), kk.data(), 2, nullptr, nullptr, cnt.data()) == LOFTR_OK && cnt[1] == 0);
  EXPECT(loftr_undistort_points_host(nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, cnt.data()) == LOFTR_OK);
  EXPECT(loftr_undistort_points_host(d.data(), im.data(), 6, K.data(), kk.data(), 2, u.data(), oku.data(), nullptr) == LOFTR_ERR_BAD_ARG);
  printf("bundle_radial_host_driver: all cases passed\n");
  return 0;
}
