// Stand-alone check of the host routine of global positioning (csrc/position.hip) under the host sanitizers: the
// breadth-first levels and the CSR indexing are where a host bug would sit.  No GPU is touched.  Build and run on the CPU:
//   hipcc --offload-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined loftr_amd/csrc/position.hip \
//         tools/position_host_check.cpp -o /tmp/position_host_check && /tmp/position_host_check
// The program builds its own scene (it is not the tests' `small()` scene: other points, from its own generator): 5 cameras on a ring,
// 40 points seen by 4 cameras each, a path as the tree with every other edge stored child first; then the same with an image outside
// the graph, a tree edge without a direction, a point with one usable observation, and every error bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../include/loftr_global.h"

namespace {

struct Rng {
  uint64_t s;
  double uniform() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0; }
};

struct Scene {
  int n = 5;
  std::vector<long> offsets{0}, cam_offsets;
  std::vector<int> image, cam_obs, tree_image;
  std::vector<float> xy;
  std::vector<double> K, R, tree_t, c;
  std::vector<uint8_t> in_graph;
  int root = 0;
};

void look_at(const double* c, double* R) {
  double z[3] = {-c[0], -c[1], -c[2]};
  const double nz = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
  for (double& v : z) v /= nz;
  double x[3] = {z[2], 0.0, -z[0]};                                      // (0, 1, 0) x z
  const double nx = std::sqrt(x[0] * x[0] + x[2] * x[2]);
  for (double& v : x) v /= nx;
  const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
  for (int k = 0; k < 3; ++k) { R[k] = x[k]; R[3 + k] = y[k]; R[6 + k] = z[k]; }
}

Scene make_scene(int T) {
  Scene s;
  Rng rng{12345};
  const int n = s.n;
  s.K.resize(9 * n); s.R.resize(9 * n); s.c.resize(3 * n); s.in_graph.assign(n, 1);
  for (int i = 0; i < n; ++i) {
    const double a = 2.0 * 3.14159265358979323846 * i / n;
    double* c = &s.c[3 * i];
    c[0] = 6.0 * std::cos(a); c[1] = 0.3 * std::sin(3 * a); c[2] = 6.0 * std::sin(a);
    look_at(c, &s.R[9 * i]);
    const double K[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};
    for (int k = 0; k < 9; ++k) s.K[9 * i + k] = K[k];
  }
  for (int t = 0; t < T; ++t) {
    const double X[3] = {3 * rng.uniform() - 1.5, 3 * rng.uniform() - 1.5, 3 * rng.uniform() - 1.5};
    const int skip = (int)(rng.uniform() * n) % n;
    for (int i = 0; i < n; ++i) {
      if (i == skip) continue;
      const double* R = &s.R[9 * i];
      const double d[3] = {X[0] - s.c[3 * i], X[1] - s.c[3 * i + 1], X[2] - s.c[3 * i + 2]};
      double p[3];
      for (int r = 0; r < 3; ++r) p[r] = R[3 * r] * d[0] + R[3 * r + 1] * d[1] + R[3 * r + 2] * d[2];
      s.image.push_back(i);
      s.xy.push_back((float)(500 * p[0] / p[2] + 320 + rng.uniform() - 0.5));
      s.xy.push_back((float)(500 * p[1] / p[2] + 240 + rng.uniform() - 0.5));
    }
    s.offsets.push_back((long)s.image.size());
  }
  s.cam_offsets.assign(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    for (size_t o = 0; o < s.image.size(); ++o) if (s.image[o] == i) s.cam_obs.push_back((int)o);
    s.cam_offsets[i + 1] = (long)s.cam_obs.size();
  }
  for (int i = 0; i + 1 < n; ++i) {
    const int a = i % 2 ? i + 1 : i, b = i % 2 ? i : i + 1;                // every other edge stored child first
    s.tree_image.push_back(a); s.tree_image.push_back(b);
    const double* R = &s.R[9 * b];
    const double d[3] = {s.c[3 * a] - s.c[3 * b], s.c[3 * a + 1] - s.c[3 * b + 1], s.c[3 * a + 2] - s.c[3 * b + 2]};
    for (int r = 0; r < 3; ++r) s.tree_t.push_back(R[3 * r] * d[0] + R[3 * r + 1] * d[1] + R[3 * r + 2] * d[2]);
  }
  return s;
}

int run(const char* name, Scene& s, long want_bits, int max_iters = 50) {
  const long T = (long)s.offsets.size() - 1, N = (long)s.image.size(), Et = (long)s.tree_image.size() / 2;
  std::vector<double> centres(3 * s.n), depth(N ? N : 1), info(4);
  std::vector<float> xyz(T ? 3 * T : 1);
  std::vector<uint8_t> obs_state(N ? N : 1), cam_state(s.n), active(T ? T : 1);
  std::vector<long> counts(16);
  const int st = loftr_global_positions_host(s.offsets.data(), T, s.image.data(), s.xy.data(), N, s.cam_offsets.data(), s.cam_obs.data(),
                                             s.K.data(), s.R.data(), s.in_graph.data(), s.n, s.root, s.tree_image.data(), s.tree_t.data(), Et,
                                             0.1, max_iters, 30, 1e-2, 1e-7, 8, centres.data(), xyz.data(), depth.data(), obs_state.data(),
                                             cam_state.data(), active.data(), counts.data(), info.data());
  std::printf("%-18s status %d, error bits %ld, trials %ld, accepted %ld, pcg %ld, active obs %ld, free %ld, cost %.3e -> %.3e\n", name, st,
              counts[1], counts[0], counts[2], counts[3], counts[4], counts[6], info[0], info[1]);
  const bool ok = want_bits ? (st == LOFTR_ERR_BAD_ARG && counts[1] == want_bits) : (st == LOFTR_OK && counts[1] == 0);
  if (!ok) std::printf("  UNEXPECTED (wanted error bits %ld)\n", want_bits);
  return ok ? 0 : 1;
}

}  // namespace

int main() {
  int bad = 0;
  Scene s = make_scene(40);
  bad += run("small", s, 0);
  bad += run("start values", s, 0, 0);
  { Scene e = make_scene(0); e.image.clear(); bad += run("no tracks", e, 0); }
  { Scene e = s; e.in_graph[4] = 0; e.tree_image.resize(6); e.tree_t.resize(9); bad += run("outside graph", e, 0); }
  { Scene e = s; e.tree_t[3] = e.tree_t[4] = e.tree_t[5] = 0.0; e.tree_t[6] = INFINITY; bad += run("no direction", e, 0); }
  { Scene e = s; for (long o = e.offsets[3] + 1; o < e.offsets[4]; ++o) e.xy[2 * o] = NAN; bad += run("one usable", e, 0); }
  { Scene e = s; e.image[5] = e.n; bad += run("image outside", e, 1 | 4); }
  { Scene e = s; e.offsets[3] = e.offsets[2] - 1; bad += run("offsets descend", e, 2); }
  { Scene e = s; std::swap(e.cam_obs[0], e.cam_obs[1]); bad += run("grouping", e, 4); }
  { Scene e = s; e.root = e.n; bad += run("root outside", e, 8); }
  { Scene e = s; e.tree_image[5] = e.n; bad += run("edge outside", e, 16); }
  { Scene e = s; e.tree_image[6] = 1; e.tree_image[7] = 3; bad += run("end reached twice", e, 16); }
  { Scene e = s; e.tree_image[0] = 1; e.tree_image[1] = 2; bad += run("edge never reached", e, 16); }
  std::printf(bad ? "FAILED: %d case(s)\n" : "all cases as expected\n", bad);
  return bad ? 1 : 0;
}
