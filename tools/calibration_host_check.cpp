// Stand-alone check of the host routine of view-graph calibration (csrc/calib.hip) under the host sanitizers: the
// incidence lists and the workspace carving are where a host bug would sit.  No GPU is touched.  Build and run on the CPU:
//   hipcc --offload-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined loftr_amd/csrc/calib.hip \
//         tools/calibration_host_check.cpp -o /tmp/calibration_host_check && /tmp/calibration_host_check
// The program builds its own scene (it is not the tests' `small()` scene: its own generator): 5 cameras on a ring that look past the
// centre, every pair an edge with the exact F of the two cameras; then the same with shared cameras, an image without edges, invalid
// edges, held groups, no edges at all, max_iters = 0, a bound rejection, and every error bit.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>
#include "../include/loftr_calib.h"

namespace {

struct Rng {
  uint64_t s;
  double uniform() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0; }
};

struct Scene {
  int n = 5, G = 5;
  std::vector<int> edge_image, weight, group, inc;
  std::vector<double> F, pp, f0, f_true;
  std::vector<long> offsets;
};

void look_at(const double* c, const double* target, double* R) {
  double z[3] = {target[0] - c[0], target[1] - c[1], target[2] - c[2]};
  const double nz = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
  for (double& v : z) v /= nz;
  double x[3] = {z[2], 0.0, -z[0]};                                      // (0, 1, 0) x z
  const double nx = std::sqrt(x[0] * x[0] + x[2] * x[2]);
  for (double& v : x) v /= nx;
  const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
  for (int k = 0; k < 3; ++k) { R[k] = x[k]; R[3 + k] = y[k]; R[6 + k] = z[k]; }
}

void mul(const double* a, const double* b, double* o) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[3 * r + c] = a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c] + a[3 * r + 2] * b[6 + c];
}

// the stable ascending grouping of the edge ends by the group of their image
void make_lists(Scene& s) {
  const int E2 = (int)s.edge_image.size();
  s.inc.resize(E2);
  std::iota(s.inc.begin(), s.inc.end(), 0);
  auto key = [&](int code) { const int i = s.edge_image[code]; return (i >= 0 && i < s.n) ? std::min(std::max(s.group[i], 0), s.G - 1) : 0; };
  std::stable_sort(s.inc.begin(), s.inc.end(), [&](int a, int b) { return key(a) < key(b); });
  s.offsets.assign(s.G + 1, 0);
  for (int code = 0; code < E2; ++code) s.offsets[key(code) + 1] += 1;
  for (int g = 0; g < s.G; ++g) s.offsets[g + 1] += s.offsets[g];
}

Scene make_scene() {
  Scene s;
  Rng rng{2024};
  const int n = s.n;
  std::vector<double> R(9 * n), c(3 * n);
  for (int i = 0; i < n; ++i) {
    const double a = 2.0 * 3.14159265358979323846 * i / n;
    c[3 * i] = 6.0 * std::cos(a); c[3 * i + 1] = rng.uniform() - 0.5; c[3 * i + 2] = 6.0 * std::sin(a);
    const double target[3] = {2 * rng.uniform() - 1, 2 * rng.uniform() - 1, 2 * rng.uniform() - 1};
    look_at(&c[3 * i], target, &R[9 * i]);
    s.f_true.push_back(600.0 + 500.0 * rng.uniform());
    s.f0.push_back(1200.0);
    s.pp.push_back(500.0); s.pp.push_back(375.0);
    s.group.push_back(i);
  }
  for (int a = 0; a < n; ++a)
    for (int b = a + 1; b < n; ++b) {
      // x_b = R_b R_a^T x_a + R_b (c_a - c_b);  F = K_b^-T [t]x R_ab K_a^-1
      double Rat[9], Rab[9], t[3], E[9], Kb[9], Ka[9], tmp[9], F[9];
      for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) Rat[3 * r + k] = R[9 * a + 3 * k + r];
      mul(&R[9 * b], Rat, Rab);
      for (int r = 0; r < 3; ++r)
        t[r] = R[9 * b + 3 * r] * (c[3 * a] - c[3 * b]) + R[9 * b + 3 * r + 1] * (c[3 * a + 1] - c[3 * b + 1]) + R[9 * b + 3 * r + 2] * (c[3 * a + 2] - c[3 * b + 2]);
      const double tx[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
      mul(tx, Rab, E);
      auto kinv = [&](int i, double* K, bool transposed) {
        const double f = s.f_true[i];
        const double m[9] = {1 / f, 0, -500.0 / f, 0, 1 / f, -375.0 / f, 0, 0, 1};
        for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) K[3 * r + k] = transposed ? m[3 * k + r] : m[3 * r + k];
      };
      kinv(b, Kb, true); kinv(a, Ka, false);
      mul(Kb, E, tmp); mul(tmp, Ka, F);
      double nf = 0;
      for (double v : F) nf += v * v;
      nf = std::sqrt(nf);
      for (double v : F) s.F.push_back((double)(float)(v / nf));
      s.edge_image.push_back(a); s.edge_image.push_back(b);
      s.weight.push_back(40 + 10 * (a + b));
    }
  make_lists(s);
  return s;
}

struct Params { double loss = 0.05, max_resid = 0.05, prior = 1e-3; int cap = 100; double lo = 0.2, hi = 5.0; int min_edges = 1, max_iters = 50, pcg = 30; };

int run(const char* name, Scene& s, long want_bits, const Params& p = Params(), double want_err = 0.0) {
  const long E = (long)s.weight.size();
  std::vector<double> scale(s.G), focal(s.n), resid(E ? E : 1), info(4);
  std::vector<uint8_t> estate(E ? E : 1), gstate(s.G);
  std::vector<long> counts(16);
  const int st = loftr_calibrate_view_graph_host(E ? s.edge_image.data() : nullptr, E ? s.F.data() : nullptr, E ? s.weight.data() : nullptr, E,
                                                 s.pp.data(), s.f0.data(), s.group.data(), s.n, s.G, s.offsets.data(), E ? s.inc.data() : nullptr,
                                                 p.loss, p.max_resid, p.prior, p.cap, p.lo, p.hi, p.min_edges, p.max_iters, p.pcg, 1e-2, 1e-9,
                                                 scale.data(), focal.data(), E ? resid.data() : nullptr, E ? estate.data() : nullptr, gstate.data(),
                                                 counts.data(), info.data());
  double err = 0.0;
  for (int i = 0; i < s.n; ++i) err = std::max(err, std::fabs(focal[i] / s.f_true[i] - 1.0));
  std::printf("%-18s status %d, error bits %ld, trials %ld, accepted %ld, pcg %ld, valid %ld, free %ld, outliers %ld, bound %ld, cost %.3e -> %.3e, "
              "focal error %.2e\n", name, st, counts[1], counts[0], counts[2], counts[3], counts[4], counts[5], counts[6], counts[8], info[0], info[1], err);
  bool ok = want_bits ? (st == LOFTR_ERR_BAD_ARG && counts[1] == want_bits) : (st == LOFTR_OK && counts[1] == 0);
  if (ok && want_err > 0.0) ok = err <= want_err;
  if (!ok) std::printf("  UNEXPECTED (wanted error bits %ld, focal error <= %.1e)\n", want_bits, want_err);
  return ok ? 0 : 1;
}

}  // namespace

int main() {
  int bad = 0;
  Scene s = make_scene();
  bad += run("small", s, 0, Params(), 0.01);                                  // exact F: the prior's pull alone, well below 1 %
  { Params p; p.prior = 0.0; bad += run("no prior", s, 0, p, 1e-5); }
  { Params p; p.max_iters = 0; bad += run("start values", s, 0, p); }
  { Params p; p.pcg = 0; bad += run("no cg iterations", s, 0, p); }
  { Params p; p.lo = 0.9; p.hi = 1.1; bad += run("bounds", s, 0, p); }
  { Params p; p.min_edges = 5; bad += run("all held", s, 0, p); }
  { Scene e = s; e.G = 2; e.group = {0, 0, 1, 1, 1}; e.f_true = {800, 800, 900, 900, 900}; make_lists(e); bad += run("shared cameras", e, 0); }
  { Scene e = s; e.G = 1; e.group.assign(5, 0); make_lists(e); bad += run("one camera", e, 0); }
  { Scene e = s; e.n = 6; e.G = 6; e.group.push_back(5); e.f0.push_back(900); e.f_true.push_back(900); e.pp.push_back(500); e.pp.push_back(375);
    make_lists(e); bad += run("image without edge", e, 0); }
  { Scene e = s; e.weight[0] = 0; e.weight[3] = -2; e.F[9 * 5 + 4] = NAN; e.F[9 * 7] = INFINITY; for (int k = 0; k < 9; ++k) e.F[9 * 9 + k] = 0.0;
    bad += run("invalid edges", e, 0); }
  { Scene e = s; e.edge_image.clear(); e.weight.clear(); e.F.clear(); make_lists(e); bad += run("no edges", e, 0); }
  { Scene e = s; e.edge_image[5] = e.n; bad += run("image outside", e, 1); }
  { Scene e = s; e.edge_image[4] = -1; bad += run("image negative", e, 1); }
  { Scene e = s; e.edge_image[6] = e.edge_image[7]; bad += run("self edge", e, 1 | 4); }
  { Scene e = s; e.group[4] = e.G; bad += run("group outside", e, 2); }
  { Scene e = s; e.group[0] = -1; bad += run("group negative", e, 2); }
  { Scene e = s; std::swap(e.inc[0], e.inc[1]); bad += run("slots swapped", e, 4); }
  { Scene e = s; e.inc[7] = 2 * 10; bad += run("slot outside", e, 4); }
  { Scene e = s; e.inc[0] = -1; bad += run("slot negative", e, 4); }
  { Scene e = s; e.offsets[2] += 1; bad += run("offsets shifted", e, 4); }
  { Scene e = s; e.offsets[0] = -1; bad += run("offsets start", e, 4); }
  { Scene e = s; e.offsets[5] -= 1; bad += run("offsets end", e, 4); }
  { Scene e = s; e.f0[2] = 0.0; bad += run("focal zero", e, 8); }
  { Scene e = s; e.f0[4] = NAN; bad += run("focal nan", e, 8); }
  { Scene e = s; e.pp[3] = INFINITY; bad += run("pp infinite", e, 8); }
  { Scene e = s; e.edge_image[5] = e.n; e.group[0] = 9; e.f0[1] = -1; std::swap(e.inc[e.offsets[2]], e.inc[e.offsets[2] + 1]); bad += run("every bit", e, 15); }
  std::printf(bad ? "FAILED: %d case(s)\n" : "all cases as expected\n", bad);
  return bad ? 1 : 0;
}
