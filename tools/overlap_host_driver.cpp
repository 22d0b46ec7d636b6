// Stand-alone driver of the host routine of view overlap (csrc/overlap.hip) for a sanitizer pass on the CPU: the hand-placed points of
// tests/_overlap_cases.py (on the image edge and the border, z = 0 and behind, the angle and the scale at equality, max_scale2 = inf),
// unusable entries, invalid views, the empty tables (an empty list, V = 0, T = 0, n = 0, m = 0) and the two error bits.  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/overlap_host_driver.cpp loftr_amd/csrc/overlap.hip -o driver
//   ./driver
// It uses no GPU.  Inputs and outputs live in exactly-sized heap blocks, so that a read or write past an end is caught.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../include/loftr_hip.h"

struct View { double f, cx, cy, cz, ppx; bool minus_x; };                 // a camera at (cx, cy, cz): identity rotation, or its axis along -x

struct Case {
  std::vector<long> offsets{0};
  std::vector<int> point;
  std::vector<float> xyz;
  std::vector<uint8_t> point_ok, src_ok, tgt_ok;
  std::vector<double> Ks, Ts, Kt, Tt, hw;
  double border = 0.0, cos_min = -1.0, max_scale2 = INFINITY;
  static void push(const View& v, std::vector<double>& K, std::vector<double>& T) {
    const double k[9] = {v.f, 0, v.ppx, 0, v.f, 240, 0, 0, 1};
    const double id[16] = {1, 0, 0, -v.cx, 0, 1, 0, -v.cy, 0, 0, 1, -v.cz, 0, 0, 0, 1};
    const double mx[16] = {0, 0, 1, -v.cz, 0, 1, 0, -v.cy, -1, 0, 0, v.cx, 0, 0, 0, 1};              // t = -R c
    K.insert(K.end(), k, k + 9);
    T.insert(T.end(), v.minus_x ? mx : id, (v.minus_x ? mx : id) + 16);
  }
  void source(const View& v, std::vector<int> list, bool ok = true) {
    push(v, Ks, Ts);
    src_ok.push_back(ok);
    point.insert(point.end(), list.begin(), list.end());
    offsets.push_back((long)point.size());
  }
  void target(const View& v, double H = 480, double W = 640, bool ok = true) {
    push(v, Kt, Tt);
    tgt_ok.push_back(ok);
    hw.push_back(H); hw.push_back(W);
  }
  int pt(float x, float y, float z, bool ok = true) {
    xyz.push_back(x); xyz.push_back(y); xyz.push_back(z);
    point_ok.push_back(ok);
    return (int)point_ok.size() - 1;
  }
};

template <class T> static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

static int run(Case& c, std::vector<int>* overlap, std::vector<int>* n_vis, std::vector<long>* counts_out) {
  const int n = (int)c.src_ok.size(), m = (int)c.tgt_ok.size();
  std::vector<int> o((size_t)n * m, -7), v((size_t)n, -7);
  std::vector<long> counts(8, -7);
  const int st = loftr_view_overlap_host(n ? c.offsets.data() : nullptr, ptr(c.point), (long)c.point.size(), ptr(c.xyz), ptr(c.point_ok),
                                         (long)c.point_ok.size(), ptr(c.Ks), ptr(c.Ts), ptr(c.src_ok), n, ptr(c.Kt), ptr(c.Tt), ptr(c.tgt_ok),
                                         ptr(c.hw), m, c.border, c.cos_min, c.max_scale2, ptr(o), ptr(v), counts.data());
  if (overlap) *overlap = o;
  if (n_vis) *n_vis = v;
  if (counts_out) *counts_out = counts;
  return st;
}

static const View kOrigin{512, 0, 0, 0, 320, false};

// one source at the origin; a point (x, y, 4) projects to (128 x + 320, 128 y + 240) in a target of the same pose
static Case edges(double border) {
  Case c;
  std::vector<int> list;
  const float e = 9.5367431640625e-07f;                                   // 2^-20
  for (float x : {-2.5f, -2.5f - e, 2.5f, 2.5f - e, -2.0f, -2.0f - e, 2.0f, 2.0f - e}) list.push_back(c.pt(x, 0, 4));
  for (float y : {-1.875f, -1.875f - e, 1.875f, 1.875f - e, -1.375f, 1.375f}) list.push_back(c.pt(0, y, 4));
  list.push_back(c.pt(0, 0, 4, false));                                   // not ok
  list.push_back(c.pt(NAN, 0, 4));
  list.push_back(c.pt(0, INFINITY, 4));
  c.source(kOrigin, list);
  c.target(kOrigin);
  c.border = border;
  return c;
}

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  std::vector<int> o, v;
  std::vector<long> counts;
  Case c = edges(0.0);
  EXPECT(run(c, &o, &v, &counts) == LOFTR_OK && o[0] == 10 && v[0] == 14 && (counts == std::vector<long>{14, 0, 1, 1, 1, 0, 0, 0}));
  c = edges(64.0);
  EXPECT(run(c, &o, &v, &counts) == LOFTR_OK && o[0] == 3 && v[0] == 14);
  // z = 0, behind, in front
  Case z;
  z.source(kOrigin, {z.pt(0, 0, 4)});
  z.target({512, 1, 0, 4, 320, false}); z.target({512, 0, 0, 4, 320, false}); z.target({512, 0, 0, 5, 320, false}); z.target({512, 0, 0, 3, 320, false});
  EXPECT(run(z, &o, &v, &counts) == LOFTR_OK && (o == std::vector<int>{0, 0, 0, 1}) && counts[3] == 4 && counts[4] == 1);
  // the angle at equality: perpendicular rays with cos_min = 0, then just above; 0.8 x 20 rounds to 16
  Case a;
  a.source(kOrigin, {a.pt(0, 0, 4)});
  a.target({512, 4, 0, 4, 320, true});
  a.target({512, 3, 0, 0, 512, false}, 480, 1024);
  a.cos_min = 0.0;
  EXPECT(run(a, &o, nullptr, nullptr) == LOFTR_OK && (o == std::vector<int>{1, 1}));
  a.cos_min = 0.8;
  EXPECT(run(a, &o, nullptr, nullptr) == LOFTR_OK && (o == std::vector<int>{0, 1}));
  a.cos_min = nextafter(0.8, 1.0);
  EXPECT(run(a, &o, nullptr, nullptr) == LOFTR_OK && (o == std::vector<int>{0, 0}));
  // the scale at equality: distances 4 and 8 at equal focals, focals 512 and 256 at equal distance
  Case s;
  const int p = s.pt(0, 0, 4);
  s.source(kOrigin, {p}); s.source({512, 0, 0, -4, 320, false}, {p});
  s.target({512, 0, 0, -4, 320, false}); s.target({256, 0, 0, 0, 320, false});
  s.max_scale2 = 4.0;
  EXPECT(run(s, &o, nullptr, nullptr) == LOFTR_OK && (o == std::vector<int>{1, 1, 1, 1}));
  s.max_scale2 = nextafter(4.0, 0.0);
  EXPECT(run(s, &o, nullptr, nullptr) == LOFTR_OK && (o == std::vector<int>{0, 0, 1, 1}));
  s.max_scale2 = INFINITY;
  EXPECT(run(s, &o, nullptr, nullptr) == LOFTR_OK && (o == std::vector<int>{1, 1, 1, 1}));
  // invalid views: a source switched off, fx = 0, a NaN pose; a target switched off, with H = 0, W = NaN
  Case i = edges(0.0);
  i.source(kOrigin, {0, 4}, false); i.source({0, 0, 0, 0, 320, false}, {0, 4}); i.source(kOrigin, {0, 4});
  i.Ts[16 * 3 + 3] = NAN;
  i.target(kOrigin, 480, 640, false); i.target(kOrigin, 0, 640); i.target(kOrigin, 480, NAN); i.target({512, 0, 0, 0, INFINITY, false});
  EXPECT(run(i, &o, &v, &counts) == LOFTR_OK && (v == std::vector<int>{14, 0, 0, 0}) && counts[2] == 1 && counts[3] == 1 && counts[4] == 1 && o[0] == 10);
  // the parameters
  Case b = edges(0.0);
  b.border = -1.0; EXPECT(run(b, nullptr, nullptr, nullptr) == LOFTR_ERR_BAD_ARG);
  b.border = 0.0; b.cos_min = NAN; EXPECT(run(b, nullptr, nullptr, nullptr) == LOFTR_ERR_BAD_ARG);
  b.cos_min = 0.5; b.max_scale2 = 0.5; EXPECT(run(b, nullptr, nullptr, nullptr) == LOFTR_ERR_BAD_ARG);
  // an empty list, V = 0, T = 0, n = 0, m = 0
  Case e1 = edges(0.0);
  e1.source(kOrigin, {});
  EXPECT(run(e1, &o, &v, &counts) == LOFTR_OK && v[1] == 0 && o[1] == 0 && counts[2] == 2);
  Case e2;
  e2.pt(0, 0, 4); e2.source(kOrigin, {}); e2.target(kOrigin);
  EXPECT(run(e2, &o, &v, &counts) == LOFTR_OK && o[0] == 0 && counts[0] == 0);
  Case e3;
  e3.source(kOrigin, {}); e3.target(kOrigin);
  EXPECT(run(e3, &o, &v, &counts) == LOFTR_OK && o[0] == 0 && counts[2] == 1 && counts[3] == 1);
  Case e4;
  e4.pt(0, 0, 4); e4.target(kOrigin);
  EXPECT(run(e4, &o, &v, &counts) == LOFTR_OK && counts[2] == 0 && counts[3] == 1);
  Case e5 = edges(0.0);
  e5.Kt.clear(); e5.Tt.clear(); e5.tgt_ok.clear(); e5.hw.clear();
  EXPECT(run(e5, &o, &v, &counts) == LOFTR_OK && v[0] == 14 && counts[3] == 0 && counts[4] == 0);
  Case e6;
  EXPECT(run(e6, &o, &v, &counts) == LOFTR_OK && (counts == std::vector<long>(8, 0)));
  // the error bits: nothing is read through the bad value
  Case bad = edges(0.0);
  bad.point[3] = (int)bad.point_ok.size();
  EXPECT(run(bad, nullptr, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[1] == 1);
  bad = edges(0.0); bad.point[0] = -1;
  EXPECT(run(bad, nullptr, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[1] == 1);
  bad = edges(0.0); bad.offsets[0] = 1;
  EXPECT(run(bad, nullptr, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[1] == 2);
  bad = edges(0.0); bad.offsets[1] += 5;
  EXPECT(run(bad, nullptr, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[1] == 2);
  bad = edges(0.0); bad.source(kOrigin, {0}); bad.offsets[1] = bad.offsets[2] + 1; bad.point[2] = 1 << 30;
  EXPECT(run(bad, nullptr, nullptr, &counts) == LOFTR_ERR_BAD_ARG && counts[1] == 3);
  printf("overlap_host_driver: all cases passed\n");
  return 0;
}
