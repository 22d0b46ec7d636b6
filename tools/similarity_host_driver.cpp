// Stand-alone driver of the host similarity estimator and of loftr_transform_model_host (csrc/similarity.hip) for a sanitizer pass on
// the CPU: hand-written cases (M = 0, 2, 3, a collinear set, an exact set, a set with outliers; a model with an unposed NaN image,
// out of place and in place).  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/similarity_host_driver.cpp loftr_amd/csrc/similarity.hip -o driver
//   ./driver
// It uses no GPU.  Inputs and outputs live in exactly-sized heap blocks, so that a read or write past an end is caught.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/loftr_hip.h"

template <class T> static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// a rotation by `angle` about the unit axis (ax, ay, az) (Rodrigues)
static void rotation(double ax, double ay, double az, double angle, double* R) {
  const double c = cos(angle), s = sin(angle), v = 1 - c;
  const double r[9] = {c + ax * ax * v, ax * ay * v - az * s, ax * az * v + ay * s, ay * ax * v + az * s, c + ay * ay * v,
                       ay * az * v - ax * s, az * ax * v - ay * s, az * ay * v + ax * s, c + az * az * v};
  memcpy(R, r, sizeof(r));
}

struct Result { double s, R[9], t[3]; std::vector<uint8_t> in; long n; int status; };

static Result estimate(std::vector<double>& src, std::vector<double>& dst, int with_scale, double thresh, unsigned seed) {
  const long M = (long)src.size() / 3;
  Result r;
  r.in.assign(M, 7);
  r.status = loftr_estimate_similarity(ptr(src), ptr(dst), M, with_scale, thresh, 0.999f, seed, &r.s, r.R, r.t, ptr(r.in), &r.n);
  return r;
}

static std::vector<double> moved(const std::vector<double>& src, double s, const double* R, const double* t) {
  std::vector<double> dst(src.size());
  for (size_t i = 0; i < src.size() / 3; ++i)
    for (int k = 0; k < 3; ++k) dst[3 * i + k] = s * (R[3 * k] * src[3 * i] + R[3 * k + 1] * src[3 * i + 1] + R[3 * k + 2] * src[3 * i + 2]) + t[k];
  return dst;
}

static bool no_model(const Result& r) {
  bool zero = r.s == 0;
  for (double v : r.R) zero = zero && v == 0;
  for (double v : r.t) zero = zero && v == 0;
  for (uint8_t b : r.in) zero = zero && b == 0;
  return r.status == LOFTR_OK && r.n == -1 && zero;
}

int main() {
  double R[9];
  rotation(0.6, 0.0, 0.8, 0.9, R);
  const double t[3] = {0.5, -2.0, 3.0}, s = 1.7;
  std::vector<double> cloud;
  unsigned long long x = 88172645463325252ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (double)(x >> 11) / 9007199254740992.0 * 2 - 1; };
  for (int i = 0; i < 3 * 40; ++i) cloud.push_back(3 * rnd());

  for (int M : {0, 2}) {                                                  // too few correspondences
    std::vector<double> a(cloud.begin(), cloud.begin() + 3 * M), b = moved(a, s, R, t);
    EXPECT(no_model(estimate(a, b, 1, 0.01, 0)));
  }
  {                                                                       // M = 3: the minimal sample is the model
    std::vector<double> a(cloud.begin(), cloud.begin() + 9), b = moved(a, s, R, t);
    const Result r = estimate(a, b, 1, 1e-6, 0);
    EXPECT(r.status == LOFTR_OK && r.n == 3 && fabs(r.s - s) < 1e-9);
    for (int k = 0; k < 9; ++k) EXPECT(fabs(r.R[k] - R[k]) < 1e-9);
    double s1, R1[9], t1[3];
    int ns = -1;
    EXPECT(loftr_similarity_minimal(a.data(), b.data(), 0, &s1, R1, t1, &ns) == LOFTR_OK && ns == 1 && s1 == 1.0);
    EXPECT(loftr_similarity_minimal(nullptr, b.data(), 0, &s1, R1, t1, &ns) == LOFTR_ERR_BAD_ARG);
  }
  {                                                                       // collinear: every sample is degenerate
    std::vector<double> a;
    for (int i = 0; i < 12; ++i) { a.push_back(0.3 * i); a.push_back(-0.1 * i + 1); a.push_back(0.7 * i - 2); }
    std::vector<double> b = moved(a, s, R, t);
    EXPECT(no_model(estimate(a, b, 1, 0.01, 3)));
  }
  {                                                                       // exact: every correspondence is an inlier, both modes
    std::vector<double> a = cloud, b = moved(a, s, R, t), c = moved(a, 1.0, R, t);
    const Result r = estimate(a, b, 1, 1e-6, 1);
    EXPECT(r.status == LOFTR_OK && r.n == 40 && fabs(r.s - s) < 1e-9);
    for (int k = 0; k < 3; ++k) EXPECT(fabs(r.t[k] - t[k]) < 1e-8);
    const Result q = estimate(a, c, 0, 1e-6, 1);
    EXPECT(q.status == LOFTR_OK && q.n == 40 && q.s == 1.0);
  }
  {                                                                       // outliers: a third of the destinations grossly moved
    std::vector<double> a = cloud, b = moved(a, s, R, t);
    for (int i = 0; i < 40; i += 3) b[3 * i + (i % 3)] += 5.0 + i;
    const Result r = estimate(a, b, 1, 0.01, 5);
    EXPECT(r.status == LOFTR_OK && r.n == 26);
    for (int i = 0; i < 40; ++i) EXPECT(r.in[i] == (i % 3 != 0));
    EXPECT(fabs(r.s - s) < 1e-9);
  }
  {                                                                       // bad arguments
    std::vector<double> a = cloud, b = cloud;
    std::vector<uint8_t> in(40);
    double s1, R1[9], t1[3];
    long n;
    EXPECT(loftr_estimate_similarity(nullptr, b.data(), 40, 1, 0.1, 0.999f, 0, &s1, R1, t1, in.data(), &n) == LOFTR_ERR_BAD_ARG);
    EXPECT(loftr_estimate_similarity(a.data(), b.data(), -1, 1, 0.1, 0.999f, 0, &s1, R1, t1, in.data(), &n) == LOFTR_ERR_BAD_ARG);
    EXPECT(loftr_estimate_similarity(a.data(), b.data(), 40, 1, 0.1, 0.999f, 0, &s1, R1, t1, in.data(), nullptr) == LOFTR_ERR_BAD_ARG);
  }
  {                                                                       // moving a model: 5 points, 3 images (the middle one unposed, NaN)
    std::vector<float> xyz = {0, 0, 0, 1, 2, 3, -1, 0.5f, 2, NAN, 1, 1, 4, 4, 4}, out(15);
    std::vector<double> T(48, 0.0), To(48);
    std::vector<uint8_t> posed = {1, 0, 1};
    double Rc[9];
    rotation(0.0, 1.0, 0.0, 0.4, Rc);
    for (int i = 0; i < 3; ++i) {
      for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T[16 * i + 4 * r + c] = Rc[3 * r + c]; T[16 * i + 4 * r + 3] = 0.1 * i + r; }
      T[16 * i + 15] = 1.0;
    }
    for (int k = 0; k < 16; ++k) T[16 + k] = NAN;
    EXPECT(loftr_transform_model_host(xyz.data(), 5, T.data(), posed.data(), 3, &s, R, t, out.data(), To.data()) == LOFTR_OK);
    EXPECT(memcmp(&To[16], &T[16], 16 * sizeof(double)) == 0 && To[15] == 1.0 && To[12] == 0.0 && isnan(out[9]));
    // the camera coordinates of a moved point through the moved pose are s times the original ones
    const double X[3] = {1, 2, 3};
    for (int r = 0; r < 3; ++r) {
      const double before = T[4 * r] * X[0] + T[4 * r + 1] * X[1] + T[4 * r + 2] * X[2] + T[4 * r + 3];
      const double after = To[4 * r] * out[3] + To[4 * r + 1] * out[4] + To[4 * r + 2] * out[5] + To[4 * r + 3];
      EXPECT(fabs(after - s * before) < 1e-5);
    }
    std::vector<float> xyz2 = xyz;
    std::vector<double> T2 = T;
    EXPECT(loftr_transform_model_host(xyz2.data(), 5, T2.data(), posed.data(), 3, &s, R, t, xyz2.data(), T2.data()) == LOFTR_OK);   // in place
    EXPECT(memcmp(xyz2.data(), out.data(), 15 * sizeof(float)) == 0 && memcmp(T2.data(), To.data(), 48 * sizeof(double)) == 0);
    EXPECT(loftr_transform_model_host(nullptr, 0, nullptr, nullptr, 0, &s, R, t, nullptr, nullptr) == LOFTR_OK);                      // empty
    EXPECT(loftr_transform_model_host(nullptr, 5, T.data(), posed.data(), 3, &s, R, t, out.data(), To.data()) == LOFTR_ERR_BAD_ARG);
  }
  printf(failures ? "%d check(s) FAILED\n" : "similarity host driver: all checks passed\n", failures);
  return failures ? 1 : 0;
}
