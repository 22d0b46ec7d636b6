// Stand-alone driver of the host estimators (pose.hip, geometry.hip, absolute_pose.hip) for a sanitizer pass on the CPU: it reads the
// cases written by `python tools/host_estimators_ab.py --dump CASES.bin` and calls every entry point once per case.  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/host_estimators_driver.cpp loftr_amd/csrc/pose.hip loftr_amd/csrc/geometry.hip loftr_amd/csrc/absolute_pose.hip -o driver
//   ./driver CASES.bin
// It uses no GPU.  Inputs and outputs live in exactly-sized heap blocks, so that a read or write past an end is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../include/loftr_hip.h"

template <class T>
static std::vector<T> take(FILE* fh, size_t n) {
  std::vector<T> v(n ? n : 1);                               // (an empty input still needs a non-null pointer)
  if (n && fread(v.data(), sizeof(T), n, fh) != n) { fprintf(stderr, "short read\n"); exit(2); }
  return v;
}

int main(int argc, char** argv) {
  FILE* fh = argc == 2 ? fopen(argv[1], "rb") : nullptr;
  if (!fh) { fprintf(stderr, "usage: %s CASES.bin\n", argv[0]); return 2; }
  long calls = 0, models = 0;
  int32_t h[4];
  while (fread(h, sizeof(int32_t), 4, fh) == 4) {
    const int kind = h[0], model = h[2];
    const size_t n = (size_t)h[1];
    const unsigned seed = (unsigned)h[3];
    long cnt = -1;
    int ns = 0, st = 0;
    std::vector<uint8_t> inl(n ? n : 1);                       // (an empty pair still needs a non-null mask)
    std::vector<float> R(9), t(3);
    if (kind == 0) {
      auto q0 = take<double>(fh, 2 * n), q1 = take<double>(fh, 2 * n);
      std::vector<double> E(90);
      st = loftr_five_point(q0.data(), q1.data(), (int)n, E.data(), &ns);
    } else if (kind == 1) {
      auto p0 = take<float>(fh, 2 * n), p1 = take<float>(fh, 2 * n), K0 = take<float>(fh, 9), K1 = take<float>(fh, 9);
      st = loftr_estimate_pose(p0.data(), p1.data(), (long)n, K0.data(), K1.data(), 0.5f, 0.99999f, seed, R.data(), t.data(), inl.data(), &cnt);
    } else if (kind == 2) {
      auto p0 = take<double>(fh, 2 * n), p1 = take<double>(fh, 2 * n);
      std::vector<double> mats(27);
      st = loftr_geometry_minimal(p0.data(), p1.data(), model, mats.data(), &ns);
    } else if (kind == 3) {
      auto p0 = take<float>(fh, 2 * n), p1 = take<float>(fh, 2 * n);
      st = loftr_estimate_geometry(p0.data(), p1.data(), (long)n, model, model == 0 ? 3.0f : 1.0f, 0.999f, seed, R.data(), inl.data(), &cnt);
    } else if (kind == 4) {
      auto X = take<double>(fh, 9), f = take<double>(fh, 9);
      std::vector<double> Rs(36), ts(12);
      st = loftr_p3p(X.data(), f.data(), Rs.data(), ts.data(), &ns);
    } else if (kind == 5) {
      auto X = take<float>(fh, 3 * n), kpts = take<float>(fh, 2 * n), K = take<float>(fh, 9);
      st = loftr_estimate_absolute_pose(X.data(), kpts.data(), (long)n, K.data(), 3.0f, 0.999f, seed, R.data(), t.data(), inl.data(), &cnt);
    } else {
      fprintf(stderr, "unknown case kind %d\n", kind);
      return 2;
    }
    if (st != LOFTR_OK) { fprintf(stderr, "call %ld (kind %d) returned %d\n", calls, kind, st); return 1; }
    ++calls;
    models += cnt > 0 || ns > 0;
  }
  fclose(fh);
  printf("%ld host calls, %ld with a model\n", calls, models);
  return 0;
}
