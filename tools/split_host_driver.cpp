// Stand-alone driver of the host routine of track splitting (csrc/split.hip) for a sanitizer pass on the CPU: the hand-written cases of
// tests/_split_cases.py (the minimal conflict and its reversed order, ties, a duplicated edge, the descending chain under 32 / 3 / 0
// rounds, two inconsistent components beside consistent tracks and a loose keypoint, a self edge, E = 0, K = 0, T = 0, min_track_len
// 1 / 2 / 3, every error bit an entry point can be given), a seeded random graph, and the two list walks of split_core.h on lists
// that are too long (the only way to reach error bit 16).  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/split_host_driver.cpp loftr_amd/csrc/split.hip -o driver
//   ./driver
// It uses no GPU.  Inputs and outputs live in exactly-sized heap blocks, so that a read or write past an end is caught.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/loftr_hip.h"
#include "../loftr_amd/csrc/split_core.h"

struct Edge { int u, v; float conf; };
struct Out {
  std::vector<int> id, len, rounds;
  std::vector<uint8_t> state;
  long counts[16];
  int status;
};

template <class T> static T* exact(const std::vector<T>& v) {               // a heap block of exactly v.size() items (nullptr for none)
  if (v.empty()) return nullptr;
  T* p = new T[v.size()];
  memcpy(p, v.data(), sizeof(T) * v.size());
  return p;
}

static Out run(const std::vector<Edge>& edges, const std::vector<int>& kp_image, const std::vector<int>& track_id, const std::vector<uint8_t>& ok,
               int n_images, int min_len = 2, int max_rounds = 32) {
  std::vector<int> e;
  std::vector<float> c;
  for (const Edge& x : edges) { e.push_back(x.u); e.push_back(x.v); c.push_back(x.conf); }
  const long E = (long)edges.size(), K = (long)kp_image.size(), T = (long)ok.size();
  int *pe = exact(e), *pi = exact(kp_image), *pt = exact(track_id);
  float* pc = exact(c);
  uint8_t* po = exact(ok);
  int *id = K ? new int[K] : nullptr, *len = K ? new int[K] : nullptr, *rounds = max_rounds ? new int[max_rounds] : nullptr;
  uint8_t* state = E ? new uint8_t[E] : nullptr;
  Out o;
  o.status = loftr_split_tracks_host(pe, pc, E, pi, pt, K, po, T, n_images, min_len, max_rounds, id, len, state, rounds, o.counts);
  if (o.status == LOFTR_OK) {
    o.id.assign(id, id + K); o.len.assign(len, len + K); o.state.assign(state, state + E); o.rounds.assign(rounds, rounds + max_rounds);
  }
  delete[] pe; delete[] pi; delete[] pt; delete[] pc; delete[] po; delete[] id; delete[] len; delete[] rounds; delete[] state;
  return o;
}

static int failures = 0;
static void expect(bool ok, const char* what) {
  if (!ok) { ++failures; printf("FAILED: %s\n", what); }
}
static bool counts_are(const Out& o, std::vector<long> head) {
  for (size_t i = 0; i < 16; ++i) if (o.counts[i] != (i < head.size() ? head[i] : 0)) return false;
  return true;
}

int main() {
  const std::vector<Edge> minimal = {{0, 2, 0.9f}, {2, 1, 0.6f}};
  const std::vector<int> im3 = {0, 0, 1}, t3 = {0, 0, 0};
  {
    Out o = run(minimal, im3, t3, {0}, 2);
    expect(o.status == 0 && o.id == std::vector<int>({0, -1, 0}) && o.state == std::vector<uint8_t>({1, 2}) && o.len[0] == 2 && o.rounds[0] == 1 &&
           o.rounds[1] == 0 && counts_are(o, {1, 0, 0, 1, 1, 0, 1, 3, 2, 1, 2}), "minimal");
    o = run({minimal[1], minimal[0]}, im3, t3, {0}, 2);
    expect(o.status == 0 && o.id == std::vector<int>({0, -1, 0}) && o.state == std::vector<uint8_t>({2, 1}), "minimal, weaker edge first");
    o = run(minimal, im3, t3, {0}, 2, 3);
    expect(o.status == 0 && o.id == std::vector<int>({-1, -1, -1}) && counts_are(o, {0, 0, 0, 1, 1, 0, 1, 3, 0, 1, 2}), "min_track_len 3");
    o = run(minimal, im3, t3, {0}, 2, 1);
    expect(o.status == 0 && o.id == std::vector<int>({0, 1, 0}) && o.len[1] == 1 && o.counts[0] == 2 && o.counts[8] == 3, "min_track_len 1");
    o = run(minimal, im3, t3, {0}, 2, 2, 0);
    expect(o.status == 0 && o.id == std::vector<int>({-1, -1, -1}) && o.state == std::vector<uint8_t>({3, 3}) && counts_are(o, {0, 0, 0, 0, 0, 2, 1, 3, 0, 0, 1}),
           "max_rounds 0");
    o = run(minimal, im3, t3, {1}, 2);
    expect(o.status == 0 && o.id == std::vector<int>({0, 0, 0}) && counts_are(o, {1, 0, 2}), "a track marked consistent is frozen");
    o = run({minimal[0], minimal[0], minimal[1]}, im3, t3, {0}, 2);
    expect(o.status == 0 && o.state == std::vector<uint8_t>({1, 1, 2}) && o.rounds[0] == 1, "a duplicated edge");
  }
  {
    Out o = run({{0, 2, 0.5f}, {2, 3, 0.5f}, {3, 1, 0.5f}}, {0, 0, 1, 2}, {0, 0, 0, 0}, {0}, 3);
    expect(o.status == 0 && o.id == std::vector<int>({0, -1, 0, 0}) && o.state == std::vector<uint8_t>({1, 1, 2}) && o.rounds[0] == 1 && o.rounds[1] == 1 &&
           o.rounds[2] == 0 && counts_are(o, {1, 0, 0, 2, 1, 0, 1, 4, 3, 2, 3}), "ties go to the lower edge");
  }
  {
    std::vector<Edge> chain = {{0, 2, 0.95f}};
    std::vector<int> images = {0, 0};
    for (int k = 2; k < 10; ++k) chain.push_back({k, k + 1, 0.95f - 0.05f * (float)(k - 1)});
    chain.push_back({10, 1, 0.3f});
    for (int i = 1; i < 10; ++i) images.push_back(i);
    const std::vector<int> tracks(11, 0);
    Out o = run(chain, images, tracks, {0}, 10);
    expect(o.status == 0 && counts_are(o, {1, 0, 0, 9, 1, 0, 1, 11, 10, 9, 10}) && o.id[1] == -1 && o.id[10] == 0 && o.rounds[8] == 1 && o.rounds[9] == 0,
           "the descending chain takes 9 rounds");
    o = run(chain, images, tracks, {0}, 10, 2, 3);
    expect(o.status == 0 && counts_are(o, {1, 0, 0, 3, 0, 7, 1, 11, 4, 3, 4}) && o.id[4] == 0 && o.id[5] == -1, "the chain after 3 rounds is open");
    o = run(chain, images, tracks, {0}, 10, 2, 0);
    expect(o.status == 0 && counts_are(o, {0, 0, 0, 0, 0, 10, 1, 11, 0, 0, 1}), "the chain without a round");
  }
  {
    const std::vector<Edge> mixed = {{0, 4, 0.9f}, {4, 9, 0.9f}, {1, 5, 0.8f}, {5, 2, 0.7f}, {3, 6, 0.6f}, {7, 10, 0.5f}, {7, 11, 0.5f}, {8, 12, 0.4f}, {6, 8, 0.3f},
                                     {13, 12, 0.2f}};
    const std::vector<int> images = {0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2}, tracks = {0, 1, 1, 2, 0, 1, 2, 3, 4, 0, 3, 3, 4, -1};
    Out o = run(mixed, images, tracks, {1, 0, 1, 0, 1}, 3);
    expect(o.status == 0 && o.id == std::vector<int>({0, 1, -1, 2, 0, 1, 2, 3, 4, 0, 3, -1, 4, -1}) &&
           o.state == std::vector<uint8_t>({0, 0, 1, 2, 0, 1, 2, 0, 0, 0}) && counts_are(o, {5, 0, 6, 2, 2, 0, 2, 6, 4, 1, 2}), "mixed");
  }
  {
    Out o = run({}, im3, t3, {0}, 2);
    expect(o.status == 0 && counts_are(o, {0, 0, 0, 0, 0, 0, 1, 3, 0, 0, 1}), "E = 0");
    o = run({{0, 1, 0.5f}}, {0, 1}, {-1, -1}, {}, 2);
    expect(o.status == 0 && o.id == std::vector<int>({-1, -1}) && counts_are(o, {0, 0, 1}), "T = 0");
    o = run({}, {}, {}, {}, 0);
    expect(o.status == 0 && counts_are(o, {}), "K = 0");
    o = run({{0, 0, 0.5f}, {0, 1, 0.4f}}, {0, 1}, {0, 0}, {0}, 2);
    expect(o.status == 0 && o.id == std::vector<int>({0, 0}) && o.state == std::vector<uint8_t>({1, 1}), "a self edge is internal");
  }
  {
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    expect(run({{0, 3, 0.9f}, {2, 1, 0.6f}}, im3, t3, {0}, 2).counts[1] == 1 && run({{0, 2, 0.9f}, {-1, 1, 0.6f}}, im3, t3, {0}, 2).counts[1] == 1, "bit 1");
    expect(run(minimal, im3, {0, 1, 0}, {0}, 2).counts[1] == 2 && run(minimal, im3, {0, -2, 0}, {0}, 2).counts[1] == 2 &&
           run(minimal, {0, 0, 2}, t3, {0}, 2).counts[1] == 2 && run(minimal, {-1, 0, 1}, t3, {0}, 2).counts[1] == 2, "bit 2");
    expect(run(minimal, {0, 1, 0}, t3, {0}, 2).counts[1] == 4, "bit 4");
    expect(run({{0, 2, nan}, {2, 1, 0.6f}}, im3, t3, {0}, 2).counts[1] == 8 && run({{0, 2, 0.9f}, {2, 1, inf}}, im3, t3, {0}, 2).counts[1] == 8 &&
           run({{0, 2, -0.1f}, {2, 1, 0.6f}}, im3, t3, {0}, 2).counts[1] == 8, "bit 8");
    Out o = run({{0, 7, nan}, {2, 1, 0.6f}}, {1, 0, 5}, {0, 9, 0}, {0}, 2);
    expect(o.status == LOFTR_ERR_BAD_ARG && counts_are(o, {0, 15}), "every bit at once");
    expect(run({{0, 0, 0.5f}}, {}, {}, {}, 0).counts[1] == 1, "edges without keypoints");
  }
  {                                                                          // a seeded random graph: every numbered track visits an image once
    uint64_t s = 88172645463325252ull;
    auto rnd = [&s](int n) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (int)(s % (uint64_t)n); };
    const int K = 600, E = 900, n = 12;
    std::vector<int> images(K), tracks(K);
    for (int k = 0; k < K; ++k) { images[k] = k * n / K; tracks[k] = k % 7; }
    std::vector<Edge> edges;
    for (int e = 0; e < E; ++e) edges.push_back({rnd(K), rnd(K), 0.25f * (float)(1 + rnd(3))});
    Out o = run(edges, images, tracks, {0, 0, 1, 0, 0, 1, 0}, n);
    bool once = o.status == 0;
    std::vector<std::vector<int>> seen((size_t)(o.status == 0 ? o.counts[0] : 0), std::vector<int>(n, 0));
    for (int k = 0; once && k < K; ++k)
      if (o.id[k] >= 0 && tracks[k] != 2 && tracks[k] != 5 && ++seen[(size_t)o.id[k]][images[k]] > 1) once = false;
    expect(once && o.counts[5] == 0, "a random graph: consistent tracks, no open edge");
  }
  {                                                                          // the walks on lists that no valid input produces
    const int n = 3;
    std::vector<int> next = {1, 2, 3, 4, -1, -1}, image = {0, 0, 0, 0, 0, 2}, label(6, 0);            // a list of five in image 0; one in image 2
    expect(split::shared_image(next.data(), image.data(), n, 0, 5) == -1, "a list longer than n_images is not followed");
    next = {1, 0, -1};                                                       // a cycle
    image = {0, 0, 2};
    expect(split::shared_image(next.data(), image.data(), 2, 0, 2) == -1, "a cyclic list ends the walk");
    next = {1, 0, -1};
    label = {0, 0, 2};
    expect(split::splice(next.data(), label.data(), 1, 0, 2) == -1, "a cyclic list ends the splice");
    next = {-1, -1, -1};
    label = {0, 1, 2};
    expect(split::splice(next.data(), label.data(), 3, 0, 2) == 2 && next == std::vector<int>({2, -1, -1}) && label == std::vector<int>({0, 1, 0}), "a splice of two");
    expect(split::splice(next.data(), label.data(), 3, 0, 1) == 3 && next == std::vector<int>({1, 2, -1}) && label == std::vector<int>({0, 0, 0}), "a splice in the middle");
  }
  printf(failures ? "%d FAILED\n" : "split host driver: all cases pass\n", failures);
  return failures != 0;
}
