// Track splitting (consistent tracks grown again inside the components that visit an image twice): what the host routine (split.hip)
// and the kernels (split_gpu.hip) share.  Everything here is integer, compiled from this one text for both sides, so host and device
// take identical decisions.  The rule is stated in include/loftr_hip.h and DESIGN §24:
//   * the checks of an edge and of a keypoint, and the error bits a failed check raises;
//   * which edges are open (both ends in ONE track that visits an image twice);
//   * a component is a singly linked list of its keypoints in ascending index (`next`, -1 ends it), whose head is its label; kp_image
//     does not descend, so the list ascends by image as well;
//   * the walk of two lists in step that finds a shared image, and the splice of two disjoint lists into one;
//   * the word of a candidate is atlas_core.h's `conf_bits << 32 | (0xFFFFFFFF - e)`: ONE unsigned 64-bit max picks "greatest
//     confidence, then lowest edge"; 0 is the empty entry.
// Every walk is bounded by n_images + 1 steps on each side: a list that is longer (which no valid input produces) raises kTooLong
// instead of being followed.
#pragma once
#include "atlas_core.h"

namespace split {

constexpr int kCounts = 16;
enum Count { kTracks = 0, kErrors = 1, kIgnoredEdges = 2, kInternalEdges = 3, kConflictEdges = 4, kOpenEdges = 5, kBadTracks = 6,
             kBadKeypoints = 7, kRescued = 8, kRounds = 9, kLargest = 10 };
enum : int { kBadEdge = 1, kBadKeypoint = 2, kDescends = 4, kBadConf = 8, kTooLong = 16 };       // error bits
enum State : uint8_t { kIgnored = 0, kInternal = 1, kConflict = 2, kOpen = 3 };                   // of an edge
constexpr unsigned kNoKeypoint = 0xFFFFFFFFu;    // the empty entry of the per-track minimum

// sizes the routines index with int and pack into the word
ATLAS_HD bool sizes_ok(long E, long K, long T, int n_images, int max_rounds) {
  return E >= 0 && K >= 0 && T >= 0 && n_images >= 0 && max_rounds >= 0 && E <= atlas::kMaxMatches && K < (1L << 31) && T < (1L << 31) &&
         max_rounds < (1 << 20);
}

// the error bits of edge e; reads nothing through a bad value
ATLAS_HD int check_edge(const int* edge_kp, const float* edge_conf, long K, long e) {
  int err = 0;
  const int u = edge_kp[2 * e], v = edge_kp[2 * e + 1];
  if (u < 0 || u >= K || v < 0 || v >= K) err |= kBadEdge;
  const float c = edge_conf[e];
  if (!atlas::is_finite(c) || !(c >= 0.f)) err |= kBadConf;
  return err;
}

// the error bits of keypoint k
ATLAS_HD int check_keypoint(const int* kp_image, const int* track_id, long T, int n_images, long k) {
  int err = 0;
  const int i = kp_image[k], t = track_id[k];
  if (t < -1 || t >= T || i < 0 || i >= n_images) err |= kBadKeypoint;
  if (k > 0 && kp_image[k - 1] > i) err |= kDescends;
  return err;
}

// keypoint k belongs to a track that visits an image twice (checked tables)
ATLAS_HD bool is_free(const int* track_id, const uint8_t* track_ok, long k) {
  const int t = track_id[k];
  return t >= 0 && track_ok[t] == 0;
}

// step 1: edge e is open (checked tables)
ATLAS_HD bool edge_open(const int* edge_kp, const int* track_id, const uint8_t* track_ok, long e) {
  const int u = edge_kp[2 * e], v = edge_kp[2 * e + 1];
  return track_id[u] == track_id[v] && is_free(track_id, track_ok, u);
}

// step 3, propose: the lists headed a and b share an image -> 1, share none -> 0, one of them is longer than n_images -> -1.
// Two equal heads share an image, as do two keypoints of one image.
ATLAS_HD int shared_image(const int* next, const int* kp_image, int n_images, int a, int b) {
  int steps_a = 0, steps_b = 0;
  while (a >= 0 && b >= 0) {
    const int ia = kp_image[a], ib = kp_image[b];
    if (ia == ib) return 1;
    if (ia < ib) {
      a = next[a];
      if (++steps_a > n_images) return -1;
    } else {
      b = next[b];
      if (++steps_b > n_images) return -1;
    }
  }
  return 0;
}

// step 3, merge: the disjoint lists headed lo < hi become one list in ascending keypoint index, headed lo, and every member takes
// the label lo -> the members of the list, or -1 when it is longer than 2 n_images + 1 (nothing is followed further).  Touches only
// the members of the two lists.
ATLAS_HD int splice(int* next, int* label, int n_images, int lo, int hi) {
  const long bound = 2L * n_images + 1;
  int a = next[lo], b = hi, tail = lo, members = 1;
  label[lo] = lo;
  while (a >= 0 || b >= 0) {
    const bool take_a = b < 0 || (a >= 0 && a < b);
    const int k = take_a ? a : b;
    if (take_a) a = next[a]; else b = next[b];
    next[tail] = k;
    label[k] = lo;
    tail = k;
    if (++members > bound) { next[tail] = -1; return -1; }
  }
  next[tail] = -1;
  return members;
}

}  // namespace split
