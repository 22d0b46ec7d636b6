// Track splitting, host routine (plain C++ on host arrays, integers only): inside every track that visits an image twice the keypoints
// start as components of one and are grown again along the kept matches, strongest first, never joining two components that share an
// image (the contract is in include/loftr_hip.h).  The constraint is the one incremental SfM pipelines keep while they
// build tracks; this is a statement of that idea as a round-based, order-defined rule, NOT of any pipeline's source.
// This function DEFINES the result: loftr_split_tracks (split_gpu.hip) reproduces it bit for bit, which is why every per-item step
// lives in split_core.h.  It is written as plain loops over the edges in order, one round after the other.
#include <stdint.h>
#include <vector>
#include "../../include/loftr_hip.h"
#include "split_core.h"

using namespace split;

extern "C" int loftr_split_tracks_host(const int* edge_kp, const float* edge_conf, long E, const int* kp_image, const int* track_id, long K,
                                       const uint8_t* track_ok, long T, int n_images, int min_track_len, int max_rounds, int* track_id_new,
                                       int* track_len_new, uint8_t* edge_state, int* round_accepted, long* counts) {
  if (!counts || E < 0 || K < 0 || T < 0 || n_images < 0 || min_track_len < 1 || max_rounds < 0) return LOFTR_ERR_BAD_ARG;
  if (E > 0 && (!edge_kp || !edge_conf || !edge_state)) return LOFTR_ERR_BAD_ARG;
  if (K > 0 && (!kp_image || !track_id || !track_id_new || !track_len_new)) return LOFTR_ERR_BAD_ARG;
  if ((T > 0 && !track_ok) || (max_rounds > 0 && !round_accepted)) return LOFTR_ERR_BAD_ARG;
  if (!sizes_ok(E, K, T, n_images, max_rounds)) return LOFTR_ERR_UNSUPPORTED;
  int err = 0;
  for (long e = 0; e < E; ++e) err |= check_edge(edge_kp, edge_conf, K, e);
  for (long k = 0; k < K; ++k) err |= check_keypoint(kp_image, track_id, T, n_images, k);
  for (int c = 0; c < kCounts; ++c) counts[c] = 0;
  counts[kErrors] = err;
  if (err) return LOFTR_ERR_BAD_ARG;

  // step 2: frozen labels (the smallest keypoint of a consistent track), components of one elsewhere, -1 outside every track
  std::vector<unsigned> track_min((size_t)T, kNoKeypoint);
  for (long k = 0; k < K; ++k)
    if (track_id[k] >= 0 && (unsigned)k < track_min[(size_t)track_id[k]]) track_min[(size_t)track_id[k]] = (unsigned)k;
  std::vector<int> label((size_t)K), next((size_t)K, -1);
  for (long k = 0; k < K; ++k) label[(size_t)k] = track_id[k] < 0 ? -1 : (track_ok[track_id[k]] ? (int)track_min[(size_t)track_id[k]] : (int)k);
  std::vector<uint8_t> state((size_t)E);
  for (long e = 0; e < E; ++e) state[(size_t)e] = edge_open(edge_kp, track_id, track_ok, e) ? kOpen : kIgnored;

  // step 3: the rounds
  std::vector<uint64_t> best((size_t)K);
  std::vector<long> accepted;
  std::vector<int> rounds((size_t)max_rounds, 0);
  for (int r = 0; r < max_rounds; ++r) {
    best.assign((size_t)K, 0);
    for (long e = 0; e < E; ++e) {                                                     // propose
      if (state[(size_t)e] != kOpen) continue;
      const int a = label[(size_t)edge_kp[2 * e]], b = label[(size_t)edge_kp[2 * e + 1]];
      if (a == b) { state[(size_t)e] = kInternal; continue; }
      const int shared = shared_image(next.data(), kp_image, n_images, a, b);
      if (shared < 0) { err |= kTooLong; continue; }
      if (shared) { state[(size_t)e] = kConflict; continue; }
      const uint64_t w = atlas::pack(edge_conf[e], (uint32_t)e);
      if (w > best[(size_t)a]) best[(size_t)a] = w;
      if (w > best[(size_t)b]) best[(size_t)b] = w;
    }
    if (err) break;
    accepted.clear();
    for (long e = 0; e < E; ++e) {                                                     // accept
      if (state[(size_t)e] != kOpen) continue;
      const uint64_t w = atlas::pack(edge_conf[e], (uint32_t)e);
      if (best[(size_t)label[(size_t)edge_kp[2 * e]]] == w && best[(size_t)label[(size_t)edge_kp[2 * e + 1]]] == w) accepted.push_back(e);
    }
    for (long e : accepted) {                                                          // merge
      const int a = label[(size_t)edge_kp[2 * e]], b = label[(size_t)edge_kp[2 * e + 1]];
      if (splice(next.data(), label.data(), n_images, a < b ? a : b, a < b ? b : a) < 0) err |= kTooLong;
      state[(size_t)e] = kInternal;
    }
    rounds[(size_t)r] = (int)accepted.size();
    if (err || accepted.empty()) break;
  }
  if (err) {
    counts[kErrors] = err;
    return LOFTR_ERR_BAD_ARG;
  }

  // step 5: numbering, as rule 4 of the atlas: the labels with at least min_track_len members in ascending label
  std::vector<int> len((size_t)K, 0), number((size_t)K, -1);
  for (long k = 0; k < K; ++k) if (label[(size_t)k] >= 0) ++len[(size_t)label[(size_t)k]];
  long tracks = 0;
  for (long k = 0; k < K; ++k) {
    if (label[(size_t)k] != (int)k || len[(size_t)k] < min_track_len) continue;
    number[(size_t)k] = (int)tracks;
    track_len_new[tracks++] = len[(size_t)k];
  }
  for (long k = 0; k < K; ++k) {
    if (is_free(track_id, track_ok, k) && label[(size_t)k] == (int)k && len[(size_t)k] > counts[kLargest]) counts[kLargest] = len[(size_t)k];
    const int l = label[(size_t)k];
    track_id_new[k] = l >= 0 && len[(size_t)l] >= min_track_len ? number[(size_t)l] : -1;
    if (is_free(track_id, track_ok, k)) {
      ++counts[kBadKeypoints];
      counts[kRescued] += track_id_new[k] >= 0;
    }
  }
  for (long k = tracks; k < K; ++k) track_len_new[k] = 0;
  for (long e = 0; e < E; ++e) {
    edge_state[e] = state[(size_t)e];
    ++counts[kIgnoredEdges + state[(size_t)e]];
  }
  for (long t = 0; t < T; ++t) counts[kBadTracks] += track_ok[t] == 0;
  for (int r = 0; r < max_rounds; ++r) {
    round_accepted[r] = rounds[(size_t)r];
    counts[kRounds] += rounds[(size_t)r] > 0;
  }
  counts[kTracks] = tracks;
  return LOFTR_OK;
}
