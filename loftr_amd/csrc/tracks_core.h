// The track table shared by triangulation, bundle adjustment and registration: observations grouped into spans by
// an offsets array (tracks over `offsets`, images over `cam_offsets`), the checks every stage makes before it reads through one, and the
// error bits a failed check raises.  Integer work only, compiled from this one text for the host routines and the kernels, so the two
// sides of every stage reject the same tables.  What a stage does with a rejection stays its own: the triangulation host routine returns
// LOFTR_ERR_BAD_ARG, bundle adjustment and registration raise the bits in counts.
// register_core.h states the same checks itself: it is pinned to include no other *_core.h (tests/test_registration_abi.py), so of this
// header the registration uses only sizes_ok, from register_gpu.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TRACKS_HD __host__ __device__ static inline
#else
#define TRACKS_HD static inline
#endif

namespace tracks {

enum : int { kBadImage = 1, kBadOffsets = 2, kBadGroups = 4 };                   // error bits

// span t of `offsets` [T + 1] over N items -> [*b, *e); false unless 0 first, N last, ascending, inside [0, N]
TRACKS_HD bool span(const long* offsets, long T, long N, long t, long* b, long* e) {
  *b = offsets[t]; *e = offsets[t + 1];
  return !(*b < 0 || *e < *b || *e > N || (t == 0 && *b != 0) || (t == T - 1 && *e != N));
}

// every image id of the checked span [b, e) names one of n images
TRACKS_HD bool images_ok(const int* image, long b, long e, int n) {
  for (long o = b; o < e; ++o) if (image[o] < 0 || image[o] >= n) return false;
  return true;
}

// slot k of image i's list (which starts at slot b): *o = its observation, in [0, N), of image i and above the slot before it -> 0 or
// kBadGroups.  Reads nothing through a bad value.
TRACKS_HD int group_slot(const int* cam_obs, const int* image, long N, long i, long b, long k, int* o) {
  *o = cam_obs[k];
  if (*o < 0 || *o >= N) return kBadGroups;
  if (image[*o] != i) return kBadGroups;
  if (k > b && !(cam_obs[k - 1] < *o)) return kBadGroups;
  return 0;
}

// a table the stages index with int
TRACKS_HD bool sizes_ok(long T, long N, int n) { return T >= 0 && N >= 0 && n >= 0 && T < (1L << 31) && N < (1L << 31); }

// one step of carving a workspace: `bytes` at *off, which moves on to the next multiple of 256 -> where they start
TRACKS_HD size_t carve(size_t* off, size_t bytes) {
  const size_t at = *off;
  *off = (at + bytes + 255) / 256 * 256;
  return at;
}

}  // namespace tracks
