// Stream compaction on the GPU (gfx950, wave64), shared by the keypoint atlas (atlas_gpu.hip) and the model lookup (model_lookup_gpu.hip):
// the block-level rank and scan, the open-addressing table of atlas_core.h's hash, and the one u32 scan (scan.hip) that turns per-block
// counts into offsets.  The device helpers are inlined into the kernels of the including file; every kernel that calls them runs kBlock
// threads per block.
#pragma once
#include "common.h"
#include "atlas_core.h"

namespace compact {

typedef unsigned long long u64;

constexpr int kBlock = 256;                 // threads per block of every kernel that uses these helpers
constexpr int kWaves = kBlock / 64;
constexpr int kScanItems = 4;               // elements per thread of the scan kernels: 1024 per block

// ---- block-level helpers (every thread of the block must call them) ----------------------------------------------------------------
// rank of this thread among the threads of the block with flag set, and the block's total
__device__ __forceinline__ unsigned block_rank(bool flag, unsigned* total) {
  __shared__ unsigned wsum[kWaves];
  const u64 b = __ballot(flag);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) wsum[w] = (unsigned)__popcll(b);
  __syncthreads();
  unsigned off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    if (i < w) off += wsum[i];
    tot += wsum[i];
  }
  __syncthreads();
  *total = tot;
  return off + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
}

// exclusive prefix sum of v over the block, and the block's total
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* total) {
  __shared__ unsigned wsum[kWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  unsigned off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    if (i < w) off += wsum[i];
    tot += wsum[i];
  }
  __syncthreads();
  *total = tot;
  return off + inc - v;
}

inline long blocks_of(long n) { return (n + kBlock - 1) / kBlock; }
inline long scan_blocks(long n) { return (n + (long)kBlock * kScanItems - 1) / ((long)kBlock * kScanItems); }

// the u32 scan (scan.hip): data[0, n) <- its exclusive prefix sums, *total <- the sum; partials [scan_blocks(n)]; n > 0
// -> LOFTR_OK or LOFTR_ERR_LAUNCH
int scan_u32(unsigned* data, long n, unsigned* partials, long* total, hipStream_t s);

// ---- the open-addressing table (keys / vals [cap] u64, cap a power of two at load <= 0.5, zero = empty) ---------------------------
// slot of `key`, claimed if absent.  The probe ends: the table always holds an empty slot.
__device__ __forceinline__ u64 table_claim(u64* __restrict__ keys, u64 mask, u64 key) {
  u64 h = atlas::hash64(key) & mask;
  for (;;) {
    const u64 prev = atomicCAS(&keys[h], 0ull, key);
    if (prev == 0ull || prev == key) return h;
    h = (h + 1) & mask;
  }
}
// value of `key` in a table that a previous kernel filled; 0 if absent
__device__ __forceinline__ u64 table_find(const u64* __restrict__ keys, const u64* __restrict__ vals, u64 mask, u64 key) {
  u64 h = atlas::hash64(key) & mask;
  for (u64 n = 0; n <= mask; ++n) {
    const u64 k = keys[h];
    if (k == key) return vals[h];
    if (k == 0ull) return 0ull;
    h = (h + 1) & mask;
  }
  return 0ull;
}

}  // namespace compact
