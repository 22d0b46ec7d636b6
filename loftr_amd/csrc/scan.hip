// The one u32 scan of the compaction stages (compact_gpu.h): reduce / scan / downsweep over blocks of kBlock * kScanItems elements.
// Integer adds only, so the result does not depend on any order.
#include "compact_gpu.h"

namespace {

using namespace compact;

__global__ void scan_reduce_kernel(const unsigned* __restrict__ data, long n, unsigned* __restrict__ partials) {
  const long base = ((long)blockIdx.x * kBlock + threadIdx.x) * kScanItems;
  unsigned v = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) v += base + j < n ? data[base + j] : 0u;
  unsigned tot;
  block_excl_scan(v, &tot);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}
// one block: partials[0, nb) <- exclusive prefix sums
__global__ void scan_partials_kernel(unsigned* __restrict__ partials, long nb, long* __restrict__ total) {
  unsigned carry = 0;
  for (long base = 0; base < nb; base += kBlock) {
    const long i = base + threadIdx.x;
    const unsigned v = i < nb ? partials[i] : 0u;
    unsigned tot;
    const unsigned ex = block_excl_scan(v, &tot);
    if (i < nb) partials[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = (long)carry;
}
__global__ void scan_down_kernel(unsigned* __restrict__ data, long n, const unsigned* __restrict__ partials) {
  const long base = ((long)blockIdx.x * kBlock + threadIdx.x) * kScanItems;
  unsigned x[kScanItems], v = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    x[j] = base + j < n ? data[base + j] : 0u;
    v += x[j];
  }
  unsigned tot;
  unsigned run = partials[blockIdx.x] + block_excl_scan(v, &tot);
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    if (base + j < n) data[base + j] = run;
    run += x[j];
  }
}

}  // namespace

int compact::scan_u32(unsigned* data, long n, unsigned* partials, long* total, hipStream_t s) {
  const long nb = scan_blocks(n);
  hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, data, n, partials);
  hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kBlock), 0, s, partials, nb, total);
  hipLaunchKernelGGL(scan_down_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, data, n, partials);
  LOFTR_CHECK_LAUNCH();
  return LOFTR_OK;
}
