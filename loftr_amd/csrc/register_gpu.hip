// The correspondence table of the unposed images on the GPU: loftr_register_corr_host (register.hip) with the same result bit for bit
// (DESIGN §19).  Every per-item step is register_core.h's, compiled from the same text; what this file adds is only how the work is
// spread over threads:
//   a thread per track      offset checks, obs_track and the correspondence flag of each of its observations;
//   a wave per image        the grouping check and n_corr: ballot / popcount over the image's list in steps of 64;
//   one workgroup           the candidates' ranks and offsets: the images in blocks of kRankBlock with a carry, an exclusive scan per block;
//   a wave per image        the rows of a candidate: its list again in steps of 64, lane position = running base + the number of set
//                           ballot bits below the lane.
// A fixed launch schedule on the caller's stream: no readback, no grid-wide barrier, no persistent or waiting kernel, no captured graph.
// No value that a kernel writes to device memory is read in the same kernel; the error word is raised with integer atomics by the first
// two kernels and only read by the last two.  Plain C++, ordinary vector stores.
#include "common.h"
#include "register_core.h"
#include "stage_timer.h"
#include "tracks_core.h"

namespace {

using namespace reg;

constexpr int kThreads = 256;
constexpr int kRankBlock = LOFTR_REGISTER_RANK_BLOCK;                            // images per step of reg_rank_kernel
constexpr int kRankWaves = kRankBlock / 64;
static_assert(kRankBlock % 64 == 0 && kRankBlock <= 1024, "reg_rank_kernel is one workgroup of whole waves");

__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// grid ceil(T / 256) x 256
__global__ void __launch_bounds__(kThreads) reg_track_kernel(Ctx c) {
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= c.T) return;
  const int err = track_flags(c, t);
  if (err) atomicOr(c.err, err);
}

// a wave per image, grid ceil(n / 4) x 256.  Reads the observation arrays only through checked indices, so it needs no flag; a flag
// byte that reg_track_kernel left unwritten (bad offsets) can only reach a count that the raised error bit voids.
__global__ void __launch_bounds__(kThreads) reg_count_kernel(Ctx c) {
  const long i = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (i >= c.n) return;                                                          // wave-uniform
  long b, e;
  int err = 0, cnt = 0;
  if (!group_range(c, i, &b, &e)) { err = kBadGroups; b = e = 0; }
  for (long k0 = b; k0 < e; k0 += 64) {
    const long k = k0 + lane;
    bool corr = false;
    if (k < e) err |= group_check(c, i, b, k, &corr);
    cnt += __popcll(__ballot(corr));
  }
  for (int m = 32; m >= 1; m >>= 1) err |= __shfl_xor(err, m, 64);
  if (lane == 0) {
    c.img_corr[i] = c.posed[i] ? 0 : cnt;
    if (err) atomicOr(c.err, err);
  }
}

// one workgroup of kRankBlock threads
__global__ void __launch_bounds__(kRankBlock) reg_rank_kernel(Ctx c) {
  __shared__ long s_p[kRankWaves], s_c[kRankWaves];
  __shared__ unsigned long long s_tot[3];
  __shared__ int s_max;
  const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64;
  const int err = *c.err;
  if (err) {                                                                     // uniform
    if (tid == 0) write_error(c, err);
    return;
  }
  if (tid < 3) s_tot[tid] = 0;
  if (tid == 3) s_max = 0;
  long carry_p = 0, carry_c = 0, unposed = 0, seen = 0, all = 0;
  int largest = 0;
  for (long base = 0; base < c.n; base += kRankBlock) {
    const long i = base + tid;
    int cnt = 0;
    bool cand = false;
    if (i < c.n) {
      cnt = c.img_corr[i];
      cand = candidate(c, i, cnt);
      unposed += c.posed[i] == 0;
      seen += c.posed[i] == 0 && cnt >= 1;
      all += cnt;
      largest = cnt > largest ? cnt : largest;
    }
    const unsigned long long m = __ballot(cand);
    const long mine = cand ? cnt : 0;
    long inc = mine;                                                             // inclusive scan over the wave
    for (int s = 1; s < 64; s <<= 1) {
      const long u = __shfl_up(inc, s, 64);
      if (lane >= s) inc += u;
    }
    if (lane == 63) { s_p[wave] = __popcll(m); s_c[wave] = inc; }
    __syncthreads();
    long p0 = carry_p, c0 = carry_c;
    for (int w = 0; w < kRankWaves; ++w) {
      if (w < wave) { p0 += s_p[w]; c0 += s_c[w]; }
      carry_p += s_p[w];
      carry_c += s_c[w];
    }
    if (i < c.n) {
      const long r = p0 + lanes_below(m, lane);
      c.n_corr[i] = cnt;
      c.cand_rank[i] = cand ? (int)r : -1;
      if (cand) { c.cand_image[r] = (int)i; c.cand_offsets[r] = c0 + inc - mine; }
    }
    __syncthreads();
  }
  __syncthreads();
  atomicAdd(&s_tot[0], (unsigned long long)unposed);
  atomicAdd(&s_tot[1], (unsigned long long)seen);
  atomicAdd(&s_tot[2], (unsigned long long)all);
  atomicMax(&s_max, largest);
  __syncthreads();
  if (tid == 0) {
    c.cand_offsets[carry_p] = carry_c;
    c.counts[0] = carry_c; c.counts[1] = carry_p; c.counts[2] = 0; c.counts[3] = (long)s_tot[0]; c.counts[4] = (long)s_tot[1];
    c.counts[5] = (long)s_tot[2]; c.counts[6] = s_max; c.counts[7] = 0;
  }
}

// a wave per image, grid ceil(n / 4) x 256
__global__ void __launch_bounds__(kThreads) reg_write_kernel(Ctx c) {
  const long i = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (i >= c.n || *c.err) return;                                                // wave-uniform
  const int r = c.cand_rank[i];
  if (r < 0) return;
  long row = c.cand_offsets[r];
  const long b = c.cam_offsets[i], e = c.cam_offsets[i + 1];
  for (long k0 = b; k0 < e; k0 += 64) {
    const long k = k0 + lane;
    const int o = k < e ? c.cam_obs[k] : 0;
    const bool corr = k < e && c.obs_corr[o] != 0;
    const unsigned long long m = __ballot(corr);
    if (corr) write_row(c, row + lanes_below(m, lane), r, o);
    row += __popcll(m);
  }
}

}  // namespace

extern "C" size_t loftr_register_corr_workspace_bytes(long T, long N, int n_images) {
  if (!tracks::sizes_ok(T, N, n_images)) return 0;
  Ctx c{};
  c.T = T; c.N = N; c.n = n_images;
  return layout(c, nullptr);
}

extern "C" int loftr_register_corr(const long* offsets, long T, const int* obs_image, const float* obs_xy, long N, const float* xyz,
                                   const uint8_t* status, const uint8_t* posed, int n_images, const long* cam_offsets, const int* cam_obs,
                                   int min_corr, int* n_corr, int* cand_rank, int* cand_image, long* cand_offsets, float* corr_xyz,
                                   float* corr_xy, long* corr_bid, int* corr_obs, long* counts, void* ws, size_t ws_bytes, float* stage_ms,
                                   void* stream) {
  LOFTR_CHECK_ARG(offsets && cam_offsets && cand_offsets && counts && ws && T >= 0 && N >= 0 && n_images >= 0);
  LOFTR_CHECK_ARG(T == 0 || (xyz && status));
  LOFTR_CHECK_ARG(N == 0 || (obs_image && obs_xy && cam_obs && corr_xyz && corr_xy && corr_bid && corr_obs));
  LOFTR_CHECK_ARG(n_images == 0 || (posed && n_corr && cand_rank && cand_image));
  LOFTR_CHECK_ARG(min_corr >= kMinCorr);
  LOFTR_CHECK_ARG((T > 0 && n_images > 0) || N == 0);                            // observations outside every track or image
  if (!tracks::sizes_ok(T, N, n_images)) return LOFTR_ERR_UNSUPPORTED;
  Ctx c{};
  c.offsets = offsets; c.T = T; c.image = obs_image; c.xy = obs_xy; c.N = N; c.xyz = xyz; c.status = status; c.posed = posed; c.n = n_images;
  c.cam_offsets = cam_offsets; c.cam_obs = cam_obs; c.min_corr = min_corr;
  c.n_corr = n_corr; c.cand_rank = cand_rank; c.cand_image = cand_image; c.cand_offsets = cand_offsets;
  c.corr_xyz = corr_xyz; c.corr_xy = corr_xy; c.corr_bid = corr_bid; c.corr_obs = corr_obs; c.counts = counts;
  if (ws_bytes < layout(c, nullptr)) return LOFTR_ERR_WORKSPACE;
  layout(c, (char*)ws);
  hipStream_t s = (hipStream_t)stream;
  StageTimer timer(stage_ms, LOFTR_REGISTER_STAGES, s);
  bool failed = false;
  auto after = [&]() {
    if (hipGetLastError() != hipSuccess) failed = true;
    timer.mark();
  };
  auto blocks = [](long items, long per) { return dim3((unsigned)(items > 0 ? (items + per - 1) / per : 1)); };
  if (hipMemsetAsync(c.err, 0, sizeof(int), s) != hipSuccess) return LOFTR_ERR_LAUNCH;
  timer.mark();
  hipLaunchKernelGGL(reg_track_kernel, blocks(T, kThreads), dim3(kThreads), 0, s, c); after();
  hipLaunchKernelGGL(reg_count_kernel, blocks(n_images, kThreads / 64), dim3(kThreads), 0, s, c); after();
  hipLaunchKernelGGL(reg_rank_kernel, dim3(1), dim3(kRankBlock), 0, s, c); after();
  hipLaunchKernelGGL(reg_write_kernel, blocks(n_images, kThreads / 64), dim3(kThreads), 0, s, c); after();
  const int timed = timer.finish();
  return failed ? LOFTR_ERR_LAUNCH : timed;
}
