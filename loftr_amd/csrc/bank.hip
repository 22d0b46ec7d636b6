// Feature banks: the two kernels that read backbone maps, with the batch index of the map replaced by a slot of a bank
// (one loftr_fmap holding the maps of many images, slot = batch index).  A pair list then runs the backbone once per image
// and matches pairs of slots (loftr_amd/pairs.py).  The per-element arithmetic is that of pos_encode_flatten_kernel
// (misc.hip) and gather_windows_kernel (fine.hip): a pair matched from a bank gives the bits of the same pair matched from
// stacked maps.  Those kernels are left as they are; this translation unit holds the slot-indexed copies.
//   Slot offsets are 64-bit ((long)slot * sn: a bank passes 2^31 elements at ~220 fine maps of 640 x 480).  A slot id
//   outside [0, n_slots) -- which the Python binding refuses before any launch -- reads nothing: its outputs are NaN.
//   The kernel names share no base name with a kernel of profiles/pmc_traffic.json: bench.py identifies that table's build by
//   the machine code of every kernel whose name contains one of its entries' base names.
#include "common.h"
#include "fine.h"

namespace {

__device__ __forceinline__ bool slot_ok(int slot, int n_slots) { return slot >= 0 && slot < n_slots; }

// out[r] = flatten(bank[slot_ids[r]] + pe): pos_encode_flatten_kernel with the map of output row r read from its slot.
//   grid (ceil(HW/32), ceil(C/32), n), block (32, 8)
template <bool CL>
__global__ void bank_posenc_kernel(loftr_fmap f, int n_slots, const int32_t* __restrict__ slot_ids,
                                   const float* __restrict__ pe, int pe_h, int pe_w, float* __restrict__ out, int C) {
  __shared__ float tile[32][33];
  const int H = f.H, W = f.W, HW = H * W;
  const int n = blockIdx.z, hw0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int slot = slot_ids[n];
  const bool ok = slot_ok(slot, n_slots);
  const float* in = f.data + (ok ? (long)slot * f.sn : 0L);
  for (int k = threadIdx.y; k < 32; k += 8) {
    const int c = c0 + k, hw = hw0 + threadIdx.x;
    float v = 0.f;
    if (c < C && hw < HW) {
      const int y = hw / W, x = hw - y * W;
      v = pe[((long)c * pe_h + y) * pe_w + x];
      if (!CL && ok) v += in[(long)c * f.sc + (long)y * f.sh + (long)x * f.sw];
    }
    tile[k][threadIdx.x] = v;
  }
  __syncthreads();
  for (int k = threadIdx.y; k < 32; k += 8) {
    const int hw = hw0 + k, c = c0 + threadIdx.x;
    if (hw < HW && c < C) {
      float v = tile[threadIdx.x][k];
      if (CL && ok) { const int y = hw / W, x = hw - y * W; v += in[(long)y * f.sh + (long)x * f.sw + c]; }
      out[((long)n * HW + hw) * C + c] = ok ? v : __builtin_nanf("");
    }
  }
}

// gather_windows_kernel with the fine map of pair b read from bank slot slot0[b] / slot1[b] (b = b_ids[m], pair-local).
//   grid (M, 2), Cf threads (Cf even, a multiple of 32).
__global__ void bank_windows_kernel(loftr_fmap f0, loftr_fmap f1, int n_slots0, int n_slots1,
                                    const int32_t* __restrict__ slot0, const int32_t* __restrict__ slot1,
                                    const int64_t* __restrict__ b_ids, const int64_t* __restrict__ i_ids,
                                    const int64_t* __restrict__ j_ids, int M, int w0c, int w1c, int stride, int W, int Cf,
                                    sp_t* __restrict__ win0, sp_t* __restrict__ win1) {
  const int m = blockIdx.x, side = blockIdx.y;
  const loftr_fmap f = side ? f1 : f0;
  const int wc = side ? w1c : w0c;
  const long cell = side ? j_ids[m] : i_ids[m];
  const long b = b_ids[m];
  const int slot = (side ? slot1 : slot0)[b];
  const bool ok = slot_ok(slot, side ? n_slots1 : n_slots0);
  const int cy = (int)(cell / wc) * stride, cx = (int)(cell % wc) * stride;
  const int r = W / 2;
  sp_t* out = (side ? win1 : win0) + (long)m * W * W * Cf;
  for (int c = threadIdx.x; c < Cf; c += blockDim.x) {
    const float* base = f.data + (ok ? (long)slot * f.sn : 0L) + (long)c * f.sc;
    for (int wy = 0; wy < W; ++wy) {
      const int y = cy + wy - r;
      for (int wx = 0; wx < W; ++wx) {
        const int x = cx + wx - r;
        float v = ok ? 0.f : __builtin_nanf("");
        if (ok && y >= 0 && y < f.H && x >= 0 && x < f.W) v = base[(long)y * f.sh + (long)x * f.sw];
        sp_store(out + (wy * W + wx) * Cf, c, v, true);
      }
    }
  }
}

struct SlotWindows {
  loftr_fmap f0, f1; int n_slots0, n_slots1; const int32_t *slot0, *slot1;
  const int64_t *b_ids, *i_ids, *j_ids; int M, w0c, w1c, stride, W, Cf;
};
int launch_slot_windows(const void* ctx, sp_t* win0, sp_t* win1, hipStream_t st) {
  const SlotWindows& a = *(const SlotWindows*)ctx;
  hipLaunchKernelGGL(bank_windows_kernel, dim3(a.M, 2), dim3(a.Cf < 64 ? 64 : a.Cf), 0, st, a.f0, a.f1, a.n_slots0, a.n_slots1,
                     a.slot0, a.slot1, a.b_ids, a.i_ids, a.j_ids, a.M, a.w0c, a.w1c, a.stride, a.W, a.Cf, win0, win1);
  return LOFTR_OK;
}

}  // namespace

extern "C" int loftr_pos_encode_flatten_gather(const loftr_fmap* bank, int n_slots, const int32_t* slot_ids, int n,
                                               const float* pe, int pe_h, int pe_w, float* out, int C, void* stream) {
  LOFTR_CHECK_ARG(n >= 0);
  if (n == 0) return LOFTR_OK;
  LOFTR_CHECK_ARG(bank && bank->data && slot_ids && pe && out && n_slots > 0 && C > 0 && bank->H > 0 && bank->W > 0 &&
                  bank->H <= pe_h && bank->W <= pe_w);
  const dim3 grid(ceil_div(bank->H * bank->W, 32), ceil_div(C, 32), n), block(32, 8);
  if (bank->sc == 1)
    hipLaunchKernelGGL((bank_posenc_kernel<true>), grid, block, 0, (hipStream_t)stream, *bank, n_slots, slot_ids, pe,
                       pe_h, pe_w, out, C);
  else
    hipLaunchKernelGGL((bank_posenc_kernel<false>), grid, block, 0, (hipStream_t)stream, *bank, n_slots, slot_ids, pe,
                       pe_h, pe_w, out, C);
  LOFTR_CHECK_LAUNCH();
  return LOFTR_OK;
}

extern "C" int loftr_fine_preprocess_gather(const loftr_fmap* bank_f0, int n_slots0, const int32_t* slot0,
                                            const loftr_fmap* bank_f1, int n_slots1, const int32_t* slot1,
                                            const float* feat_c0, const float* feat_c1, int L, int S, int Cc,
                                            const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids,
                                            int M, int w0c, int w1c, int stride, int W, int Cf,
                                            const float* down_w, const float* down_b, const float* merge_w,
                                            const float* merge_b, float* out0, float* out1, void* ws,
                                            size_t ws_bytes, void* stream) {
  LOFTR_CHECK_ARG(M >= 0);
  if (M == 0) return LOFTR_OK;
  LOFTR_CHECK_ARG(bank_f0 && bank_f1 && bank_f0->data && bank_f1->data && slot0 && slot1 && n_slots0 > 0 && n_slots1 > 0);
  LOFTR_CHECK_ARG(b_ids && i_ids && j_ids && out0 && out1);
  LOFTR_CHECK_ARG(w0c > 0 && w1c > 0 && stride > 0 && W > 0 && (W & 1) && Cf > 0 && Cf <= 1024);
  const SlotWindows sw{*bank_f0, *bank_f1, n_slots0, n_slots1, slot0, slot1, b_ids, i_ids, j_ids, M, w0c, w1c, stride, W, Cf};
  return fine_preprocess_run(WindowGather{launch_slot_windows, &sw}, feat_c0, feat_c1, L, S, Cc, b_ids, i_ids, j_ids, M, W, Cf,
                             down_w, down_b, merge_w, merge_b, out0, out1, ws, ws_bytes, (hipStream_t)stream);
}
