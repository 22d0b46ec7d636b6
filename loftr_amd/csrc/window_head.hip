// The last convolution of the FPN fine head (3x3 / stride 1 / pad 1, no BatchNorm, no activation: resnet_fpn.py:66-77, the
// second conv3x3 of layer1_outconv2) evaluated ONLY at the W x W fine windows of the matched coarse cells.
//   reference: src/loftr/backbone/resnet_fpn.py:113-116 (x1_out), src/loftr/loftr_module/fine_preprocess.py:40-47 (the unfold rows kept)
//
// The fine map has one consumer in the inference forward, the window gather of FinePreprocess: M matches keep 2 M x 25 of its
// pixels (25 % at the bench's 765 matches per 640 x 480 pair).  Here the implicit GEMM of conv3x3_duo.h runs with a packed list
// of window pixels as its M dimension instead of an 8 x 32 image tile, and its epilogue writes the SP window rows [M, 25, Cout]
// that the merge_feat GEMM consumes -- no fp32 fine map, no gather launch.
//
// Same arithmetic as the dense kernel, so the same bits: v_mfma_f32_32x32x16_f16 on zero accumulators, k order (channel group,
// half, tap column kx, tap row ky), the three products in the order lo.hi, hi.lo, hi.hi, the all-padding second half of the last
// channel group skipped (Cin = 196: 13 half steps), the dense epilogue's expression, then gather_windows_kernel's SP encoding.
// An output element's sum does not depend on the tile row it sits in: the windows equal a gather of the dense map bit for bit
// (tests/test_hip_window_head.py).
//
// Tiling.  A workgroup of 4 waves owns 128 tile rows = 5 windows x 25 pixels, packed densely (125 of 128 rows; window
// w = side * M + m).  Wave v owns tile rows 32 v .. 32 v + 31 and all four 32-column tiles.  Per window the
// (W+2)^2 = 7 x 7 input patch is staged in LDS per half channel group (64-byte rows, chunk swizzle and double buffer as in
// conv3x3_duo.h; rows outside the image come from the zero page); the A fragment of a lane is its pixel's patch row plus the
// tap's constant row offset ky * 7 + kx.  Weight ring (one tap x one 16-wide k-step per stage, NB stages, NB - 1 ahead), one
// barrier per step and the vmcnt bookkeeping are those of the dense kernel.
#include "conv_prepared.h"
#include "fine.h"

namespace whead {

constexpr int WIN = 5, WP = WIN + 2, WW = WIN * WIN, PP = WP * WP;       // window side, patch side, pixels of each
constexpr int NT = 4, NB = 4, LA = NB - 1;                                // 32-column tiles, weight ring stages, stages in flight

constexpr int WV = 4, ROWS = WV * 32, NWIN = ROWS / WW;                   // waves, tile rows, windows of a workgroup
constexpr int PROWS = NWIN * PP, PSLOTS = (PROWS + 15) / 16, PQ = PSLOTS / WV;   // 1 KB DMA slots (16 rows) of a patch half; per wave
constexpr int PHALF_BYTES = PSLOTS * 1024;
constexpr int BSLOTS = NT * 32 / 16, BQ = BSLOTS / WV, BSTAGE_BYTES = BSLOTS * 1024;
constexpr int TAB_OFF = 2 * PHALF_BYTES + NB * BSTAGE_BYTES;
constexpr int LDS_BYTES = TAB_OFF + ROWS * 8;                             // row table: output offset, flags
static_assert(PSLOTS % WV == 0 && BSLOTS % WV == 0, "every wave issues the same number of DMA slots (vmcnt bookkeeping)");
static_assert(LDS_BYTES * 2 <= 160 * 1024, "two workgroups per CU");

struct WinHeadArgs {
  const sp_t* x0; const sp_t* x1;         // [N, H, W, Cp] SP: output of the head's first convolution for the image0 / image1 batch
  int H, W, Cp, Cin;
  const sp_t* w; int K;                   // [Cout, 9 * Cp] SP (prepared filter)
  const float* bias; const float* wscale;
  const sp_t* zeros;
  const int64_t* b_ids; const int64_t* i_ids; const int64_t* j_ids;
  int M, w0c, w1c, stride;
  int Cout;                               // ceil32(Cout) == NT * 32
  int act;                                // 0 none (this layer), 1 ReLU, 2 LeakyReLU(0.01)
  sp_t* win0; sp_t* win1;                 // [M, 25, NT * 32] SP
};

// Window w of the launch (w = side * M + m): top-left pixel of its 5 x 5 window in the fine map, image index and side.
struct WinPos { int b, y0, x0, side; };
__device__ __forceinline__ WinPos window_pos(const WinHeadArgs& p, int w) {
  const int side = w >= p.M ? 1 : 0, m = w - side * p.M;
  const long cell = side ? p.j_ids[m] : p.i_ids[m];
  const int wc = side ? p.w1c : p.w0c;
  WinPos o;
  o.b = (int)p.b_ids[m];
  o.y0 = (int)(cell / wc) * p.stride - WIN / 2;
  o.x0 = (int)(cell % wc) * p.stride - WIN / 2;
  o.side = side;
  return o;
}

__global__ __launch_bounds__(WV * 64, 2) void window_head_kernel(WinHeadArgs p) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef const __attribute__((address_space(1))) void* gbl_ptr_t;
  __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];
  char* const patch_base = lds;
  char* const bring_base = lds + 2 * PHALF_BYTES;
  int* const row_off = reinterpret_cast<int*>(lds + TAB_OFF);      // dword offset of the tile row's window pixel in win0 / win1, -1: no such row
  int* const row_flag = row_off + ROWS;                            // bit 0: side, bit 1: the pixel lies inside the map

  const int tile = blockIdx.x, nwin = 2 * p.M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 5, tx = lane & 31;
  const int drow = lane >> 2, dpos = lane & 3;                  // DMA: row inside a 16-row slot, 16-B position inside the 64-B row

  // ---- row table: tile row r = (window r / 25 of the tile, pixel r % 25 of the window)
  if (tid < ROWS) {
    const int wl = tid / WW, px = tid - wl * WW, w = tile * NWIN + wl;
    int off = -1, flag = 0;
    if (wl < NWIN && w < nwin) {
      const WinPos wp = window_pos(p, w);
      const int y = wp.y0 + px / WIN, x = wp.x0 + px % WIN;
      const bool in = (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
      off = ((w - wp.side * p.M) * WW + px) * (NT * 32);
      flag = wp.side | (in ? 2 : 0);
    }
    row_off[tid] = off;
    row_flag[tid] = flag;
  }

  // ---- DMA source offsets (dwords): the chunk a lane fetches is fixed by (row, position); half / group / tap are added at issue
  int poff[PQ];                                                 // -1: outside the image / no such window / unused slot -> zero page
  unsigned pside = 0;                                           // bit q: patch row q of this lane reads x1
#pragma unroll
  for (int q = 0; q < PQ; ++q) {
    const int s_ = q * WV + wave, r = s_ * 16 + drow;
    const int wl = r / PP, rem = r - wl * PP, py = rem / WP, px = rem - py * WP;
    const int w = tile * NWIN + wl;
    const bool live = r < PROWS && w < nwin;
    const WinPos wp = window_pos(p, live ? w : 0);
    const int gy = wp.y0 - 1 + py, gx = wp.x0 - 1 + px;
    const int c = dpos ^ ((r >> 2) & 3);
    const bool in = live && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
    poff[q] = in ? ((wp.b * p.H + gy) * p.W + gx) * p.Cp + (((c & 1) + ((c >> 1) << 2)) << 2) : -1;
    pside |= (unsigned)wp.side << q;
  }
  int boff[BQ];
#pragma unroll
  for (int q = 0; q < BQ; ++q) {
    const int r = (q * WV + wave) * 16 + drow;
    const int c = dpos ^ ((r >> 2) & 3);
    boff[q] = min(r, p.Cout - 1) * p.K + (((c & 1) + ((c >> 1) << 2)) << 2);      // rows >= Cout: clamped copies (never stored)
  }
  const int gpt = p.Cp >> 5;
  // channels >= Cin of the last group are zero padding (activations AND folded weights): when they fill its whole second k-step
  // that half is skipped -- exact, and the rule of the dense kernel
  const int nhalf = 2 * gpt - (p.Cin <= (gpt - 1) * 32 + 16 ? 1 : 0), ns = nhalf * 9;

#define WH_ISSUE_PATCH(q_)                                                                                  \
  {                                                                                                         \
    const sp_t* xa__ = p.x0;                                                                                \
    const sp_t* xb__ = p.x1;                                                                                \
    asm volatile("" : "+s"(xa__), "+s"(xb__));                                                              \
    const int ko__ = ((q_) >> 1) * 32 + ((q_) & 1) * 8;                                                     \
    char* dst__ = patch_base + ((q_) & 1) * PHALF_BYTES;                                                \
    _Pragma("unroll") for (int q = 0; q < PQ; ++q) {                                                        \
      const sp_t* g__ = poff[q] >= 0 ? (((pside >> q) & 1u) ? xb__ : xa__) + (poff[q] + ko__) : p.zeros;    \
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)g__, (lds_ptr_t)(dst__ + (q * WV + wave) * 1024), 16, 0, 0); \
    }                                                                                                       \
  }
  // weight stage of step (half q_, index i_ = kx * 3 + ky inside the half): tap ky * 3 + kx
#define WH_ISSUE_B(q_, i_, stage_)                                                                          \
  {                                                                                                         \
    const sp_t* wb__ = p.w;                                                                                 \
    asm volatile("" : "+s"(wb__));                                                                          \
    const int kx__ = (i_) / 3, ky__ = (i_) - kx__ * 3;                                                      \
    const int ko__ = (ky__ * 3 + kx__) * p.Cp + ((q_) >> 1) * 32 + ((q_) & 1) * 8;                          \
    char* dst__ = bring_base + (stage_) * BSTAGE_BYTES;                                                 \
    _Pragma("unroll") for (int q = 0; q < BQ; ++q) {                                                        \
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(wb__ + (boff[q] + ko__)), (lds_ptr_t)(dst__ + (q * WV + wave) * 1024), 16, 0, 0); \
    }                                                                                                       \
  }

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  int bbase[NT];                                                // byte offset of this lane's hi fragment of column tile j inside a stage
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int br = j * 32 + tx;
    bbase[j] = br * 64 + ((g ^ ((br >> 2) & 3)) << 4);
  }
  // patch row of this lane's pixel at tap (0, 0); tap (ky, kx) adds ky * WP + kx.  Tile rows beyond the last window read row 0.
  int arow;
  {
    const int r = wave * 32 + tx, wl = r / WW, px = r - wl * WW;
    arow = wl < NWIN ? wl * PP + (px / WIN) * WP + px % WIN : 0;
  }
#define WH_LOAD_A(h_, l_, sP_, toff_)                                                                       \
  {                                                                                                         \
    const int pr__ = arow + (toff_);                                                                        \
    const int ab__ = pr__ * 64 + ((g ^ ((pr__ >> 2) & 3)) << 4);                                            \
    h_ = *reinterpret_cast<const h16x8*>((sP_) + ab__);                                                     \
    l_ = *reinterpret_cast<const h16x8*>((sP_) + (ab__ ^ 32));                                              \
  }
#define WH_LOAD_B(h_, l_, sB_, j_)                                                                          \
  {                                                                                                         \
    h_ = *reinterpret_cast<const h16x8*>((sB_) + bbase[j_]);                                                \
    l_ = *reinterpret_cast<const h16x8*>((sB_) + (bbase[j_] ^ 32));                                         \
  }

  // ---- prologue: patch half 0, weight stages 0 .. LA-1 (ns >= 9 > LA)
  WH_ISSUE_PATCH(0);
#pragma unroll
  for (int s = 0; s < LA; ++s) WH_ISSUE_B(0, s, s);
  int q3 = 0, i3 = LA;                                         // (half, index) of the step whose weights are issued next, LA ahead
  int stage = 0;                                               // ring stage of the running step
  bool patch_m1 = false, patch_m2 = false;                     // a patch half was issued one / two steps ago
  h16x8 ah, al, bh0, bl0;                                      // A fragment and first B fragment of the running step
  LOFTR_WAITCNT_VM((LA - 1) * BQ);                             // patch half 0 and weight stage 0 have landed
  __builtin_amdgcn_s_barrier();
  WH_LOAD_A(ah, al, patch_base, 0);
  WH_LOAD_B(bh0, bl0, bring_base, 0);

  __builtin_amdgcn_s_setprio(1);
  int s = 0;
  for (int hq = 0; hq < nhalf; ++hq) {
    const char* sP = patch_base + (hq & 1) * PHALF_BYTES;
    const char* sPn = patch_base + ((hq + 1) & 1) * PHALF_BYTES;
#pragma unroll
    for (int i = 0; i < 9; ++i) {                              // i = kx * 3 + ky
      {   // weight stage s + 1 has landed once only what was issued after it is outstanding: stage s + 2 and a patch half issued
          // in one of the last LA - 1 steps (loads retire in order)
        const bool w2 = s + 2 < ns;
        const bool pp = patch_m1 || patch_m2;
        if (w2 && pp) LOFTR_WAITCNT_VM(BQ + PQ);
        else if (pp) LOFTR_WAITCNT_VM(PQ);
        else if (w2) LOFTR_WAITCNT_VM(BQ);
        else LOFTR_WAITCNT_VM(0);
      }
      __builtin_amdgcn_s_barrier();
      if (s + LA < ns) WH_ISSUE_B(q3, i3, stage + LA >= NB ? stage + LA - NB : stage + LA);
      if (++i3 == 9) { i3 = 0; ++q3; }
      patch_m2 = patch_m1;
      patch_m1 = false;
      if (i == 0 && hq + 1 < nhalf) { WH_ISSUE_PATCH(hq + 1); patch_m1 = true; }
      const char* sB = bring_base + stage * BSTAGE_BYTES;
      const int nstage = stage + 1 == NB ? 0 : stage + 1;
      // the fragments of the NEXT step are read during this one (after the last step: harmless reads of stale LDS)
      h16x8 nah, nal;
      if (i < 8) { WH_LOAD_A(nah, nal, sP, ((i + 1) % 3) * WP + (i + 1) / 3); }
      else { WH_LOAD_A(nah, nal, sPn, 0); }
      h16x8 ch = bh0, cl = bl0;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        h16x8 nh, nl;
        if (j + 1 < NT) { WH_LOAD_B(nh, nl, sB, j + 1); }
        else { WH_LOAD_B(nh, nl, bring_base + nstage * BSTAGE_BYTES, 0); }
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, ch, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, cl, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, ch, acc[j], 0, 0, 0);
        ch = nh; cl = nl;
      }
      bh0 = ch; bl0 = cl;
      ah = nah; al = nal;
      stage = nstage;
      ++s;
    }
  }
#undef WH_LOAD_B
#undef WH_LOAD_A
#undef WH_ISSUE_B
#undef WH_ISSUE_PATCH
  __builtin_amdgcn_s_setprio(0);

  // ---- epilogue: the dense kernel's value (bias, no activation: act(x) = max(x, 1 * x)), then the window gather's SP word; zeros
  // for window pixels outside the map (F.unfold's padding)
  const bool odd = lane & 1;
  const float slope = p.act == 1 ? 0.f : p.act == 2 ? 0.01f : 1.f;      // (a run-time value, as in the dense kernel: the same instructions)
  int roff[16], rflag[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
    roff[r] = row_off[row];
    rflag[r] = row_flag[row];
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = j * 32 + tx, colc = min(col, p.Cout - 1);
    const bool creal = col < p.Cout;                                          // (the SP row's pad channels are written as zeros)
    const float bia = p.bias ? p.bias[colc] : 0.f;
    const float wsc = p.wscale[colc];                                         // undo the filter rows' power-of-two scales (the input is stored unscaled)
    f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float xv = fmaf(acc[j][r], wsc, bia);
      v[r] = creal ? fmaxf(xv, slope * xv) : 0.f;
    }
    uint32_t w16[16];
    sp_words16(v, odd, w16);
    const int lane_sp = j * 32 + (odd ? 16 : 0) + (tx >> 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (roff[r] >= 0) {
        sp_t* o = (rflag[r] & 1) ? p.win1 : p.win0;
        o[(unsigned)(roff[r] + lane_sp)] = (rflag[r] & 2) ? w16[r] : 0u;
      }
    }
  }
}

struct HeadWindows { WinHeadArgs a; };

int launch_head_windows(const void* ctx, sp_t* win0, sp_t* win1, hipStream_t st) {
  const HeadWindows& h = *(const HeadWindows*)ctx;
  WinHeadArgs a = h.a;
  a.win0 = win0; a.win1 = win1;
  const int nwin = 2 * a.M;
  hipLaunchKernelGGL(window_head_kernel, dim3(ceil_div(nwin, NWIN)), dim3(WV * 64), 0, st, a);
  LOFTR_CHECK_LAUNCH();
  return LOFTR_OK;
}

// Argument checks and the kernel's argument block (everything but the window tiles).
int head_windows_args(const uint32_t* h_sp0, const uint32_t* h_sp1, int N, int H, int Wm, int Cin, const void* prepared,
                      size_t prepared_bytes, int Cout, const int64_t* b_ids, const int64_t* i_ids,
                      const int64_t* j_ids, int M, int w0c, int w1c, int stride, int W, HeadWindows& o) {
  LOFTR_CHECK_ARG(h_sp0 && h_sp1 && prepared && b_ids && i_ids && j_ids);
  LOFTR_CHECK_ARG(N > 0 && H > 0 && Wm > 0 && Cin > 0 && Cout > 0 && M > 0 && w0c > 0 && w1c > 0 && stride > 0);
  if (W != WIN || ceil32(Cout) != NT * 32) return LOFTR_ERR_UNSUPPORTED;
  const int Cp = ceil32(Cin);
  if ((long)N * H * Wm * Cp >= (1L << 31) || (long)M * WW * NT * 32 >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  ConvPrepared pr;
  if (!conv_prepared_layout(const_cast<void*>(prepared), prepared_bytes, Cin, Cout, 3, 3, pr)) return LOFTR_ERR_WORKSPACE;
  WinHeadArgs& a = o.a;
  a.x0 = h_sp0; a.x1 = h_sp1; a.H = H; a.W = Wm; a.Cp = Cp; a.Cin = Cin;
  a.w = pr.wsp; a.K = 9 * Cp; a.bias = pr.bias; a.wscale = pr.wscale; a.zeros = pr.zeros;
  a.b_ids = b_ids; a.i_ids = i_ids; a.j_ids = j_ids; a.M = M; a.w0c = w0c; a.w1c = w1c; a.stride = stride;
  a.Cout = Cout; a.act = 0; a.win0 = nullptr; a.win1 = nullptr;
  return LOFTR_OK;
}

}  // namespace whead

extern "C" int loftr_window_head(const uint32_t* h_sp0, const uint32_t* h_sp1, int N, int H, int Wm, int Cin,
                                 const void* prepared, size_t prepared_bytes, int Cout, const int64_t* b_ids,
                                 const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int W,
                                 uint32_t* win0_sp, uint32_t* win1_sp, void* stream) {
  LOFTR_CHECK_ARG(M >= 0);
  if (M == 0) return LOFTR_OK;
  LOFTR_CHECK_ARG(win0_sp && win1_sp);
  whead::HeadWindows hw;
  const int rc = whead::head_windows_args(h_sp0, h_sp1, N, H, Wm, Cin, prepared, prepared_bytes, Cout, b_ids, i_ids, j_ids,
                                          M, w0c, w1c, stride, W, hw);
  if (rc != LOFTR_OK) return rc;
  return whead::launch_head_windows(&hw, win0_sp, win1_sp, (hipStream_t)stream);
}

extern "C" int loftr_fine_preprocess_window_head(const uint32_t* h_sp0, const uint32_t* h_sp1, int N, int H, int Wm, int Cin,
                                                 const void* prepared, size_t prepared_bytes,
                                                 const float* feat_c0, const float* feat_c1, int L, int S, int Cc,
                                                 const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M,
                                                 int w0c, int w1c, int stride, int W, int Cf,
                                                 const float* down_w, const float* down_b, const float* merge_w,
                                                 const float* merge_b, float* out0, float* out1, void* ws, size_t ws_bytes,
                                                 void* stream) {
  LOFTR_CHECK_ARG(M >= 0);
  if (M == 0) return LOFTR_OK;
  LOFTR_CHECK_ARG(out0 && out1 && Cf > 0);
  whead::HeadWindows hw;
  const int rc = whead::head_windows_args(h_sp0, h_sp1, N, H, Wm, Cin, prepared, prepared_bytes, Cf, b_ids, i_ids, j_ids,
                                          M, w0c, w1c, stride, W, hw);
  if (rc != LOFTR_OK) return rc;
  if (Cf != whead::NT * 32) return LOFTR_ERR_UNSUPPORTED;          // the window tiles are rows of Cf dwords
  return fine_preprocess_run(WindowGather{whead::launch_head_windows, &hw}, feat_c0, feat_c1, L, S, Cc, b_ids, i_ids, j_ids, M, W, Cf,
                             down_w, down_b, merge_w, merge_b, out0, out1, ws, ws_bytes, (hipStream_t)stream);
}
