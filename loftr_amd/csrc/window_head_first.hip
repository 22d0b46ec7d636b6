// BOTH convolutions of the FPN fine head (layer1_outconv2: 3x3 + BN + LeakyReLU, 3x3) evaluated only where the W x W fine windows of
// the matched coarse cells need them.
//   reference: src/loftr/backbone/resnet_fpn.py:66-77, :113-116 (x1_out), src/loftr/loftr_module/fine_preprocess.py:40-47
//
// window_head.hip moved the head's LAST convolution to the 5 x 5 windows; its input, the output of the head's FIRST convolution, then
// has one consumer that reads the 7 x 7 neighbourhood of each window: 2 M x 49 of the map's pixels (49 % at the bench's 765 matches
// per 640 x 480 pair).  Two kernels, one template:
//   * first (kernel A): the first convolution (Cin -> 196, folded BN, LeakyReLU) at the 7 x 7 neighbourhoods, from the FPN top-down
//     map t1 (SP [N, H, W, Cp] per image batch) into a scratch tensor SP [2 M, 49, 224]: window w = side * M + m, row py * 7 + px =
//     pixel (y0 - 1 + py, x0 - 1 + px) of the 5 x 5 window whose top-left pixel is (y0, x0).  Rows outside the map are ZERO words --
//     they are the second convolution's zero padding, not a convolution of padded input; pad channels 196 .. 223 are zeros.
//   * last (kernel B): window_head_kernel's loop, arithmetic and epilogue with its 7 x 7 patches staged from that scratch tensor
//     (contiguous rows, no bounds to test: the zeros are stored).
//
// Same arithmetic as the dense kernels (conv3x3_duo.h Cfg<7,2,4,8,2> for the first, Cfg<4,2,4> for the last), so the same bits:
// v_mfma_f32_32x32x16_f16 on zero accumulators, k order (channel group, half, tap column kx, tap row ky), the three products in the
// order lo.hi, hi.lo, hi.hi, the all-padding second half of the last channel group skipped (Cin = 196: 13 half steps), the dense
// epilogue's expression fmaf(acc, wscale, bias), max(x, slope * x), then the SP encoding.  An element's sum does not depend on the tile
// row it sits in (tests/test_hip_window_head_first.py compares with torch.equal).
//
// Tiling of the first kernel.  One 8-wave workgroup owns 5 windows x 49 = 245 of 256 tile rows; wave = wn * 4 + wr owns the row tiles
// 2 wr, 2 wr + 1 and the column tiles 4 wn .. (4 + 3 of the 7, as the dense 224-column kernel splits them): 128 accumulator registers.
// Per window the 9 x 9 input patch is staged per half channel group (5 x 81 rows of 64 B, double buffered: 2 x 26 KB); the weight ring
// is the dense kernel's (one tap x one 16-wide k-step per stage: 224 rows x 64 B, NB stages, NB - 1 ahead): 111 KB of LDS, one
// workgroup per CU.  A lane's A fragment is its pixel's patch row plus ky * 9 + kx.  Chunk swizzle, zero-page sourcing of patch rows
// outside the image, one barrier per step and the vmcnt bookkeeping follow window_head.hip; DMA slots a wave has no row for go to a
// 1 KB scratch area so that every wave issues the same number of loads.
#include "conv_prepared.h"
#include "fine.h"

namespace whf {

constexpr int NWIN = 5;                                                   // windows of a workgroup
constexpr int NB = 4, LA = NB - 1;                                        // weight ring stages, stages in flight

// OUT: side of the square of output pixels per window (7: the neighbourhood, 5: the window); NT 32-column tiles; WM x WN waves, a wave
// owns RW 32-row tiles and NJ (the last split: NT - NJ) column tiles; PACKED: the input is the first kernel's scratch tensor.
template <int OUT_, int NT_, int WM_, int WN_, int RW_, bool PACKED_>
struct Cfg {
  static constexpr int OUT = OUT_, PS = OUT_ + 2, OO = OUT_ * OUT_, PP = PS * PS;
  static constexpr int NT = NT_, WM = WM_, WN = WN_, RW = RW_, WAVES = WM_ * WN_, NJ = (NT_ + WN_ - 1) / WN_;
  static constexpr bool PACKED = PACKED_;
  static constexpr int ROWS = WM * RW * 32;
  static constexpr int PROWS = NWIN * PP, PSLOTS = (PROWS + 15) / 16, PQ = (PSLOTS + WAVES - 1) / WAVES;   // 1 KB DMA slots (16 rows) of a patch half; per wave
  static constexpr int PHALF_BYTES = PSLOTS * 1024;
  static constexpr int BSLOTS = NT * 32 / 16, BQ = (BSLOTS + WAVES - 1) / WAVES, BSTAGE_BYTES = BSLOTS * 1024;
  static constexpr int SCR_OFF = 2 * PHALF_BYTES + NB * BSTAGE_BYTES;     // 1 KB: destination of the unused DMA slots
  static constexpr int TAB_OFF = SCR_OFF + 1024;
  static constexpr int LDS_BYTES = TAB_OFF + ROWS * 8;                    // row table: output offset, flags
  static constexpr int WG_PER_CU = WAVES == 4 ? 2 : 1;
  static_assert(NWIN * OO <= ROWS, "the windows' output pixels fit the tile rows");
  static_assert(LDS_BYTES * WG_PER_CU <= 160 * 1024, "LDS");
  static_assert(WN == 1 || NT - (WN - 1) * NJ >= NJ - 1, "the last column split owns NJ or NJ - 1 tiles");
};
using First = Cfg<7, 7, 4, 2, 2, false>;
using Last = Cfg<5, 4, 4, 1, 1, true>;

struct Args {
  const sp_t* x0; const sp_t* x1;         // maps [N, H, W, Cp] SP of the image0 / image1 batch; PACKED: neighbourhood rows [M, PP, Cp] of side 0 / 1
  int H, W, Cp, Cin;
  const sp_t* w; int K;                   // [Cout, 9 * Cp] SP (prepared filter)
  const float* bias; const float* wscale;
  const sp_t* zeros;
  const int64_t* b_ids; const int64_t* i_ids; const int64_t* j_ids;
  int M, w0c, w1c, stride;
  int Cout;                               // ceil32(Cout) == NT * 32
  int act;                                // 0 none, 1 ReLU, 2 LeakyReLU(0.01)
  sp_t* out0; sp_t* out1;                 // [M, OUT * OUT, NT * 32] SP of side 0 / 1
};

// Window w of the launch (w = side * M + m): top-left pixel of its OUT x OUT square of output pixels, image index and side.
struct WinPos { int b, y0, x0, side; };
template <int OUT>
__device__ __forceinline__ WinPos window_pos(const Args& p, int w) {
  const int side = w >= p.M ? 1 : 0, m = w - side * p.M;
  const long cell = side ? p.j_ids[m] : p.i_ids[m];
  const int wc = side ? p.w1c : p.w0c;
  WinPos o;
  o.b = (int)p.b_ids[m];
  o.y0 = (int)(cell / wc) * p.stride - OUT / 2;
  o.x0 = (int)(cell % wc) * p.stride - OUT / 2;
  o.side = side;
  return o;
}

template <typename CF>
__global__ __launch_bounds__(CF::WAVES * 64, CF::WG_PER_CU) void window_nbhd_kernel(Args p) {
  constexpr int OUT = CF::OUT, PS = CF::PS, OO = CF::OO, PP = CF::PP, NT = CF::NT, RW = CF::RW, NJ = CF::NJ;
  constexpr int WAVES = CF::WAVES, WM = CF::WM, ROWS = CF::ROWS, PQ = CF::PQ, BQ = CF::BQ;
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef const __attribute__((address_space(1))) void* gbl_ptr_t;
  __shared__ __attribute__((aligned(16))) char lds[CF::LDS_BYTES];
  char* const patch_base = lds;
  char* const bring_base = lds + 2 * CF::PHALF_BYTES;
  char* const scratch = lds + CF::SCR_OFF;
  int* const row_off = reinterpret_cast<int*>(lds + CF::TAB_OFF);  // dword offset of the tile row's pixel in out0 / out1, -1: no such row
  int* const row_flag = row_off + ROWS;                            // bit 0: side, bit 1: the pixel lies inside the map

  const int tile = blockIdx.x, nwin = 2 * p.M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 5, tx = lane & 31;
  const int wr = wave % WM, wn = wave / WM;                     // this wave's row tiles and column split
  const int jc0 = wn * NJ;                                      // its first column tile
  const int nj = min(NJ, NT - jc0);                             // ... and how many it owns (wave-uniform)
  const int drow = lane >> 2, dpos = lane & 3;                  // DMA: row inside a 16-row slot, 16-B position inside the 64-B row

  // ---- row table: tile row r = (window r / OO of the tile, pixel r % OO of the window)
  if (tid < ROWS) {
    const int wl = tid / OO, px = tid - wl * OO, w = tile * NWIN + wl;
    int off = -1, flag = 0;
    if (wl < NWIN && w < nwin) {
      const WinPos wp = window_pos<OUT>(p, w);
      const int y = wp.y0 + px / OUT, x = wp.x0 + px % OUT;
      const bool in = (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
      off = ((w - wp.side * p.M) * OO + px) * (NT * 32);
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
    const int s_ = q * WAVES + wave, r = s_ * 16 + drow;
    const int wl = r / PP, rem = r - wl * PP, py = rem / PS, px = rem - py * PS;
    const int w = tile * NWIN + wl;
    const bool live = s_ < CF::PSLOTS && r < CF::PROWS && w < nwin;
    const WinPos wp = window_pos<OUT>(p, live ? w : 0);
    const int c = dpos ^ ((r >> 2) & 3);
    const int coff = ((c & 1) + ((c >> 1) << 2)) << 2;
    if (CF::PACKED) {                                           // row rem of the window's stored neighbourhood (zeros stored outside the map)
      poff[q] = live ? ((w - wp.side * p.M) * PP + rem) * p.Cp + coff : -1;
    } else {
      const int gy = wp.y0 - 1 + py, gx = wp.x0 - 1 + px;
      const bool in = live && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
      poff[q] = in ? ((wp.b * p.H + gy) * p.W + gx) * p.Cp + coff : -1;
    }
    pside |= (unsigned)wp.side << q;
  }
  int boff[BQ];
#pragma unroll
  for (int q = 0; q < BQ; ++q) {
    const int r = (q * WAVES + wave) * 16 + drow;
    const int c = dpos ^ ((r >> 2) & 3);
    boff[q] = min(r, p.Cout - 1) * p.K + (((c & 1) + ((c >> 1) << 2)) << 2);      // rows >= Cout: clamped copies (never stored)
  }
  const int gpt = p.Cp >> 5;
  // channels >= Cin of the last group are zero padding (activations AND folded weights): when they fill its whole second k-step
  // that half is skipped -- exact, and the rule of the dense kernel
  const int nhalf = 2 * gpt - (p.Cin <= (gpt - 1) * 32 + 16 ? 1 : 0), ns = nhalf * 9;

  // (base pointers laundered per issue: otherwise the 64-bit DMA addresses are hoisted out of the loop and spilled)
#define WHF_ISSUE_PATCH(q_)                                                                                 \
  {                                                                                                         \
    const sp_t* xa__ = p.x0;                                                                                \
    const sp_t* xb__ = p.x1;                                                                                \
    asm volatile("" : "+s"(xa__), "+s"(xb__));                                                              \
    const int ko__ = ((q_) >> 1) * 32 + ((q_) & 1) * 8;                                                     \
    char* dst__ = patch_base + ((q_) & 1) * CF::PHALF_BYTES;                                                \
    _Pragma("unroll") for (int q = 0; q < PQ; ++q) {                                                        \
      const sp_t* g__ = poff[q] >= 0 ? (((pside >> q) & 1u) ? xb__ : xa__) + (poff[q] + ko__) : p.zeros;    \
      char* d__ = (q * WAVES + wave < CF::PSLOTS) ? dst__ + (q * WAVES + wave) * 1024 : scratch;            \
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)g__, (lds_ptr_t)d__, 16, 0, 0);                           \
    }                                                                                                       \
  }
  // weight stage of step (half q_, index i_ = kx * 3 + ky inside the half): tap ky * 3 + kx
#define WHF_ISSUE_B(q_, i_, stage_)                                                                         \
  {                                                                                                         \
    const sp_t* wb__ = p.w;                                                                                 \
    asm volatile("" : "+s"(wb__));                                                                          \
    const int kx__ = (i_) / 3, ky__ = (i_) - kx__ * 3;                                                      \
    const int ko__ = (ky__ * 3 + kx__) * p.Cp + ((q_) >> 1) * 32 + ((q_) & 1) * 8;                          \
    char* dst__ = bring_base + (stage_) * CF::BSTAGE_BYTES;                                                 \
    _Pragma("unroll") for (int q = 0; q < BQ; ++q) {                                                        \
      char* d__ = (q * WAVES + wave < CF::BSLOTS) ? dst__ + (q * WAVES + wave) * 1024 : scratch;            \
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(wb__ + (boff[q] + ko__)), (lds_ptr_t)d__, 16, 0, 0);     \
    }                                                                                                       \
  }

  f32x16 acc[RW][NJ];
#pragma unroll
  for (int i = 0; i < RW; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  int bbase[NJ];                                                // byte offset of this lane's hi fragment of the wave's column tile j inside a stage
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int br = min(jc0 + j, NT - 1) * 32 + tx;
    bbase[j] = br * 64 + ((g ^ ((br >> 2) & 3)) << 4);
  }
  // patch row of this lane's pixel at tap (0, 0), per row tile; tap (ky, kx) adds ky * PS + kx.  Tile rows beyond the last window read row 0.
  int arow[RW];
#pragma unroll
  for (int i = 0; i < RW; ++i) {
    const int r = (wr * RW + i) * 32 + tx, wl = r / OO, px = r - wl * OO;
    arow[i] = wl < NWIN ? wl * PP + (px / OUT) * PS + px % OUT : 0;
  }
#define WHF_LOAD_A(h_, l_, sP_, i_, toff_)                                                                  \
  {                                                                                                         \
    const int pr__ = arow[i_] + (toff_);                                                                    \
    const int ab__ = pr__ * 64 + ((g ^ ((pr__ >> 2) & 3)) << 4);                                            \
    h_ = *reinterpret_cast<const h16x8*>((sP_) + ab__);                                                     \
    l_ = *reinterpret_cast<const h16x8*>((sP_) + (ab__ ^ 32));                                              \
  }
#define WHF_LOAD_B(h_, l_, off_)       /* off_: byte offset inside the ring (stages are multiples of 1 KB: ^ 32 stays inside the row) */ \
  {                                                                                                         \
    h_ = *reinterpret_cast<const h16x8*>(bring_base + (off_));                                              \
    l_ = *reinterpret_cast<const h16x8*>(bring_base + ((off_) ^ 32));                                       \
  }

  // ---- prologue: patch half 0, weight stages 0 .. LA-1 (ns >= 9 > LA)
  WHF_ISSUE_PATCH(0);
#pragma unroll
  for (int s = 0; s < LA; ++s) WHF_ISSUE_B(0, s, s);
  int q3 = 0, i3 = LA;                                         // (half, index) of the step whose weights are issued next, LA ahead
  int stage = 0;                                               // ring stage of the running step
  bool patch_m1 = false, patch_m2 = false;                     // a patch half was issued one / two steps ago
  h16x8 ah[RW], al[RW], bh0, bl0;                              // A fragments and first B fragment of the running step
  LOFTR_WAITCNT_VM((LA - 1) * BQ);                             // patch half 0 and weight stage 0 have landed
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int i = 0; i < RW; ++i) WHF_LOAD_A(ah[i], al[i], patch_base, i, 0);
  WHF_LOAD_B(bh0, bl0, bbase[0]);

  __builtin_amdgcn_s_setprio(1);
  int s = 0;
  for (int hq = 0; hq < nhalf; ++hq) {
    const char* sP = patch_base + (hq & 1) * CF::PHALF_BYTES;
    const char* sPn = patch_base + ((hq + 1) & 1) * CF::PHALF_BYTES;
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
      if (s + LA < ns) WHF_ISSUE_B(q3, i3, stage + LA >= NB ? stage + LA - NB : stage + LA);
      if (++i3 == 9) { i3 = 0; ++q3; }
      patch_m2 = patch_m1;
      patch_m1 = false;
      if (i == 0 && hq + 1 < nhalf) { WHF_ISSUE_PATCH(hq + 1); patch_m1 = true; }
      const int nstage = stage + 1 == NB ? 0 : stage + 1;
      const int sB = stage * CF::BSTAGE_BYTES, sBn = nstage * CF::BSTAGE_BYTES;
      // the fragments of the NEXT step are read during this one (after the last step: harmless reads of stale LDS)
      h16x8 nah[RW], nal[RW];
#pragma unroll
      for (int ii = 0; ii < RW; ++ii) {
        if (i < 8) { WHF_LOAD_A(nah[ii], nal[ii], sP, ii, ((i + 1) % 3) * PS + (i + 1) / 3); }
        else { WHF_LOAD_A(nah[ii], nal[ii], sPn, ii, 0); }
      }
      h16x8 ch = bh0, cl = bl0;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (CF::WN > 1 && j >= nj) continue;                   // (wave-uniform: the last column split owns one tile fewer)
        h16x8 nh, nl;
        const bool more = j + 1 < NJ && (CF::WN == 1 || j + 1 < nj);
        const int nb = more ? sB + bbase[j + 1 < NJ ? j + 1 : 0] : sBn + bbase[0];
        WHF_LOAD_B(nh, nl, nb);
#pragma unroll
        for (int ii = 0; ii < RW; ++ii) acc[ii][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[ii], ch, acc[ii][j], 0, 0, 0);
#pragma unroll
        for (int ii = 0; ii < RW; ++ii) acc[ii][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ii], cl, acc[ii][j], 0, 0, 0);
#pragma unroll
        for (int ii = 0; ii < RW; ++ii) acc[ii][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ii], ch, acc[ii][j], 0, 0, 0);
        ch = nh; cl = nl;
      }
      bh0 = ch; bl0 = cl;
#pragma unroll
      for (int ii = 0; ii < RW; ++ii) { ah[ii] = nah[ii]; al[ii] = nal[ii]; }
      stage = nstage;
      ++s;
    }
  }
#undef WHF_LOAD_B
#undef WHF_LOAD_A
#undef WHF_ISSUE_B
#undef WHF_ISSUE_PATCH
  __builtin_amdgcn_s_setprio(0);

  // ---- epilogue: the dense kernel's value (folded BN shift, activation act(x) = max(x, slope * x)), then the SP word; zero words for
  // pixels outside the map (the next convolution's zero padding / F.unfold's padding)
  const bool odd = lane & 1;
  const float slope = p.act == 1 ? 0.f : p.act == 2 ? 0.01f : 1.f;      // (a run-time value, as in the dense kernel: the same instructions)
#pragma unroll
  for (int i = 0; i < RW; ++i) {
    int roff[16], rflag[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (wr * RW + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
      roff[r] = row_off[row];
      rflag[r] = row_flag[row];
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (CF::WN > 1 && j >= nj) continue;
      const int col = (jc0 + j) * 32 + tx, colc = min(col, p.Cout - 1);
      const bool creal = col < p.Cout;                                          // (the SP row's pad channels are written as zeros)
      const float bia = p.bias ? p.bias[colc] : 0.f;
      const float wsc = p.wscale[colc];                                         // undo the filter rows' power-of-two scales (the input is stored unscaled)
      f32x16 v;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float xv = fmaf(acc[i][j][r], wsc, bia);
        v[r] = creal ? fmaxf(xv, slope * xv) : 0.f;
      }
      uint32_t w16[16];
      sp_words16(v, odd, w16);
      const int lane_sp = (jc0 + j) * 32 + (odd ? 16 : 0) + (tx >> 1);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (roff[r] >= 0) {
          sp_t* o = (rflag[r] & 1) ? p.out1 : p.out0;
          o[(unsigned)(roff[r] + lane_sp)] = (rflag[r] & 2) ? w16[r] : 0u;
        }
      }
    }
  }
}

// The two launches' argument blocks (everything but the output pointers).
struct HeadWindows2 { Args first, last; sp_t* nb; };

template <typename CF>
int launch(Args a, sp_t* out0, sp_t* out1, hipStream_t st) {
  a.out0 = out0; a.out1 = out1;
  hipLaunchKernelGGL((window_nbhd_kernel<CF>), dim3(ceil_div(2 * a.M, NWIN)), dim3(CF::WAVES * 64), 0, st, a);
  LOFTR_CHECK_LAUNCH();
  return LOFTR_OK;
}

int launch_first(const HeadWindows2& h, hipStream_t st) {
  return launch<First>(h.first, h.nb, h.nb + (size_t)h.first.M * First::OO * (First::NT * 32), st);
}

int launch_head_windows2(const void* ctx, sp_t* win0, sp_t* win1, hipStream_t st) {
  const HeadWindows2& h = *(const HeadWindows2*)ctx;
  const int rc = launch_first(h, st);
  if (rc != LOFTR_OK) return rc;
  return launch<Last>(h.last, win0, win1, st);
}

int ids_args(const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int W, Args& a) {
  LOFTR_CHECK_ARG(b_ids && i_ids && j_ids && M > 0 && w0c > 0 && w1c > 0 && stride > 0);
  if (W != Last::OUT) return LOFTR_ERR_UNSUPPORTED;
  if ((long)2 * M * First::OO * (First::NT * 32) >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  a.b_ids = b_ids; a.i_ids = i_ids; a.j_ids = j_ids; a.M = M; a.w0c = w0c; a.w1c = w1c; a.stride = stride;
  a.out0 = nullptr; a.out1 = nullptr;
  return LOFTR_OK;
}

// Argument block of the first kernel: t1 maps -> neighbourhood rows.
int first_args(const uint32_t* t_sp0, const uint32_t* t_sp1, int N, int H, int Wm, int Cin, const void* prepared, size_t prepared_bytes,
               int Cout, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int W,
               Args& a) {
  LOFTR_CHECK_ARG(t_sp0 && t_sp1 && prepared && N > 0 && H > 0 && Wm > 0 && Cin > 0 && Cout > 0);
  const int rc = ids_args(b_ids, i_ids, j_ids, M, w0c, w1c, stride, W, a);
  if (rc != LOFTR_OK) return rc;
  if (Cin != 196 || Cout != 196) return LOFTR_ERR_UNSUPPORTED;             // the head of ResNetFPN_8_2: 196 -> 196 -> 128
  const int Cp = ceil32(Cin);
  if ((long)N * H * Wm * Cp >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  ConvPrepared pr;
  if (!conv_prepared_layout(const_cast<void*>(prepared), prepared_bytes, Cin, Cout, 3, 3, pr)) return LOFTR_ERR_WORKSPACE;
  a.x0 = t_sp0; a.x1 = t_sp1; a.H = H; a.W = Wm; a.Cp = Cp; a.Cin = Cin;
  a.w = pr.wsp; a.K = 9 * Cp; a.bias = pr.bias; a.wscale = pr.wscale; a.zeros = pr.zeros;
  a.Cout = Cout; a.act = 2;
  return LOFTR_OK;
}

// Argument block of the last kernel: neighbourhood rows nb [2 M, 49, 224] -> window rows.  H / Wm: the map the windows lie in.
int last_args(const uint32_t* nb_sp, int H, int Wm, int Cin, const void* prepared, size_t prepared_bytes, int Cout,
              const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int W, Args& a) {
  LOFTR_CHECK_ARG(nb_sp && prepared && H > 0 && Wm > 0 && Cin > 0 && Cout > 0);
  const int rc = ids_args(b_ids, i_ids, j_ids, M, w0c, w1c, stride, W, a);
  if (rc != LOFTR_OK) return rc;
  if (Cin != 196 || Cout != 128) return LOFTR_ERR_UNSUPPORTED;
  const int Cp = ceil32(Cin);
  ConvPrepared pr;
  if (!conv_prepared_layout(const_cast<void*>(prepared), prepared_bytes, Cin, Cout, 3, 3, pr)) return LOFTR_ERR_WORKSPACE;
  a.x0 = nb_sp; a.x1 = nb_sp + (size_t)M * Last::PP * Cp; a.H = H; a.W = Wm; a.Cp = Cp; a.Cin = Cin;
  a.w = pr.wsp; a.K = 9 * Cp; a.bias = pr.bias; a.wscale = pr.wscale; a.zeros = pr.zeros;
  a.Cout = Cout; a.act = 0;
  return LOFTR_OK;
}

static_assert(Last::PP == First::OO && First::NT * 32 == 224, "the last kernel's patch rows are the first kernel's output rows");

}  // namespace whf

extern "C" int loftr_window_head_first(const uint32_t* t_sp0, const uint32_t* t_sp1, int N, int H, int Wm, int Cin,
                                       const void* prepared, size_t prepared_bytes, int Cout, const int64_t* b_ids,
                                       const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int W,
                                       uint32_t* nb_sp, void* stream) {
  LOFTR_CHECK_ARG(M >= 0);
  if (M == 0) return LOFTR_OK;
  LOFTR_CHECK_ARG(nb_sp);
  whf::HeadWindows2 h;
  const int rc = whf::first_args(t_sp0, t_sp1, N, H, Wm, Cin, prepared, prepared_bytes, Cout, b_ids, i_ids, j_ids, M, w0c, w1c, stride,
                                 W, h.first);
  if (rc != LOFTR_OK) return rc;
  h.nb = nb_sp;
  return whf::launch_first(h, (hipStream_t)stream);
}

extern "C" int loftr_window_head_last(const uint32_t* nb_sp, int H, int Wm, int Cin, const void* prepared, size_t prepared_bytes,
                                      int Cout, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M, int w0c,
                                      int w1c, int stride, int W, uint32_t* win0_sp, uint32_t* win1_sp, void* stream) {
  LOFTR_CHECK_ARG(M >= 0);
  if (M == 0) return LOFTR_OK;
  LOFTR_CHECK_ARG(win0_sp && win1_sp);
  whf::Args a;
  const int rc = whf::last_args(nb_sp, H, Wm, Cin, prepared, prepared_bytes, Cout, b_ids, i_ids, j_ids, M, w0c, w1c, stride, W, a);
  if (rc != LOFTR_OK) return rc;
  return whf::launch<whf::Last>(a, win0_sp, win1_sp, (hipStream_t)stream);
}

extern "C" int loftr_fine_preprocess_window_head2(const uint32_t* t_sp0, const uint32_t* t_sp1, int N, int H, int Wm, int Cin,
                                                  const void* prepared0, size_t prepared0_bytes, int Cmid,
                                                  const void* prepared1, size_t prepared1_bytes,
                                                  const float* feat_c0, const float* feat_c1, int L, int S, int Cc,
                                                  const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M,
                                                  int w0c, int w1c, int stride, int W, int Cf,
                                                  const float* down_w, const float* down_b, const float* merge_w,
                                                  const float* merge_b, float* out0, float* out1, void* ws, size_t ws_bytes,
                                                  uint32_t* nb_sp, void* stream) {
  LOFTR_CHECK_ARG(M >= 0);
  if (M == 0) return LOFTR_OK;
  LOFTR_CHECK_ARG(out0 && out1 && Cf > 0 && nb_sp && prepared0 && prepared1);
  whf::HeadWindows2 h;
  int rc = whf::first_args(t_sp0, t_sp1, N, H, Wm, Cin, prepared0, prepared0_bytes, Cmid, b_ids, i_ids, j_ids, M, w0c, w1c, stride, W,
                           h.first);
  if (rc != LOFTR_OK) return rc;
  rc = whf::last_args(nb_sp, H, Wm, Cmid, prepared1, prepared1_bytes, Cf, b_ids, i_ids, j_ids, M, w0c, w1c, stride, W, h.last);
  if (rc != LOFTR_OK) return rc;
  h.nb = nb_sp;
  return fine_preprocess_run(WindowGather{whf::launch_head_windows2, &h}, feat_c0, feat_c1, L, S, Cc, b_ids, i_ids, j_ids, M, W, Cf,
                             down_w, down_b, merge_w, merge_b, out0, out1, ws, ws_bytes, (hipStream_t)stream);
}
