// The ONE kernel text of the FPN fine head's convolutions (layer1_outconv2: 3x3 + BN + LeakyReLU, 3x3; both 3x3 / stride 1 / pad 1)
// evaluated only where the W x W fine windows of the matched coarse cells need them, its argument block and their builder.
//   reference: src/loftr/backbone/resnet_fpn.py:66-77, :113-116 (x1_out), src/loftr/loftr_module/fine_preprocess.py:40-47
//
// Three instantiations, in two translation units:
//   window_head.hip        Cfg<5,4,4,1,1,false>  the last convolution at the 5 x 5 windows, patches read from the dense map
//   window_head_first.hip  Cfg<7,7,4,2,2,false>  the first convolution at the 7 x 7 neighbourhoods of the windows
//                          Cfg<5,4,4,1,1,true>   the last convolution, patches read from the first one's packed rows
//
// Why the includer names the kernel (#define WINDOW_KERNEL_NAME before the #include).  profiles/pmc_traffic.json is valid for a build
// as long as every device function whose mangled name contains one of its keys keeps its name and its machine code
// (tools/kernel_code_hash.py); window_nbhd_kernel is a key.  So the two instantiations of window_head_first.hip must stay
// whf::window_nbhd_kernel<whf::Cfg<...>>(whf::Args) byte for byte, and the third must NOT carry that name (it would join the hashed set).
// Moving the body into a __device__ function behind thin __global__ wrappers was tried and changes the code of both existing
// instantiations (by value and by reference); the unchanged __global__ text under an includer-supplied name leaves them identical.
// The name must not contain any key of the table (conv_kernel, linear_kernel, select_kernel, gather_windows_kernel, window_nbhd_kernel).
//
// Same arithmetic as the dense kernels (conv3x3_duo.h Cfg<7,2,4,8,2> for the first, Cfg<4,2,4> for the last), so the same bits:
// v_mfma_f32_32x32x16_f16 on zero accumulators, k order (channel group, half, tap column kx, tap row ky), the three products in the
// order lo.hi, hi.lo, hi.hi, the all-padding second half of the last channel group skipped (Cin = 196: 13 half steps), the dense
// epilogue's expression fmaf(acc, wscale, bias), max(x, slope * x), then the SP encoding (for the windows: gather_windows_kernel's).
// An element's sum does not depend on the tile row it sits in: the outputs equal a gather of the dense map bit for bit
// (tests/test_hip_window_head.py, tests/test_hip_window_head_first.py compare with torch.equal).
//
// Tiling.  A workgroup owns NWIN = 5 windows x OUT x OUT output pixels, packed densely into its WM x RW 32-row tiles (window
// w = side * M + m); wave = wn * WM + wr owns the row tiles RW wr .. and the column tiles NJ wn .. (the last split may own one fewer).
// Per window the (OUT + 2)^2 input patch is staged in LDS per half channel group (64-byte rows, chunk swizzle and double buffer as in
// conv3x3_duo.h; rows outside the image come from the zero page); the A fragment of a lane is its pixel's patch row plus the tap's
// constant row offset ky * (OUT + 2) + kx.  Weight ring (one tap x one 16-wide k-step per stage, NB stages, NB - 1 ahead), one barrier
// per step and the vmcnt bookkeeping are those of the dense kernel; DMA slots a wave has no row for go to a 1 KB scratch area so that
// every wave issues the same number of loads (never addressed where the slot counts divide by the waves, as at 4 waves: 1 KB of LDS).
//   Cfg<5,4,4,1,1,*>: 4 waves, 125 of 128 rows, 5 x 49 patch rows, 66 KB of LDS, two workgroups per CU.
//   Cfg<7,7,4,2,2,false>: 8 waves, 245 of 256 rows, 128 accumulator registers, 5 x 81 patch rows (2 x 26 KB), 224 weight rows per
//   stage: 111 KB of LDS, one workgroup per CU.
#pragma once
#include "conv_prepared.h"
#include "fine.h"

#ifndef WINDOW_KERNEL_NAME
#error "define WINDOW_KERNEL_NAME (the kernel template's name in this translation unit) before including window_conv.h"
#endif

namespace whf {

constexpr int WIN = 5;                                                    // side of the fine windows (the only W supported)
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
__global__ __launch_bounds__(CF::WAVES * 64, CF::WG_PER_CU) void WINDOW_KERNEL_NAME(Args p) {
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

// (static: the body names this translation unit's kernel)
template <typename CF>
static int launch(Args a, sp_t* out0, sp_t* out1, hipStream_t st) {
  a.out0 = out0; a.out1 = out1;
  hipLaunchKernelGGL((WINDOW_KERNEL_NAME<CF>), dim3(ceil_div(2 * a.M, NWIN)), dim3(CF::WAVES * 64), 0, st, a);
  LOFTR_CHECK_LAUNCH();
  return LOFTR_OK;
}

// What an entry point accepts beyond the kernel's own shape rules (they differ per entry: include/loftr_hip.h).
struct Limits {
  long span;                              // dwords of the largest tensor written through 32-bit offsets; must stay below 2^31
  int Cin, Cout;                          // the only channel counts accepted; 0: any
};

// Argument checks and the argument block of one launch of Cfg CF (everything but the output pointers).  x0 / x1: the SP maps
// [N, H, Wm, ceil32(Cin)] of the two image batches; PACKED: x0 = the neighbourhood rows of both sides [2 M, PP, ceil32(Cin)], x1 and N
// unused, H / Wm the map the windows lie in.  Bad arguments are reported before unsupported shapes, those before a short filter buffer.
template <typename CF>
static int make_args(const sp_t* x0, const sp_t* x1, int N, int H, int Wm, int Cin, const void* prepared, size_t prepared_bytes, int Cout,
                     int act, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride,
                     int W, const Limits& lim, Args& a) {
  LOFTR_CHECK_ARG(x0 && (CF::PACKED || (x1 && N > 0)) && prepared && b_ids && i_ids && j_ids);
  LOFTR_CHECK_ARG(H > 0 && Wm > 0 && Cin > 0 && Cout > 0 && M > 0 && w0c > 0 && w1c > 0 && stride > 0);
  if (W != WIN || ceil32(Cout) != CF::NT * 32 || lim.span >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  if ((lim.Cin && Cin != lim.Cin) || (lim.Cout && Cout != lim.Cout)) return LOFTR_ERR_UNSUPPORTED;
  const int Cp = ceil32(Cin);
  if (!CF::PACKED && (long)N * H * Wm * Cp >= (1L << 31)) return LOFTR_ERR_UNSUPPORTED;
  ConvPrepared pr;
  if (!conv_prepared_layout(const_cast<void*>(prepared), prepared_bytes, Cin, Cout, 3, 3, pr)) return LOFTR_ERR_WORKSPACE;
  a.x0 = x0; a.x1 = CF::PACKED ? x0 + (size_t)M * CF::PP * Cp : x1; a.H = H; a.W = Wm; a.Cp = Cp; a.Cin = Cin;
  a.w = pr.wsp; a.K = 9 * Cp; a.bias = pr.bias; a.wscale = pr.wscale; a.zeros = pr.zeros;
  a.b_ids = b_ids; a.i_ids = i_ids; a.j_ids = j_ids; a.M = M; a.w0c = w0c; a.w1c = w1c; a.stride = stride;
  a.Cout = Cout; a.act = act; a.out0 = nullptr; a.out1 = nullptr;
  return LOFTR_OK;
}

}  // namespace whf
