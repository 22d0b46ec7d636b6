// BOTH convolutions of the FPN fine head (layer1_outconv2: 3x3 + BN + LeakyReLU, 3x3) evaluated only where the W x W fine windows of
// the matched coarse cells need them.
//   reference: src/loftr/backbone/resnet_fpn.py:66-77, :113-116 (x1_out), src/loftr/loftr_module/fine_preprocess.py:40-47
//
// window_head.hip moved the head's LAST convolution to the 5 x 5 windows; its input, the output of the head's FIRST convolution, then
// has one consumer that reads the 7 x 7 neighbourhood of each window: 2 M x 49 of the map's pixels (49 % at the bench's 765 matches
// per 640 x 480 pair).  Two instantiations of the kernel text of window_conv.h (arithmetic, tiling and the reason for the #define there):
//   * First (kernel A): the first convolution (Cin -> 196, folded BN, LeakyReLU) at the 7 x 7 neighbourhoods, from the FPN top-down
//     map t1 (SP [N, H, W, Cp] per image batch) into a scratch tensor SP [2 M, 49, 224]: window w = side * M + m, row py * 7 + px =
//     pixel (y0 - 1 + py, x0 - 1 + px) of the 5 x 5 window whose top-left pixel is (y0, x0).  Rows outside the map are ZERO words --
//     they are the second convolution's zero padding, not a convolution of padded input; pad channels 196 .. 223 are zeros.
//   * Last (kernel B): window_head.hip's kernel with its 7 x 7 patches staged from that scratch tensor (contiguous rows, no bounds to
//     test: the zeros are stored).
#define WINDOW_KERNEL_NAME window_nbhd_kernel
#include "window_conv.h"

namespace whf {

using First = Cfg<7, 7, 4, 2, 2, false>;
using Last = Cfg<5, 4, 4, 1, 1, true>;
static_assert(Last::OUT == WIN && Last::PP == First::OO && First::NT * 32 == 224, "the last kernel's patch rows are the first kernel's output rows");

// The two launches' argument blocks (everything but the output pointers).
struct HeadWindows2 { Args first, last; sp_t* nb; };

static int launch_first(const HeadWindows2& h, hipStream_t st) {
  return launch<First>(h.first, h.nb, h.nb + (size_t)h.first.M * First::OO * (First::NT * 32), st);
}

static int launch_head_windows2(const void* ctx, sp_t* win0, sp_t* win1, hipStream_t st) {
  const HeadWindows2& h = *(const HeadWindows2*)ctx;
  const int rc = launch_first(h, st);
  if (rc != LOFTR_OK) return rc;
  return launch<Last>(h.last, win0, win1, st);
}

// The head of ResNetFPN_8_2, 196 -> 196 -> 128, with the scratch tensor [2 M, 49, 224] inside 32-bit offsets.
static Limits limits(int M, int Cout) { return Limits{(long)2 * M * First::OO * (First::NT * 32), 196, Cout}; }

// Argument block of the first kernel: t1 maps -> neighbourhood rows.
static int first_args(const uint32_t* t_sp0, const uint32_t* t_sp1, int N, int H, int Wm, int Cin, const void* prepared, size_t prepared_bytes,
                      int Cout, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride,
                      int W, Args& a) {
  return make_args<First>(t_sp0, t_sp1, N, H, Wm, Cin, prepared, prepared_bytes, Cout, 2, b_ids, i_ids, j_ids, M, w0c, w1c, stride, W,
                          limits(M, 196), a);
}

// Argument block of the last kernel: neighbourhood rows nb [2 M, 49, 224] -> window rows.  H / Wm: the map the windows lie in.
static int last_args(const uint32_t* nb_sp, int H, int Wm, int Cin, const void* prepared, size_t prepared_bytes, int Cout,
                     const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int W, Args& a) {
  return make_args<Last>(nb_sp, nullptr, 0, H, Wm, Cin, prepared, prepared_bytes, Cout, 0, b_ids, i_ids, j_ids, M, w0c, w1c, stride, W,
                         limits(M, 128), a);
}

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
