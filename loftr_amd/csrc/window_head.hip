// The last convolution of the FPN fine head (3x3 / stride 1 / pad 1, no BatchNorm, no activation: resnet_fpn.py:66-77, the
// second conv3x3 of layer1_outconv2) evaluated ONLY at the W x W fine windows of the matched coarse cells.
//   reference: src/loftr/backbone/resnet_fpn.py:113-116 (x1_out), src/loftr/loftr_module/fine_preprocess.py:40-47 (the unfold rows kept)
//
// The fine map has one consumer in the inference forward, the window gather of FinePreprocess: M matches keep 2 M x 25 of its
// pixels (25 % at the bench's 765 matches per 640 x 480 pair).  Here the implicit GEMM of conv3x3_duo.h runs with a packed list
// of window pixels as its M dimension instead of an 8 x 32 image tile, and its epilogue writes the SP window rows [M, 25, Cout]
// that the merge_feat GEMM consumes -- no fp32 fine map, no gather launch.
//
// The kernel is the text of window_conv.h (arithmetic, tiling and the reason for the #define there) at 4 waves, 5 windows x 25 pixels
// per workgroup, 7 x 7 patches read from the dense map: the windows equal a gather of the dense map bit for bit
// (tests/test_hip_window_head.py).
#define WINDOW_KERNEL_NAME window_head_kernel
#include "window_conv.h"

namespace whf {

using Head = Cfg<5, 4, 4, 1, 1, false>;
static_assert(Head::OUT == WIN, "the kernel's output square is the fine window");

static int launch_head_windows(const void* ctx, sp_t* win0, sp_t* win1, hipStream_t st) {
  return launch<Head>(*(const Args*)ctx, win0, win1, st);
}

// Argument block for any Cin and any Cout of four column tiles, with one side's window rows [M, 25, 128] inside 32-bit offsets.
static int head_args(const uint32_t* h_sp0, const uint32_t* h_sp1, int N, int H, int Wm, int Cin, const void* prepared,
                     size_t prepared_bytes, int Cout, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M,
                     int w0c, int w1c, int stride, int W, Args& a) {
  return make_args<Head>(h_sp0, h_sp1, N, H, Wm, Cin, prepared, prepared_bytes, Cout, 0, b_ids, i_ids, j_ids, M, w0c, w1c, stride, W,
                         Limits{(long)M * Head::OO * (Head::NT * 32), 0, 0}, a);
}

}  // namespace whf

extern "C" int loftr_window_head(const uint32_t* h_sp0, const uint32_t* h_sp1, int N, int H, int Wm, int Cin,
                                 const void* prepared, size_t prepared_bytes, int Cout, const int64_t* b_ids,
                                 const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int W,
                                 uint32_t* win0_sp, uint32_t* win1_sp, void* stream) {
  LOFTR_CHECK_ARG(M >= 0);
  if (M == 0) return LOFTR_OK;
  LOFTR_CHECK_ARG(win0_sp && win1_sp);
  whf::Args a;
  const int rc = whf::head_args(h_sp0, h_sp1, N, H, Wm, Cin, prepared, prepared_bytes, Cout, b_ids, i_ids, j_ids, M, w0c, w1c, stride,
                                W, a);
  if (rc != LOFTR_OK) return rc;
  return whf::launch_head_windows(&a, win0_sp, win1_sp, (hipStream_t)stream);
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
  whf::Args a;
  const int rc = whf::head_args(h_sp0, h_sp1, N, H, Wm, Cin, prepared, prepared_bytes, Cf, b_ids, i_ids, j_ids, M, w0c, w1c, stride, W, a);
  if (rc != LOFTR_OK) return rc;
  if (Cf != whf::Head::NT * 32) return LOFTR_ERR_UNSUPPORTED;      // the window tiles are rows of Cf dwords
  return fine_preprocess_run(WindowGather{whf::launch_head_windows, &a}, feat_c0, feat_c1, L, S, Cc, b_ids, i_ids, j_ids, M, W, Cf,
                             down_w, down_b, merge_w, merge_b, out0, out1, ws, ws_bytes, (hipStream_t)stream);
}
