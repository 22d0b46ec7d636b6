// Layout of a prepared (BatchNorm-folded, SP) convolution filter buffer, shared by conv.hip (which fills and consumes it) and
// window_head.hip (which consumes the fine head's second filter).
#pragma once
#include "gemm.h"

// Folded weights live in a caller-owned buffer laid out [SP weights Cout x K][bias Cout][inverse row scales Cout][zero page 256 B]
// (loftr_conv_workspace_bytes): conv_prepare fills it, conv_run consumes it.
struct ConvPrepared { sp_t* wsp; float* bias; float* wscale; sp_t* zeros; };
static inline bool conv_prepared_layout(void* buf, size_t bytes, int Cin, int Cout, int KH, int KW, ConvPrepared& o) {
  WsAlloc wa(buf, bytes);
  o.wsp = wa.take<sp_t>((size_t)Cout * KH * KW * ceil32(Cin));
  o.bias = wa.take<float>(Cout);
  o.wscale = wa.take<float>(Cout);
  o.zeros = wa.take<sp_t>(64);
  return wa.ok();
}
