"""Case tables, restated dispatch arithmetic, float64 references, tolerances and modelled mistakes of the inference backbone's edge tests.

tests/test_hip_backbone_edges.py (GPU) runs the ResNet-FPN forward's kernels -- conv_kernel<CfgD> (strided / 1x1 layers and the fused FPN
top-down step), conv3x3_duo_kernel in its 128 k / 192 / 224 column forms and its remainder form, the generic conv3x3_kernel,
stem_conv_kernel, upsample_add_kernel (csrc/conv.hip, csrc/conv3x3_duo.h) -- against PyTorch on the CPU in FLOAT64 at the sizes where their
hand-written work distribution changes path: the 256-row x 128-column tiles of the implicit GEMM (M = 1, 255, 256, 257, a tile that spans
several images, more row tiles than XCDs, 1 / 2 / 3 k-tiles against the three-stage DMA ring, fewer than 128 or 129 output columns), the
8 x 32 pixel tiles of the patch kernels (maps of one or two rows, a last tile column with one valid pixel, 1 / 7 / 8 / 9 tiles against the
XCD rounding of the grid), the stem's 8 x 32 tiles and channel lanes, the bilinear step's clamps at maps of one row or column.
tests/test_backbone_edges_oracle.py (CPU) holds every condition stated here and shows that the comparison can fail.

Reference: ref64 = F.conv2d / F.batch_norm / F.interpolate(align_corners=True) on the float64 casts of the float32 inputs, ref32 the same
in float32; noise = max|ref32 - ref64|, scale = max|ref64|.  Two bounds (tolerance / channel_tolerance below): the whole tensor against
K noise + 1e-6 scale, capped by the bound tests/test_hip_backbone.py already holds the operation to; and, on maps of at least 256 output
pixels, every channel against ITS OWN maximum (conv_rowscale_kernel scales each filter row so that every channel is fp32-accurate whatever
its magnitude next to the others: one number over the tensor's maximum cannot see a small channel that lost its low half).

Inputs are seeded by the case's name.  Weight variants: "rows" multiplies filter row 1 by 2^-10 and row 2 by 2^6; "bnedge" gives
BatchNorm channel 1 gamma = 0 (sp_row_scale(0): the channel must be act(bias) at every pixel) and channel 2 a running variance of 1e-4 (eps
is a tenth of it)."""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

# ---- tolerance --------------------------------------------------------------------------------------------------------------------------
# whole tensor:  err <= min(K[family] noise + 1e-6 scale, CAP[kind] scale)
# per channel :  max_pix err_c / max_pix |ref64_c| <= K_CH[family][output] (max_pix |ref32_c - ref64_c| / max_pix |ref64_c|) + 1e-6
# K = twice the largest err / noise measured on an MI355X over the family's cases and outputs, rounded up to an integer (the rule of
# tests/_encoder_edge_cases.py; the factor 2 covers other summation orders, which a later rewrite of a kernel is allowed).  The caps are the
# bounds of tests/test_hip_backbone.py.  The lines of profiles/backbone_edges_accuracy.txt the constants were taken from:
#   K["gemm"]    =  8 <- 3.911  conv  g_nine_full                gemm     sp    tensor  err 1.182e-05 noise 3.023e-06
#   K["duo128"]  = 13 <- 6.215  conv  c_512to512_9x33x1          duo128   sp    tensor  err 1.022e-05 noise 1.644e-06
#   K["duo192"]  =  8 <- 3.958  conv  c_196to192_8x32_res        duo192   sp    tensor  err 1.053e-05 noise 2.660e-06
#   K["wide224"] =  9 <- 4.378  conv  c_196to196_9x33_res        wide224  sp    tensor  err 1.030e-05 noise 2.352e-06
#   K["rem"]     = 10 <- 4.927  conv  c_196to196_9x33_rem_res    rem      sp    tensor  err 1.236e-05 noise 2.509e-06
#   K["generic"] =  6 <- 2.766  conv  c_128to128_9x65_duo0       generic  sp    tensor  err 5.827e-06 noise 2.107e-06
#   K["stem"]    =  5 <- 2.115  stem  s_1x1_c40_b1_crop          stem     sp    tensor  err 3.734e-08 noise 1.765e-08
#   K["up"]      =  8 <- 4.000  up    u_1x1_c40_b1               up       sp    tensor  err 4.768e-07 noise 1.192e-07
#   K["fused"]   =  3 <- 1.209  up    f_1x7_c40_b3               fused    sp    tensor  err 1.449e-06 noise 1.199e-06
#   K["net"]     =  8 <- 3.991  net   n_16_4_48x80_b1            net      coars tensor  err 4.037e-05 noise 1.012e-05
# K["duo128"] is above 12 for the 512 -> 512 layer alone (every other duo128 case stays below 3.3): its sums have 4608 terms, whose operands
# the kernels hold as fp16 hi + lo pairs -- 22 bits, a relative 2^-23 per operand that float32's own run does not have -- so the distance to
# float64 grows like sqrt(K) 2^-23 on top of the accumulation error, while the noise of the CPU's blocked float32 sums barely grows; at
# 1.78e-6 of the scale it is still a tenth of the 2e-5 cap.
#
# Per channel the SP and the fp32 output have constants of their own.  The fp32 output's largest ratios are extreme values -- the ratio of two
# per-channel maxima over a few hundred pixels, the worst of up to 512 channels -- of errors that are themselves at 1 .. 2.6e-6 of a channel's
# maximum.  The SP output's come from the FORMAT, not from the kernels: a value is stored as fp16 hi + fp16 lo, and below |x| = 2^-3 the lo
# half is a subnormal fp16 with a spacing of 2^-24, an ABSOLUTE floor of 2^-25 = 3.0e-8.  The filter row scaled by 2^-10 has a channel maximum
# of 4e-3, the floor is 7e-6 of it (its fp32 output sits at 1.2e-6: conv_rowscale_kernel does keep the small row fp32-accurate); the stem's
# channel 62 at 16 x 64 is almost everywhere negative before the ReLU, maximum 4.9e-3, floor 6.1e-6.  Activations of the network are O(1)
# per channel (BatchNorm), so the floor is 3e-8 there.  With these constants the SP bound of an ordinary channel is 3.5e-5 of its maximum,
# a seventh of what a lost lo half (2^-12) costs.
#   K_CH["gemm"]["f32"]    = 17 <-  8.336  conv  g_nine_full                gemm     f32   channel err 1.917e-06
#   K_CH["gemm"]["sp"]     = 55 <- 27.059  conv  g_rows                     gemm     sp    channel err 6.360e-06
#   K_CH["duo128"]["f32"]  = 23 <- 11.233  conv  c_512to512_9x33x1          duo128   f32   channel err 2.630e-06
#   K_CH["duo128"]["sp"]   = 69 <- 34.117  conv  c_128to256_9x33_rows       duo128   sp    channel err 8.095e-06
#   K_CH["duo192"]["f32"]  = 19 <-  9.356  conv  c_196to192_8x32_res        duo192   f32   channel err 1.680e-06
#   K_CH["duo192"]["sp"]   = 57 <- 28.314  conv  c_196to192_9x33_rows       duo192   sp    channel err 5.585e-06
#   K_CH["wide224"]["f32"] = 22 <- 10.997  conv  c_196to196_9x33_res        wide224  f32   channel err 1.963e-06
#   K_CH["wide224"]["sp"]  = 62 <- 30.708  conv  c_196to196_9x33_rows       wide224  sp    channel err 7.028e-06
#   K_CH["rem"]["sp"]      = 53 <- 26.244  conv  c_196to196_9x33_rem_rows   rem      sp    channel err 6.966e-06
#   K_CH["generic"]["f32"] =  9 <-  4.292  conv  c_128to128_9x33_duo0       generic  f32   channel err 1.092e-06
#   K_CH["generic"]["sp"]  = 57 <- 28.145  conv  c_96to160_9x33_rows        generic  sp    channel err 6.489e-06
#   K_CH["stem"]["sp"]     = 66 <- 32.664  stem  s_16x64_c128_b1            stem     sp    channel err 7.440e-06
#   K_CH["up"]["sp"]       =  3 <-  1.077  up    u_8x16_c512_b1             up       sp    channel err 5.502e-07
#   K_CH["fused"]["sp"]    =  5 <-  2.041  up    f_8x8_c196_b1              fused    sp    channel err 4.404e-07
CAP = {"conv": 2e-5, "stem": 3e-6, "fused": 3e-6, "up": 2e-6, "net": 5e-5}
K = {"gemm": 8, "duo128": 13, "duo192": 8, "wide224": 9, "rem": 10, "generic": 6, "stem": 5, "up": 8, "fused": 3, "net": 8}
K_CH = {"gemm": {"f32": 17, "sp": 55}, "duo128": {"f32": 23, "sp": 69}, "duo192": {"f32": 19, "sp": 57}, "wide224": {"f32": 22, "sp": 62}, "rem": {"sp": 53},
        "generic": {"f32": 9, "sp": 57}, "stem": {"sp": 66}, "up": {"sp": 3}, "fused": {"sp": 5}}
CHANNEL_MIN_PIXELS = 256      # below it a channel's few values can cancel to near zero: ref32 itself sits at 1.5e-5 of a channel's maximum at M = 1
DETECTION_FACTOR = 10.0       # a modelled mistake sits this many tolerances from ref64 ...
PRECISION_FLOOR = 2.0         # ... the dropped low half of one channel group of 16 (Cin = 512) at least this many


def tolerance(kind, family, noise, scale):
    return min(K[family] * noise + 1e-6 * scale, CAP[kind] * scale)


def channel_tolerance(family, out, noise_rel):
    """out: "sp" or "f32", the output the values were read from."""
    return K_CH[family][out] * noise_rel + 1e-6


# ---- the kernels' work distribution, restated ---------------------------------------------------------------------------------------------
NUM_XCD = 8                                    # csrc/common.h: xcd_grid / xcd_tile
BM, BN, NS, BK = 256, 128, 3, 32               # CfgD = GemmCfg<256, 128, 4, 2, 3> (csrc/conv.hip)
TY, TX = 8, 32                                 # pixel tile of every 3x3 patch kernel (c3::TY, c3d::Cfg<..>::TY = WM * RW = 8)
STEM_TY, STEM_TX, STEM_LANES = 8, 32, 128
DEVICE_CUS = 256                               # persistent_grid: an MI355X has 256 CUs


def _cdiv(a, b):
    return -(-a // b)


def ceil32(c):
    return _cdiv(c, 32) * 32


def out_hw(H, W, k, stride):
    pad = k // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def conv_path(cout, k, stride, *, conv_patch=1, conv_duo=1, rem=False, want_f32=False, up=False):
    """The branch of conv_run (csrc/conv.hip) a shape takes: "duo128" (Cfg<4, 2, 4>), "duo192" (Cfg<6, 2, 4, 8, 2>), "rem"
    (Cfg<6, 2, 4, 8, 2, true> + conv_rem_gather_kernel), "wide224" (Cfg<7, 2, 4, 8, 2>), "generic" (conv3x3_kernel), "gemm" (conv_kernel)."""
    coutp = ceil32(cout)
    if conv_patch and k == 3 and stride == 1 and not up:
        if conv_duo and coutp % 128 == 0:
            return "duo128"
        if conv_duo and coutp == 192:
            return "duo192"
        wide = bool(conv_duo) and coutp == 224
        if wide and rem and 1 <= cout - 192 <= 7 and not want_f32:
            return "rem"
        return "wide224" if wide else "generic"
    return "gemm"


GemmPlan = namedtuple("GemmPlan", "M tiles_m tiles_n nk chunk grid idle images_in_tile0 last_rows nact_last")
PatchPlan = namedtuple("PatchPlan", "tiles_x tiles_y tiles tiles_n chunk nvirt grid idle last_col_valid last_row_valid")


def gemm_plan(B, cin, cout, k, stride, H, W):
    """conv_kernel<CfgD>: rows = output pixels, tile (tm, tn) from xcd_tile; idle = workgroups of xcd_grid that return at once."""
    Ho, Wo = out_hw(H, W, k, stride)
    M, coutp = B * Ho * Wo, ceil32(cout)
    tiles_m, tiles_n = _cdiv(M, BM), _cdiv(coutp, BN)
    chunk = _cdiv(tiles_m, NUM_XCD)
    grid = NUM_XCD * chunk * tiles_n
    live = sum(1 for wg in range(grid) if xcd_tile(wg, tiles_m, tiles_n) is not None)
    assert live == tiles_m * tiles_n
    images0 = (min(BM, M) - 1) // (Ho * Wo) + 1
    return GemmPlan(M, tiles_m, tiles_n, k * k * ceil32(cin) // BK, chunk, grid, grid - live, images0, M - (tiles_m - 1) * BM,
                    _cdiv(coutp - (tiles_n - 1) * BN, 32))


def xcd_tile(wg, tiles_m, tiles_n):
    """(tile_m, tile_n) of workgroup `wg`, or None where the kernel returns (csrc/common.h)."""
    xcd, slot = wg % NUM_XCD, wg // NUM_XCD
    chunk = _cdiv(tiles_m, NUM_XCD)
    local, tm = slot // tiles_n, xcd * chunk + slot // tiles_n
    return (tm, slot % tiles_n) if local < chunk and tm < tiles_m else None


def patch_plan(B, cout, H, W, path, persist_cap=0, shared_gpu=False):
    """The 3x3 / stride-1 kernels: 8 x 32 pixel tiles; column tiles of 128 (duo128, generic) or one of 192 / 224."""
    tiles_x, tiles_y = _cdiv(W, TX), _cdiv(H, TY)
    tiles = B * tiles_x * tiles_y
    tiles_n = _cdiv(ceil32(cout), 128) if path in ("duo128", "generic") else 1
    chunk = _cdiv(tiles, NUM_XCD)
    nvirt = NUM_XCD * chunk * tiles_n
    grid = nvirt
    if path == "generic" and not shared_gpu:                      # persistent_grid
        cus = persist_cap // NUM_XCD * NUM_XCD if persist_cap >= NUM_XCD else DEVICE_CUS
        grid = min(nvirt, cus)
    return PatchPlan(tiles_x, tiles_y, tiles, tiles_n, chunk, nvirt, grid, nvirt - tiles * tiles_n, W - (tiles_x - 1) * TX, H - (tiles_y - 1) * TY)


def stem_grid(B, H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return _cdiv(Wo, STEM_TX), _cdiv(Ho, STEM_TY), B


# ---- convolution cases ------------------------------------------------------------------------------------------------------------------
ConvCase = namedtuple("ConvCase", "name family B cin cout k stride H W act bn res switches rem shared weights edges")
ACT_NAMES = {0: "none", 1: "relu", 2: "leaky"}


def plan_of(c):
    sw = dict(c.switches)
    if c.family == "gemm":
        return gemm_plan(c.B, c.cin, c.cout, c.k, c.stride, c.H, c.W)
    return patch_plan(c.B, c.cout, c.H, c.W, c.family, sw.get("conv_persist_cap", 0), c.shared)


def _ho_wo(c):
    return out_hw(c.H, c.W, c.k, c.stride)


CONV_EDGES = {
    # conv_kernel<CfgD>
    "M_1": lambda c, p: p.M == 1 and p.grid == NUM_XCD * p.tiles_n and p.idle == 7 * p.tiles_n,
    "M_255": lambda c, p: p.M == 255 and p.tiles_m == 1,
    "M_256_full_epilogue_only": lambda c, p: p.M == 256 and p.tiles_m == 1 and p.last_rows == BM,
    "M_257": lambda c, p: p.M == 257 and p.tiles_m == 2 and p.last_rows == 1,
    "H_1": lambda c, p: c.H == 1,
    "tile0_holds_rows_of_3_or_more_images": lambda c, p: p.images_in_tile0 >= 3,
    "tile0_holds_rows_of_5_images": lambda c, p: p.images_in_tile0 == 5,
    "odd_size_stride_2_last_window_reads_padding": lambda c, p: c.stride == 2 and c.k == 3 and c.H % 2 == 1 and c.W % 2 == 1
        and (_ho_wo(c)[0] - 1) * 2 - 1 + 2 == c.H and (_ho_wo(c)[1] - 1) * 2 - 1 + 2 == c.W,
    "odd_size_stride_2_1x1": lambda c, p: c.stride == 2 and c.k == 1 and c.H % 2 == 1 and c.W % 2 == 1,
    "9_full_row_tiles": lambda c, p: p.tiles_m == 9 and p.last_rows == BM and p.chunk == 2,
    "10_row_tiles_last_ragged": lambda c, p: p.tiles_m == 10 and 0 < p.last_rows < BM,
    "chunk_2_some_workgroup_returns": lambda c, p: p.chunk == 2 and p.idle > 0,
    "nk_1": lambda c, p: p.nk == 1,
    "nk_2": lambda c, p: p.nk == 2,
    "nk_3": lambda c, p: p.nk == 3 == NS,
    "coutp_32": lambda c, p: ceil32(c.cout) == 32 and p.nact_last == 1,
    "coutp_64": lambda c, p: ceil32(c.cout) == 64 and p.nact_last == 2,
    "cout_129": lambda c, p: c.cout == 129 and p.tiles_n == 2 and p.nact_last == 1,
    "cin_no_multiple_of_32": lambda c, p: c.cin % 32 != 0,
    "wide_512": lambda c, p: c.cout == 512 and p.tiles_n == 4 and p.tiles_m >= 2,
    "cin_512": lambda c, p: c.cin == 512,
    "conv_patch_0": lambda c, p: dict(c.switches).get("conv_patch") == 0 and c.k == 3 and c.stride == 1 and c.family == "gemm",
    "residual": lambda c, p: c.res,
    # 3x3 / stride 1
    "map_1x1": lambda c, p: (c.H, c.W) == (1, 1),
    "map_1x33": lambda c, p: (c.H, c.W) == (1, 33) and p.last_col_valid == 1,
    "map_2x2": lambda c, p: (c.H, c.W) == (2, 2),
    "map_7x31": lambda c, p: (c.H, c.W) == (7, 31) and p.tiles_x == p.tiles_y == 1,
    "map_8x32": lambda c, p: (c.H, c.W) == (8, 32) and p.last_col_valid == TX and p.last_row_valid == TY,
    "map_9x33": lambda c, p: (c.H, c.W) == (9, 33) and p.last_col_valid == 1 and p.last_row_valid == 1,
    "map_9x65": lambda c, p: (c.H, c.W) == (9, 65) and p.tiles_x == 3 and p.last_col_valid == 1,
    "both_halo_rows_outside": lambda c, p: c.H <= 2,
    "W_below_32": lambda c, p: c.W < 32,
    "last_tile_column_has_1_valid_pixel": lambda c, p: p.last_col_valid == 1 and p.tiles_x >= 2,
    "tiles_1": lambda c, p: p.tiles == 1 and p.idle == 7 * p.tiles_n,
    "tiles_7": lambda c, p: p.tiles == 7 and p.idle == p.tiles_n,
    "tiles_8": lambda c, p: p.tiles == 8 and p.idle == 0,
    "tiles_9": lambda c, p: p.tiles == 9 and p.chunk == 2 and p.idle == 7 * p.tiles_n,
    "tiles_12": lambda c, p: p.tiles == 12 and p.chunk == 2,
    "cout_224": lambda c, p: c.cout == 224,
    "cout_384": lambda c, p: c.cout == 384 and p.tiles_n == 3,
    "cout_193": lambda c, p: c.cout == 193,
    "persist_cap_8": lambda c, p: dict(c.switches).get("conv_persist_cap") == 8 and p.grid == 8 and p.nvirt > p.grid,
    "shared_gpu": lambda c, p: c.shared and c.family == "generic" and p.grid == p.nvirt,
    "conv_duo_0": lambda c, p: dict(c.switches).get("conv_duo") == 0 and c.family == "generic" and ceil32(c.cout) % 128 == 0,
    "remainder_form": lambda c, p: c.rem and c.family == "rem",
    # weights
    "rows_of_very_different_size": lambda c, p: c.weights == "rows" and not c.bn,
    "bn_gamma_0_and_tiny_variance": lambda c, p: c.weights == "bnedge" and c.bn,
}

# 3x3 / stride-1 maps: (B, H, W) -> B * tiles
MAPS = {"1x1": (1, 1, 1), "1x1x7": (7, 1, 1), "1x33": (4, 1, 33), "2x2": (9, 2, 2), "2x2x1": (1, 2, 2), "7x31": (7, 7, 31), "8x32": (8, 8, 32),
        "9x33": (2, 9, 33), "9x33x1": (1, 9, 33), "9x65": (2, 9, 65)}
MAP_EDGES = {"1x1": ("map_1x1", "both_halo_rows_outside", "W_below_32", "tiles_1"), "1x1x7": ("map_1x1", "tiles_7"),
             "1x33": ("map_1x33", "both_halo_rows_outside", "last_tile_column_has_1_valid_pixel", "tiles_8"),
             "2x2": ("map_2x2", "both_halo_rows_outside", "W_below_32", "tiles_9"), "2x2x1": ("map_2x2", "tiles_1"),
             "7x31": ("map_7x31", "W_below_32", "tiles_7"), "8x32": ("map_8x32", "tiles_8"),
             "9x33": ("map_9x33", "last_tile_column_has_1_valid_pixel", "tiles_8"), "9x33x1": ("map_9x33",),
             "9x65": ("map_9x65", "last_tile_column_has_1_valid_pixel", "tiles_12")}
ALL_MAPS = ("1x1", "1x33", "2x2", "7x31", "8x32", "9x33", "9x65")


def _build_conv_cases():
    cases, n = [], [0]

    def add(name, family, B, cin, cout, k, stride, H, W, *edges, res=False, switches=(), rem=False, shared=False, weights="plain", act=None, bn=None):
        i = n[0]
        n[0] += 1
        act = i % 3 if act is None else act                       # activations and BatchNorm cycle through the table ...
        bn = (i // 3) % 2 == 0 if bn is None else bn              # (... and conv_coverage() checks every family met all of them)
        cases.append(ConvCase(name, family, B, cin, cout, k, stride, H, W, act, bn, res, tuple(sorted(dict(switches).items())), rem, shared, weights, edges))

    # strided / 1x1: conv_kernel<CfgD>
    add("g_m1", "gemm", 1, 32, 32, 1, 1, 1, 1, "M_1", "nk_1", "coutp_32", "H_1")
    add("g_m255", "gemm", 1, 128, 128, 1, 1, 15, 17, "M_255")
    add("g_m256", "gemm", 1, 32, 128, 1, 1, 16, 16, "M_256_full_epilogue_only", "nk_1")
    add("g_m257_h1", "gemm", 1, 64, 196, 1, 2, 1, 513, "M_257", "H_1", "nk_2", "odd_size_stride_2_1x1")
    add("g_five_images", "gemm", 5, 128, 196, 3, 2, 13, 17, "tile0_holds_rows_of_5_images", "tile0_holds_rows_of_3_or_more_images")
    add("g_odd_s2", "gemm", 1, 128, 196, 3, 2, 31, 31, "odd_size_stride_2_last_window_reads_padding")
    add("g_nine_full", "gemm", 3, 256, 512, 3, 2, 48, 64, "9_full_row_tiles", "chunk_2_some_workgroup_returns", "wide_512")
    add("g_ten_tiles", "gemm", 3, 96, 256, 1, 1, 25, 31, "10_row_tiles_last_ragged", "chunk_2_some_workgroup_returns", "nk_3")
    add("g_512", "gemm", 3, 512, 512, 1, 1, 24, 32, "wide_512", "cin_512", "9_full_row_tiles")
    add("g_512_s2", "gemm", 3, 256, 512, 1, 2, 31, 33, "wide_512", "odd_size_stride_2_1x1")
    add("g_cout129", "gemm", 2, 128, 129, 1, 1, 9, 13, "cout_129")
    add("g_cin40", "gemm", 2, 40, 40, 3, 2, 9, 13, "cin_no_multiple_of_32", "coutp_64", "odd_size_stride_2_last_window_reads_padding")
    add("g_patch0_res", "gemm", 2, 196, 196, 3, 1, 9, 33, "conv_patch_0", "residual", "cin_no_multiple_of_32", res=True, switches={"conv_patch": 0})
    add("g_five_images_res", "gemm", 5, 128, 196, 3, 2, 13, 17, "tile0_holds_rows_of_5_images", "residual", res=True, act=1, bn=True)
    add("g_rows", "gemm", 3, 96, 256, 1, 1, 25, 31, "rows_of_very_different_size", weights="rows", bn=False)
    add("g_bnedge", "gemm", 5, 128, 196, 3, 2, 13, 17, "bn_gamma_0_and_tiny_variance", weights="bnedge", bn=True)

    # 3x3 / stride 1
    def add3(family, cin, cout, maps, *edges, **kw):
        for m in maps:
            B, H, W = MAPS[m]
            tag = "".join(f"_{k_.replace('conv_', '')}{v}" for k_, v in sorted(dict(kw.get("switches", ())).items())) + ("_shared" if kw.get("shared") else "") \
                + ("_rem" if kw.get("rem") else "") + ("_res" if kw.get("res") else "") + (f"_{kw['weights']}" if kw.get("weights") else "")
            add(f"c_{cin}to{cout}_{m}{tag}", family, B, cin, cout, 3, 1, H, W, *(MAP_EDGES[m] + edges), **kw)

    add3("duo128", 16, 128, ALL_MAPS)
    add3("duo128", 128, 256, ("1x1x7", "9x33", "9x65"))
    add3("duo128", 512, 512, ("1x1x7", "2x2x1", "9x33x1"), "cin_512")
    add3("duo128", 256, 384, ("1x33", "9x33"), "cout_384")
    add3("duo128", 128, 256, ("9x33",), "residual", res=True)
    add3("duo192", 196, 192, ("1x1", "2x2", "7x31", "9x33", "9x65"), "cin_no_multiple_of_32")
    add3("duo192", 196, 192, ("8x32",), "residual", res=True)
    add3("wide224", 196, 196, ALL_MAPS, "cin_no_multiple_of_32")
    add3("wide224", 128, 224, ("1x33", "8x32"), "cout_224")
    add3("wide224", 64, 193, ("2x2", "9x33"), "cout_193")
    add3("wide224", 196, 196, ("9x33",), "residual", res=True)
    add3("generic", 64, 40, ALL_MAPS)
    add3("generic", 96, 160, ("1x1", "7x31", "9x65"))
    add3("generic", 64, 40, ("9x65",), "persist_cap_8", switches={"conv_persist_cap": 8})
    add3("generic", 64, 40, ("9x33",), "shared_gpu", shared=True)
    add3("generic", 128, 128, ("9x33", "9x65"), "conv_duo_0", switches={"conv_duo": 0})
    add3("generic", 96, 160, ("9x33",), "residual", res=True)
    add3("rem", 196, 196, ("9x33",), "remainder_form", rem=True)
    add3("rem", 196, 196, ("9x33",), "remainder_form", "residual", rem=True, res=True)
    for fam, cin, cout, kw in (("duo128", 128, 256, {}), ("duo192", 196, 192, {}), ("wide224", 196, 196, {}), ("generic", 96, 160, {}),
                               ("rem", 196, 196, {"rem": True})):
        add3(fam, cin, cout, ("9x33",), "rows_of_very_different_size", weights="rows", bn=False, **kw)
        add3(fam, cin, cout, ("9x33",), "bn_gamma_0_and_tiny_variance", weights="bnedge", bn=True, **kw)
    return cases


CONV_CASES = _build_conv_cases()
CONV_BY_NAME = {c.name: c for c in CONV_CASES}
assert len(CONV_BY_NAME) == len(CONV_CASES)
FAMILIES = ("gemm", "duo128", "duo192", "wide224", "rem", "generic")


def conv_modes(c):
    """Which outputs a case is run with: SP only, fp32 only, both (the remainder form has no fp32 output)."""
    return ("sp",) if c.rem else ("sp", "f32", "both")


def conv_edge_failures():
    out = [(c.name, e) for c in CONV_CASES for e in c.edges if not CONV_EDGES[e](c, plan_of(c))]
    for c in CONV_CASES:                                          # the family a case is listed under is the branch conv_run takes
        sw = dict(c.switches)
        for mode in conv_modes(c):
            got = conv_path(c.cout, c.k, c.stride, conv_patch=sw.get("conv_patch", 1), conv_duo=sw.get("conv_duo", 1), rem=c.rem, want_f32=mode != "sp")
            if got != c.family:
                out.append((c.name, mode, got))
    return out


def conv_coverage():
    """family -> what its cases cover; every family meets every activation, BatchNorm on and off, and a residual."""
    cov = {}
    for f in FAMILIES:
        cs = [c for c in CONV_CASES if c.family == f]
        cov[f] = dict(acts={c.act for c in cs}, bn={c.bn for c in cs}, res={c.res for c in cs}, weights={c.weights for c in cs}, n=len(cs))
    return cov


assert not conv_edge_failures(), conv_edge_failures()
assert all(c.edges for c in CONV_CASES) and {e for c in CONV_CASES for e in c.edges} == set(CONV_EDGES), set(CONV_EDGES) - {e for c in CONV_CASES for e in c.edges}
for _f, _v in conv_coverage().items():
    assert _v["acts"] == {0, 1, 2} and _v["bn"] == {True, False} and _v["res"] == {True, False} and _v["weights"] == {"plain", "rows", "bnedge"}, (_f, _v)


def conv_flops(c):
    Ho, Wo = _ho_wo(c)
    return 2 * c.B * Ho * Wo * c.cout * c.cin * c.k * c.k


# (the two 256 -> 512 / 512 -> 512 cases of the issue's table are the largest: 5.4 and 1.2 GFlop; every other case stays below 1.5)
assert sorted(conv_flops(c) for c in CONV_CASES)[-2] <= 1.5e9 and max(conv_flops(c) for c in CONV_CASES) <= 5.5e9


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _act(y, act):
    return y if act == 0 else (F.relu(y) if act == 1 else F.leaky_relu(y, 0.01))


GAMMA0_CH, TINY_VAR_CH, TINY_VAR = 1, 2, 1e-4
SMALL_ROW, LARGE_ROW = 1, 2


@functools.lru_cache(maxsize=None)
def conv_inputs(name):
    """Seeded float32 tensors of a case (torch, CPU; shared by every test: do not modify): x [B, cin, H, W], w [cout, cin, k, k], bn
    (gamma, beta, mean, var, eps) or None, res [B, cout, Ho, Wo] or None."""
    c = CONV_BY_NAME[name]
    g = _gen(name)
    Ho, Wo = _ho_wo(c)
    x = torch.randn(c.B, c.cin, c.H, c.W, generator=g)
    w = torch.randn(c.cout, c.cin, c.k, c.k, generator=g) * (2.0 / (c.cin * c.k * c.k)) ** 0.5
    bn = None
    if c.bn:
        bn = [1.0 + 0.2 * torch.randn(c.cout, generator=g), 0.1 * torch.randn(c.cout, generator=g), 0.1 * torch.randn(c.cout, generator=g),
              0.5 + torch.rand(c.cout, generator=g), 1e-5]
    if c.weights == "rows":
        w[SMALL_ROW] *= 2.0 ** -10
        w[LARGE_ROW] *= 2.0 ** 6
    if c.weights == "bnedge":
        bn[0][GAMMA0_CH] = 0.0
        bn[1][GAMMA0_CH] = 0.3                                   # (positive: the channel is not zero under ReLU either)
        bn[3][TINY_VAR_CH] = TINY_VAR
    res = torch.randn(c.B, c.cout, Ho, Wo, generator=g) if c.res else None
    return dict(case=c, x=x, w=w, bn=bn, res=res)


CONV_MUTATIONS = ("left_tap_reads_previous_rows_last_pixel", "one_tap_of_last_pixel_of_ragged_tile_reads_zero", "tile_takes_image_of_its_first_row",
                  "last_input_channel_dropped", "odd_H_stride_2_last_row_outside", "bn_eps_left_out", "residual_added_after_activation",
                  "lo_part_of_one_channel_group_dropped")


def conv_mutation_applies(c, m):
    Ho, Wo = _ho_wo(c)
    if m == "left_tap_reads_previous_rows_last_pixel":
        return c.k == 3 and c.H >= 2
    if m == "one_tap_of_last_pixel_of_ragged_tile_reads_zero":
        return (c.B * Ho * Wo) % BM != 0 if c.family == "gemm" else (c.W % TX != 0 or c.H % TY != 0)
    if m == "tile_takes_image_of_its_first_row":
        return c.family == "gemm" and c.B > 1 and any((t * BM) // (Ho * Wo) != (min(t * BM + BM, c.B * Ho * Wo) - 1) // (Ho * Wo) for t in range(_cdiv(c.B * Ho * Wo, BM)))
    if m in ("last_input_channel_dropped", "lo_part_of_one_channel_group_dropped"):
        return True
    if m == "odd_H_stride_2_last_row_outside":
        return c.stride == 2 and c.H % 2 == 1
    if m == "bn_eps_left_out":
        return c.weights == "bnedge"                             # (elsewhere the variance is 0.5 .. 1.5 and eps = 1e-5 moves the result by 5e-6)
    if m == "residual_added_after_activation":
        return c.res and c.act != 0
    raise KeyError(m)


def conv_forward(i, dt, mutation=None):
    """The case's operation in dtype `dt` on the CPU -> [B, cout, Ho, Wo].  mutation: one modelled kernel mistake built in."""
    c = i["case"]
    x, w = i["x"].to(dt), i["w"].to(dt)
    pad, Ho, Wo = c.k // 2, *_ho_wo(c)
    if mutation == "last_input_channel_dropped":
        x = x.clone(); x[:, c.cin - 1] = 0
    elif mutation == "odd_H_stride_2_last_row_outside":
        x = x.clone(); x[:, :, c.H - 1] = 0
    elif mutation == "lo_part_of_one_channel_group_dropped":     # the first 32-channel group of x rounded to fp16
        x = x.clone(); x[:, :32] = x[:, :32].half().to(dt)
    if mutation == "left_tap_reads_previous_rows_last_pixel":
        xp = F.pad(x, (1, 1, 1, 1))
        xp[:, :, 2:c.H + 1, 0] = x[:, :, :c.H - 1, c.W - 1]
        y = F.conv2d(xp, w, stride=c.stride)
    else:
        y = F.conv2d(x, w, stride=c.stride, padding=pad)
    if mutation == "one_tap_of_last_pixel_of_ragged_tile_reads_zero":   # the centre tap of the last output pixel
        y[c.B - 1, :, Ho - 1, Wo - 1] -= w[:, :, pad, pad] @ x[c.B - 1, :, (Ho - 1) * c.stride, (Wo - 1) * c.stride]
    elif mutation == "tile_takes_image_of_its_first_row":
        hw = Ho * Wo
        gr = torch.arange(c.B * hw)
        src = ((gr // BM) * BM // hw) * hw + gr % hw
        y = y.permute(0, 2, 3, 1).reshape(c.B * hw, c.cout)[src].reshape(c.B, Ho, Wo, c.cout).permute(0, 3, 1, 2).contiguous()
    if i["bn"] is not None:
        gmm, beta, mean, var, eps = i["bn"]
        if mutation == "bn_eps_left_out":
            y = (y - mean.to(dt)[:, None, None]) / var.to(dt).sqrt()[:, None, None] * gmm.to(dt)[:, None, None] + beta.to(dt)[:, None, None]
        else:
            y = F.batch_norm(y, mean.to(dt), var.to(dt), gmm.to(dt), beta.to(dt), False, 0.0, eps)
    if i["res"] is not None and mutation != "residual_added_after_activation":
        y = y + i["res"].to(dt)
    y = _act(y, c.act)
    if i["res"] is not None and mutation == "residual_added_after_activation":
        y = y + i["res"].to(dt)
    return y


def _stats(ref64, ref32, channel_axis=1, pixels=None):
    """noise, scale and the per-channel figures of a reference pair (numpy float64 arrays [B, C, H, W])."""
    d = np.abs(ref32 - ref64)
    axes = tuple(a for a in range(ref64.ndim) if a != channel_axis)
    ch_scale = np.abs(ref64).max(axis=axes)
    live = ch_scale > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ch_noise = np.where(live, d.max(axis=axes) / ch_scale, 0.0)
    _freeze(ch_scale, ch_noise, live)
    return dict(noise=float(d.max()), scale=float(np.abs(ref64).max()), ch_scale=ch_scale, ch_noise=ch_noise, live=live)


def _pair(fn):
    """ref64 / ref32 as read-only float64 numpy arrays."""
    with torch.no_grad():
        r64, r32 = fn(torch.float64).numpy(), fn(torch.float32).double().numpy()
    _freeze(r64, r32)
    return r64, r32


@functools.lru_cache(maxsize=None)
def conv_reference(name):
    i = conv_inputs(name)
    r64, r32 = _pair(lambda dt: conv_forward(i, dt))
    c = i["case"]
    out = dict(ref64=r64, ref32=r32, channels=c.B * r64.shape[2] * r64.shape[3] >= CHANNEL_MIN_PIXELS, **_stats(r64, r32))
    if c.weights == "bnedge":                                    # act(beta) of the gamma = 0 channel, in float32 as the kernels form it
        b = np.float32(i["bn"][1][GAMMA0_CH].item())
        out["gamma0_value"] = float(b if c.act == 0 or b > 0 else (np.float32(0.0) if c.act == 1 else np.float32(0.01) * b))
    return out


def channel_error(got, ref):
    """max over the live channels of (a channel's largest error / its largest |ref64|), and per channel."""
    axes = tuple(a for a in range(got.ndim) if a != 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(ref["live"], np.abs(got - ref["ref64"]).max(axis=axes) / ref["ch_scale"], 0.0)
    return e


def channel_failures(got, ref, family, out, skip=()):
    """Channels outside channel_tolerance: [(channel, error, bound)]; the largest error / noise ratio over the live channels."""
    e = channel_error(got, ref)
    bound = channel_tolerance(family, out, ref["ch_noise"])
    bad = [(int(ch), float(e[ch]), float(bound[ch])) for ch in np.flatnonzero(e > bound) if ch not in skip]
    use = ref["live"].copy()
    use[list(skip)] = False
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(use & (ref["ch_noise"] > 0), e / ref["ch_noise"], 0.0)
    return bad, float(ratio.max()) if ratio.size else 0.0, float(e[use].max()) if use.any() else 0.0


def distance_in_tolerances(mut, ref, kind, family, skip=()):
    """How far a mutated float64 result sits from ref64, in units of the tolerances the GPU test applies (the larger of the two checks)."""
    d = float(np.abs(mut - ref["ref64"]).max()) / tolerance(kind, family, ref["noise"], ref["scale"])
    if ref.get("channels"):
        e = channel_error(mut, ref)
        use = ref["live"].copy()
        use[list(skip)] = False
        d = max(d, float((e / channel_tolerance(family, "sp", ref["ch_noise"]))[use].max()))       # (the SP output's: the wider of the two)
    return d


# ---- exact cases: integer inputs, no BatchNorm, no activation -----------------------------------------------------------------------------
# x in [-8, 8], w in [-2, 2], residual in [-8, 8], all integers: every fp16 hi part is exact, every lo part zero, the filter rows' scales are
# powers of two, every partial sum is an integer number of the row's granules and below 2^24 of them (K <= 4608): the result equals the
# integer convolution EXACTLY in any summation order -- the check that does not move when a kernel's k order changes.
def _exact_names():
    seen, out = set(), []
    for c in CONV_CASES:
        key = (c.family, c.B, c.cin, c.cout, c.k, c.stride, c.H, c.W, c.switches, c.shared, c.rem, c.res)
        if c.weights == "plain" and key not in seen:
            seen.add(key)
            out.append(c.name)
    return out


EXACT_CONV = _exact_names()
assert {CONV_BY_NAME[n].family for n in EXACT_CONV} == set(FAMILIES) and {e for n in EXACT_CONV for e in CONV_BY_NAME[n].edges} >= set(CONV_EDGES) - {
    "rows_of_very_different_size", "bn_gamma_0_and_tiny_variance"}


@functools.lru_cache(maxsize=None)
def exact_conv(name):
    """(x, w, res or None, expected) as float32 torch tensors holding integers; expected from the float64 convolution (exact)."""
    c = CONV_BY_NAME[name]
    g = _gen("exact " + name)
    Ho, Wo = _ho_wo(c)
    x = torch.randint(-8, 9, (c.B, c.cin, c.H, c.W), generator=g).float()
    w = torch.randint(-2, 3, (c.cout, c.cin, c.k, c.k), generator=g).float()
    res = torch.randint(-8, 9, (c.B, c.cout, Ho, Wo), generator=g).float() if c.res else None
    y = F.conv2d(x.double(), w.double(), stride=c.stride, padding=c.k // 2)
    if res is not None:
        y = y + res.double()
    return x, w, res, y


def first_difference(got, want):
    """None, or (count, (image, y, x, channel), got, want) of two [B, C, H, W] arrays."""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    if not len(bad):
        return None
    order = np.lexsort((bad[:, 1], bad[:, 3], bad[:, 2], bad[:, 0]))
    b, ch, y, x = (int(v) for v in bad[order[0]])
    return len(bad), (b, y, x, ch), float(got[b, ch, y, x]), float(want[b, ch, y, x])


# ---- stem ----------------------------------------------------------------------------------------------------------------------------------
StemCase = namedtuple("StemCase", "name B C0 H W crop edges")
STEM_EDGES = {
    "map_1x1": lambda c, g: (c.H, c.W) == (1, 1) and g[:2] == (1, 1),
    "odd_size": lambda c, g: c.H % 2 == 1 and c.W % 2 == 1,
    "output_exactly_one_tile": lambda c, g: ((c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1) == (STEM_TY, STEM_TX) and g[:2] == (1, 1),
    "output_one_past_the_tile": lambda c, g: ((c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1) == (STEM_TY + 1, STEM_TX + 1) and g[:2] == (2, 2),
    "several_tiles_ragged": lambda c, g: g[0] >= 2 and g[1] >= 4 and ((c.H - 1) // 2 + 1) % STEM_TY and ((c.W - 1) // 2 + 1) % STEM_TX,
    "all_lanes": lambda c, g: c.C0 == STEM_LANES,
    "idle_lanes_no_pad_channels": lambda c, g: c.C0 < STEM_LANES and c.C0 % 32 == 0,
    "pad_channels": lambda c, g: c.C0 % 32 != 0 and ceil32(c.C0) > c.C0,
    "strided_view": lambda c, g: c.crop,
    "batch_3": lambda c, g: c.B == 3,
}


def _build_stem_cases():
    cases = []
    for si, (H, W, e) in enumerate(((1, 1, ("map_1x1", "odd_size")), (15, 63, ("output_exactly_one_tile", "odd_size")), (16, 64, ("output_exactly_one_tile",)),
                                    (17, 65, ("output_one_past_the_tile", "odd_size")), (50, 71, ("several_tiles_ragged",)))):
        for ci, (C0, ce) in enumerate(((128, "all_lanes"), (96, "idle_lanes_no_pad_channels"), (40, "pad_channels"), (8, "pad_channels"))):
            B, crop = (3 if (si + ci) % 2 else 1), (si + ci // 2) % 2 == 1
            cases.append(StemCase(f"s_{H}x{W}_c{C0}_b{B}{'_crop' if crop else ''}", B, C0, H, W, crop,
                                  e + (ce,) + (("strided_view",) if crop else ()) + (("batch_3",) if B == 3 else ())))
    return cases


STEM_CASES = _build_stem_cases()
STEM_BY_NAME = {c.name: c for c in STEM_CASES}
STEM_UNSUPPORTED_C0 = 160
assert len(STEM_BY_NAME) == len(STEM_CASES) == 20
assert not [(c.name, e) for c in STEM_CASES for e in c.edges if not STEM_EDGES[e](c, stem_grid(c.B, c.H, c.W))]
assert {e for c in STEM_CASES for e in c.edges} == set(STEM_EDGES)
for _C0 in (128, 96, 40, 8):      # every channel count with and without a strided view, at B = 1 and 3
    assert {(c.crop, c.B) for c in STEM_CASES if c.C0 == _C0} >= {(True, 1), (False, 1), (True, 3), (False, 3)} or \
        ({c.crop for c in STEM_CASES if c.C0 == _C0} == {True, False} and {c.B for c in STEM_CASES if c.C0 == _C0} == {1, 3})
CROP_Y, CROP_X = 3, 5


@functools.lru_cache(maxsize=None)
def stem_inputs(name):
    """x is a [B, 1, H, W] float32 tensor: contiguous, or the crop big[:, :, 3:3 + H, 5:5 + W] of a larger image (a strided view)."""
    c = STEM_BY_NAME[name]
    g = _gen(name)
    big = torch.rand(c.B, 1, c.H + 9, c.W + 11, generator=g) if c.crop else None
    x = big[:, :, CROP_Y:CROP_Y + c.H, CROP_X:CROP_X + c.W] if c.crop else torch.rand(c.B, 1, c.H, c.W, generator=g)
    w = torch.randn(c.C0, 1, 7, 7, generator=g) * 0.1
    bn = [1.0 + 0.2 * torch.randn(c.C0, generator=g), 0.1 * torch.randn(c.C0, generator=g), 0.1 * torch.randn(c.C0, generator=g),
          0.5 + torch.rand(c.C0, generator=g), 1e-5]
    return dict(case=c, big=big, x=x, w=w, bn=bn)


STEM_MUTATIONS = ("last_channel_group_unwritten",)


def stem_forward(i, dt, mutation=None):
    gmm, beta, mean, var, eps = i["bn"]
    y = F.conv2d(i["x"].to(dt), i["w"].to(dt), stride=2, padding=3)
    y = F.relu(F.batch_norm(y, mean.to(dt), var.to(dt), gmm.to(dt), beta.to(dt), False, 0.0, eps))
    if mutation == "last_channel_group_unwritten":
        y = y.clone(); y[:, (i["case"].C0 - 1) // 32 * 32:] = 0
    return y


@functools.lru_cache(maxsize=None)
def stem_reference(name):
    i = stem_inputs(name)
    r64, r32 = _pair(lambda dt: stem_forward(i, dt))
    return dict(ref64=r64, ref32=r32, channels=r64.shape[0] * r64.shape[2] * r64.shape[3] >= CHANNEL_MIN_PIXELS, **_stats(r64, r32))


@functools.lru_cache(maxsize=None)
def exact_stem(name):
    """Integer image and filter, no BatchNorm: (x, w, expected = relu(conv)) -- exact in float32 in any order (49 products of at most 16)."""
    c = STEM_BY_NAME[name]
    g = _gen("exact " + name)
    x = torch.randint(-8, 9, (c.B, 1, c.H, c.W), generator=g).float()
    w = torch.randint(-2, 3, (c.C0, 1, 7, 7), generator=g).float()
    return x, w, F.relu(F.conv2d(x.double(), w.double(), stride=2, padding=3))


# ---- FPN top-down step: upsample2x_add and conv1x1_upsample_add ----------------------------------------------------------------------------
UpCase = namedtuple("UpCase", "name fused B C cin Hl Wl edges")
UP_EDGES = {
    "low_1x1": lambda c: (c.Hl, c.Wl) == (1, 1),
    "low_one_row": lambda c: c.Hl == 1 and c.Wl > 1,
    "low_one_column": lambda c: c.Wl == 1 and c.Hl > 1,
    "low_2x2": lambda c: (c.Hl, c.Wl) == (2, 2),
    "fused_M_256": lambda c: c.fused and c.B * 4 * c.Hl * c.Wl == 256,
    "fused_M_260_ragged": lambda c: c.fused and c.B * 4 * c.Hl * c.Wl == 260,
    "fused_M_512": lambda c: c.fused and c.B * 4 * c.Hl * c.Wl == 512 and c.B == 1,
    "fused_tile_spans_images": lambda c: c.fused and c.B >= 3 and 4 * c.Hl * c.Wl < BM // 2,
    "several_images": lambda c: c.B >= 3,
    "five_images_3x4": lambda c: c.B == 5 and (c.Hl, c.Wl) == (3, 4),
    "pad_channels": lambda c: c.C % 32 != 0,
    "C_512": lambda c: c.C == 512,
    "C_below_128": lambda c: c.C == 40,
    "map_15x20": lambda c: (c.Hl, c.Wl) == (15, 20),
    "map_8x16": lambda c: (c.Hl, c.Wl) == (8, 16),
}
UP_CHANNELS = (40, 128, 196, 256, 512)


def _build_up_cases():
    cases = []
    sizes = ((1, 1, ("low_1x1",)), (1, 7, ("low_one_row",)), (7, 1, ("low_one_column",)), (2, 2, ("low_2x2",)), (8, 16, ("map_8x16",)), (15, 20, ("map_15x20",)))
    for fused in (False, True):
        for si, (Hl, Wl, e) in enumerate(sizes):
            for ci, C in enumerate(UP_CHANNELS):
                B = 3 if (si + ci) % 2 else 1
                ce = {40: ("pad_channels", "C_below_128"), 196: ("pad_channels",), 512: ("C_512",)}.get(C, ())
                extra = (("several_images",) if B == 3 else ()) + (("fused_M_512",) if fused and B == 1 and (Hl, Wl) == (8, 16) else ()) \
                    + (("fused_tile_spans_images",) if fused and B == 3 and 4 * Hl * Wl < BM // 2 else ())
                cases.append(UpCase(f"{'f' if fused else 'u'}_{Hl}x{Wl}_c{C}_b{B}", fused, B, C, 128 if C != 128 else 196, Hl, Wl, e + ce + extra))
        for C in (196, 512):
            cases.append(UpCase(f"{'f' if fused else 'u'}_3x4_c{C}_b5", fused, 5, C, 128, 3, 4,
                                ("five_images_3x4", "several_images") + (("fused_tile_spans_images",) if fused else ())))
    cases.append(UpCase("f_8x8_c196_b1", True, 1, 196, 128, 8, 8, ("fused_M_256", "pad_channels")))
    cases.append(UpCase("f_5x13_c256_b1", True, 1, 256, 40, 5, 13, ("fused_M_260_ragged",)))
    return cases


UP_CASES = _build_up_cases()
UP_BY_NAME = {c.name: c for c in UP_CASES}
assert len(UP_BY_NAME) == len(UP_CASES)
assert not [(c.name, e) for c in UP_CASES for e in c.edges if not UP_EDGES[e](c)]
assert {e for c in UP_CASES for e in c.edges} == set(UP_EDGES)
assert all({(c.Hl, c.Wl, c.C) for c in UP_CASES if c.fused == f} >= {(h, w, C) for h, w in ((1, 1), (1, 7), (7, 1), (2, 2), (8, 16), (15, 20)) for C in UP_CHANNELS}
           for f in (False, True))


@functools.lru_cache(maxsize=None)
def up_inputs(name):
    c = UP_BY_NAME[name]
    g = _gen(name)
    low = torch.randn(c.B, c.C, c.Hl, c.Wl, generator=g)
    if c.fused:
        return dict(case=c, low=low, x=torch.randn(c.B, c.cin, 2 * c.Hl, 2 * c.Wl, generator=g), w=torch.randn(c.C, c.cin, 1, 1, generator=g) / c.cin ** 0.5)
    return dict(case=c, low=low, lat=torch.randn(c.B, c.C, 2 * c.Hl, 2 * c.Wl, generator=g))


UP_MUTATIONS = ("bilinear_uses_the_align_corners_false_scale",)


def up_forward(i, dt, mutation=None):
    c = i["case"]
    lat = F.conv2d(i["x"].to(dt), i["w"].to(dt)) if c.fused else i["lat"].to(dt)
    return lat + F.interpolate(i["low"].to(dt), scale_factor=2.0, mode="bilinear", align_corners=mutation != "bilinear_uses_the_align_corners_false_scale")


@functools.lru_cache(maxsize=None)
def up_reference(name):
    i = up_inputs(name)
    r64, r32 = _pair(lambda dt: up_forward(i, dt))
    return dict(ref64=r64, ref32=r32, channels=r64.shape[0] * r64.shape[2] * r64.shape[3] >= CHANNEL_MIN_PIXELS, **_stats(r64, r32))


def up_kind(c):
    return "fused" if c.fused else "up"


# ---- whole network --------------------------------------------------------------------------------------------------------------------------
NetCase = namedtuple("NetCase", "name resolution dims B H W edges")
NET_CASES = [NetCase(f"n_{r[0]}_{r[1]}_{H}x{W}_b{B}", r, d, B, H, W, e)
             for r, d, shapes in (((8, 2), (128, 196, 256), ((8, 8, "coarse_map_1x1"), (8, 264, "coarse_map_1x33"), (24, 40, "coarse_map_3x5"))),
                                  ((16, 4), (128, 196, 256, 512), ((16, 16, "coarse_map_1x1"), (48, 80, "coarse_map_3x5"))))
             for H, W, e in shapes for B in (1, 3)]
NET_BY_NAME = {c.name: c for c in NET_CASES}
assert len(NET_BY_NAME) == 10
for _c in NET_CASES:
    _ch, _cw = _c.H // _c.resolution[0], _c.W // _c.resolution[0]
    assert _c.H % _c.resolution[0] == 0 and _c.W % _c.resolution[0] == 0 and f"coarse_map_{_ch}x{_cw}" == _c.edges, _c


def net_module(c):
    """The backbone of a case with seeded weights and BatchNorm statistics (float32, CPU, eval)."""
    from loftr_amd.backbone import build_backbone
    cfg = {"backbone_type": "ResNetFPN", "resolution": c.resolution, "resnetfpn": {"initial_dim": 128, "block_dims": list(c.dims)}}
    torch.manual_seed(zlib.crc32(repr(c.resolution).encode()))
    m = build_backbone(cfg).eval()
    g = _gen("bn " + repr(c.resolution))
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            n = mod.num_features
            mod.weight.data = 1.0 + 0.2 * torch.randn(n, generator=g)
            mod.bias.data = 0.1 * torch.randn(n, generator=g)
            mod.running_mean.data = 0.1 * torch.randn(n, generator=g)
            mod.running_var.data = 0.5 + torch.rand(n, generator=g)
    return m


@functools.lru_cache(maxsize=None)
def net_reference(name):
    """x [B, 1, H, W] and, per output (coarse, fine), ref64 / ref32 / noise / scale of the module's own forward on the CPU."""
    c = NET_BY_NAME[name]
    x = torch.rand(c.B, 1, c.H, c.W, generator=_gen(name))
    with torch.no_grad():
        m = net_module(c)
        r32 = [t.double().numpy().copy() for t in m(x)]
        r64 = [t.numpy().copy() for t in m.double()(x.double())]
    outs = []
    for a, b in zip(r64, r32):
        _freeze(a, b)
        outs.append(dict(ref64=a, ref32=b, noise=float(np.abs(a - b).max()), scale=float(np.abs(a).max())))
    return dict(case=c, x=x, outs=outs)


# ---- position in the batch: the same image three times, at different offsets inside a row tile / different tiles of the grid ---------------
POSITION_CONV = ("g_five_images", "g_cout129", "g_cin40", "g_m255", "c_16to128_9x33", "c_196to192_9x33", "c_196to196_9x33", "c_64to40_9x33", "c_196to196_9x33_rem")
POSITION_STEM = ("s_17x65_c40_b3", "s_50x71_c40_b1_crop", "s_1x1_c128_b1")
POSITION_UP = ("u_3x4_c196_b5", "f_3x4_c196_b5", "f_1x7_c196_b3")
assert set(POSITION_CONV) <= set(CONV_BY_NAME) and set(POSITION_STEM) <= set(STEM_BY_NAME) and set(POSITION_UP) <= set(UP_BY_NAME), \
    (set(POSITION_CONV) - set(CONV_BY_NAME), set(POSITION_STEM) - set(STEM_BY_NAME), set(POSITION_UP) - set(UP_BY_NAME))
for _n in POSITION_CONV:          # three images: the second and third start inside a row tile (implicit GEMM) / on another tile of the grid
    _c = CONV_BY_NAME[_n]
    assert _c.family != "gemm" or (_ho_wo(_c)[0] * _ho_wo(_c)[1]) % BM != 0

# ---- guard bands: the ragged and the minimal cases ------------------------------------------------------------------------------------------
GUARD_WORD = 0x7E007E00            # an SP word of two fp16 NaNs
GUARD_OUT_WORDS = 4096
GUARD_CONV = tuple(c.name for c in CONV_CASES if c.weights == "plain" and not c.switches and conv_flops(c) < 1.2e9 and
                   ((c.family == "gemm" and (c.B * _ho_wo(c)[0] * _ho_wo(c)[1]) % BM != 0) or (c.family != "gemm" and (c.H % TY != 0 or c.W % TX != 0))))
GUARD_STEM = tuple(c.name for c in STEM_CASES if (c.H, c.W) in ((1, 1), (17, 65), (50, 71)))
GUARD_UP = tuple(c.name for c in UP_CASES if not c.fused and ((c.Hl, c.Wl) in ((1, 1), (1, 7), (7, 1), (3, 4)) or c.name == "u_15x20_c196_b3"))
GUARD_FUSED = tuple(c.name for c in UP_CASES if c.fused and ((c.Hl, c.Wl) in ((1, 1), (1, 7), (7, 1), (3, 4), (5, 13))))
assert {CONV_BY_NAME[n].family for n in GUARD_CONV} == set(FAMILIES) and len(GUARD_STEM) == 12 and len(GUARD_UP) >= 17 and len(GUARD_FUSED) >= 17
