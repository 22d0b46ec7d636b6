"""Case tables, float64 references and tolerances of the edge tests of the matching heads' backward.

tests/test_hip_head_bwd_edges.py (GPU) compares, at the sizes where their hand-written work distribution changes path,
  * ops.dual_softmax_bwd and autograd.dual_softmax_match(...)["conf_matrix"].backward(G)   (csrc/dual_softmax_bwd.h: dsb::row_dot_kernel /
    dsim_kernel, one wave per row, 4 rows per block, lanes stride 64 over S; col_dot_part_kernel, 256 columns per block, RCH = 32 chunks
    of ceil(L / 32) rows; the forward's statistics and store passes re-run -- the sweep at C = 256, the generic 128 x 128 tiles otherwise);
  * ops.sinkhorn_bwd and autograd.sinkhorn_match(...)["conf_matrix_with_bin"].backward(G)   (csrc/sinkhorn_bwd.h: otb::row_step_kernel, one
    wave per PADDED row; col_step_kernel, 256 padded columns per block, 32 chunks over the L + 1 rows; col_merge_kernel; dbin_kernel, 1024
    threads over N (L + S + 1) entries; ot_iterate re-run with save_u / save_v in its narrow, wide and fallback variants);
  * ops.fine_match_bwd   (csrc/train_bwd.hip: one wave per match, 4 per block, a 64-channel stride with a `c < C` guard);
  * LoFTRLoss's d loss_c / d conf and d loss_f / d expec_f on synthetic leaves   (loss_grad_dense_kernel: 1024 blocks stride over the N L
    rows, 256 threads stride over S; loss_grad_gather_kernel / loss_grad_bins_kernel / fine_loss_grad_kernel: 256 entries per block)
with references in FLOAT64.  tests/test_head_bwd_oracle.py (CPU) holds every condition stated here and shows that the comparison can fail.

References.  The two heads are restated in torch (`dual_softmax_head`, `sinkhorn_head`) and run under torch.autograd on the CPU, on the
float64 casts of the float32 inputs (ref64) and on the inputs themselves (ref32); `retain_grad()` on the score matrix BEFORE the mask fill
(d sim: exactly 0 where the fill cut the graph) and on the padded couplings (d Z).  The CPU test pins them to the committed grad_ds*,
grad_dense_mask, grad_ce and grad_ot* fixtures (float32) and to oracle.grad_oracle's hand-derived dual_softmax_conf_grad /
sinkhorn_conf_grad (float64, 1e-10 of the scale).  fine_match_bwd and the loss gradients: oracle.grad_oracle with dtype float64 / float32.

Inputs.  Seeded float32 descriptors with planted correspondences (spread_pairs of tests/_sinkhorn_cases.py: every token of the longer side
has a partner among the valid tokens of the other).  Masked cases use 1 x L and 1 x S grids, so that a prefix of v valid tokens IS the valid
rectangle (1, v) the model produces; everything else uses `grid` of tests/_score_sweep_cases.py.  (Its `masks` builds two fixed patterns
for its own shapes; the three patterns of this table are prefixes, stated in MASKS.)

Tolerance, per output tensor, by group (dsim; dZ; feat: the descriptor gradients; dbin; fine: d0, d1; loss):
  absolute   err = max|got - ref64| <= K_ABS[group] noise + 1e-6 scale,   noise = max|ref32 - ref64|, scale = max|ref64|;
  row-wise   (d sim, d Z, the descriptor gradients, d1)   max over rows of max_j|got - ref64| / max_j|ref64| <= K_ROW[group] (the same for
             ref32) + 1e-6, over the rows whose ref64 maximum is at least ROW_FLOOR of the tensor's scale.
d bin_score, one number, is compared twice: with ref64 under the same rule (not on the six DBIN_UNCLAIMED cases, where a side has 1 or 3
tokens), and on every case with the float64 sum of the run's OWN d Z dustbin entries, to one float32 ulp (`dbin_self_tolerance`).
Exact conditions are asserted apart: finite; d sim exactly 0 on mask-filled entries; descriptor-gradient rows of masked tokens exactly 0;
d0 exactly 0 off the centre row; grad_conf exactly 0 wherever ref64 is.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import grad_oracle as GO
from _score_sweep_cases import TEMPERATURE, grid, chunk_panels, _cdiv, _freeze
from _sinkhorn_cases import ot_plan, variants, spread_pairs, fallback_chunks, NARROW, WIDE_ITER, NARROW_MAX, ROWSTREAM_MAX

# ---- tolerance ------------------------------------------------------------------------------------------------------------------------
# K = twice the largest err / noise measured on an MI355X over all cases and tensors of the group, rounded up to an integer (the rule of
# tests/_sinkhorn_cases.py).  d sim and d Z have constants of their own: they come from different kernels.  Three ratios are beyond the 12
# the earlier suites stopped at, and are adopted for what they are:
#   * d Z, absolute (8.17 at ot_col_S62): the reference's float32 run is unusually close there (noise 1.7e-7 of the scale, a third of an
#     ulp of the largest entry), not the kernels far: err is 1.4e-6 of the scale, on the largest entry, and that is the three float32
#     roundings of z + u + v - norm in the argument of the exponential, its terms of magnitude 8 to 16 (half an ulp: 4.8e-7 .. 9.5e-7 --
#     an absolute error of the argument is a relative one of exp), as tests/_sinkhorn_cases.py found for the forward's dustbins.
#   * descriptor gradients, row-wise (6.09 at ot_col_S255 feat1): loftr_head_feat_grads forms d sim^T feat_c0 from operands split into
#     (hi, lo) fp16 halves under ONE running power-of-two scale per operand tile (csrc/head_grads.hip), so a row far below its tile's
#     maximum carries the tile's absolute error; float32 matmul rounds row by row.  5.1e-5 is a quarter of the 2e-4 that
#     tests/test_hip_grad.py::test_head_feat_grads_vs_fp64 holds that kernel to row by row.
#   * d bin_score (8.17 at ot_C128_masked): it is the sum of the dustbin entries of d Z and inherits their error, which does not average
#     out: every entry of the dustbin row carries the rounding of the one u_L in its exponential's argument, every entry of the dustbin
#     column that of v_S.  err is 3.2e-6 of |d bin_score| there, float32 torch happens to be at 4e-7.  The self check below is the sharp one.
# The lines of profiles/head_bwd_accuracy.txt the constants were taken from:
#   K_ABS["dsim"] =  4 <- 1.52   ds_mask_b_257x160      dsim       dsim  abs err 5.174e-07 noise 3.394e-07 err/noise   1.52 scale 5.572e-01
#   K_ROW["dsim"] =  4 <- 1.81   ds_C32                 dsim       dsim  row err 3.270e-06 noise 1.808e-06 err/noise   1.81 scale 7.595e-01
#   K_ABS["dZ"]   = 17 <- 8.17   ot_col_S62             dZ         dZ    abs err 7.533e-06 noise 9.218e-07 err/noise   8.17 scale 5.545e+00
#   K_ROW["dZ"]   =  8 <- 3.64   ot_row_L257            dZ         dZ    row err 2.703e-05 noise 7.436e-06 err/noise   3.64 scale 1.177e+01
#   K_ABS["feat"] =  5 <- 2.12   ot_col_S960            feat0      feat  abs err 2.030e-08 noise 9.596e-09 err/noise   2.12 scale 1.297e-02
#   K_ROW["feat"] = 13 <- 6.09   ot_col_S255            feat1      feat  row err 5.147e-05 noise 8.445e-06 err/noise   6.09 scale 1.261e-02
#   K_ABS["dbin"] = 17 <- 8.17   ot_C128_masked         dbin       dbin  abs err 3.586e-05 noise 4.391e-06 err/noise   8.17 scale 1.107e+01
#   K_ABS["fine"] =  7 <- 3.16   fine_peaked            d0         fine  abs err 3.849e-06 noise 1.217e-06 err/noise   3.16 scale 2.336e-01
#   K_ROW["fine"] =  6 <- 2.80   fine_C96               d1         fine  row err 6.130e-05 noise 2.192e-05 err/noise   2.80 scale 1.929e-01
#   K_ABS["loss"] =  2 <- 1.00   loss_k0_M1             grad_conf  loss  abs err 1.176e-08 noise 1.176e-08 err/noise   1.00 scale 8.297e-01
# (the loss kernels evaluate each entry in double and round once: their error IS float32's rounding of the result.)
K_ABS = {"dsim": 4, "dZ": 17, "feat": 5, "dbin": 17, "fine": 7, "loss": 2}
K_ROW = {"dsim": 4, "dZ": 8, "feat": 13, "fine": 6}
ROW_FLOOR = 1e-7            # below the smallest share of the scale any row with a gradient has in the table (3.4e-7: ds_col_S1, where a row of d sim is
                            # t_i - A_i c, a difference); the CPU test asserts that no such row is left out
DETECTION_FACTOR = 10.0     # a modelled mistake sits this many tolerances from ref64 in at least one compared tensor, on every case it applies to
GROUP = {"dsim": "dsim", "dZ": "dZ", "feat0": "feat", "feat1": "feat", "dbin": "dbin", "d0": "fine", "d1": "fine", "grad_conf": "loss",
         "grad_expec": "loss"}
ROW_CHECKED = ("dsim", "dZ", "feat0", "feat1", "d1")


def abs_tolerance(key, noise, scale):
    return K_ABS[GROUP[key]] * noise + 1e-6 * scale


def row_tolerance(key, noise_row):
    return K_ROW[GROUP[key]] * noise_row + 1e-6


def row_ratio(x, ref64, rows):
    """max over the rows `rows` (bool, ref64's shape without its last axis) of max_j|x - ref64| / max_j|ref64|."""
    if not rows.any():
        return 0.0
    num, den = np.abs(x - ref64).max(-1), np.abs(ref64).max(-1)
    return float((num[rows] / den[rows]).max())


def checked_rows(ref64):
    den = np.abs(ref64).max(-1)
    return (den >= ROW_FLOOR * den.max()) & (den > 0)


def measure(got, r):
    """[(tensor, check, err, noise, scale, tolerance)] of `got` ({tensor: array}) against the reference record r."""
    out = []
    for k, v in got.items():
        v = np.asarray(v, np.float64)
        out.append((k, "abs", float(np.abs(v - r["ref64"][k]).max()), r["noise"][k], r["scale"][k], abs_tolerance(k, r["noise"][k], r["scale"][k])))
        if k in ROW_CHECKED:
            out.append((k, "row", row_ratio(v, r["ref64"][k], r["rows"][k]), r["noise_row"][k], r["scale"][k], row_tolerance(k, r["noise_row"][k])))
    return out


def distance_in_tolerances(got, r):
    d = 0.0
    for _, _, err, _, _, tol in measure(got, r):
        d = max(d, err / tol if tol > 0 else (0.0 if err == 0 else math.inf))
    return d


def _record(ref64, ref32, keys):
    """noise, scale, checked rows and row-wise noise of the tensors `keys`."""
    f = lambda a: np.asarray(a, np.float64)
    rows = {k: checked_rows(f(ref64[k])) for k in keys if k in ROW_CHECKED}
    return dict(ref64=ref64, ref32=ref32, noise={k: float(np.abs(f(ref32[k]) - f(ref64[k])).max()) for k in keys},
                scale={k: float(np.abs(f(ref64[k])).max()) for k in keys}, rows=rows,
                noise_row={k: row_ratio(f(ref32[k]), f(ref64[k]), rows[k]) for k in rows})


# ---- the kernels' work distribution, restated -------------------------------------------------------------------------------------------
RCH, WAVES, LANES, COLS = 32, 4, 64, 256       # row chunks of the column passes; rows (waves) per block; lane stride; columns per block
TILE, WARPS = 128, 2                            # GemmCfg<128, 128, 2, 2>: PI = ceil(L / 128) 2, PJ = ceil(S / 128) 2 (make_geometry)
DBIN_THREADS, LOSS_BLOCKS = 1024, 1024


def col_chunks(rows):
    """(rows per chunk, non-empty chunks, rows in the last non-empty chunk) of col_dot_part_kernel / col_step_kernel over `rows` rows."""
    per = _cdiv(rows, RCH)
    n = _cdiv(rows, per)
    return per, n, rows - (n - 1) * per


def generic_partials(L, S):
    """(PI, PJ, rows in the last row tile, columns in the last column tile) of the C != 256 path."""
    return _cdiv(L, TILE) * WARPS, _cdiv(S, TILE) * WARPS, L - (_cdiv(L, TILE) - 1) * TILE, S - (_cdiv(S, TILE) - 1) * TILE


assert [col_chunks(L) for L in (1, 31, 32, 33, 65, 257)] == [(1, 1, 1), (1, 31, 1), (1, 32, 1), (2, 17, 1), (3, 22, 2), (9, 29, 5)]
assert [col_chunks(L + 1) for L in (1, 30, 31, 32, 63, 257)] == [(1, 2, 1), (1, 31, 1), (1, 32, 1), (2, 17, 1), (2, 32, 2), (9, 29, 6)]
assert chunk_panels(961) == [16, 15] and 961 % 32 == 1
assert generic_partials(129, 127) == (4, 2, 1, 127) and generic_partials(33, 257) == (2, 6, 33, 1)

# ---- the two heads: cases ----------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name head N L S C iters bin_score G mask amp want1 seed edges")
# planted weight, descriptor amplitude, weight of a token's further partners relative to its first, background.  ds: the `flat` regime of
# tests/_score_sweep_cases.py (planted scores of 5 at temperature 0.1, further partners 3); ot: the `ot` regime of tests/_sinkhorn_cases.py (planted scores of 6, no temperature).
REGIMES = {"ds": (0.5, 1.0, 0.6, 0.25), "ot": (1.5, 2.0, 0.6, 0.25)}
BIN_SCORE, SKH_ITERS = 1.0, 3
SEEDS = {"ds_G_loss": 2}      # name -> seed other than 0: column 256, alone in the second 256-column block and the fifth lane stride, has to carry
                              # a supervised (full-weight) pair, or the loss gradient has nothing to lose there (seed 0: a further partner)
# valid prefixes (v0, v1) by pattern and pair; pairs not listed are whole.  a: pair 0's valid extent ends inside a row chunk (and inside a
# lane stride), pair 1 keeps rows 0 .. 31 only (from 32 on: whole dead 32-row units of the sweep), pair 2 whole;  b: pair 0 has ONE valid
# token on each side, pair 1 whole, pair 2 ends inside a chunk on both sides.  c (N = 2, the C != 256 shape): rows and columns end inside
# the first tile (pair 0), the columns alone (pair 1).
MASKS = {
    ("a", 257, 160): {0: (100, 109), 1: (32, 160)},
    ("b", 257, 160): {0: (1, 1), 2: (230, 75)},
    ("a", 33, 257): {0: (21, 200), 1: (32, 257)},
    ("b", 33, 257): {0: (1, 1), 2: (29, 130)},
    ("c", 129, 127): {0: (100, 90), 1: (129, 100)},
}
# Iteration-variant cases (S = 5119 .. 12288 at L = 3 or 129): the upstream gradient is dense but for the dustbin row (`norow`).  With L
# tokens against S the dustbin row supplies 1 - L / S of every column's mass, Pc_Lj is that close to 1, and d Z_Lj = D_Lj - dv_j Pc_Lj
# with dv_j = D_Lj + (the real rows' share) cancels to L / S of its operands: 6e-4 at L = 3, where float32 torch is 1.7e-4 of the scale
# off.  With D_Lj = 0 nothing cancels (float32 torch within 3e-6 of the scale on d Z, row by row too); the re-run iteration kernels, which
# is what these cases are in the table for, are the same.
# d bin_score is NOT compared with ref64 on the cases below.  One side has 1 or 3 tokens there: the dustbin row (or column) holds nearly
# all the mass whatever bin_score is, d L / d bin_score is a sum of N (L + S + 1) entries of d Z that cancels to 1e-2 .. 1e-5 of their size
# under every upstream gradient, and float32 torch is 7e-5 .. 7e-3 of |d bin_score| off.  What is held there instead: every dustbin entry
# of d Z against ref64 (absolute and row by row), and d bin_score against the float64 sum of those entries of the SAME run.
DBIN_UNCLAIMED = ("ot_row_L1", "ot_col_S1", "ot_var_S5119", "ot_var_S5120", "ot_var_S12287", "ot_var_S12288")
DBIN_TOLERANCE_SHARE = 1e-3   # where d bin_score IS compared with ref64 its tolerance stays below this share of |d bin_score| (CPU test)

EDGES = {
    # dual softmax, rows
    "one_row": lambda c: c.L == 1 and col_chunks(c.L) == (1, 1, 1),
    "last_chunk_empty": lambda c: c.L == 31 and col_chunks(c.L)[:2] == (1, 31),
    "one_row_per_chunk": lambda c: c.L == 32 and col_chunks(c.L) == (1, 32, 1),
    "two_rows_per_chunk_15_empty": lambda c: c.L == 33 and col_chunks(c.L) == (2, 17, 1),
    "22_chunks_last_of_two": lambda c: c.L == 65 and col_chunks(c.L) == (3, 22, 2),
    "29_chunks_last_of_five": lambda c: c.L == 257 and col_chunks(c.L) == (9, 29, 5),
    "block_spans_two_pairs": lambda c: c.N > 1 and _rows(c) % WAVES != 0,
    "rows_mod4_1": lambda c: c.N * _rows(c) % WAVES == 1,
    "rows_mod4_2": lambda c: c.N * _rows(c) % WAVES == 2,
    "rows_mod4_3": lambda c: c.N * _rows(c) % WAVES == 3,
    "rows_mod4_0": lambda c: c.N * _rows(c) % WAVES == 0,
    # columns (ds: S; ot: S + 1 padded columns)
    "one_column": lambda c: c.S == 1,
    "below_one_stride": lambda c: _cols(c) == LANES - 1,
    "one_stride": lambda c: _cols(c) == LANES,
    "second_stride_of_one": lambda c: _cols(c) == LANES + 1,
    "below_one_block": lambda c: _cols(c) == COLS - 1,
    "one_block": lambda c: _cols(c) == COLS,
    "second_block_of_one": lambda c: _cols(c) == COLS + 1,
    "two_sweep_chunks_ragged_panel": lambda c: c.C == 256 and c.S == 961 and chunk_panels(c.S) == [16, 15] and c.S % 32 == 1,
    "aligned": lambda c: c.head == "ot" and ot_plan(c.N, c.L, c.S).aligned and c.S % 4 == 0,
    "unaligned": lambda c: c.head == "ot" and not ot_plan(c.N, c.L, c.S).aligned,
    # masks
    "masked": lambda c: c.mask is not None,
    "mask_ends_inside_chunk": lambda c: any(v0 % col_chunks(_rows(c))[0] != 0 and 1 < v0 < c.L for v0, _ in MASKS[(c.mask, c.L, c.S)].values()),
    "mask_dead_units_from_32": lambda c: any(v0 == 32 < c.L for v0, _ in MASKS[(c.mask, c.L, c.S)].values()),
    "mask_one_token": lambda c: (1, 1) in MASKS[(c.mask, c.L, c.S)].values(),
    "mask_one_pair_whole": lambda c: len(MASKS[(c.mask, c.L, c.S)]) < c.N,
    # upstream gradients
    "G_dense": lambda c: c.G == "dense",
    "G_sparse": lambda c: c.G == "sparse",
    "G_loss": lambda c: c.G == "loss",
    "G_rows": lambda c: c.G == "rows",
    "G_bins": lambda c: c.G == "bins",
    "G_norow": lambda c: c.G == "norow",
    # the generic score path
    "generic_C32": lambda c: c.C == 32,
    "generic_C128": lambda c: c.C == 128,
    "generic_second_row_tile_of_one": lambda c: c.C != 256 and generic_partials(c.L, c.S) == (4, 2, 1, 127),
    "generic_third_column_tile_of_one": lambda c: c.C != 256 and generic_partials(c.L, c.S) == (2, 6, 33, 1),
    # Sinkhorn
    "padded_rows_2": lambda c: c.L + 1 == 2,
    "padded_rows_31": lambda c: c.L + 1 == 31 and col_chunks(c.L + 1)[:2] == (1, 31),
    "padded_rows_32": lambda c: c.L + 1 == 32 and col_chunks(c.L + 1) == (1, 32, 1),
    "padded_rows_33": lambda c: c.L + 1 == 33 and col_chunks(c.L + 1) == (2, 17, 1),
    "padded_rows_64": lambda c: c.L + 1 == 64 and col_chunks(c.L + 1) == (2, 32, 2),
    "padded_rows_258": lambda c: c.L + 1 == 258 and col_chunks(c.L + 1) == (9, 29, 6),
    "last_narrow": lambda c: c.S + 1 == NARROW_MAX and variants(c.S)[0] == NARROW and ot_plan(c.N, c.L, c.S).rowstream,
    "first_wide": lambda c: c.S == NARROW_MAX and variants(c.S)[0] == WIDE_ITER and ot_plan(c.N, c.L, c.S).rowstream,
    "last_wide": lambda c: c.S + 1 == ROWSTREAM_MAX and variants(c.S)[0] == WIDE_ITER and ot_plan(c.N, c.L, c.S).rowstream,
    "first_fallback": lambda c: c.S == ROWSTREAM_MAX and not ot_plan(c.N, c.L, c.S).rowstream,
    "fallback_two_rows_per_chunk": lambda c: not ot_plan(c.N, c.L, c.S).rowstream and fallback_chunks(c.L)[0] == 2,
    "iters_0": lambda c: c.iters == 0,
    "iters_1": lambda c: c.iters == 1,
    "iters_2": lambda c: c.iters == 2,
    "bin_low": lambda c: c.bin_score == -3.0,
    "dbin_below_1024": lambda c: c.N * (c.L + c.S + 1) < DBIN_THREADS,
    "dbin_above_1024": lambda c: c.N * (c.L + c.S + 1) > DBIN_THREADS,
    "only_feat_c0": lambda c: not c.want1,
}


def _rows(c):
    return c.L + (c.head == "ot")


def _cols(c):
    return c.S + (c.head == "ot")


def _mod4(N, rows):
    return f"rows_mod4_{N * rows % WAVES}"


def _build_cases():
    cases = []

    def add(name, head, N, L, S, *edges, C=256, iters=SKH_ITERS, bin_score=BIN_SCORE, G="dense", mask=None, amp=1.0, want1=True):
        e = list(edges) + [_mod4(N, L + (head == "ot")), "G_" + G]
        if head == "ot":
            e += ["aligned" if S % 4 == 0 else "unaligned", "dbin_below_1024" if N * (L + S + 1) < DBIN_THREADS else "dbin_above_1024"]
        if mask is not None:
            e += ["masked"]
        cases.append(Case(name, head, N, L, S, C, iters, float(bin_score), G, mask, amp, want1, SEEDS.get(name, 0), tuple(e)))
    # dual softmax
    for L, e in ((1, "one_row"), (31, "last_chunk_empty"), (32, "one_row_per_chunk"), (33, "two_rows_per_chunk_15_empty"),
                 (65, "22_chunks_last_of_two"), (257, "29_chunks_last_of_five")):
        add(f"ds_row_L{L}", "ds", 3, L, 160, e, *(("block_spans_two_pairs",) if L % 4 else ()))
    add("ds_row_N2_L33", "ds", 2, 33, 160, "two_rows_per_chunk_15_empty", "block_spans_two_pairs")
    for S, e in ((1, "one_column"), (63, "below_one_stride"), (64, "one_stride"), (65, "second_stride_of_one"), (255, "below_one_block"),
                 (256, "one_block"), (257, "second_block_of_one"), (961, "two_sweep_chunks_ragged_panel")):
        add(f"ds_col_S{S}", "ds", 3, 33, S, e, "block_spans_two_pairs")
    for L, S in ((257, 160), (33, 257)):
        add(f"ds_mask_a_{L}x{S}", "ds", 3, L, S, "mask_ends_inside_chunk", "mask_dead_units_from_32", "mask_one_pair_whole", mask="a")
        add(f"ds_mask_b_{L}x{S}", "ds", 3, L, S, "mask_one_token", "mask_ends_inside_chunk", "mask_one_pair_whole", mask="b")
    for G in ("dense", "sparse", "loss", "rows"):
        add(f"ds_G_{G}", "ds", 3, 65, 257, "second_block_of_one", G=G)
    for C in (32, 128):
        add(f"ds_C{C}", "ds", 2, 129, 127, f"generic_C{C}", "generic_second_row_tile_of_one", C=C)
        add(f"ds_C{C}_masked", "ds", 2, 129, 127, f"generic_C{C}", "generic_second_row_tile_of_one", C=C, mask="c")
    add("ds_C128_33x257", "ds", 2, 33, 257, "generic_C128", "generic_third_column_tile_of_one", C=128)
    # Sinkhorn
    for L, e in ((1, "padded_rows_2"), (30, "padded_rows_31"), (31, "padded_rows_32"), (32, "padded_rows_33"), (63, "padded_rows_64"),
                 (257, "padded_rows_258")):
        add(f"ot_row_L{L}", "ot", 3, L, 160, e, *(("block_spans_two_pairs",) if (L + 1) % 4 else ()))
    for S, e in ((1, "one_column"), (62, "below_one_stride"), (63, "one_stride"), (64, "second_stride_of_one"), (254, "below_one_block"),
                 (255, "one_block"), (256, "second_block_of_one"), (960, None), (961, None)):
        add(f"ot_col_S{S}", "ot", 3, 33, S, *((e,) if e else ()), "block_spans_two_pairs")
    for S, e in ((5119, "last_narrow"), (5120, "first_wide"), (12287, "last_wide"), (12288, "first_fallback")):
        add(f"ot_var_S{S}", "ot", 2, 3, S, e, G="norow")
    add("ot_var_129x12288", "ot", 1, 129, 12288, "first_fallback", "fallback_two_rows_per_chunk", G="norow")
    for it in (0, 1, 2):
        add(f"ot_iters{it}", "ot", 2, 33, 65, f"iters_{it}", iters=it)
    for L, S in ((257, 160), (33, 257)):
        add(f"ot_mask_a_{L}x{S}", "ot", 3, L, S, "mask_ends_inside_chunk", "mask_dead_units_from_32", "mask_one_pair_whole", mask="a")
        add(f"ot_mask_b_{L}x{S}", "ot", 3, L, S, "mask_one_token", "mask_ends_inside_chunk", "mask_one_pair_whole", mask="b")
    add("ot_C128_masked", "ot", 2, 129, 127, "generic_C128", "generic_second_row_tile_of_one", C=128, mask="c")
    for G in ("dense", "loss", "bins"):
        add(f"ot_G_{G}", "ot", 3, 63, 257, "padded_rows_64", G=G)
    add("ot_bin-3", "ot", 2, 33, 65, "bin_low", bin_score=-3.0)
    add("ot_only_feat_c0", "ot", 2, 33, 65, "only_feat_c0", want1=False)
    return cases


CASES = _build_cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
DS_CASES = [c for c in CASES if c.head == "ds"]
OT_CASES = [c for c in CASES if c.head == "ot"]


def edge_failures():
    return [(c.name, e) for c in CASES for e in c.edges if not EDGES[e](c)]


assert not edge_failures(), edge_failures()
assert {e for c in CASES for e in c.edges} == set(EDGES), set(EDGES) - {e for c in CASES for e in c.edges}
assert max(c.N * (c.L + 1) * (c.S + 1) for c in CASES if c.S < 5000) == 3 * 258 * 161 and max(c.N * c.L * c.S for c in CASES) == 129 * 12288


def hw(c):
    """The two token grids: 1 x n where the case is masked (a valid prefix is then a valid rectangle), else the most nearly square."""
    return ((1, c.L), (1, c.S)) if c.mask is not None else (grid(c.L), grid(c.S))


def valid_tokens(c):
    """(v0 [N, L], v1 [N, S]) bool, or (None, None)."""
    if c.mask is None:
        return None, None
    v0, v1 = np.ones((c.N, c.L), bool), np.ones((c.N, c.S), bool)
    for n, (a, b) in MASKS[(c.mask, c.L, c.S)].items():
        assert 0 < a <= c.L and 0 < b <= c.S and n < c.N
        v0[n, a:] = False
        v1[n, b:] = False
    return v0, v1


# ---- the two heads, restated in torch ----------------------------------------------------------------------------------------------------
def dual_softmax_head(f0, f1, temperature, keep=None, hold=None):
    """conf_matrix [N, L, S] (coarse_matching.py:105-119).  hold: a dict that receives `raw` (the scores before the mask fill) and `sim`
    (after it), their gradients retained."""
    C = f0.shape[-1]
    raw = torch.einsum("nlc,nsc->nls", f0, f1) / (C * temperature)
    sim = raw if keep is None else raw.masked_fill(~keep, -1e9)
    if hold is not None:
        raw.retain_grad(); sim.retain_grad()
        hold.update(raw=raw, sim=sim)
    return torch.softmax(sim, 1) * torch.softmax(sim, 2)


def sinkhorn_head(f0, f1, alpha, iters, keep=None, hold=None):
    """conf_matrix_with_bin [N, L + 1, S + 1] = exp(log_optimal_transport(sim, alpha, iters)) (coarse_matching.py:121-132, SuperGlue's
    log_sinkhorn_iterations unrolled).  hold receives `Z`, the padded couplings, gradient retained."""
    N, L, C = f0.shape
    S = f1.shape[1]
    raw = torch.einsum("nlc,nsc->nls", f0, f1) / C
    sim = raw if keep is None else raw.masked_fill(~keep, -1e9)
    Z = torch.cat([torch.cat([sim, alpha.expand(N, L, 1)], -1), alpha.expand(N, 1, S + 1)], 1)
    if hold is not None:
        Z.retain_grad()
        hold.update(Z=Z)
    one = lambda x: torch.tensor(float(x), dtype=f0.dtype)
    norm = -(one(L) + one(S)).log()
    log_mu = torch.cat([norm.expand(L), one(S).log()[None] + norm])[None].expand(N, -1)
    log_nu = torch.cat([norm.expand(S), one(L).log()[None] + norm])[None].expand(N, -1)
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Z + v.unsqueeze(1), dim=2)
        v = log_nu - torch.logsumexp(Z + u.unsqueeze(2), dim=1)
    return (Z + u.unsqueeze(2) + v.unsqueeze(1) - norm).exp()


def run_head(head, f0, f1, G, dtype, temperature=TEMPERATURE, bin_score=BIN_SCORE, iters=SKH_ITERS, v0=None, v1=None):
    """The head under torch.autograd on the CPU in `dtype`: {conf, dsim | dZ, dbin, feat0, feat1} as numpy arrays (+ dsim_filled: the
    gradient at the scores AFTER the mask fill, which a backward that forgets the cut would hand on)."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)                       # (a copy: the shared inputs are read-only)
    a, b = t(f0).requires_grad_(True), t(f1).requires_grad_(True)
    keep = None if v0 is None else torch.tensor(v0[:, :, None] & v1[:, None, :])
    hold = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                          # one summation order whatever the thread count: ref32's distance to ref64 is a constant of the table
    try:
        if head == "ds":
            out = dual_softmax_head(a, b, temperature, keep, hold)
        else:
            alpha = torch.tensor(float(bin_score), dtype=dtype, requires_grad=True)
            out = sinkhorn_head(a, b, alpha, iters, keep, hold)
        out.backward(t(G))
    finally:
        torch.set_num_threads(threads)
    res = dict(conf=out.detach().numpy(), feat0=a.grad.numpy(), feat1=b.grad.numpy())
    if head == "ds":
        res.update(dsim=hold["raw"].grad.numpy(), dsim_filled=hold["sim"].grad.numpy())
    else:
        res.update(dZ=hold["Z"].grad.numpy(), dbin=np.atleast_1d(alpha.grad.numpy()))
    return res


HEAD_OUTPUTS = {"ds": ("dsim", "feat0", "feat1"), "ot": ("dZ", "dbin", "feat0", "feat1")}


def outputs_of(c):
    """The tensors of a case that are compared with ref64."""
    return tuple(k for k in HEAD_OUTPUTS[c.head] if (c.want1 or k != "feat1") and not (k == "dbin" and c.name in DBIN_UNCLAIMED))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Seeded float32 descriptors with planted correspondences, valid tokens, grids and the upstream gradient.  Read-only."""
    c = CASE_BY_NAME[name]
    weight, amp, more, background = REGIMES[c.head]
    rng = np.random.default_rng([c.N, c.L, c.S, c.C, c.seed, c.head == "ot"])
    f0 = rng.standard_normal((c.N, c.L, c.C)).astype(np.float32) * np.float32(amp * c.amp)
    f1 = rng.standard_normal((c.N, c.S, c.C)).astype(np.float32) * np.float32(amp * c.amp * background)
    v0, v1 = valid_tokens(c)
    corr = []
    for n in range(c.N):
        i0 = np.arange(c.L) if v0 is None else np.flatnonzero(v0[n])
        i1 = np.arange(c.S) if v1 is None else np.flatnonzero(v1[n])
        rows, cols, first = spread_pairs(i0, i1, rng)
        w = np.where(first, weight, more * weight).astype(np.float32)
        np.add.at(f1[n], cols, w[:, None] * f0[n, rows])
        corr.append((rows, cols, first))
    pad = c.head == "ot"
    shape = (c.N, c.L + pad, c.S + pad)
    planted = np.zeros(shape, bool)
    gt = np.zeros((c.N, c.L, c.S), np.float32)
    for n, (rows, cols, first) in enumerate(corr):
        planted[n, rows, cols] = True
        gt[n, rows[first], cols[first]] = 1
    dense = rng.standard_normal(shape).astype(np.float32)
    if c.G == "dense":
        G = dense
    elif c.G == "sparse":
        G = np.where(planted, dense, np.float32(0))
    elif c.G == "rows":                              # the rows' magnitudes span e^-14 = 8e-7
        G = dense * np.exp(-14.0 * rng.random((c.N, shape[1], 1))).astype(np.float32)
    elif c.G == "norow":                             # dense but for the dustbin row (see the iteration-variant cases)
        G = dense.copy()
        G[:, -1, :] = 0
    elif c.G == "bins":
        G = dense.copy()
        G[:, :-1, :-1] = 0
    elif c.G == "loss":                              # ref64's own loss gradient at ref64's own confidences: a fixed float32 input
        conf = run_head(c.head, f0, f1, np.zeros(shape, np.float32), torch.float64, bin_score=c.bin_score, iters=c.iters, v0=v0, v1=v1)["conf"]
        G = (GO.sparse_sinkhorn_loss_grad(conf, gt) if pad else GO.coarse_loss_grad(conf, gt, coarse_type="focal", sparse_spvs=False)).astype(np.float32)
    else:
        raise KeyError(c.G)
    G = np.ascontiguousarray(G, np.float32)
    _freeze(f0, f1, G, v0, v1, planted)
    return dict(case=c, f0=f0, f1=f1, G=G, v0=v0, v1=v1, hw=hw(c), corr=corr, planted=planted)


@functools.lru_cache(maxsize=None)
def reference(name):
    i = inputs(name)
    c = i["case"]
    kw = dict(bin_score=c.bin_score, iters=c.iters, v0=i["v0"], v1=i["v1"])
    ref64, ref32 = (run_head(c.head, i["f0"], i["f1"], i["G"], dt, **kw) for dt in (torch.float64, torch.float32))
    assert all(v.dtype == np.float64 for v in ref64.values()) and all(v.dtype == np.float32 for v in ref32.values())
    _freeze(*ref64.values(), *ref32.values())
    return _record(ref64, ref32, HEAD_OUTPUTS[c.head])


def dustbin_terms(dZ):
    """The N (L + S + 1) entries of d Z that d bin_score is the sum of (dustbin column, dustbin row with the corner), in float64."""
    dZ = np.asarray(dZ, np.float64)
    return np.concatenate([dZ[:, :-1, -1], dZ[:, -1, :]], axis=1)


def dbin_self_check(dZ, dbin):
    """(|dbin - sum|, tolerance): d bin_score against the float64 sum of the dustbin entries of the d Z it came with.  dbin_kernel adds the
    float32 entries in double and rounds once, so the two agree to one float32 ulp of the sum (1.2e-7), plus double's own rounding of the
    additions (1e-12 of sum |terms|, generous).  A corner counted twice, a pair read at another offset or a stride off by one is not a
    rounding."""
    t = dustbin_terms(dZ)
    return abs(float(np.asarray(dbin, np.float64).reshape(-1)[0]) - float(t.sum())), 1.2e-7 * abs(float(t.sum())) + 1e-12 * float(np.abs(t).sum())


def keep_of(i):
    return None if i["v0"] is None else i["v0"][:, :, None] & i["v1"][:, None, :]


# ---- the backward once more in float64 numpy, from its pieces, with one mistake built in -------------------------------------------------
DS_MUTATIONS = ("col_sum_omits_last_chunk", "row_sum_omits_last_stride", "factor_2_dropped", "mask_fill_not_zeroed", "r_and_c_exchanged")
OT_MUTATIONS = ("du_overwritten_at_T", "one_reverse_iteration_fewer", "col_sums_omit_dustbin_row", "log_mu_of_dustbin_for_all_rows",
                "corner_twice_in_dbin", "corner_left_out_of_dbin", "second_pair_dustbins_at_first_offset")


def mutation_applies(c, m):
    if c.head == "ds":
        return {"mask_fill_not_zeroed": c.mask is not None, "r_and_c_exchanged": c.L != c.S}.get(m, True)
    if m in ("corner_twice_in_dbin", "corner_left_out_of_dbin", "second_pair_dustbins_at_first_offset"):
        return c.N > 1 or m != "second_pair_dustbins_at_first_offset"        # (every case: the self check sees them where ref64 is not asked)
    if m == "col_sums_omit_dustbin_row" and c.G == "norow":
        return False                                  # (that row's D is 0 there: its share of the column sums is below the tolerance)
    if c.iters == 0:
        return False                                  # (nothing is summed over a step without an iteration)
    if m == "log_mu_of_dustbin_for_all_rows":
        return c.S > 1                                # (S = 1: log_mu of the dustbin row is log 1 + norm, that of every row)
    if m == "one_reverse_iteration_fewer":            # with 1 or 3 tokens on a side, and at 129 x 12288, the iteration has converged after two
        return min(c.L, c.S) > 3 and c.S < NARROW_MAX     # rounds: the first round's share of the gradient is below the tolerance (0.0 .. 1.7)
    return True


def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def dual_softmax_bwd_float64(name, mutation=None):
    """{dsim, feat0, feat1} from r_i, c_j and the elementwise combination, as csrc/dual_softmax_bwd.h forms them.  mutation None
    reproduces ref64 (tested)."""
    i = inputs(name)
    c = i["case"]
    f0, f1, G = i["f0"].astype(np.float64), i["f1"].astype(np.float64), i["G"].astype(np.float64)
    k = 1.0 / (c.C * TEMPERATURE)
    keep = keep_of(i)
    sim = np.einsum("nlc,nsc->nls", f0, f1) * k
    if keep is not None:
        sim = np.where(keep, sim, -1e9)
    A, B = _softmax(sim, 1), _softmax(sim, 2)
    t = G * A * B
    r, cj = t.sum(2), t.sum(1)
    if mutation == "col_sum_omits_last_chunk":
        per, n, _ = col_chunks(c.L)
        cj = t[:, :(n - 1) * per].sum(1)
    elif mutation == "row_sum_omits_last_stride":
        r = t[:, :, :LANES * ((c.S - 1) // LANES)].sum(2)
    two = 1.0 if mutation == "factor_2_dropped" else 2.0
    if mutation == "r_and_c_exchanged":
        d = two * t - A * r[:, :, None] - B * cj[:, None, :]
    else:
        d = two * t - B * r[:, :, None] - A * cj[:, None, :]
    if keep is not None and mutation != "mask_fill_not_zeroed":
        d = np.where(keep, d, 0.0)
    return dict(dsim=d, feat0=np.einsum("nls,nsc->nlc", d, f1) * k, feat1=np.einsum("nls,nlc->nsc", d, f0) * k)


def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def sinkhorn_bwd_float64(name, mutation=None):
    """{dZ, dbin, feat0, feat1}: the reverse pass of csrc/sinkhorn_bwd.h step by step.  mutation None reproduces ref64 (tested)."""
    i = inputs(name)
    c = i["case"]
    N, L, S, T = c.N, c.L, c.S, c.iters
    f0, f1, G = i["f0"].astype(np.float64), i["f1"].astype(np.float64), i["G"].astype(np.float64)
    keep = keep_of(i)
    sim = np.einsum("nlc,nsc->nls", f0, f1) / c.C
    if keep is not None:
        sim = np.where(keep, sim, -1e9)
    Z = np.full((N, L + 1, S + 1), c.bin_score)
    Z[:, :L, :S] = sim
    norm = -math.log(L + S)
    log_mu = np.full(L + 1, norm); log_mu[L] = math.log(S) + norm
    log_nu = np.full(S + 1, norm); log_nu[S] = math.log(L) + norm
    us, vs = [], [np.zeros((N, S + 1))]
    for _ in range(T):
        us.append(log_mu - _lse(Z + vs[-1][:, None, :], 2))
        vs.append(log_nu - _lse(Z + us[-1][:, :, None], 1))
    if T == 0:
        us.append(np.zeros((N, L + 1)))
    live = np.ones(L + 1); live[L] = 0.0 if mutation == "col_sums_omit_dustbin_row" else 1.0       # the rows a column sum sees
    log_mu_step = np.full(L + 1, log_mu[L]) if mutation == "log_mu_of_dustbin_for_all_rows" else log_mu
    D = G * np.exp(Z + us[-1][:, :, None] + vs[-1][:, None, :] - norm)
    dZ = D.copy()
    du, dv = D.sum(2), (D * live[None, :, None]).sum(1)
    for t in range(T, 1 if mutation == "one_reverse_iteration_fewer" else 0, -1):
        Pc = np.exp(Z + us[t - 1][:, :, None] + vs[t][:, None, :] - log_nu[None, None, :])
        step = dv[:, None, :] * Pc
        dZ -= step
        du = -step.sum(2) if (mutation == "du_overwritten_at_T" or t < T) else du - step.sum(2)
        Pr = np.exp(Z + vs[t - 1][:, None, :] + us[t - 1][:, :, None] - log_mu_step[None, :, None])
        step = du[:, :, None] * Pr
        dZ -= step
        dv = -(step * live[None, :, None]).sum(1)
    corner = dZ[:, L, S].sum()
    bins = lambda n: dZ[n, L, :].sum() + dZ[n, :L, S].sum()
    if mutation == "second_pair_dustbins_at_first_offset":
        dbin = sum(bins(0 if n == 1 else n) for n in range(N))
    else:
        dbin = sum(bins(n) for n in range(N))
    dbin += corner if mutation == "corner_twice_in_dbin" else -corner if mutation == "corner_left_out_of_dbin" else 0.0
    dsim = dZ[:, :L, :S] if keep is None else np.where(keep, dZ[:, :L, :S], 0.0)
    out = dict(dZ=dZ, dbin=np.atleast_1d(dbin), feat0=np.einsum("nls,nsc->nlc", dsim, f1) / c.C)
    if c.want1:
        out["feat1"] = np.einsum("nls,nlc->nsc", dsim, f0) / c.C
    return out


def head_bwd_float64(name, mutation=None):
    return (dual_softmax_bwd_float64 if CASE_BY_NAME[name].head == "ds" else sinkhorn_bwd_float64)(name, mutation)


def exact_violations(c, i, got):
    """The exact conditions a result misses: d sim non-zero on a mask-filled entry, a masked token's descriptor-gradient row non-zero."""
    bad = []
    if not all(np.isfinite(v).all() for v in got.values()):
        bad.append("not finite")
    if i["v0"] is not None:
        if "dsim" in got and np.any(np.asarray(got["dsim"])[~keep_of(i)] != 0):
            bad.append("dsim on mask-filled entries")
        if np.any(np.asarray(got["feat0"])[~i["v0"]] != 0) or ("feat1" in got and np.any(np.asarray(got["feat1"])[~i["v1"]] != 0)):
            bad.append("descriptor gradient of a masked token")
    return bad


@functools.lru_cache(maxsize=None)
def facts(name):
    i, r = inputs(name), reference(name)
    c = i["case"]
    keys = HEAD_OUTPUTS[c.head]
    f = dict(finite=all(bool(np.isfinite(r[k][o]).all()) for k in ("ref64", "ref32") for o in keys), noise=r["noise"], scale=r["scale"],
             noise_row=r["noise_row"], exact=exact_violations(c, i, {k: r["ref64"][k] for k in keys}))
    # the rows the row-wise check leaves out, and how many of them are not identically zero in ref64
    f["left_out"] = {k: int((~r["rows"][k] & (np.abs(r["ref64"][k]).max(-1) > 0)).sum()) for k in r["rows"]}
    f["zero_rows"] = {k: int((np.abs(r["ref64"][k]).max(-1) == 0).sum()) for k in r["rows"]}
    f["min_row_share"] = {k: float((np.abs(r["ref64"][k]).max(-1) / r["scale"][k])[np.abs(r["ref64"][k]).max(-1) > 0].min()) for k in r["rows"]}
    base = head_bwd_float64(name)
    f["formula_distance"] = {k: float(np.abs(base[k] - r["ref64"][k]).max()) / r["scale"][k] for k in base if k in outputs_of(c)}
    f["self_check"] = dbin_self_check(r["ref64"]["dZ"], r["ref64"]["dbin"]) if c.head == "ot" else (0.0, 1.0)
    if c.head == "ds":
        o = GO.dual_softmax_conf_grad(i["f0"], i["f1"], i["G"], TEMPERATURE, i["v0"], i["v1"])
        pairs = (("feat0", o[0]), ("feat1", o[1]))
    else:
        o = GO.sinkhorn_conf_grad(i["f0"], i["f1"], c.bin_score, i["G"], c.iters, i["v0"], i["v1"])
        pairs = (("feat0", o[0]), ("feat1", o[1]), ("dbin", np.atleast_1d(o[2])))
    f["oracle_distance"] = {k: float(np.abs(v - r["ref64"][k]).max()) / r["scale"][k] for k, v in pairs if k in outputs_of(c)}
    f["mutation_distance"] = {}
    for m in (DS_MUTATIONS if c.head == "ds" else OT_MUTATIONS):
        if mutation_applies(c, m):
            got = head_bwd_float64(name, m)
            err, tol = dbin_self_check(got["dZ"], got["dbin"]) if c.head == "ot" else (0.0, 1.0)
            got = {k: v for k, v in got.items() if k in outputs_of(c)}
            f["mutation_distance"][m] = math.inf if exact_violations(c, i, got) else max(distance_in_tolerances(got, r), err / tol)
    return f


# ---- fine_match_bwd ---------------------------------------------------------------------------------------------------------------------
FineCase = namedtuple("FineCase", "name M W C peaked seed plain")
FINE_SEEDS = {}
_fine = lambda name, M, W, C, peaked=False, plain=False: FineCase(name, M, W, C, peaked, FINE_SEEDS.get(name, 0), plain)
FINE_CASES = ([_fine(f"fine_M{M}", M, 5, 128) for M in (1, 3, 4, 5, 1025)] + [_fine(f"fine_W{W}", 37, W, 128) for W in (2, 3, 7, 8)] +
              [_fine(f"fine_C{C}", 37, 5, C) for C in (32, 64, 96, 160)] + [_fine("fine_peaked", 37, 5, 128, peaked=True), _fine("fine_M1_plain", 1, 5, 128, plain=True)])
FINE_BY_NAME = {c.name: c for c in FINE_CASES}
# fine_peaked: every match but the first and the last has one window position planted at 0.45 .. 0.65 of its centre descriptor, which puts
# 0.8 .. 0.97 of the heat map there.  (Descriptors times 40 put ALL of it on one position: the variance E[x^2] - E[x]^2 is then below
# float32's rounding of E[x]^2, the clamp at 1e-10 is closed or the float32 variance has no relative accuracy, and nothing is left to
# compare but zeros.)  fine_M1_plain: the one match an ordinary one -- fine_M1's only match is the uniform one, whose d0 is exactly 0.
FINE_MUTATIONS = ("std_term_dropped", "centre_index_rounded_down", "last_channel_stride_not_written")
assert [(-(-c.M // WAVES), c.M % WAVES) for c in FINE_CASES[:5]] == [(1, 1), (1, 3), (1, 0), (2, 1), (257, 1)]      # blocks, waves in the last (0: full)
assert [c.W * c.W for c in FINE_CASES[5:9]] == [4, 9, 49, 64] and [(_cdiv(c.C, LANES), c.C % LANES) for c in FINE_CASES[9:13]] == [(1, 32), (1, 0), (2, 32), (3, 32)]


def fine_mutation_applies(c, m):
    return {"centre_index_rounded_down": c.W % 2 == 0, "last_channel_stride_not_written": c.C % LANES != 0}.get(m, True)


@functools.lru_cache(maxsize=None)
def fine_inputs(name):
    """Windows as make_golden_grad.build_inputs draws them, a dense d expec_f (non-zero std column); match 0 has a uniform heat map
    (f1 = 0: d0 is exactly 0 there), the last match a one-hot one (variance clamp closed: nothing flows through std) -- M = 1 has the
    uniform one only, or (`plain`) an ordinary one."""
    c = FINE_BY_NAME[name]
    rng = np.random.default_rng([c.M, c.W, c.C, int(c.peaked), c.seed])
    WW = c.W * c.W
    f0 = rng.standard_normal((c.M, WW, c.C)).astype(np.float32)
    f1 = (0.6 * f0[:, WW // 2:WW // 2 + 1, :] * (rng.random((c.M, WW, 1)) < 0.2) + rng.standard_normal((c.M, WW, c.C))).astype(np.float32)
    if c.peaked:
        f1[np.arange(c.M), rng.integers(0, WW, c.M)] += rng.uniform(0.45, 0.65, (c.M, 1)).astype(np.float32) * f0[:, WW // 2]
    if not c.plain:
        f1[0] = 0
    if c.M > 1:
        f1[-1, WW // 3] = np.float32(40.0) * f0[-1, WW // 2]
    g = rng.standard_normal((c.M, 3)).astype(np.float32)
    g[:, 2] = np.where(np.abs(g[:, 2]) < 0.1, 0.5, g[:, 2])
    _freeze(f0, f1, g)
    return dict(case=c, f0=f0, f1=f1, g=g)


@functools.lru_cache(maxsize=None)
def fine_reference(name):
    i = fine_inputs(name)
    ref = {}
    for key, dt in (("ref64", np.float64), ("ref32", np.float32)):
        d0, d1 = GO.fine_matching_grad(i["f0"], i["f1"], i["g"], dtype=dt)
        assert d0.dtype == dt and d1.dtype == dt
        ref[key] = dict(d0=d0, d1=d1)
    return _record(ref["ref64"], ref["ref32"], ("d0", "d1"))


def fine_mutated(name, m):
    i = fine_inputs(name)
    c = i["case"]
    WW = c.W * c.W
    if m == "std_term_dropped":
        g = i["g"].copy(); g[:, 2] = 0
        d0, d1 = GO.fine_matching_grad(i["f0"], i["f1"], g)
    elif m == "centre_index_rounded_down":            # (WW - 1) / 2 as the centre: the same pass on f0 with the two rows exchanged
        a, b = WW // 2, (WW - 1) // 2
        f0 = i["f0"].copy(); f0[:, [a, b]] = f0[:, [b, a]]
        d0, d1 = GO.fine_matching_grad(f0, i["f1"], i["g"])
        d0[:, [a, b]] = d0[:, [b, a]]
    elif m == "last_channel_stride_not_written":
        d0, d1 = GO.fine_matching_grad(i["f0"], i["f1"], i["g"])
        d0[:, :, LANES * (c.C // LANES):] = 0
        d1[:, :, LANES * (c.C // LANES):] = 0
    else:
        raise KeyError(m)
    return dict(d0=d0, d1=d1)


# ---- the loss gradients ------------------------------------------------------------------------------------------------------------------
LossCase = namedtuple("LossCase", "name kind M masked")
LOSS_SHAPE = (5, 257, 300)                    # 1285 rows > 1024 blocks (a second round of the row loop), S = 300 > 256 threads (of the column loop)
LOSS_HW = ((1, 257), (15, 20))
KIND = {0: ("focal", True, "dual_softmax"), 1: ("focal", True, "sinkhorn"), 2: ("focal", False, "dual_softmax"), 3: ("cross_entropy", False, "dual_softmax")}
LOSS_CASES = [LossCase(f"loss_k{k}_M{M}{'_masked' if mk else ''}", k, M, mk) for k in range(4) for M in (0, 1, 256, 257) for mk in (False, True)]
LOSS_BY_NAME = {c.name: c for c in LOSS_CASES}
LOSS_MUTATIONS = ("rows_beyond_1024_not_written", "columns_beyond_256_not_written", "clamp_open_everywhere")
assert LOSS_SHAPE[0] * LOSS_SHAPE[1] > LOSS_BLOCKS and LOSS_SHAPE[2] > COLS and [_cdiv(M, 256) for M in (1, 256, 257)] == [1, 1, 2]
CLOSED_LOW, CLOSED_HIGH = np.float32(5e-7), np.float32(1 - 5e-7)
assert CLOSED_LOW < np.float32(1e-6) and CLOSED_HIGH > np.float32(1 - 1e-6) and CLOSED_HIGH < 1


def loss_cfg(kind, fine_type="l2_with_std"):
    ctype, sparse, match_type = KIND[kind]
    return {"loftr": {"loss": dict(coarse_type=ctype, coarse_weight=1.0, focal_alpha=0.25, focal_gamma=2.0, pos_weight=1.0, neg_weight=1.0,
                                   fine_type=fine_type, fine_weight=1.0, fine_correct_thr=1.0),
                      "match_coarse": dict(match_type=match_type, sparse_spvs=sparse)}}


def loss_mutation_applies(c, m):
    return c.kind >= 2 if m != "clamp_open_everywhere" else (c.kind >= 2 or c.M >= 256 or c.kind == 1)


@functools.lru_cache(maxsize=None)
def loss_inputs(name):
    """A synthetic confidence volume in (0, 1) ([N, L + 1, S + 1] for kind 1) with entries on both closed sides of the clamp -- among
    the supervised entries too --, unique ground-truth ids (one per row and column of a pair), and masks: valid rectangles, pair 3's
    mask1 all zero (kind 1's `any1`)."""
    c = LOSS_BY_NAME[name]
    N, L, S = LOSS_SHAPE
    pad = c.kind == 1
    rng = np.random.default_rng([c.kind, c.M, c.masked])
    conf = (rng.random((N, L + pad, S + pad)) ** 4 * 0.98 + 0.01).astype(np.float32)
    pick = rng.random(conf.shape)
    conf[pick < 0.01] = CLOSED_LOW
    conf[pick > 0.99] = CLOSED_HIGH
    b = (np.arange(c.M) % N).astype(np.int64)
    pi, pj = [rng.permutation(np.arange(1, L)) for _ in range(N)], [rng.permutation(S) for _ in range(N)]
    i = np.array([pi[n][m // N] for m, n in enumerate(b)], np.int64)
    j = np.array([pj[n][m // N] for m, n in enumerate(b)], np.int64)
    for m in range(c.M):                          # the supervised entries: two of five on a closed side of the clamp (the open ones away from 0: a positive at 1e-6
                                                  # has a gradient of 1e5, beside which a lost row of negatives is below any tolerance)
        conf[b[m], i[m], j[m]] = (CLOSED_LOW, CLOSED_HIGH, np.float32(0.5), np.float32(0.9), np.float32(0.97))[m % 5] if c.M > 1 else np.float32(0.3)
    gt = np.zeros((N, L, S), np.float32)
    gt[b, i, j] = 1
    m0 = m1 = None
    if c.masked:
        (h0, w0), (h1, w1) = LOSS_HW
        m0, m1 = np.ones((N, h0, w0), bool), np.ones((N, h1, w1), bool)
        m0[0, :, 200:], m1[0, 12:], m1[1, :, 17:], m0[2, :, 31:] = False, False, False, False
        m1[3] = False
    _freeze(conf, b, i, j, gt, m0, m1)
    return dict(case=c, conf=conf, b=b, i=i, j=j, gt=gt, m0=m0, m1=m1)


def _loss_grad(inp, conf, dtype):
    c = inp["case"]
    w = None if inp["m0"] is None else (inp["m0"].reshape(LOSS_SHAPE[0], -1)[:, :, None] & inp["m1"].reshape(LOSS_SHAPE[0], -1)[:, None, :]).astype(dtype)
    if c.kind == 1:
        return GO.sparse_sinkhorn_loss_grad(conf, inp["gt"], w, dtype=dtype)
    return GO.coarse_loss_grad(conf, inp["gt"], w, coarse_type=KIND[c.kind][0], sparse_spvs=KIND[c.kind][1], dtype=dtype)


def loss_value(inp):
    """loss_c in float64 (oracle.train_oracle.coarse_loss)."""
    from oracle import train_oracle as TO
    c = inp["case"]
    w = None if inp["m0"] is None else (inp["m0"].reshape(LOSS_SHAPE[0], -1)[:, :, None] & inp["m1"].reshape(LOSS_SHAPE[0], -1)[:, None, :]).astype(np.float64)
    return float(TO.coarse_loss(inp["conf"], inp["gt"], w, coarse_type=KIND[c.kind][0], sparse_spvs=KIND[c.kind][1], match_type=KIND[c.kind][2]))


@functools.lru_cache(maxsize=None)
def loss_reference(name):
    inp = loss_inputs(name)
    ref64, ref32 = dict(grad_conf=_loss_grad(inp, inp["conf"], np.float64)), dict(grad_conf=_loss_grad(inp, inp["conf"], np.float32))
    assert ref64["grad_conf"].dtype == np.float64 and ref32["grad_conf"].dtype == np.float32
    return _record(ref64, ref32, ("grad_conf",))


def loss_mutated(name, m):
    inp = loss_inputs(name)
    N, L, S = LOSS_SHAPE
    g = loss_reference(name)["ref64"]["grad_conf"].copy()
    if m == "rows_beyond_1024_not_written":
        g.reshape(N * L, S)[LOSS_BLOCKS:] = 0
    elif m == "columns_beyond_256_not_written":
        g[:, :, COLS:] = 0
    elif m == "clamp_open_everywhere":            # the same values, clamped beforehand: every entry counts as inside the clamp
        g = _loss_grad(inp, np.clip(inp["conf"], np.float32(1e-6), np.float32(1 - 1e-6)), np.float64)
    else:
        raise KeyError(m)
    return dict(grad_conf=g)


FineLossCase = namedtuple("FineLossCase", "name M fine_type correct")
FINE_LOSS_CASES = [FineLossCase(f"floss_M{M}_{ft}_{'correct' if ok else 'none'}", M, ft, ok) for M in (1, 256, 257) for ft in ("l2", "l2_with_std")
                   for ok in (True, False)]
FINE_LOSS_BY_NAME = {c.name: c for c in FINE_LOSS_CASES}


@functools.lru_cache(maxsize=None)
def fine_loss_inputs(name):
    c = FINE_LOSS_BY_NAME[name]
    rng = np.random.default_rng([c.M, c.fine_type == "l2", c.correct])
    e = (0.5 * rng.standard_normal((c.M, 3))).astype(np.float32)
    e[:, 2] = rng.uniform(0.1, 1.0, c.M).astype(np.float32)
    if c.M > 1:
        e[1, 2] = 1e-3
    gt = (rng.uniform(-1.4, 1.4, (c.M, 2)) if c.correct else 1.5 + rng.random((c.M, 2))).astype(np.float32)
    if c.correct:
        gt[0] = (0.3, -0.2)
    _freeze(e, gt)
    return dict(case=c, expec_f=e, gt=gt)


@functools.lru_cache(maxsize=None)
def fine_loss_reference(name):
    i = fine_loss_inputs(name)
    c = i["case"]
    ref64, ref32 = (dict(grad_expec=GO.fine_loss_grad(i["expec_f"], i["gt"], c.fine_type, 1.0, True, dtype=dt)) for dt in (np.float64, np.float32))
    assert ref64["grad_expec"].dtype == np.float64 and ref32["grad_expec"].dtype == np.float32
    return _record(ref64, ref32, ("grad_expec",))
