"""Case table, float64 reference and tolerances of the Sinkhorn passes' edge tests.

tests/test_hip_sinkhorn_edges.py (GPU) compares `ops.coarse_match(match_type="sinkhorn", want_assign=True, thr=0.0)` at C = 256 with the
numpy oracle evaluated in float64 at the sizes where the hand-written work distribution of csrc/sinkhorn.h and of ot_plan /
ot_pass_launch / ot_iterate (csrc/coarse_match.hip) changes path:
  * the row-streaming passes (otp::ot_pass_kernel): a workgroup owns a contiguous range of `rpws` rows and works through it R rows per
    round (rows beyond the range re-read row L - 1 and are neutralised); thread t owns the four-column groups q = t + NT k, k < G4; the
    group q == S >> 2 holds the S % 4 last scores and then the dustbin column.  Narrow variant (S + 1 <= 5120): NT = 256, G4 = 5, R = 2;
    wide (S + 1 <= 12288): NT = 512, G4 = 6, R = 1 for the iterations and NT = 1024, G4 = 3, R = 1 for the last pass, the next round's
    row prefetched into a second register set;
  * ot_col_merge2_kernel: the `wgs` column partials of a pair in clamped loads of eight, plus the dustbin row's analytic term;
  * wider rows (S + 1 > 12288): ot_row_lse_kernel, ot_col_part_kernel (OT_RCH = 128 row chunks of ceil((L + 1) / 128) rows, 64-column
    blocks), ot_col_merge_kernel, and ot_finalize_kernel on the 128 x 128 tile geometry -- a path no other test reaches;
  * ot_rowkill_kernel / ot_colkill_kernel and the last pass's `kill` bit mask (skh_prefilter), ot_assign_bins_kernel (dustbin column,
    dustbin row and corner of conf_matrix_with_bin).
tests/test_sinkhorn_oracle.py (CPU) holds every condition stated here and shows that the comparison can fail.

Reference: `oracle.loftr_oracle.sinkhorn_conf` on the float64 casts of the float32 inputs (ref64) and on the inputs themselves (ref32).
Two regions are compared: "conf" (conf_matrix and the inner block of conf_matrix_with_bin, on the valid entries) and "bins" (the dustbin
column of ALL rows, the dustbin row of ALL columns, the corner: a masked row's dustbin entry is as well conditioned as any other).  Per
region noise_abs = max|ref32 - ref64|, noise_rel = max|ref32 - ref64| / ref64, scale = max ref64, over the entries the check uses.

Two checks per region.  The ABSOLUTE one is the project's, with TOL_CONF max(1, scale) as its cap (assignment entries are not bounded by
1: at skh_iters = 0 they are exp(score) (L + S)).  Where conf is of the order 1 / (L S) it cannot see a row or column sum that lost or
doubled a term; the RELATIVE one can.  It uses the entries >= REL_FLOOR of conf, which include every row's and column's maximum, and every
dustbin entry (all are >= BIN_FLOOR), and its bound stays below 1 / (2 max(L + 1, S + 1)) on every case.

Inputs: seeded float32 descriptors with planted correspondences, as in tests/_score_sweep_cases.py: every token of the longer side has
a partner (spread_pairs), so every row and column maximum is a planted entry that leads its runner-up by MARGIN_FACTOR relative tolerances in ref64 and
the match ids are those of `coarse_match_select(ref64)` exactly.  Prefilter cases (`half`): half of the shorter side's tokens get ONE
partner, the others none, so that about half of the rows go to the dustbin -- and every valid row's and column's dustbin entry differs
from its best real entry by ten relative tolerances at least, so the kill decision does not hang on float32 rounding.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from oracle import loftr_oracle as O
from _cases import TOL_CONF
from _score_sweep_cases import C, REL_FLOOR, MARGIN_FACTOR, grid, border_rm, _freeze, _top2_margin, _cdiv

# ---- tolerance ------------------------------------------------------------------------------------------------------------------------
# err_abs <= min(K_ABS * noise_abs + 1e-6 * scale, TOL_CONF * max(1, scale)),   err_rel <= K_REL * noise_rel + 1e-6,   per region.
# K = twice the largest err / noise measured on an MI355X over all cases and outputs of the region, rounded up to an integer (the
# factor 2 covers summation-order differences between machines, as in tests/_score_sweep_cases.py).  The two regions have constants of
# their own: they come from different kernels (conf: the last pass, v_exp_f32; bins: ot_assign_bins_kernel, expf) and float32's own noise
# differs.  The largest ratios of the dustbins are cases where the oracle's float32 run is unusually close to float64 (L = 3: a column
# sum has four terms; noise_rel 6.9e-7), not cases where the kernels are far: 2.4e-6 is five roundings of terms of magnitude 10 in
# alpha + u + v - norm (half a unit in the last place of 10 is 4.8e-7).  With the dustbins' constants on conf, the conf bound of the
# widest cases would no longer stay below 1 / (2 (S + 1)).  The lines of profiles/sinkhorn_accuracy.txt the constants were taken from:
#   K_ABS["conf"] =  5 <- 2.39   col_S1                   conf  abs err 1.863e-07 noise 7.795e-08
#   K_REL["conf"] =  3 <- 1.47   col_S2                   conf  rel err 1.643e-06 noise 1.116e-06
#   K_ABS["bins"] = 11 <- 5.28   mask_one_side_3x33x1025  bins  abs err 8.295e-06 noise 1.572e-06
#   K_REL["bins"] =  7 <- 3.50   fb_3x12351               bins  rel err 2.412e-06 noise 6.882e-07
K_ABS = {"conf": 5, "bins": 11}
K_REL = {"conf": 3, "bins": 7}
BIN_FLOOR = 1e-30         # the relative check's floor on the dustbin entries: a peaked row's is exp(bin_score - 36) of its best entry, far below
                           # REL_FLOOR and as exact as any (the smallest normal float32 is 1.2e-38)
DETECTION_FACTOR = 10.0    # a modelled mistake sits this many relative tolerances from ref64 on the cases with S <= DETECTION_S ...
DETECTION_S = 1025
DETECTION_FLOOR = 2.0      # ... and this many on every case it applies to


def abs_tolerance(region, noise_abs, scale):
    return min(K_ABS[region] * noise_abs + 1e-6 * scale, TOL_CONF * max(1.0, scale))


def rel_tolerance(region, noise_rel):
    return K_REL[region] * noise_rel + 1e-6


# ---- the kernels' work distribution, restated -------------------------------------------------------------------------------------------
BM, WM = 128, 2                                # GemmCfg<128, 128, 2, 2>: g.PI = ceil(L / BM) * WM (make_geometry)
OT_RCH = 128
ROWSTREAM_MAX, NARROW_MAX = 4 * 512 * 6, 4 * 256 * 5        # S + 1 <= 12288: row-streaming;  S + 1 <= 5120: its 256-thread variant
Variant = namedtuple("Variant", "NT G4 R")
NARROW, WIDE_ITER, WIDE_FINAL = Variant(256, 5, 2), Variant(512, 6, 1), Variant(1024, 3, 1)
Plan = namedtuple("Plan", "rowstream wide aligned wgs rpws capP")


def ot_plan(N, L, S):
    """ot_plan of csrc/coarse_match.hip with g.PI of make_geometry (capP: the ceiling its workgroup count was clamped to)."""
    rowstream, wide, aligned = S + 1 <= ROWSTREAM_MAX, S + 1 > NARROW_MAX, S % 4 == 0
    if not rowstream:
        return Plan(False, wide, aligned, 0, 0, 0)
    R = 1 if wide else 2
    capP = min(max(_cdiv(L, 256) * 8, _cdiv(L, BM) * WM), OT_RCH)
    wgs = (256 if wide else 768) // N
    wgs = max(1, min(wgs, capP))
    wgs = min(wgs, _cdiv(L, R))
    rpws = _cdiv(_cdiv(L, wgs), R) * R
    return Plan(True, wide, aligned, _cdiv(L, rpws), rpws, capP)


def variants(S):
    """(iteration variant, last-pass variant) of ot_pass_launch."""
    return (NARROW, NARROW) if S + 1 <= NARROW_MAX else (WIDE_ITER, WIDE_FINAL)


def tail_owner(S, v):
    """(thread, k, element) of the dustbin column: group S >> 2 is owned by thread q % NT at k = q // NT; the dustbin follows S % 4 scores."""
    q = S >> 2
    assert q // v.NT < v.G4, (S, v)
    return q % v.NT, q // v.NT, S % 4


def row_ranges(N, L, S):
    p = ot_plan(N, L, S)
    return [(w * p.rpws, min((w + 1) * p.rpws, L)) for w in range(p.wgs)]


def fallback_chunks(L):
    """(rows per chunk, number of non-empty chunks) of ot_col_part_kernel over the L + 1 rows."""
    per = _cdiv(L + 1, OT_RCH)
    return per, _cdiv(L + 1, per)


for _S in range(1, ROWSTREAM_MAX):            # every row-streaming size fits its variants: 4 NT G4 >= S + 1
    for _v in variants(_S):
        assert 4 * _v.NT * _v.G4 >= _S + 1
assert variants(5119) == (NARROW, NARROW) and variants(5120) == (WIDE_ITER, WIDE_FINAL) and ot_plan(1, 1, 12287).rowstream and not ot_plan(1, 1, 12288).rowstream

# ---- edges: what a case is in the table for, as a predicate of the case and its plan ----------------------------------------------------
EDGES = {
    # column edges
    "tail_in_group_0": lambda c, p: not p.wide and c.S >> 2 == 0 and tail_owner(c.S, NARROW)[:2] == (0, 0),
    "tail_in_group_1": lambda c, p: not p.wide and c.S >> 2 == 1 and tail_owner(c.S, NARROW)[:2] == (1, 0),
    "tail_before_wave_boundary": lambda c, p: not p.wide and tail_owner(c.S, NARROW)[:2] == (63, 0) and c.S % 4 == 3,
    "tail_on_wave_boundary": lambda c, p: not p.wide and tail_owner(c.S, NARROW)[:2] == (64, 0),
    "tail_last_of_k0": lambda c, p: not p.wide and tail_owner(c.S, NARROW)[:2] == (255, 0) and c.S % 4 == 3,
    "tail_first_of_k1": lambda c, p: not p.wide and tail_owner(c.S, NARROW)[:2] == (0, 1),
    "tail_last_of_k3": lambda c, p: not p.wide and tail_owner(c.S, NARROW)[:2] == (255, 3) and c.S % 4 == 3,
    "tail_first_of_k4": lambda c, p: not p.wide and tail_owner(c.S, NARROW)[:2] == (0, 4),
    "last_narrow_aligned": lambda c, p: not p.wide and p.aligned and tail_owner(c.S, NARROW) == (255, 4, 0),
    "last_narrow": lambda c, p: not p.wide and c.S + 1 == NARROW_MAX and tail_owner(c.S, NARROW) == (255, 4, 3),
    "first_wide_aligned": lambda c, p: p.wide and p.rowstream and p.aligned and c.S == NARROW_MAX and tail_owner(c.S, WIDE_ITER)[:2] == (256, 2)
        and tail_owner(c.S, WIDE_FINAL)[:2] == (256, 1),
    "first_wide_unaligned": lambda c, p: p.wide and p.rowstream and c.S == NARROW_MAX + 1 and c.S % 4 == 1,
    "iter_tail_last_of_k2": lambda c, p: p.rowstream and tail_owner(c.S, WIDE_ITER) == (511, 2, 3),
    "iter_tail_first_of_k3": lambda c, p: p.rowstream and tail_owner(c.S, WIDE_ITER)[:2] == (0, 3) and tail_owner(c.S, WIDE_FINAL)[:2] == (512, 1),
    "final_tail_last_of_k1": lambda c, p: p.rowstream and tail_owner(c.S, WIDE_FINAL) == (1023, 1, 3),
    "final_tail_first_of_k2": lambda c, p: p.rowstream and tail_owner(c.S, WIDE_FINAL)[:2] == (0, 2) and tail_owner(c.S, WIDE_ITER)[:2] == (0, 4),
    "outdoor_105x105": lambda c, p: p.rowstream and p.wide and c.S == 105 * 105 and c.S % 4 == 1,
    "last_wide_aligned": lambda c, p: p.rowstream and p.aligned and tail_owner(c.S, WIDE_ITER) == (511, 5, 0) and tail_owner(c.S, WIDE_FINAL) == (1023, 2, 0),
    "last_wide": lambda c, p: p.rowstream and c.S + 1 == ROWSTREAM_MAX and tail_owner(c.S, WIDE_ITER) == (511, 5, 3)
        and tail_owner(c.S, WIDE_FINAL) == (1023, 2, 3),
    # the separate-kernel path
    "fallback": lambda c, p: not p.rowstream,
    "fallback_first": lambda c, p: not p.rowstream and c.S + 1 == ROWSTREAM_MAX + 1 and (c.S + 1) % 64 == 1,      # the dustbin alone in the last 64-column block
    "fallback_unaligned": lambda c, p: not p.rowstream and c.S % 4 == 1 and (c.S + 1) % 64 not in (0, 1),
    "fallback_full_blocks": lambda c, p: not p.rowstream and (c.S + 1) % 64 == 0,
    "fallback_one_row_block": lambda c, p: c.L + 1 == 4 and fallback_chunks(c.L) == (1, 4),                    # one block of ot_row_lse_kernel; 124 of the 128 chunks empty
    "fallback_two_rows_per_chunk": lambda c, p: fallback_chunks(c.L)[0] == 2 and (c.L + 1) % 2 == 1 and c.L % BM != 0 and c.L > BM,
    # row-range edges
    "one_row": lambda c, p: c.L == 1 and (p.wgs, p.rpws) == (1, 2),                                            # one real and one phantom row
    "one_workgroup": lambda c, p: p.rowstream and p.wgs == 1 and c.L <= p.rpws,
    "odd_short_last_range": lambda c, p: not p.wide and p.wgs >= 2 and (c.L - (p.wgs - 1) * p.rpws) % 2 == 1 and c.L % p.rpws != 0,
    "merge_clamped_loads": lambda c, p: p.rowstream and p.wgs > 8 and p.wgs % 8 != 0,
    "merge_clamped_loads_short_last": lambda c, p: p.rowstream and p.wgs > 8 and p.wgs % 8 != 0 and c.L % p.rpws != 0,
    "workgroup_ceiling": lambda c, p: p.rowstream and _cdiv(c.L, 256) * 8 > OT_RCH == p.capP and 768 // c.N > OT_RCH and 8 < p.wgs <= OT_RCH,
    "wide_no_prefetch": lambda c, p: p.wide and p.rowstream and p.rpws == 1 and p.wgs == c.L,
    "wide_prefetch_short_last": lambda c, p: p.wide and p.rowstream and p.rpws >= 2 and 2 <= c.L - (p.wgs - 1) * p.rpws < p.rpws,
    "wide_equal_ranges": lambda c, p: p.wide and p.rowstream and p.rpws >= 2 and c.L % p.rpws == 0,
    "batch_9": lambda c, p: c.N == 9,
    "batch_1": lambda c, p: c.N == 1,
    # settings
    "iters_0": lambda c, p: c.iters == 0,
    "iters_1": lambda c, p: c.iters == 1,
    "iters_10": lambda c, p: c.iters == 10,
    "bin_low": lambda c, p: c.bin_score == -2.0 and not c.prefilter,
    "bin_high_all_dropped": lambda c, p: c.bin_score == 8.0 and c.prefilter,
    "peaked": lambda c, p: c.regime == "peaked",
    "narrow": lambda c, p: p.rowstream and not p.wide,
    "wide": lambda c, p: p.rowstream and p.wide,
    "prefilter": lambda c, p: c.prefilter and c.regime == "half",
    "prefilter_square": lambda c, p: c.prefilter and c.L == c.S and p.aligned,
    "prefilter_tail_kill": lambda c, p: c.prefilter and not p.aligned and not p.wide,       # (a kill in the tail group: asserted on the reference, CPU test)
    "masked": lambda c, p: c.name in MASKS,
    "masked_one_side": lambda c, p: border_rm(c.L, c.S) == 0 and all(len({im for (n, im) in MASKS[c.name] if n == k}) <= 1 for k in range(c.N)),
    "masked_both": lambda c, p: border_rm(c.L, c.S) == 1 and any({(n, 0), (n, 1)} <= set(MASKS[c.name]) for n in range(c.N)),
    "masked_dead_range": lambda c, p: any(im == 0 and vw == grid(c.L)[1] and any(r0 >= vh * vw for r0, r1 in row_ranges(c.N, c.L, c.S))
                                          for (n, im), (vh, vw) in MASKS[c.name].items()),
    "masked_ends_inside_group": lambda c, p: any(im == 1 and ((vh - 1) * grid(c.S)[1] + vw) % 4 != 0 for (n, im), (vh, vw) in MASKS[c.name].items()),
}

# ---- cases -----------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name N L S iters bin_score regime prefilter seed edges")
# planted weight, descriptor amplitude, weight of a token's further partners relative to its first, background.  ot: the inputs of the
# existing Sinkhorn tests (planted score weight amp^2 = 6); peaked: planted scores of 36, as the e2e_peaked_ot golden; half: the
# prefilter recipe (one partner for half of the shorter side's tokens).
REGIMES = {"ot": (1.5, 2.0, 0.6, 0.25), "peaked": (2.25, 4.0, 0.6, 0.25), "half": (3.0, 2.0, None, 0.5)}
BIN_SCORE, SKH_ITERS, PREFILTER_BIN = 1.0, 3, 2.0
# peaked: the descriptors are multiples of 1 / 4, so that their products and the sums of 256 of them are exact in float32 (and in the
# score GEMM's half-precision operands): a score of 36 formed in float32 carries a rounding error of about 2e-5, which only a
# row's or column's dominating entry sheds in the normalisation -- float32's own relative noise would be 4e-5 at the column maxima and
# dustbins, and three times that is no longer below 1 / (2 (S + 1)) on the wide shapes.  With exact scores the peaked cases compare the
# PASSES at large magnitudes; the score store at ordinary inputs is pinned by tests/test_hip_score_sweep_edges.py.
PEAKED_QUANTUM = 0.25
SEEDS = {"row_L4097": 7, "set_fallback_peaked": 2, "pre_2x40x12321": 6}                                # name -> seed other than 0 (chosen where a condition on the inputs missed with seed 0)
# valid rectangles (vh, vw) at the top left, by (pair, image); every other image is whole
MASKS = {
    "mask_one_side_3x33x1025": {(0, 0): (2, 9), (1, 1): (24, 38), (2, 0): (3, 8)},
    "mask_both_3x63x960": {(0, 0): (6, 8), (0, 1): (27, 30), (1, 1): (30, 29), (2, 0): (5, 9), (2, 1): (28, 32)},
    "mask_dead_range_3x64x160": {(0, 0): (6, 8), (1, 1): (9, 14), (2, 0): (4, 8), (2, 1): (10, 13)},
    "mask_inside_group_3x33x957": {(0, 1): (27, 31), (1, 0): (3, 9), (2, 1): (29, 30)},
    "pre_mask_3x257x961": {(0, 1): (29, 28), (1, 0): (1, 200), (2, 1): (31, 30)},
}
SETTINGS_SHAPES = (("narrow", 3, 33, 1025), ("wide", 2, 40, 5121), ("fallback", 2, 20, 12321))


def _build_cases():
    cases = []

    def add(name, N, L, S, *edges, iters=SKH_ITERS, bin_score=BIN_SCORE, regime="ot", prefilter=False):
        cases.append(Case(name, N, L, S, iters, float(bin_score), regime, prefilter, SEEDS.get(name, 0), edges))
    # column edges, narrow variant
    for S, e in ((1, "tail_in_group_0"), (2, "tail_in_group_0"), (3, "tail_in_group_0"), (4, "tail_in_group_1"), (5, "tail_in_group_1"),
                 (255, "tail_before_wave_boundary"), (256, "tail_on_wave_boundary"), (257, "tail_on_wave_boundary"),
                 (1023, "tail_last_of_k0"), (1024, "tail_first_of_k1"), (1025, "tail_first_of_k1"),
                 (4095, "tail_last_of_k3"), (4096, "tail_first_of_k4"), (4097, "tail_first_of_k4"),
                 (5116, "last_narrow_aligned"), (5119, "last_narrow")):
        add(f"col_S{S}", 3, 33, S, e, "narrow")
    # column edges, wide variant
    for S, e in ((5120, "first_wide_aligned"), (5121, "first_wide_unaligned"), (6143, "iter_tail_last_of_k2"), (6144, "iter_tail_first_of_k3"),
                 (6145, "iter_tail_first_of_k3"), (8191, "final_tail_last_of_k1"), (8192, "final_tail_first_of_k2"), (8193, "final_tail_first_of_k2"),
                 (11025, "outdoor_105x105"), (12284, "last_wide_aligned"), (12287, "last_wide")):
        add(f"col_S{S}", 2, 40, S, e, "wide", "wide_equal_ranges")
    # the separate-kernel path
    for S, e in ((12288, "fallback_first"), (12321, "fallback_unaligned"), (12351, "fallback_full_blocks")):
        for L, f in ((3, "fallback_one_row_block"), (130, "fallback_two_rows_per_chunk")):
            add(f"fb_{L}x{S}", 2, L, S, "fallback", e, f)
    # row-range edges
    add("row_L1", 3, 1, 160, "one_row", "one_workgroup", "narrow")
    add("row_L2", 3, 2, 160, "one_workgroup", "narrow")
    add("row_L33", 3, 33, 160, "odd_short_last_range", "narrow")
    add("row_L291", 3, 291, 160, "merge_clamped_loads_short_last", "odd_short_last_range", "narrow")
    add("row_L300", 3, 300, 160, "merge_clamped_loads", "narrow")
    add("row_L4097", 1, 4097, 33, "workgroup_ceiling", "merge_clamped_loads", "narrow")
    add("row_wide_L5", 2, 5, 5121, "wide_no_prefetch")
    add("row_wide_L45", 2, 45, 5121, "wide_prefetch_short_last")
    add("n9_narrow", 9, 33, 1025, "batch_9", "narrow")
    add("n9_wide", 9, 20, 5121, "batch_9", "wide")
    add("n1_narrow", 1, 33, 1025, "batch_1", "narrow")
    add("n1_wide", 1, 40, 5121, "batch_1", "wide")
    # settings
    for tag, N, L, S in SETTINGS_SHAPES:
        path = "fallback" if tag == "fallback" else tag
        for it in (0, 1, 10):
            add(f"set_{tag}_iters{it}", N, L, S, f"iters_{it}", path, iters=it)
        add(f"set_{tag}_bin-2", N, L, S, "bin_low", path, bin_score=-2.0)
        add(f"set_{tag}_bin8", N, L, S, "bin_high_all_dropped", path, bin_score=8.0, prefilter=True)
        add(f"set_{tag}_peaked", N, L, S, "peaked", path, regime="peaked")
    # prefilter
    add("pre_3x300x300", 3, 300, 300, "prefilter", "prefilter_square", "narrow", bin_score=PREFILTER_BIN, regime="half", prefilter=True)
    add("pre_3x257x957", 3, 257, 957, "prefilter", "prefilter_tail_kill", bin_score=PREFILTER_BIN, regime="half", prefilter=True)
    add("pre_2x70x5120", 2, 70, 5120, "prefilter", "wide", bin_score=PREFILTER_BIN, regime="half", prefilter=True)
    add("pre_2x40x12321", 2, 40, 12321, "prefilter", "fallback", bin_score=PREFILTER_BIN, regime="half", prefilter=True)
    add("pre_mask_3x257x961", 3, 257, 961, "prefilter", "masked", "masked_one_side", bin_score=PREFILTER_BIN, regime="half", prefilter=True)
    # masks
    add("mask_one_side_3x33x1025", 3, 33, 1025, "masked", "masked_one_side")
    add("mask_both_3x63x960", 3, 63, 960, "masked", "masked_both")
    add("mask_dead_range_3x64x160", 3, 64, 160, "masked", "masked_dead_range")
    add("mask_inside_group_3x33x957", 3, 33, 957, "masked", "masked_ends_inside_group", "masked_one_side")
    return cases


CASES = _build_cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def edge_failures():
    """[(case, edge)] where a case is not at the edge it is in the table for."""
    return [(c.name, e) for c in CASES for e in c.edges if not EDGES[e](c, ot_plan(c.N, c.L, c.S))]


assert not edge_failures(), edge_failures()
assert all(c.edges for c in CASES) and {e for c in CASES for e in c.edges} == set(EDGES)
assert max(c.N * c.L * c.S for c in CASES) <= 3.5e6 and max(c.L for c in CASES if c.S > NARROW_MAX) <= 130
assert set(MASKS) <= set(CASE_BY_NAME)


def expects_no_match(c):
    return c.prefilter and c.bin_score == 8.0


def masks(c):
    """(m0 [N, h0, w0], m1 [N, h1, w1]) bool valid rectangles at the top left, or (None, None)."""
    if c.name not in MASKS:
        return None, None
    (h0, w0), (h1, w1) = grid(c.L), grid(c.S)
    m = [np.ones((c.N, h0, w0), bool), np.ones((c.N, h1, w1), bool)]
    for (n, im), (vh, vw) in MASKS[c.name].items():
        assert 0 < vh <= m[im].shape[1] and 0 < vw <= m[im].shape[2] and (vh, vw) != m[im].shape[1:]
        m[im][n, vh:] = False
        m[im][n, :, vw:] = False
    return m[0], m[1]


def spread_pairs(v0, v1, rng):
    """(rows, cols, first) as `correspondences` of the score-sweep table -- every token of the longer side has one partner, tokens of the
    shorter side several, one of them (`first`) at the full weight -- with BOTH sides permuted: there the full-weight partners are the
    first tokens of the longer side, which on a wide grid are all border cells and would leave the selection nothing to select."""
    nr, nc = len(v0), len(v1)
    t = np.arange(max(nr, nc))
    rows, cols = v0[rng.permutation(nr)[t % nr]], v1[rng.permutation(nc)[t % nc]]
    return rows, cols, t < min(nr, nc)


def half_pairs(v0, v1, rng):
    """One partner for half of the shorter side's valid tokens: (rows, cols, first)."""
    k = max(1, min(len(v0), len(v1)) // 2)
    return v0[rng.permutation(len(v0))[:k]], v1[rng.permutation(len(v1))[:k]], np.ones(k, bool)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Seeded float32 descriptors, masks, grids.  Shared by every test: read-only."""
    c = CASE_BY_NAME[name]
    weight, amp, more, background = REGIMES[c.regime]
    rng = np.random.default_rng([c.N, c.L, c.S, c.seed])
    f0 = rng.standard_normal((c.N, c.L, C)).astype(np.float32) * np.float32(amp)
    if c.regime == "peaked":
        f0 = np.round(f0 / np.float32(PEAKED_QUANTUM)) * np.float32(PEAKED_QUANTUM)
    f1 = rng.standard_normal((c.N, c.S, C)).astype(np.float32) * np.float32(amp)
    f1 *= np.float32(background)
    m0, m1 = masks(c)
    corr = []
    for n in range(c.N):
        v0 = np.arange(c.L) if m0 is None else np.flatnonzero(m0[n].reshape(-1))
        v1 = np.arange(c.S) if m1 is None else np.flatnonzero(m1[n].reshape(-1))
        rows, cols, first = half_pairs(v0, v1, rng) if c.regime == "half" else spread_pairs(v0, v1, rng)
        w = np.where(first, weight, (more or 1.0) * weight).astype(np.float32)
        np.add.at(f1[n], cols, w[:, None] * f0[n, rows])
        corr.append((rows, cols, first))
    if c.regime == "peaked":
        f1 = np.round(f1 / np.float32(PEAKED_QUANTUM)) * np.float32(PEAKED_QUANTUM)
    _freeze(f0, f1, m0, m1)
    return dict(case=c, f0=f0, f1=f1, m0=m0, m1=m1, hw0=grid(c.L), hw1=grid(c.S), border_rm=border_rm(c.L, c.S), corr=corr)


def flat_masks(i):
    c = i["case"]
    if i["m0"] is None:
        return np.ones((c.N, c.L), bool), np.ones((c.N, c.S), bool)
    return i["m0"].reshape(c.N, -1), i["m1"].reshape(c.N, -1)


def bins_of(assign):
    """The dustbin entries of an assignment matrix [N, L + 1, S + 1] as one array [N, L + S + 1]: column, then row with the corner."""
    return np.concatenate([assign[:, :-1, -1], assign[:, -1, :]], axis=1)


def _oracle(i, dt):
    c = i["case"]
    m0, m1 = (None, None) if i["m0"] is None else flat_masks(i)
    return O.sinkhorn_conf(i["f0"].astype(dt), i["f1"].astype(dt), dt(c.bin_score), c.iters, m0, m1, prefilter=c.prefilter)


def _region(ref64, ref32, use, floor=REL_FLOOR):
    relset = use & (ref64 >= floor)
    d = np.abs(ref32 - ref64)
    _freeze(relset)
    return dict(use=use, relset=relset, noise_abs=float(d[use].max()), scale=float(ref64[use].max()),
                noise_rel=float((d[relset] / ref64[relset]).max()) if relset.any() else 0.0)


@functools.lru_cache(maxsize=2)               # (volumes of up to 3.2 M float64 entries: the figures of facts() are what stays cached)
def reference(name):
    """ref64 / ref32 of conf and of the dustbin entries, the two regions with their noise and scale, the dropped rows / columns, the
    reference selection."""
    i = inputs(name)
    c = i["case"]
    (conf64, assign64), (conf32, assign32) = _oracle(i, np.float64), _oracle(i, np.float32)
    assert conf64.dtype == np.float64 and conf32.dtype == np.float32 and np.array_equal(conf64, assign64[:, :-1, :-1])
    v0, v1 = flat_masks(i)
    valid = v0[:, :, None] & v1[:, None, :]
    bins64, bins32 = bins_of(assign64), bins_of(assign32)
    # rows / columns the prefilter drops: the dustbin is the arg-max of the unfiltered assignment row / column (first index wins a tie)
    if c.prefilter:
        raw = _oracle(dict(i, case=c._replace(prefilter=False)), np.float64)[1]
        rowkill, colkill = (raw.argmax(axis=2) == c.S)[:, :-1], (raw.argmax(axis=1) == c.L)[:, :-1]
        with np.errstate(divide="ignore", invalid="ignore"):
            row_ratio = np.abs(raw[:, :-1, -1] / raw[:, :-1, :-1].max(axis=2) - 1.0)[v0]
            col_ratio = np.abs(raw[:, -1, :-1] / raw[:, :-1, :-1].max(axis=1) - 1.0)[v1]
        del raw
    else:
        rowkill, colkill = np.zeros((c.N, c.L), bool), np.zeros((c.N, c.S), bool)
        row_ratio = col_ratio = np.array([np.inf])
    sel = O.coarse_match_select(conf64, 0.0, i["border_rm"], i["hw0"], i["hw1"], (i["hw0"][0] * 8, i["hw0"][1] * 8), i["m0"], i["m1"])
    _freeze(conf64, conf32, bins64, bins32, valid, rowkill, colkill)
    return dict(ref64=conf64, ref32=conf32, bins64=bins64, bins32=bins32, valid=valid, rowkill=rowkill, colkill=colkill, sel=sel,
                conf=_region(conf64, conf32, valid), bins=_region(bins64, bins32, np.ones(bins64.shape, bool), BIN_FLOOR),
                kill_margin=float(min(np.nanmin(row_ratio), np.nanmin(col_ratio))))


def rel_error(got, ref64, region):
    s = region["relset"]
    return float((np.abs(got - ref64)[s] / ref64[s]).max()) if s.any() else 0.0


def abs_error(got, ref64, region):
    return float(np.abs(got - ref64)[region["use"]].max())


# ---- the float64 iteration once more, from its pieces, with one mistake built in ---------------------------------------------------------
MUTATIONS = ("row_lse_omits_dustbin_column", "col_lse_omits_dustbin_row", "last_row_of_range_folded_twice", "row_sum_omits_tail_columns",
             "dustbin_row_mass_uses_log_L", "last_partial_dropped_in_merge", "kill_mask_shifted_by_one_group")


def mutation_applies(c, m):
    """By shape and settings (nothing is summed without an iteration)."""
    p = ot_plan(c.N, c.L, c.S)
    if m == "kill_mask_shifted_by_one_group":
        return c.prefilter and p.rowstream and not expects_no_match(c) and c.S > 4
    if c.iters == 0:
        return False
    if m in ("row_lse_omits_dustbin_column", "row_sum_omits_tail_columns") and c.regime == "peaked":
        return False                                             # a peaked row's sum IS its planted entry: the dustbin is exp(1 - 36) of it
    if m in ("row_lse_omits_dustbin_column", "col_lse_omits_dustbin_row"):
        return True
    if m == "last_row_of_range_folded_twice":                    # R = 2 and an odd range: its phantom row is row L - 1 once more
        return p.rowstream and not p.wide and c.L % 2 == 1
    if m == "row_sum_omits_tail_columns":
        return p.rowstream and c.S % 4 != 0 and c.S > 4
    if m == "dustbin_row_mass_uses_log_L":
        return c.L != c.S
    if m == "last_partial_dropped_in_merge":                     # the last workgroup's rows / the last non-empty chunk of ot_col_part_kernel
        return p.wgs >= 2 if p.rowstream else c.L >= 2
    raise KeyError(m)


def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    with np.errstate(divide="ignore"):
        return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def sinkhorn_float64(name, mutation=None):
    """(conf [N, L, S], bins [N, L + S + 1]) in float64: scores, padded with the dustbins; u = log_mu - LSE_j(Z + v) with the real rows and
    the dustbin row apart, v = log_nu - LSE_i(Z + u) as a merge of row partials and the dustbin row's term; exp(Z + u + v - norm); the
    prefilter.  mutation None reproduces oracle.sinkhorn_conf (tested)."""
    i = inputs(name)
    c = i["case"]
    N, L, S = c.N, c.L, c.S
    p = ot_plan(N, L, S)
    v0, v1 = flat_masks(i)
    sim = (i["f0"].astype(np.float64) / C ** .5) @ (i["f1"].astype(np.float64) / C ** .5).transpose(0, 2, 1)
    if i["m0"] is not None:
        sim = np.where(v0[:, :, None] & v1[:, None, :], sim, -O.INF)
    alpha, norm = c.bin_score, -math.log(L + S)
    Z = np.full((N, L + 1, S + 1), alpha)
    Z[:, :L, :S] = sim
    del sim
    log_mu = np.full(L + 1, norm); log_mu[L] = math.log(L if mutation == "dustbin_row_mass_uses_log_L" else S) + norm
    log_nu = np.full(S + 1, norm); log_nu[S] = math.log(L) + norm
    NEG = -np.inf
    colw = np.zeros(S + 1)                                      # log of the weight of a column in the REAL rows' sums
    if mutation == "row_lse_omits_dustbin_column":
        colw[S] = NEG
    elif mutation == "row_sum_omits_tail_columns":
        colw[4 * (S >> 2):S] = NEG
    rows_w = np.zeros(L + 1)                                    # log of the weight of a row in the columns' sums
    if mutation == "col_lse_omits_dustbin_row":
        rows_w[L] = NEG
    elif mutation == "last_row_of_range_folded_twice":
        rows_w[L - 1] = math.log(2.0)
    elif mutation == "last_partial_dropped_in_merge":
        if p.rowstream:
            rows_w[row_ranges(N, L, S)[-1][0]:L] = NEG
        else:
            per, chunks = fallback_chunks(L)
            rows_w[(chunks - 1) * per:] = NEG
    u, v = np.zeros((N, L + 1)), np.zeros((N, S + 1))
    for _ in range(c.iters):
        u[:, :L] = log_mu[:L] - _lse(Z[:, :L] + (v + colw)[:, None, :], 2)
        u[:, L] = log_mu[L] - _lse(alpha + v, 1)
        v = log_nu - _lse(Z + (u + rows_w)[:, :, None], 1)
    Z += u[:, :, None]
    Z += v[:, None, :]
    Z -= norm
    assign = np.exp(Z, out=Z)
    if c.prefilter:
        rk, ck = (assign.argmax(axis=2) == S)[:, :-1], (assign.argmax(axis=1) == L)[:, :-1]
        if mutation == "kill_mask_shifted_by_one_group":        # a thread applies the bits of its next group
            ck = np.concatenate([ck[:, 4:], np.zeros((N, 4), bool)], axis=1)
        assign[:, :-1, :-1][np.broadcast_to(rk[:, :, None], (N, L, S))] = 0
        assign[:, :-1, :-1][np.broadcast_to(ck[:, None, :], (N, L, S))] = 0
    return assign[:, :-1, :-1], bins_of(assign)


def distance_in_tolerances(conf, bins, r):
    """The larger of the two regions' relative errors, each in units of its relative tolerance."""
    return max(rel_error(conf, r["ref64"], r["conf"]) / rel_tolerance("conf", r["conf"]["noise_rel"]),
               rel_error(bins, r["bins64"], r["bins"]) / rel_tolerance("bins", r["bins"]["noise_rel"]))


# ---- the conditions on the inputs, as figures (cached per case; the volumes are not) ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def facts(name):
    """What tests/test_sinkhorn_oracle.py asserts, computed in one pass over the case's reference."""
    i, r = inputs(name), reference(name)
    c = i["case"]
    v0, v1 = flat_masks(i)
    x = np.where(r["valid"], r["ref64"], 0.0)
    rowmax, colmax = x.max(axis=2), x.max(axis=1)
    live_r, live_c = v0 & (rowmax > 0), v1 & (colmax > 0)        # (rows / columns the prefilter dropped have no maximum to lead)
    rm, cm = _top2_margin(x, 2)[live_r], _top2_margin(x, 1)[live_c]
    hooked = sinkhorn_float64(name)
    f = dict(finite=bool(np.isfinite(r["ref64"]).all() and np.isfinite(r["ref32"]).all() and np.isfinite(r["bins64"]).all() and np.isfinite(r["bins32"]).all()),
             conf={k: r["conf"][k] for k in ("noise_abs", "noise_rel", "scale")}, bins={k: r["bins"][k] for k in ("noise_abs", "noise_rel", "scale")},
             maxima_in_relset=bool((rowmax[live_r] >= REL_FLOOR).all() and (colmax[live_c] >= REL_FLOOR).all()),
             bins_in_relset=bool(r["bins"]["relset"].all()), min_bin=float(r["bins64"].min()),
             row_margin=float(rm.min()) if rm.size else 1.0, col_margin=float(cm.min()) if cm.size else 1.0,
             matches=len(r["sel"]["b_ids"]), matches_per_pair=np.bincount(r["sel"]["b_ids"], minlength=c.N).tolist(),
             padding_max=float(np.where(r["valid"], 0.0, r["ref64"]).max()),
             hooked_distance=max(float(np.abs(hooked[0] - r["ref64"]).max()) / max(1.0, r["conf"]["scale"]),
                                 float(np.abs(hooked[1] - r["bins64"]).max()) / max(1.0, r["bins"]["scale"])),
             row_kill_share=float(r["rowkill"][v0].mean()), col_kill_share=float(r["colkill"][v1].mean()), kill_margin=r["kill_margin"],
             tail_kills=int(r["colkill"][:, 4 * (c.S >> 2):].sum()), live_rows=int(live_r.sum()), live_cols=int(live_c.sum()),
             dead_ranges=[(n, w) for n in range(c.N) for w, (r0, r1) in enumerate(row_ranges(c.N, c.L, c.S)) if not v0[n, r0:r1].any()])
    del hooked
    f["mutation_distance"] = {m: distance_in_tolerances(*sinkhorn_float64(name, m), r) for m in MUTATIONS if mutation_applies(c, m)}
    return f
