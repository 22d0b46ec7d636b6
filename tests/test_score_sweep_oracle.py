"""CPU: the conditions tests/_score_sweep_cases.py states about its cases hold, and the float64 comparison of
tests/test_hip_score_sweep_edges.py can fail.  The chunkings sweep_plan yields, the classification of the magnitude cases' work units
by tile spread, the coverage of the relative check, its bound against 1 / (2 max(L, S)), the lead of every row and column maximum over
its runner-up and the match counts are conditions on the choice of the inputs: a case that misses one gets other inputs (another seed),
never another factor.  For every flat case and every modelled kernel mistake that applies to it, the float64 reference with the mistake
built in sits at least DETECTION_FACTOR relative tolerances from the unmodified one."""
import numpy as np
import pytest

import _score_sweep_cases as E

ALL = [c.name for c in E.CASES]
DS = [c.name for c in E.DS_CASES]


def _rel_tol(name):
    return E.rel_tolerance(E.CASE_BY_NAME[name], E.facts(name)["noise_rel"])


def test_plan_arithmetic_gives_the_intended_chunkings():
    assert E.sweep_plan(257, 160) == E.Plan(2, 5, 1, 5) and E.sweep_plan(513, 992) == E.Plan(3, 31, 2, 16)
    assert E.sweep_plan(33, 1921) == E.Plan(1, 61, 3, 21)
    assert {S: E.chunk_panels(S) for S in (957, 960, 961, 992, 1921)} == {957: [30], 960: [30], 961: [16, 15], 992: [16, 15], 1921: [21, 21, 19]}
    # one ragged panel alone, then 1 ... 5 panels with and without a ragged last one (4 = the ring's depth, 5 = its first wrap)
    assert [(E.sweep_plan(257, S).NP, S % E.PC != 0) for S in (1, 3, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160)] == \
        [(1, True), (1, True), (1, True), (1, False), (2, True), (2, True), (2, False), (3, True), (3, False), (4, True), (4, False),
         (5, True), (5, False)]
    for S in range(1, 4000):
        p = E.sweep_plan(1, S)
        assert p.PPC <= E.MAX_PPC and (p.NCH - 1) * p.PPC < p.NP <= p.NCH * p.PPC and sum(E.chunk_panels(S)) == p.NP


def test_every_edge_of_the_table_is_a_case():
    shapes = {(c.N, c.L, c.S) for c in E.DS_CASES if c.regime == "flat" and c.masked is None}
    assert {L for N, L, S in shapes if (N, S) == (3, 160)} >= {1, 31, 32, 33, 255, 256, 257, 513}
    assert {S for N, L, S in shapes if (N, L) == (3, 257)} >= {1, 3, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 957, 960, 961, 992, 1921}
    groups = sorted(N * E.sweep_plan(L, S).NCH for L, S in E.XCD_SHAPES for N in E.XCD_N)
    assert groups == [1, 2, 3, 3, 6, 8, 9, 9, 16, 18, 24, 27]          # below, on and above a multiple of the 8 XCDs
    assert all((N, L, S) in shapes for L, S in E.XCD_SHAPES for N in E.XCD_N)
    assert {c.regime for c in E.DS_CASES if (c.N, c.L, c.S) == E.MAGNITUDE_SHAPE and c.masked is None} == \
        {"flat", "peaked", "near_limit", "mixed", "all_exact"}
    assert {(c.N, c.L, c.S) for c in E.DS_CASES if c.masked} == {(3, 513, 992), (2, 257, 961), (9, 33, 160)}
    assert sorted((c.N, c.L, c.S, c.masked is not None) for c in E.OT_CASES) == \
        sorted((N, L, S, m) for N, L, S in ((3, 257, 961), (2, 33, 1921), (3, 257, 957)) for m in (False, True))
    assert max(c.N * c.L * c.S for c in E.CASES) <= max(9 * 257 * 992, 3 * 513 * 992)
    for c in E.CASES:
        assert E.border_rm(c.L, c.S) == (1 if min(E.grid(c.L) + E.grid(c.S)) >= 4 else 0)
        assert E.grid(c.L)[0] * E.grid(c.L)[1] == c.L and E.grid(c.S)[0] * E.grid(c.S)[1] == c.S


def test_mask_patterns():
    """Valid rectangles at the top left, no pair without valid tokens; the dead units of mask_3x513x992 (asserted in masks() itself);
    without border removal only one image of a pair is padded."""
    for c in E.CASES:
        if not c.masked:
            continue
        i = E.inputs(c.name)
        for m in (i["m0"], i["m1"]):
            for n in range(c.N):
                vh, vw = int(m[n].any(1).sum()), int(m[n].any(0).sum())
                assert vh > 0 and vw > 0 and m[n, :vh, :vw].all() and m[n].sum() == vh * vw
        if i["border_rm"] == 0:
            assert all(i["m0"][n].all() or i["m1"][n].all() for n in range(c.N))
        assert any(not i["m0"][n].all() for n in range(c.N)) and any(not i["m1"][n].all() for n in range(c.N))
    i = E.inputs("mask_2x257x961")
    assert any(i["m1"][n].reshape(-1)[960] for n in range(2))           # the ragged last panel's one column is valid in a pair
    m0, m1 = E.flat_masks(E.inputs("mask_3x513x992"))
    assert not m0[1, 256:].any() and not m1[2, 512:].any() and m0[1, :243].all()


@pytest.mark.parametrize("name", ALL)
def test_reference_noise_and_coverage(name):
    """ref32 stays inside half of either tolerance; the relative bound is below half of what one dropped or doubled term changes in a
    flat sum; the relative check covers all valid entries (flat) / every row's and column's maximum (other regimes)."""
    c, f = E.CASE_BY_NAME[name], E.facts(name)
    assert f["finite"]
    assert f["noise_abs"] <= E.abs_tolerance(c, f["noise_abs"], f["scale"]) / 2, (name, f["noise_abs"], f["scale"])
    assert f["noise_rel"] <= _rel_tol(name) / 2
    assert _rel_tol(name) < 1.0 / (2 * max(c.L, c.S)), (name, _rel_tol(name))
    if E.is_flat(c) or c.kind == "ot":
        assert f["all_valid_in_relset"] and f["min_valid"] >= E.REL_FLOOR, (name, f["min_valid"])
    assert f["maxima_in_relset"], name


@pytest.mark.parametrize("name", ALL)
def test_maxima_lead_their_runners_up_and_matches_are_many(name):
    c, f = E.CASE_BY_NAME[name], E.facts(name)
    need = E.MARGIN_FACTOR * _rel_tol(name)
    assert f["row_margin"] >= need and f["col_margin"] >= need, (name, f["row_margin"], f["col_margin"], need)
    if not E.is_degenerate(c):
        assert f["matches"] > 10 and min(f["matches_per_pair"]) > 0, (name, f["matches_per_pair"])
    assert E.is_degenerate(c) == (name in ("row_L1", "col_S1", "col_S3"))


def test_magnitude_cases_are_classified_as_intended():
    """Per-unit largest tile spread of the float64 scores against FAST_SPREAD = 64 with a margin of 8: the shared-reference variant of
    pass A keeps a unit while every 32 x 32 tile's spread stays below the threshold."""
    assert (E.SPREAD_LOW, E.FAST_SPREAD, E.SPREAD_HIGH) == (56.0, 64.0, 72.0)
    p = E.sweep_plan(*E.MAGNITUDE_SHAPE[1:])
    assert (p.RB, p.NCH) == (3, 2) and E.MAGNITUDE_SHAPE[2] % E.PC == 0             # six units per pair, every panel full
    sp = {r: E.facts(f"mag_{r}")["unit_spreads"] for r in ("flat", "peaked", "near_limit", "mixed", "all_exact")}
    assert sp["flat"].max() <= 16 and 16 <= sp["peaked"].max() <= 32
    assert E.NEAR_LIMIT[0] <= sp["near_limit"].max() <= E.NEAR_LIMIT[1]
    intended = E.inputs("mag_mixed")["intended"]
    assert intended.sum() == 5 and intended[0, 1].all() and intended[1, :, 1].all()
    assert (sp["mixed"][intended] >= E.SPREAD_HIGH).all() and (sp["mixed"][~intended] <= E.SPREAD_LOW).all(), sp["mixed"]
    assert (sp["all_exact"] >= E.SPREAD_HIGH).all(), sp["all_exact"]
    # the edge cases off this shape stay on the shared-reference side wherever their panels are full
    for c in E.DS_CASES:
        if c.masked is None and c.regime == "flat":
            assert E.facts(c.name)["unit_spreads"].max() <= E.SPREAD_LOW, c.name


def test_unit_spreads_use_the_kernels_tiles():
    s = np.zeros((1, 40, 70))
    s[0, 39, 69] = 5.0          # row block 0, wave 1 (rows 32 ... 39, clamped), panel 2 (columns 64 ... 69)
    s[0, 31, 31] = -2.0         # wave 0, panel 0
    assert E.unit_spreads(s, 40, 70).tolist() == [[[5.0]]]
    s = np.zeros((1, 300, 1000))
    s[0, 256, 511] = 3.0        # row block 1, chunk 0 (panels 0 ... 15)
    s[0, 255, 512] = 4.0        # row block 0, chunk 1
    assert E.unit_spreads(s, 300, 1000).tolist() == [[[0.0, 4.0], [3.0, 0.0]]]


@pytest.mark.parametrize("name", DS)
def test_hooked_dual_softmax_is_the_oracle(name):
    f = E.facts(name)
    assert f["hooked_distance"] <= 1e-12 * f["scale"]


@pytest.mark.parametrize("name,mutation", [(c.name, m) for c in E.DS_CASES if E.is_flat(c) for m in E.MUTATIONS if E.mutation_applies(c, m)])
def test_mutation_is_far_outside_the_relative_tolerance(name, mutation):
    d = E.facts(name)["mutation_distance"][mutation]
    assert d >= E.DETECTION_FACTOR * _rel_tol(name), (name, mutation, d, _rel_tol(name))


def test_every_mutation_meets_its_edge():
    applies = {m: {c.name for c in E.DS_CASES if E.is_flat(c) and E.mutation_applies(c, m)} for m in E.MUTATIONS}
    assert len(E.MUTATIONS) == 4 and all(applies.values())
    ragged = {c.name for c in E.DS_CASES if E.is_flat(c) and c.S % E.PC != 0 and c.S > 1}
    assert applies["row_sum_omits_last_column"] == ragged                                    # every ragged last panel
    assert applies["col_sum_counts_last_row_twice"] == {c.name for c in E.DS_CASES if E.is_flat(c) and c.L % E.BR != 0}      # every partial row block
    assert applies["row_sum_omits_first_column_of_chunk_1"] == {c.name for c in E.DS_CASES if E.is_flat(c) and E.sweep_plan(c.L, c.S).NCH > 1}
    assert applies["col_stats_shifted_in_last_panel"] == {c.name for c in E.DS_CASES if E.is_flat(c) and c.S % E.PC != 1}      # two columns or more in it
