"""CPU: the conditions tests/_sinkhorn_cases.py states about its cases hold, and the float64 comparison of
tests/test_hip_sinkhorn_edges.py can fail.  The restated ot_plan puts every case at the edge it is in the table for; the relative check
covers every row and column maximum and every dustbin entry and its bound stays below 1 / (2 max(L + 1, S + 1)); every maximum leads its
runner-up, and every dustbin of a prefilter case differs from its row's / column's best real entry, by ten relative tolerances; the kill
shares of the prefilter cases are inside [0.2, 0.8].  These are conditions on the choice of the inputs: a case that misses one gets
another seed (SEEDS), never another factor.  The float64 iteration restated from its pieces reproduces the oracle, and with each modelled
kernel mistake built in it sits at least DETECTION_FLOOR relative tolerances from ref64 on every case the mistake applies to, and
DETECTION_FACTOR on those with S <= DETECTION_S."""
import pytest

import _sinkhorn_cases as E

ALL = [c.name for c in E.CASES]


def _rel_tol(name, region="conf"):
    return E.rel_tolerance(region, E.facts(name)[region]["noise_rel"])


def test_plan_arithmetic_and_variant_constants():
    assert (E.NARROW, E.WIDE_ITER, E.WIDE_FINAL) == ((256, 5, 2), (512, 6, 1), (1024, 3, 1))
    assert (E.ROWSTREAM_MAX, E.NARROW_MAX, E.OT_RCH) == (12288, 5120, 128)
    # indoor 60 x 80 at N = 8 and outdoor 105 x 105 at N = 2: the shapes the plan was tuned on
    assert E.ot_plan(8, 4800, 4800) == (True, False, True, 96, 50, 128)
    assert E.ot_plan(2, 11025, 11025)[:5] == (True, True, False, 127, 87)
    assert E.ot_plan(1, 4097, 33)[:5] == (True, False, False, 121, 34) and E.ot_plan(3, 33, 160)[:5] == (True, False, True, 6, 6)
    assert E.ot_plan(2, 45, 5121)[:5] == (True, True, False, 8, 6) and E.ot_plan(2, 5, 5121)[3:5] == (5, 1)
    assert not E.ot_plan(2, 130, 12288).rowstream and E.fallback_chunks(3) == (1, 4) and E.fallback_chunks(130) == (2, 66)
    for N in (1, 2, 3, 8, 9):
        for S in (160, 5121):
            for L in range(1, 700):
                p, R = E.ot_plan(N, L, S), E.variants(S)[0].R
                ranges = E.row_ranges(N, L, S)
                assert 1 <= p.wgs <= E.OT_RCH and p.rpws % R == 0 and ranges[0][0] == 0 and ranges[-1][1] == L
                assert all(a < b for a, b in ranges) and all(ranges[k][1] == ranges[k + 1][0] for k in range(p.wgs - 1))
    assert E.tail_owner(5119, E.NARROW) == (255, 4, 3) and E.tail_owner(12287, E.WIDE_ITER) == (511, 5, 3) and E.tail_owner(12287, E.WIDE_FINAL) == (1023, 2, 3)


def test_every_case_is_at_the_edge_it_is_listed_for():
    assert not E.edge_failures()
    assert {e for c in E.CASES for e in c.edges} == set(E.EDGES)
    shapes = {(c.N, c.L, c.S) for c in E.CASES if c.regime == "ot" and c.name not in E.MASKS and (c.iters, c.bin_score, c.prefilter) == (3, 1.0, False)}
    assert {S for N, L, S in shapes if (N, L) == (3, 33)} >= {1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 5116, 5119}
    assert {S for N, L, S in shapes if (N, L) == (2, 40)} >= {5120, 5121, 6143, 6144, 6145, 8191, 8192, 8193, 11025, 12284, 12287}
    assert {(L, S) for N, L, S in shapes if N == 2 and S >= 12288} == {(L, S) for L in (3, 130) for S in (12288, 12321, 12351)}
    assert {L for N, L, S in shapes if (N, S) == (3, 160)} >= {1, 2} and (1, 4097, 33) in shapes
    assert {c.N for c in E.CASES} == {1, 2, 3, 9}
    for tag, N, L, S in E.SETTINGS_SHAPES:
        got = {(c.iters, c.bin_score, c.prefilter, c.regime) for c in E.CASES if (c.N, c.L, c.S) == (N, L, S) and c.name.startswith("set_")}
        assert got == {(0, 1.0, False, "ot"), (1, 1.0, False, "ot"), (10, 1.0, False, "ot"), (3, -2.0, False, "ot"), (3, 8.0, True, "ot"),
                       (3, 1.0, False, "peaked")}, tag
    pre = [c for c in E.CASES if c.regime == "half"]
    assert len(pre) == 5 and all(c.prefilter and 1.0 <= c.bin_score <= 4.0 for c in pre)
    assert max(c.N * c.L * c.S for c in E.CASES) <= 3.5e6
    for c in E.CASES:
        assert E.grid(c.L)[0] * E.grid(c.L)[1] == c.L and E.grid(c.S)[0] * E.grid(c.S)[1] == c.S


def test_mask_patterns():
    """Valid rectangles at the top left, no pair without valid tokens; without border removal only one image of a pair is padded; the
    dead row ranges and the valid extent that ends inside a four-column group."""
    for name in E.MASKS:
        i = E.inputs(name)
        c = i["case"]
        for m in (i["m0"], i["m1"]):
            for n in range(c.N):
                vh, vw = int(m[n].any(1).sum()), int(m[n].any(0).sum())
                assert vh > 0 and vw > 0 and m[n, :vh, :vw].all() and m[n].sum() == vh * vw
        if i["border_rm"] == 0:
            assert all(i["m0"][n].all() or i["m1"][n].all() for n in range(c.N))
        assert any(not i["m0"][n].all() for n in range(c.N)) and any(not i["m1"][n].all() for n in range(c.N))
    i = E.inputs("mask_both_3x63x960")
    assert i["border_rm"] == 1 and any(not i["m0"][n].all() and not i["m1"][n].all() for n in range(3))
    assert E.facts("mask_dead_range_3x64x160")["dead_ranges"] == [(0, 6), (0, 7), (2, 4), (2, 5), (2, 6), (2, 7)]
    m1 = E.flat_masks(E.inputs("mask_inside_group_3x33x957"))[1]
    last = [int(m1[n].nonzero()[0][-1]) for n in range(3)]
    assert last[0] == 26 * 33 + 30 and (last[0] + 1) % 4 == 1 and last[0] >> 2 < 957 >> 2


@pytest.mark.parametrize("name", ALL)
def test_reference_noise_and_coverage(name):
    """ref32 stays inside half of either tolerance in both regions; the relative bounds are below half of what one dropped or doubled
    term changes in a flat sum; the relative check covers every row's and column's maximum and every dustbin entry."""
    c, f = E.CASE_BY_NAME[name], E.facts(name)
    assert f["finite"] and f["padding_max"] == 0.0
    for region in ("conf", "bins"):
        g = f[region]
        assert g["noise_abs"] <= E.abs_tolerance(region, g["noise_abs"], g["scale"]) / 2, (name, region, g)
        assert g["noise_rel"] <= _rel_tol(name, region) / 2
        assert _rel_tol(name, region) < 1.0 / (2 * max(c.L + 1, c.S + 1)), (name, region, _rel_tol(name, region))
    assert f["maxima_in_relset"] and f["bins_in_relset"] and f["min_bin"] >= E.BIN_FLOOR, (name, f["min_bin"])


@pytest.mark.parametrize("name", ALL)
def test_maxima_lead_their_runners_up(name):
    c, f = E.CASE_BY_NAME[name], E.facts(name)
    need = E.MARGIN_FACTOR * _rel_tol(name)
    assert f["row_margin"] >= need and f["col_margin"] >= need, (name, f["row_margin"], f["col_margin"], need)
    if E.expects_no_match(c):
        assert f["matches"] == 0 and f["live_rows"] == 0 and f["live_cols"] == 0
    elif c.N * min(c.L, c.S) > 10:
        assert f["matches"] > 10 and min(f["matches_per_pair"]) > 0, (name, f["matches_per_pair"])
    else:
        assert f["matches"] > 0, name


@pytest.mark.parametrize("name", [c.name for c in E.CASES if c.prefilter])
def test_prefilter_decisions_are_clear_and_split_the_rows(name):
    c, f = E.CASE_BY_NAME[name], E.facts(name)
    assert f["kill_margin"] >= E.MARGIN_FACTOR * _rel_tol(name), (name, f["kill_margin"])
    if E.expects_no_match(c):
        assert f["row_kill_share"] == 1.0 and f["col_kill_share"] == 1.0
        return
    assert 0.2 <= f["row_kill_share"] <= 0.8, (name, f["row_kill_share"])
    if c.L == c.S:
        assert 0.2 <= f["col_kill_share"] <= 0.8, (name, f["col_kill_share"])
    if "prefilter_tail_kill" in c.edges:
        assert f["tail_kills"] >= 1 and c.S % 4 != 0, name


@pytest.mark.parametrize("name", ALL)
def test_restated_iteration_is_the_oracle(name):
    assert E.facts(name)["hooked_distance"] <= 1e-12


@pytest.mark.parametrize("name,mutation", [(c.name, m) for c in E.CASES for m in E.MUTATIONS if E.mutation_applies(c, m)])
def test_mutation_is_far_outside_the_relative_tolerance(name, mutation):
    c, d = E.CASE_BY_NAME[name], E.facts(name)["mutation_distance"][mutation]
    assert d >= (E.DETECTION_FACTOR if c.S <= E.DETECTION_S else E.DETECTION_FLOOR), (name, mutation, d)


def test_every_mutation_meets_its_edge():
    applies = {m: {c.name for c in E.CASES if E.mutation_applies(c, m)} for m in E.MUTATIONS}
    assert len(E.MUTATIONS) == 7 and all(applies.values())
    iterated = {c.name for c in E.CASES if c.iters > 0}
    flat = {c.name for c in E.CASES if c.iters > 0 and c.regime != "peaked"}                 # (a peaked row's sum is its planted entry alone)
    assert applies["col_lse_omits_dustbin_row"] == iterated and applies["row_lse_omits_dustbin_column"] == flat
    assert applies["last_row_of_range_folded_twice"] == {c.name for c in E.CASES if c.iters > 0 and c.S < E.NARROW_MAX and c.L % 2 == 1}
    assert applies["row_sum_omits_tail_columns"] == {n for n in flat if 4 < E.CASE_BY_NAME[n].S < E.ROWSTREAM_MAX and E.CASE_BY_NAME[n].S % 4 != 0}
    assert applies["last_partial_dropped_in_merge"] >= {c.name for c in E.CASES if c.iters > 0 and c.S >= E.ROWSTREAM_MAX and c.L > 1}
    assert {E.ot_plan(c.N, c.L, c.S).wide for c in E.CASES if c.name in applies["kill_mask_shifted_by_one_group"]} == {False, True}
