"""CPU side of the coarse selection's edge tests: every condition tests/_select_cases.py states holds on the oracle's own float32
confidence of the case, the numpy restatement of the kernels' selection equals the reference selection, the reference selection
reproduces the reference-generated goldens it already serves, and each modelled mistake changes the expected output of its case --
so tests/test_hip_select_edges.py can fail."""
import functools
import os

import numpy as np
import pytest

import _select_cases as E
from _cases import GOLDEN_DIR, load_case
from oracle import loftr_oracle as O


@functools.lru_cache(maxsize=None)
def _conf(name, path):
    i = E.inputs(name, path)
    conf = E.oracle_conf(i)
    assert conf.dtype == np.float32 and np.isfinite(conf).all()
    conf.flags.writeable = False
    return conf


def _thr(name, path):
    c = E.CONFIG_BY_NAME[name]
    if c.thr != "median":
        return np.float32(c.thr)
    i = E.inputs(name, path)
    return E.median_threshold(E.expected(_conf(name, path), i, 0.0)["mconf"])


@pytest.mark.parametrize("name,path", E.RUNS)
def test_model_equals_reference_selection(name, path):
    """model_select without a mistake is `expected` on every run (so a mistake's effect is the mistake's alone), and `compare` passes."""
    i, conf = E.inputs(name, path), _conf(name, path)
    thr = _thr(name, path)
    want = E.expected(conf, i, thr)
    assert E.compare(E.model_select(conf, i, thr), want, conf, i["config"].N) == []
    ids = np.stack([want["b_ids"], want["i_ids"]], 1)
    assert np.array_equal(ids, ids[np.lexsort((ids[:, 1], ids[:, 0]))])                   # the reference's order: ascending (b, i)


@pytest.mark.parametrize("path", E.CONFIG_BY_NAME["threshold"].paths)
def test_threshold_condition(path):
    i, conf = E.inputs("threshold", path), _conf("threshold", path)
    at0 = E.expected(conf, i, 0.0)
    thr = E.median_threshold(at0["mconf"])
    below = np.nextafter(thr, np.float32(0))
    assert thr.dtype == np.float32 and below.dtype == np.float32 and 0 < below < thr
    n_at, n_above = int((at0["mconf"] == thr).sum()), int((at0["mconf"] > thr).sum())
    assert n_at >= 1 and n_above >= 3
    assert len(E.expected(conf, i, thr)["mconf"]) == n_above
    assert len(E.expected(conf, i, below)["mconf"]) == n_above + n_at


@pytest.mark.parametrize("path", E.CONFIG_BY_NAME["borders_b1"].paths)
def test_border_conditions(path):
    for b in (1, 2, 3):
        i = E.inputs(f"borders_b{b}", path)
        hit = E.border_sides_hit(_conf(f"borders_b{b}", path), i)
        assert min(hit) >= 1, (b, hit)
        assert len(E.expected(_conf(f"borders_b{b}", path), i, 0.0)["b_ids"]) >= 4, b
    i, conf = E.inputs("borders_one_cell", path), _conf("borders_one_cell", path)
    want = E.expected(conf, i, 0.0)
    assert want["i_ids"].tolist() == [12, 12] and want["j_ids"].tolist() == [12, 12]     # the one interior cell of a 5 x 5 grid, both pairs
    i, conf = E.inputs("borders_no_interior", path), _conf("borders_no_interior", path)
    want = E.expected(conf, i, 0.0)
    assert len(want["b_ids"]) == 0 and not want["counts"].any()
    assert len(O.coarse_match_select(conf, 0.0, 0, (4, 5), (4, 5), (32, 40))["b_ids"]) >= 8


@pytest.mark.parametrize("path", E.CONFIG_BY_NAME["padding"].paths)
def test_padding_conditions(path):
    i, conf = E.inputs("padding", path), _conf("padding", path)
    want = E.expected(conf, i, 0.0)
    per = want["counts"][1:]
    assert per[0] >= 3 and per[1] >= 1 and per[2] == 0, per.tolist()
    m0, m1 = i["m0"].reshape(4, -1), i["m1"].reshape(4, -1)
    k = want["b_ids"] == 1
    assert m0[1, want["i_ids"][k]].all() and m1[1, want["j_ids"][k]].all()
    # pair 3: the wrapped limit lets padding rows x padding columns through, a clamped limit does not
    k = want["b_ids"] == 3
    clamped = E.model_select(conf, i, 0.0, "limit_clamped")
    assert (clamped["b_ids"] == 3).sum() == 0
    if i["path"].kind == "ds":
        assert k.sum() >= 2 and not m0[3, want["i_ids"][k]].any() and not m1[3, want["j_ids"][k]].any()
        assert E.compare(clamped, want, conf, 4) != []


def test_tie_conditions():
    for path in E.CONFIG_BY_NAME["ties"].paths:
        i, conf = E.inputs("ties", path), _conf("ties", path)
        want = E.expected(conf, i, 0.0)
        rep = E.tie_report(conf, want)
        for placement, (exact, later) in rep.items():
            assert exact and later >= (1 if placement in E.TIE_OPTIONAL else 2), (path, placement, exact, later)
        j1, j2 = E.TIE_BOTH_INTERIOR
        for b in range(2):
            assert conf[b, E.TIE_BOTH_ROW, j1] == conf[b, E.TIE_BOTH_ROW, j2] and (b, E.TIE_BOTH_ROW, j1) in set(
                zip(want["b_ids"].tolist(), want["i_ids"].tolist(), want["j_ids"].tolist())), (path, b)
        # without the matrix exactly the later-tie rows are absent
        lean = E.expected_elided(conf, i, 0.0)
        full_ids = set(zip(want["b_ids"].tolist(), want["i_ids"].tolist(), want["j_ids"].tolist()))
        lean_ids = set(zip(lean["b_ids"].tolist(), lean["i_ids"].tolist(), lean["j_ids"].tolist()))
        assert lean_ids <= full_ids and len(full_ids - lean_ids) == sum(l for _, l in rep.values())
    # j1 precedes j2; where a row is planted on j2, j1 is a border cell and j2 interior; the placements are what their names say
    planted = {j for j, _ in E.TIE_PLANTS}
    for placement, pairs in E.TIE_PLACEMENTS.items():
        assert sum(j2 in planted for _, j2 in pairs) >= (1 if placement in E.TIE_OPTIONAL else 2)
        for j1, j2 in pairs:
            y1, x1, y2, x2 = j1 // 32, j1 % 32, j2 // 32, j2 % 32
            assert j1 < j2 and (j2 not in planted or ((y1 in (0, 30) or x1 in (0, 31)) and 1 <= y2 <= 28 and 1 <= x2 <= 30))
            assert ((j1 // 32 == j2 // 32), (j1 // 512 == j2 // 512)) == \
                {"same_panel": (True, True), "same_chunk": (False, True), "same_chunk_single": (False, True), "two_chunks": (False, False)}[placement]
    assert [j1 for j1, _ in E.TIE_PLACEMENTS["same_chunk"]] == list(range(32))           # panel 0 as a whole


def test_scan_conditions():
    i, conf = E.inputs("scan", "P4_64"), _conf("scan", "P4_64")
    want = E.expected(conf, i, 0.0)
    flat = want["b_ids"] * (105 * 105) + want["i_ids"]
    assert len(flat) >= 200 and (flat >= 262144).sum() >= 3
    assert ((want["b_ids"] == 23) & (flat < 1024 * 256)).sum() >= 1
    assert flat.max() == 24 * 105 * 105 - 1                                              # the last row of the last block


def test_many_pairs_and_straddle_conditions():
    for name, path in [r for r in E.RUNS if r[0].startswith(("many_pairs", "straddle", "scales"))]:
        i, conf = E.inputs(name, path), _conf(name, path)
        want = E.expected(conf, i, 0.0)
        per = want["counts"][1:]
        if name.startswith("many_pairs"):
            assert (per >= 1).sum() >= 64, (name, path)
        elif not i["path"].prefilter:
            assert (per >= 1).all(), (name, path, per.tolist())
        if name in ("straddle", "scales") and not i["path"].prefilter:
            flat = want["b_ids"] * 91 + want["i_ids"]
            assert (flat >= 256).any() and (flat < 256).any()
        if name == "scales":
            assert np.unique(want["mkpts0_c"] / np.maximum(want["mkpts1_c"], 1e-3)).size > 4


def test_empty_conditions():
    for name, path in [r for r in E.RUNS if r[0].startswith("empty")]:
        i, conf = E.inputs(name, path), _conf(name, path)
        assert conf.max() < 0.999
        want = E.expected(conf, i, 0.999)
        assert len(want["b_ids"]) == 0 and not want["counts"].any()
        assert want["mkpts0_c"].shape == (0, 2) and want["mconf"].shape == (0,)


@pytest.mark.parametrize("mistake", E.MISTAKES)
def test_modelled_mistake_is_detected(mistake):
    name, path = E.MISTAKE_CASE[mistake]
    i, conf = E.inputs(name, path), _conf(name, path)
    thr = _thr(name, path)
    want = E.expected(conf, i, thr)
    assert E.compare(E.model_select(conf, i, thr, mistake), want, conf, i["config"].N) != [], mistake


# ---- the restatement is pinned to what the reference itself produced ---------------------------------------------------------------------
def _ids(d):
    return list(zip(np.asarray(d["b_ids"]).tolist(), np.asarray(d["i_ids"]).tolist(), np.asarray(d["j_ids"]).tolist()))


def test_reference_selection_reproduces_tie_golden():
    g = dict(np.load(os.path.join(GOLDEN_DIR, "ties_ds.npz")))
    conf = O.dual_softmax_conf(g["feat_c0"], g["feat_c1"], 0.1)
    sel = O.coarse_match_select(conf, float(g["thr"]), int(g["border_rm"]), (8, 10), (8, 10), (64, 80))
    assert _ids(sel) == _ids(g) and len(_ids(g)) > 10
    assert np.array_equal(sel["mkpts0_c"], g["mkpts0_c"]) and np.array_equal(sel["mkpts1_c"], g["mkpts1_c"])


@pytest.mark.parametrize("case", ["small_mask", "small_ot"])
def test_reference_selection_reproduces_golden(case):
    """On the conf_matrix the reference stored: its ids in its order, its coarse keypoints bitwise (masks and per-pair scales included)."""
    rc, inp, g = load_case(case)
    conf = np.asarray(g["conf_matrix"], np.float32)
    mc = inp["cfg"]["match_coarse"]
    hw0, hw1 = tuple(rc["hw0_c"]), tuple(rc["hw1_c"])
    sel = O.coarse_match_select(conf, mc["thr"], mc["border_rm"], hw0, hw1, inp["hw0_i"], inp["mask0"], inp["mask1"], inp["scale0"], inp["scale1"])
    assert _ids(sel) == _ids(g) and len(_ids(g)) > 10
    assert np.array_equal(sel["mconf"], g["mconf"])
    assert np.array_equal(sel["mkpts0_c"], g["mkpts0_c"]) and np.array_equal(sel["mkpts1_c"], g["mkpts1_c"])
