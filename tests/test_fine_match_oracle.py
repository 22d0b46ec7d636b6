"""CPU side of the fine matching's edge tests: the conditions tests/_fine_match_cases.py states hold, its float64 restatement equals
the oracle, the oracle reproduces what the reference itself produced (a golden), and each modelled mistake leaves a bound on at least
one case -- so tests/test_hip_fine_match_edges.py can fail."""
import numpy as np
import pytest

import _fine_match_cases as F
from _cases import TOL_PX, load_case
from oracle import loftr_oracle as O

NAMES = [c.name for c in F.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_case_conditions(name):
    c, i, r = F.CASE_BY_NAME[name], F.inputs(name), F.reference(name)
    assert i["f0"].shape == i["f1"].shape == (c.M, c.W * c.W, c.C) and i["f0"].dtype == np.float32
    # the restatement is the oracle, and the oracle's float32 run passes every bound (K >= 1)
    e, p, _ = F.fine_match_float64(name)
    assert np.abs(e - r["expec"]).max() <= 1e-6 and np.abs(p - r["px"]).max() <= r["ulp_px"]
    assert F.check(name, r["expec32"], r["px32"])[1] == []
    # the cap does not hide a failure
    assert r["noise_px"] <= TOL_PX / 4, r["noise_px"]
    assert r["noise_std"] <= (1e-6 if r["conditioned"] else F.STD_LOOSE / 4), r         # the loose std bound does not hide a failure either
    assert np.abs(i["mkpts1_c"]).max() == c.coords <= 2000
    # regimes
    if c.regime in ("flat", "moderate"):
        assert r["conditioned"], r["min_var"]
    if c.regime in ("onehot", "corner"):
        assert np.abs(np.abs(r["expec"][:, :2]) - np.round(np.abs(r["expec"][:, :2]) * (c.W - 1)) / (c.W - 1)).max() < (1e-4 if c.regime == "onehot" else 1e-6)   # on a grid node
    if c.regime == "onehot":
        assert r["min_var"] < 1e-10 and np.abs(r["expec"][:, 2] - 2e-5).min() < 1e-9                # both variances clamp (on a match at least)
    if c.regime == "corner":
        want = np.array([[2.0 * x / (c.W - 1) - 1, 2.0 * y / (c.W - 1) - 1] for y, x in (F.corner_of(m, c.W) for m in range(c.M))])
        assert np.abs(r["expec"][:, :2] - want).max() < 1e-6 and np.abs(np.abs(want) - 1).max() == 0
        s1 = c.scale * (i["scale1"][i["b_ids"]] if c.scaled else 1.0)
        assert np.abs(np.abs(r["px"] - i["mkpts1_c"]) - (c.W // 2) * s1).max() < 1e-3                # the full offset W // 2
    if c.regime == "shifted":
        sim = np.einsum("mc,mrc->mr", i["f0"][:, c.W * c.W // 2].astype(np.float64), i["f1"].astype(np.float64)) / c.C ** .5
        assert sim.min() > 2000 * c.C ** .5
    if c.scaled:
        b = i["b_ids"]
        assert b[0] != 0 and (c.M == 1 or ((np.diff(b) < 0).any() and len(set(b.tolist())) >= 2))
        assert (F.SCALE1[:, 0] != F.SCALE1[:, 1]).all()


def test_reference_reproduces_golden():
    """oracle.fine_matching on the windows the reference's fine transformer produced gives the reference's expec_f / mkpts1_f."""
    rc, inp, g = load_case("small_mask")
    n = len(g["feat_f0_unfold"])
    assert n >= 4
    expec, _, mk1 = O.fine_matching(g["feat_f0_unfold"], g["feat_f1_unfold"], g["mkpts0_c"][:n], g["mkpts1_c"][:n], g["b_ids"][:n],
                                    inp["hw0_i"], (inp["hw0_i"][0] // 2, inp["hw0_i"][1] // 2), scale1=inp["scale1"], has_scale0=True)
    assert np.abs(expec[:, :2] - g["expec_f"][:n, :2]).max() <= 4 * 1.7e-5      # two float32 evaluations, each within float32's own noise
    assert np.abs(expec[:, 2] - g["expec_f"][:n, 2]).max() <= F.STD_LOOSE
    assert np.abs(mk1 - g["mkpts1_f"][:n]).max() <= TOL_PX / 4


def test_regimes_cover_both_std_bounds():
    cond = {c.regime: [] for c in F.CASES}
    for c in F.CASES:
        cond[c.regime].append(F.reference(c.name)["conditioned"])
    assert all(cond["flat"]) and all(cond["moderate"]) and not any(cond["onehot"]) and not any(cond["corner"]) and not all(cond["peaked"])


@pytest.mark.parametrize("mistake", F.MISTAKES)
def test_modelled_mistake_is_detected(mistake):
    caught = []
    for name in NAMES:
        e, p, _ = F.fine_match_float64(name, mistake)
        if F.check(name, e, p)[1]:
            caught.append(name)
    assert caught, mistake
