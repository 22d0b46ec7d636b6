"""CPU: the conditions tests/_fine_bwd_cases.py states about its cases hold, and the float64 comparison of
tests/test_hip_fine_bwd_edges.py can fail.  The restated module reproduces the committed gfpre fixture (gradients of the reference's own
FinePreprocess); the restated dispatch arithmetic puts every case at the edge it is in the table for; the matches cover the corner
cells, shared cells and the 48-deep cell; ref32 stays inside half of every tolerance; and each modelled kernel mistake sits at least
DETECTION_FACTOR tolerances from ref64 in at least one output tensor on every case it applies to."""
import json
import os

import numpy as np
import pytest
import torch

import _fine_bwd_cases as E

ALL = [c.name for c in E.CASES]


def test_restated_module_reproduces_the_reference_golden():
    """float32, as the fixture was written: both outputs, the four feature gradients and every weight-gradient digest within 1e-5 of the
    tensor's maximum."""
    g = np.load(os.path.join(E.HERE, "golden", "gfpre.npz"))
    rc = json.loads(str(g["recipe"]))
    got = E.run(dict(E.MG.build(rc), W=rc["W"], stride=rc["stride"]), torch.float32)
    for k in E.MAPS:
        assert np.abs(got[k] - g[k]).max() <= 1e-5 * np.abs(g[k]).max(), (k, float(np.abs(got[k] - g[k]).max()))
    for key in E.PARAM_KEY.values():
        for part, v in E.MG.digest(key, got[key]).items():
            ref = g[part]
            scale = max(float(np.abs(ref).max()), float(g[f"{key}/absmax"]) if "/" in part else 0.0)
            assert np.abs(v - ref).max() <= 1e-5 * scale, (part, float(np.abs(v - ref).max()), scale)


def test_dispatch_arithmetic_and_edges():
    assert (E.COLSUM_ROWS, E.TALL_FROM, E.N, E.HC0, E.HC1, E.STRIDE) == (256, 16, 2, (6, 8), (5, 9), 4)
    assert E.plan(1, 5, 128)[:4] == (50, 2, (1, 50), (1, 2)) and E.plan(3, 5, 128).merge == (2, 22)
    assert E.plan(5, 5, 128).colsum_T == (1, 250) and E.plan(6, 5, 128).colsum_T == (2, 44)
    assert E.plan(64, 5, 128)[:4] == (3200, 128, (25, 128), (1, 128)) and E.plan(65, 5, 128)[:4] == (3250, 130, (26, 50), (2, 2))
    assert E.plan(41, 5, 128).merge == (17, 2) and E.plan(20, 3, 64)[:4] == (360, 40, (3, 104), (1, 40))
    assert not E.edge_failures() and {e for c in E.CASES for e in c.edges} == set(E.EDGES)
    assert {(c.M, c.Cf, c.Cc, c.W, c.layout) for c in E.CASES} == {(M, 128, 256, 5, "spread") for M in (1, 3, 5, 6, 64, 65, 41)} | {
        (48, 128, 256, 5, "one_cell"), (20, 64, 128, 3, "spread")}


@pytest.mark.parametrize("name", ALL)
def test_matches_and_reference_noise(name):
    c, f, inp = E.CASE_BY_NAME[name], E.facts(name), E.inputs(name)
    assert f["finite"]
    assert (0 <= inp["b_ids"]).all() and (inp["b_ids"] < E.N).all() and (0 <= inp["i_ids"]).all() and (inp["i_ids"] < 48).all()
    assert (0 <= inp["j_ids"]).all() and (inp["j_ids"] < 45).all() and len(inp["b_ids"]) == c.M and (np.diff(inp["b_ids"]) >= 0).all()
    if c.layout == "one_cell":                    # 48 matches on corner cell 0 of image 0, on three cells of image 1 (two of them corners)
        assert (f["cells0"], f["depth0"], f["cells1"], f["clipped"]) == (1, 48, 3, 48) and f["corners0"] == 1 and f["corners1"] == 2
    else:                                         # the four corners of both maps, as many as there are matches; a shared cell from M = 6
        assert f["corners0"] == f["corners1"] == min(c.M, 4) and f["clipped"] >= min(c.M, 3)
        assert (f["shared"] >= 1 and f["depth0"] >= 2) == (c.M >= 6)
    for k in E.OUTPUTS:
        noise, scale = f["noise"][k], f["scale"][k]
        assert scale > 0 and noise <= E.tolerance(k, noise, scale) / 2 and noise <= 1e-5 * scale, (name, k, noise, scale)


@pytest.mark.parametrize("name,mutation", [(c.name, m) for c in E.CASES for m in E.MUTATIONS if E.mutation_applies(c, m)])
def test_mutation_is_far_outside_the_tolerance(name, mutation):
    d = E.facts(name)["mutation_distance"][mutation]
    assert d >= E.DETECTION_FACTOR, (name, mutation, d)


def test_every_mutation_meets_its_edge():
    applies = {m: {c.name for c in E.CASES if E.mutation_applies(c, m)} for m in E.MUTATIONS}
    assert len(E.MUTATIONS) == 3 and applies["clipped_pixel_clamped"] == applies["colsum_last_block"] == set(ALL)
    assert applies["shared_cell_overwritten"] == {c.name for c in E.CASES if c.M >= 6}
