"""The dual-softmax score sweep (sweep::score_sweep_kernel, merge_stats_kernel, merge_colmax_kernel, select_kernel) against the numpy
oracle in FLOAT64 at its row-block, panel, ring, chunk and XCD-dealing edges, in every numerical regime of its two passes and under
padding masks; the Sinkhorn score store (pass 2 of the same sweep) at its ragged and unaligned sizes.  Cases, reference, tolerances and
the conditions the inputs meet: tests/_score_sweep_cases.py.  Every other test of the sweep at these sizes compares it with itself.

Two bounds per case: err_abs <= min(K_ABS * noise_abs + 1e-6 * scale, TOL_CONF) over the valid entries, and
err_rel <= K_REL * noise_rel + 1e-6 over the valid entries >= 1e-12 (all of them on flat inputs), where noise is the distance of the
oracle's own float32 run to its float64 run on the same case.  The relative bound is what sees a row or column sum that lost or doubled
one term.  Match ids and coarse keypoints are exactly those of the reference selection on ref64 (the inputs' maxima lead their
runners-up by ten relative tolerances), mconf is held to the absolute bound.  Each run prints its own figures before it asserts, and
appends them to the file LOFTR_EDGES_REPORT names, if set (how profiles/score_sweep_accuracy.txt was written).
"""
import os

import numpy as np
import pytest

import _score_sweep_cases as E

pytestmark = pytest.mark.gpu


def _report(line):
    path = os.environ.get("LOFTR_EDGES_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")
    print(line)


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared inputs are read-only)


def _ratio(err, noise):
    return err / noise if noise > 0 else (0.0 if err == 0 else float("inf"))


def _run(i, **kw):
    import torch
    from loftr_amd import ops
    m0, m1 = i["m0"], i["m1"]
    r = ops.coarse_match(_t(i["f0"]), _t(i["f1"]), i["hw0"], i["hw1"], thr=0.0, border_rm=i["border_rm"], scale=8.0,
                         mask0=None if m0 is None else _t(m0).flatten(-2), mask1=None if m1 is None else _t(m1).flatten(-2), **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None and hasattr(v, "cpu") else v) for k, v in r.items()}


def _check_volume(name, path, got, r, failures):
    """Finite everywhere, then the absolute and the relative bound on the entries each uses."""
    c = E.CASE_BY_NAME[name]
    assert np.isfinite(got).all(), (name, path, "not finite", int((~np.isfinite(got)).sum()))
    got = got.astype(np.float64)
    err_abs = float(np.abs(got - r["ref64"])[r["valid"]].max())
    err_rel = E.rel_error(got, r)
    tol_abs, tol_rel = E.abs_tolerance(c, r["noise_abs"], r["scale"]), E.rel_tolerance(c, r["noise_rel"])
    _report(f"{name:22s} {path:14s} abs err {err_abs:.3e} noise {r['noise_abs']:.3e} err/noise {_ratio(err_abs, r['noise_abs']):6.2f} "
            f"scale {r['scale']:.3e} | rel err {err_rel:.3e} noise {r['noise_rel']:.3e} err/noise {_ratio(err_rel, r['noise_rel']):6.2f}")
    if err_abs > tol_abs:
        failures.append((path, "abs", err_abs, tol_abs, r["noise_abs"]))
    if err_rel > tol_rel:
        failures.append((path, "rel", err_rel, tol_rel, r["noise_rel"]))


def _check_matches(name, path, out, i, r, failures):
    """Ids and coarse keypoints exactly those of the reference selection, mconf inside the absolute bound, counts consistent with b_ids,
    ids inside the valid rectangles."""
    c, sel = i["case"], r["sel"]
    b, ii, jj = out["b_ids"], out["i_ids"], out["j_ids"]
    counts = out["counts"]
    assert counts[0] == len(b) and np.array_equal(counts[1:], np.bincount(b, minlength=c.N)), (name, path, counts.tolist())
    order = np.lexsort((ii, b))
    got_ids = np.stack([b, ii, jj], 1)[order]
    want_ids = np.stack([sel["b_ids"], sel["i_ids"], sel["j_ids"]], 1)
    if got_ids.shape != want_ids.shape or not np.array_equal(got_ids, want_ids):
        diff = sorted(set(map(tuple, got_ids.tolist())) ^ set(map(tuple, want_ids.tolist())))
        failures.append((path, "ids", len(got_ids), len(want_ids), diff[:8]))
        return
    if i["m0"] is not None:
        m0, m1 = E.flat_masks(i)
        assert m0[b, ii].all() and m1[b, jj].all(), (name, path, "a match in the padding")
    assert np.array_equal(out["mkpts0_c"][order], sel["mkpts0_c"]) and np.array_equal(out["mkpts1_c"][order], sel["mkpts1_c"]), (name, path)
    err = float(np.abs(out["mconf"][order].astype(np.float64) - r["ref64"][sel["b_ids"], sel["i_ids"], sel["j_ids"]]).max()) if len(b) else 0.0
    tol = E.abs_tolerance(c, r["noise_abs"], r["scale"])
    _report(f"{name:22s} {path:14s} abs err {err:.3e} noise {r['noise_abs']:.3e} err/noise {_ratio(err, r['noise_abs']):6.2f} matches {len(b)}")
    if err > tol:
        failures.append((path, "mconf", err, tol, r["noise_abs"]))


@pytest.mark.parametrize("name", [c.name for c in E.DS_CASES])
def test_dual_softmax_sweep_vs_float64(name):
    """ops.coarse_match(match_type="dual_softmax", temperature=0.1, thr=0.0) with conf_matrix materialised (pass B tracks the arg-max per
    panel, select_kernel reads the panel back; masked: per element) and without (per-element tracking), against ref64.
    K_ABS / K_REL: see tests/_score_sweep_cases.py."""
    i, r = E.inputs(name), E.reference(name)
    failures = []
    out = _run(i, match_type="dual_softmax", temperature=E.TEMPERATURE, want_conf=True)
    _check_volume(name, "conf", out["conf_matrix"], r, failures)
    _check_matches(name, "mconf", out, i, r, failures)
    lean = _run(i, match_type="dual_softmax", temperature=E.TEMPERATURE, want_conf=False)
    assert lean["conf_matrix"] is None
    _check_matches(name, "mconf_elided", lean, i, r, failures)
    assert not failures, (name, failures)


@pytest.mark.parametrize("name", [c.name for c in E.OT_CASES])
def test_sinkhorn_score_store_vs_float64(name):
    """ops.coarse_match(match_type="sinkhorn", bin_score=1.0, skh_iters=3): conf_matrix and the inner block of conf_matrix_with_bin on the
    valid entries against oracle.sinkhorn_conf in float64 (masked entries are rounding noise of sums with |u|, |v| ~ 1e9)."""
    i, r = E.inputs(name), E.reference(name)
    failures = []
    out = _run(i, match_type="sinkhorn", bin_score=E.BIN_SCORE, skh_iters=E.SKH_ITERS, want_assign=True)
    _check_volume(name, "conf", np.where(r["valid"], out["conf_matrix"], 0.0), r, failures)
    _check_volume(name, "assign_inner", np.where(r["valid"], out["conf_matrix_with_bin"][:, :-1, :-1], 0.0), r, failures)
    _check_matches(name, "mconf", out, i, r, failures)
    assert not failures, (name, failures)
