"""The Sinkhorn passes (otp::ot_pass_kernel in its narrow and wide variants, ot_col_merge2_kernel; for rows wider than 12287 columns
ot_row_lse_kernel, ot_col_part_kernel, ot_col_merge_kernel and ot_finalize_kernel; ot_rowkill_kernel, ot_colkill_kernel,
ot_assign_bins_kernel) against the numpy oracle in FLOAT64 at their column-group, row-range and dispatch edges, at other iteration
counts and dustbin scores, with the dustbin prefilter and under padding masks.  Cases, reference, tolerances and the conditions the
inputs meet: tests/_sinkhorn_cases.py.

Per region (conf: conf_matrix and the inner block of conf_matrix_with_bin on the valid entries; bins: the dustbin column of all rows, the
dustbin row of all columns and the corner) two bounds: err_abs <= min(K_ABS * noise_abs + 1e-6 * scale, TOL_CONF * max(1, scale)) and
err_rel <= K_REL * noise_rel + 1e-6 (over the entries >= 1e-12 of conf; over every dustbin entry), where noise is the distance of the
oracle's own float32 run to its float64 run on the same case.  The relative bound is what sees a row or column sum that lost or doubled
one term.  Rows and columns the prefilter drops are exactly zero and no other compared entry is; padding entries are finite and
non-negative; match ids and coarse keypoints are exactly those of the reference selection on ref64, mconf is held to the absolute bound.
Each run prints its own figures before it asserts, and appends them to the file LOFTR_EDGES_REPORT names, if set (how
profiles/sinkhorn_accuracy.txt was written)."""
import os

import numpy as np
import pytest

import _sinkhorn_cases as E

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


def _run(i):
    import torch
    from loftr_amd import ops
    c, m0, m1 = i["case"], i["m0"], i["m1"]
    r = ops.coarse_match(_t(i["f0"]), _t(i["f1"]), i["hw0"], i["hw1"], thr=0.0, border_rm=i["border_rm"], scale=8.0, match_type="sinkhorn",
                         bin_score=c.bin_score, skh_iters=c.iters, skh_prefilter=c.prefilter, want_assign=True,
                         mask0=None if m0 is None else _t(m0).flatten(-2), mask1=None if m1 is None else _t(m1).flatten(-2))
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None and hasattr(v, "cpu") else v) for k, v in r.items()}


def _check_region(name, path, got, ref64, kind, region, failures):
    """The absolute and the relative bound on the entries each uses."""
    got = got.astype(np.float64)
    err_abs, err_rel = E.abs_error(got, ref64, region), E.rel_error(got, ref64, region)
    tol_abs, tol_rel = E.abs_tolerance(kind, region["noise_abs"], region["scale"]), E.rel_tolerance(kind, region["noise_rel"])
    _report(f"{name:28s} {path:12s} abs err {err_abs:.3e} noise {region['noise_abs']:.3e} err/noise {_ratio(err_abs, region['noise_abs']):6.2f} "
            f"scale {region['scale']:.3e} | rel err {err_rel:.3e} noise {region['noise_rel']:.3e} err/noise {_ratio(err_rel, region['noise_rel']):6.2f}")
    if err_abs > tol_abs:
        failures.append((path, "abs", err_abs, tol_abs, region["noise_abs"]))
    if err_rel > tol_rel:
        failures.append((path, "rel", err_rel, tol_rel, region["noise_rel"]))


def _check_zeros(name, path, got, r, failures):
    """Rows and columns the prefilter drops are exactly zero; no entry of the relative check is."""
    dropped = r["rowkill"][:, :, None] | r["colkill"][:, None, :]
    if (got[dropped] != 0).any():
        failures.append((path, "dropped entries not zero", int((got[dropped] != 0).sum())))
    if (got[r["conf"]["relset"]] == 0).any():
        failures.append((path, "zero outside the dropped rows and columns", int((got[r["conf"]["relset"]] == 0).sum())))


def _check_matches(name, out, i, r, failures):
    """Ids and coarse keypoints exactly those of the reference selection, mconf inside the absolute bound, counts consistent with b_ids,
    no match in the padding."""
    c, sel, region = i["case"], r["sel"], r["conf"]
    b, ii, jj = out["b_ids"], out["i_ids"], out["j_ids"]
    counts = out["counts"]
    assert counts[0] == len(b) and np.array_equal(counts[1:], np.bincount(b, minlength=c.N)), (name, counts.tolist())
    if E.expects_no_match(c):
        assert len(b) == 0 and len(sel["b_ids"]) == 0, (name, len(b))
    order = np.lexsort((ii, b))
    got_ids = np.stack([b, ii, jj], 1)[order]
    want_ids = np.stack([sel["b_ids"], sel["i_ids"], sel["j_ids"]], 1)
    if got_ids.shape != want_ids.shape or not np.array_equal(got_ids, want_ids):
        diff = sorted(set(map(tuple, got_ids.tolist())) ^ set(map(tuple, want_ids.tolist())))
        failures.append(("ids", len(got_ids), len(want_ids), diff[:8]))
        return
    m0, m1 = E.flat_masks(i)
    assert m0[b, ii].all() and m1[b, jj].all(), (name, "a match in the padding")
    assert np.array_equal(out["mkpts0_c"][order], sel["mkpts0_c"]) and np.array_equal(out["mkpts1_c"][order], sel["mkpts1_c"]), name
    err = float(np.abs(out["mconf"][order].astype(np.float64) - r["ref64"][sel["b_ids"], sel["i_ids"], sel["j_ids"]]).max()) if len(b) else 0.0
    _report(f"{name:28s} {'mconf':12s} abs err {err:.3e} noise {region['noise_abs']:.3e} err/noise {_ratio(err, region['noise_abs']):6.2f} matches {len(b)}")
    if err > E.abs_tolerance("conf", region["noise_abs"], region["scale"]):
        failures.append(("mconf", err, E.abs_tolerance("conf", region["noise_abs"], region["scale"]), region["noise_abs"]))


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_sinkhorn_vs_float64(name):
    """conf_matrix, conf_matrix_with_bin (inner block, dustbin column, dustbin row, corner) and the selection against
    oracle.sinkhorn_conf / coarse_match_select in float64.  K_ABS / K_REL: see tests/_sinkhorn_cases.py."""
    i, r = E.inputs(name), E.reference(name)
    out = _run(i)
    conf, assign = out["conf_matrix"], out["conf_matrix_with_bin"]
    assert np.isfinite(conf).all() and np.isfinite(assign).all(), (name, "not finite", int((~np.isfinite(conf)).sum()), int((~np.isfinite(assign)).sum()))
    failures = []
    _check_region(name, "conf", conf, r["ref64"], "conf", r["conf"], failures)
    _check_region(name, "assign_inner", assign[:, :-1, :-1], r["ref64"], "conf", r["conf"], failures)
    _check_region(name, "bins", E.bins_of(assign), r["bins64"], "bins", r["bins"], failures)
    _check_zeros(name, "conf", conf, r, failures)
    _check_zeros(name, "assign_inner", assign[:, :-1, :-1], r, failures)
    if not r["valid"].all():
        pad = conf[~r["valid"]]
        _report(f"{name:28s} {'padding':12s} max {float(pad.max()):.3e} min {float(pad.min()):.3e} entries {pad.size}")
        assert (pad >= 0).all(), (name, "negative confidence in the padding", float(pad.min()))
    _check_matches(name, out, i, r, failures)
    assert not failures, (name, failures)
