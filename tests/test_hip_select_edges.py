"""Coarse selection (merge_colmax_kernel, valid_hw_kernel, select_kernel, scan_blocks_kernel, scatter_kernel) against the reference
selection, EXACTLY, behind every producer of its row / column partials: threshold equality, borders wider than the interior, the
padded border's negative-slice wrap, tied row maxima across panels and sweep chunks, the second round of the block scan, many tiny
pairs per wave, per-pair x / y scales, empty outputs.  Cases, paths, reference and the conditions the inputs meet:
tests/_select_cases.py.  The reference is `oracle.loftr_oracle.coarse_match_select` on the conf_matrix the kernel itself returned, so
nothing here has a tolerance: ids in the reference's order, mconf bitwise conf[b, i, j], coarse keypoints bitwise, counts consistent.
Each run prints its figures before it asserts and appends them to the file LOFTR_EDGES_REPORT names, if set (how
profiles/select_fine_match_accuracy.txt was written)."""
import os

import numpy as np
import pytest

import _select_cases as E

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


def _run(i, thr, want_conf=None):
    import torch
    from loftr_amd import ops
    c, p = i["config"], i["path"]
    kw = dict(match_type="dual_softmax", temperature=E.TEMPERATURE, want_conf=p.want_conf if want_conf is None else want_conf) \
        if p.kind == "ds" else dict(match_type="sinkhorn", bin_score=E.BIN_SCORE, skh_iters=E.SKH_ITERS, skh_prefilter=p.prefilter)
    f0, f1 = _t(i["f0"]), _t(i["f1"])
    r = ops.coarse_match(f0, f1, c.hw0, c.hw1, thr=float(thr), border_rm=c.border, scale=E.SCALE,
                         mask0=None if i["m0"] is None else _t(i["m0"]).flatten(-2), mask1=None if i["m1"] is None else _t(i["m1"]).flatten(-2),
                         scale0=_t(i["scale0"]), scale1=_t(i["scale1"]), **kw)
    torch.cuda.synchronize()
    assert np.array_equal(f0.cpu().numpy(), i["f0"]) and np.array_equal(f1.cpu().numpy(), i["f1"]), "a descriptor tensor was written to"
    return {k: (v.cpu().numpy() if v is not None and hasattr(v, "cpu") else v) for k, v in r.items()}


def _ids(d):
    return set(zip(np.asarray(d["b_ids"]).tolist(), np.asarray(d["i_ids"]).tolist(), np.asarray(d["j_ids"]).tolist()))


def _exact(name, path, i, thr, failures, tag=""):
    """One materialised run at `thr` against the reference selection on its own conf_matrix.  Returns (out, want)."""
    out = _run(i, thr)
    conf = out["conf_matrix"]
    assert conf.dtype == np.float32 and conf.shape == (i["config"].N, i["f0"].shape[1], i["f1"].shape[1])
    want = E.expected(conf, i, thr)
    bad = E.compare(out, want, conf, i["config"].N)
    _report(f"select {name:20s} {path:8s} {tag:10s} thr {float(thr):.9g} M {len(out['b_ids'])} reference M {len(want['b_ids'])} "
            f"per pair {out['counts'][1:9].tolist()}{' ...' if i['config'].N > 8 else ''} {'exact' if not bad else 'DIFFERS'}")
    failures += [(tag, b) for b in bad]
    return out, want


def _threshold(name, path, i, failures):
    out0, _ = _exact(name, path, i, 0.0, failures, "thr0")
    assert len(out0["mconf"]) >= 8, (name, path, "too few matches to take a median from")
    thr = E.median_threshold(out0["mconf"])
    below = np.nextafter(thr, np.float32(0))
    n_at, n_above = int((out0["mconf"] == thr).sum()), int((out0["mconf"] > thr).sum())
    assert n_at >= 1                                                                   # at least one match sits exactly at thr
    at, _ = _exact(name, path, i, thr, failures, "at_median")
    lo, _ = _exact(name, path, i, below, failures, "nextafter")
    _report(f"select {name:20s} {path:8s} strict >: {n_at} at thr, {n_above} above; M(thr) {len(at['b_ids'])} M(nextafter) {len(lo['b_ids'])}")
    if len(at["b_ids"]) != n_above or (at["mconf"] <= thr).any():
        failures.append(("at_median", "a match at the threshold survived or one above it vanished", len(at["b_ids"]), n_above))
    if len(lo["b_ids"]) != n_above + n_at:
        failures.append(("nextafter", "the matches at the threshold did not come back", len(lo["b_ids"]), n_above + n_at))


def _ties(name, path, i, failures):
    p = i["path"]
    full = _run(i, 0.0, want_conf=True)
    conf = full["conf_matrix"]
    want = E.expected(conf, i, 0.0)
    rep = E.tie_report(conf, want)
    _report(f"select {name:20s} {path:8s} M {len(full['b_ids'])} exact ties / later-tie rows: "
            + ", ".join(f"{k} {'yes' if ex else 'NO'} / {later}" for k, (ex, later) in rep.items()))
    for placement, (exact, later) in rep.items():
        if placement in E.TIE_OPTIONAL and not exact:
            # single duplicated columns in different panels: pass A's shared-reference variant gives a column (reference, sum) relative
            # to its own 32 x 32 tile's maximum, and the exact variant may have redone one of two chunks' units -- equal columns, statistics
            # that differ in the last bit.  No exact tie in the returned matrix, so nothing to assert; the selection stays exact.
            _report(f"select {name:20s} {path:8s} {placement}: the duplicated columns are not bitwise equal in the returned matrix "
                    f"(column statistics depend on the tile / chunk a column sits in); placement not required")
            continue
        assert exact, (name, path, placement, "the duplicated columns are not bitwise equal in the returned conf_matrix")
        assert later >= (1 if placement in E.TIE_OPTIONAL else 2), (name, path, placement, later, "too few rows on which the reference picks the later column")
    if p.want_conf:
        failures += E.compare(full, want, conf, i["config"].N)
        return
    # conf elided: the materialised run's selection without the rows whose first tied column fails a test; same mconf bits
    failures += [("materialised", b) for b in E.compare(full, want, conf, i["config"].N)]
    lean = _run(i, 0.0)
    assert lean["conf_matrix"] is None
    want_lean = E.expected_elided(conf, i, 0.0)
    failures += [("elided", b) for b in E.compare(lean, want_lean, conf, i["config"].N)]
    absent = _ids(full) - _ids(lean)
    later_rows = {(b, r, j) for b, r, j in _ids(want) if (conf[b, r, :j] == conf[b, r, j]).any()}
    _report(f"select {name:20s} {path:8s} elided M {len(lean['b_ids'])}, absent {len(absent)} = later-tie rows {len(later_rows)}")
    if absent != later_rows or not _ids(lean) <= _ids(full):
        failures.append(("elided", "absent rows are not exactly the later-tie rows", sorted(absent ^ later_rows)[:8]))


@pytest.mark.parametrize("name,path", E.RUNS)
def test_selection_is_exactly_the_reference(name, path):
    i = E.inputs(name, path)
    c, p = i["config"], i["path"]
    failures = []
    if c.thr == "median":
        _threshold(name, path, i, failures)
    elif c.plant == "ties":
        _ties(name, path, i, failures)
    elif not p.want_conf:
        full = _run(i, c.thr, want_conf=True)
        lean = _run(i, c.thr)
        assert lean["conf_matrix"] is None
        want = E.expected_elided(full["conf_matrix"], i, c.thr)
        _report(f"select {name:20s} {path:8s} elided M {len(lean['b_ids'])} reference M {len(want['b_ids'])}")
        failures += E.compare(lean, want, full["conf_matrix"], c.N)
    else:
        out, want = _exact(name, path, i, c.thr, failures)
        if name.startswith("empty") or name == "borders_no_interior":
            assert len(out["b_ids"]) == 0 and not out["counts"].any() and out["mkpts0_c"].shape == (0, 2) and out["mconf"].shape == (0,)
        if name == "scan":
            flat = out["b_ids"] * (105 * 105) + out["i_ids"]
            assert len(flat) >= 200 and (flat >= 262144).sum() >= 3 and ((out["b_ids"] == 23) & (flat < 262144)).any()
    assert not failures, (name, path, failures)
