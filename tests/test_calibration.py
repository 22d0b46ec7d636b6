"""View-graph calibration on the CPU: the defining host routine (loftr_calibrate_view_graph_host behind
calibrate_view_graph on CPU tensors / numpy arrays) against the independent numpy oracle of _calibration_oracle.py and against ground
truth, on the seeded scenes of _calibration_cases.py; the chain SfmResult.calibrate / reconstruct_uncalibrated on an atlas."""
import os

import numpy as np
import pytest
import torch

import _calibration_cases as CC
import _calibration_oracle as CO
import loftr_amd
from loftr_amd import _lib, build as build_mod, evaluation, ops_calib
from loftr_amd.calibration import ViewGraphCalibration, calibrate_view_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# MEASURED: the largest distance of the host routine to the oracle over the scenes below (profiles/calibration_accuracy.txt, written by
# tools/calibration_accuracy.py); the assertions allow ten times that.  The conjugate-gradient leg repeats the rule, so it differs by
# rounding only (the residual more than the scale: the oracle takes it from singular values); the dense leg solves every step exactly
# and both end on ftol, so it differs by what ftol leaves.
MEASURED_SCALE_PCG, MEASURED_RESID_PCG = 2.3e-16, 3.3e-13      # measured 2.22e-16 and 3.28e-13
MEASURED_SCALE_DENSE, MEASURED_RESID_DENSE = 1.4e-8, 1.8e-8    # measured 1.32e-8 and 1.80e-8
TOL = {"pcg": (10 * MEASURED_SCALE_PCG, 10 * MEASURED_RESID_PCG), "dense": (10 * MEASURED_SCALE_DENSE, 10 * MEASURED_RESID_DENSE)}
# Noise-free scenes without the prior: the ORACLE's largest relative focal error, measured 4.2e-8 (F goes through float32); ten times.
MEASURED_EXACT = 4.2e-8
# End to end: the margins over the yardstick run recorded in profiles/calibration_accuracy.txt
MARGIN_FOCAL, MARGIN_CENTRE = 2e-3, 2.5e-3
SCENES = (("small", dict(seed=1, n=5, k=2, noise=0.3, n_points=40)),) + CC.GENERAL + CC.PLANTED + CC.SHARED


@pytest.fixture(scope="module", autouse=True)
def built():
    build_mod.build(verbose=False)


@pytest.fixture(scope="module")
def solved():
    """name -> (scene, raw arrays, the host routine's result, the oracle's two legs): computed once, shared and left unchanged"""
    out = {}
    for name, kw in SCENES:
        sc = CC.ring(**kw)
        a = CC.raw_args(sc)
        G = len(a[6]) - 1
        out[name] = (sc, a, ops_calib.calibrate_view_graph_host(*a),
                     {s: CO.calibrate(*a[:6], G, solver=s) for s in ("pcg", "dense")})
    return out


@pytest.mark.parametrize("name", [n for n, _ in SCENES])
def test_host_routine_against_the_oracle(solved, name):
    sc, a, got, legs = solved[name]
    pcg, dense = legs["pcg"], legs["dense"]
    assert got["counts"].tolist() == pcg["counts"].tolist()                 # every count: trials, accepted, pcg iterations, ...
    for leg, want in legs.items():
        assert np.array_equal(got["edge_state"], want["edge_state"]) and np.array_equal(got["group_state"], want["group_state"]), leg
        for k in (4, 5, 6, 8):
            assert got["counts"][k] == want["counts"][k], (leg, k)
        d = [np.abs(got[k] - want[k]).max() for k in ("focal_scale", "edge_resid")]
        print(f"{name} {leg}: d_scale {d[0]:.3e} d_resid {d[1]:.3e}")
        assert d[0] <= TOL[leg][0] and d[1] <= TOL[leg][1], (leg, d)
        assert np.array_equal(want["focal"], a[4] * want["focal_scale"][a[5]])
    assert np.array_equal(got["focal"], a[4] * got["focal_scale"][a[5]])      # one multiplication
    assert np.abs(got["info"][:2] - pcg["info"][:2]).max() <= 1e-12 and got["info"][2] == pcg["info"][2]


def test_recorded_figures_are_the_ones_asserted():
    text = open(os.path.join(ROOT, "profiles", "calibration_accuracy.txt")).read()
    assert "d_scale_pcg 2.220e-16, d_resid_pcg 3.278e-13, d_scale_dense 1.323e-08, d_resid_dense 1.798e-08" in text
    assert "focal excess <= 2e-3, centre excess <= 2.5e-3" in text


@pytest.mark.parametrize("name", [n for n, _ in CC.GENERAL])
def test_general_scenes_reach_five_per_cent(solved, name):
    sc, a, got, legs = solved[name]
    start = np.abs(sc.f0 / sc.f_true - 1)
    assert start.max() > 0.4                                                  # the 1.2 W start is far off
    for res in (legs["dense"], got):                                          # the dense oracle alone stays inside the cap
        err = np.abs(res["focal"] / sc.f_true - 1).max()
        print(f"{name}: largest relative focal error {err:.4f} (start {start.max():.2f})")
        assert err <= 0.05
    assert got["counts"][7] == 0 and 4 <= got["counts"][0] <= 13 and (got["group_state"] == 2).all()


@pytest.mark.parametrize("seed", (30, 31, 32))
def test_noise_free_scenes_return_the_true_focals(seed):
    sc = CC.ring(seed, n=12, k=3, noise=0.0)
    a = CC.raw_args(sc)
    assert np.all(a[4] == 1200.0)
    got = ops_calib.calibrate_view_graph_host(*a, prior_weight=0.0)
    err = np.abs(got["focal"] / sc.f_true - 1).max()
    print(f"seed {seed}: {err:.3e}")
    assert err <= 10 * MEASURED_EXACT and got["edge_resid"].max() <= 1e-6 and (got["edge_state"] == 1).all()
    # with the default prior the result is the oracle's: the prior's pull towards the start is part of the rule
    got, want = ops_calib.calibrate_view_graph_host(*a), CO.calibrate(*a[:6], 12, solver="dense")
    assert np.abs(got["focal_scale"] - want["focal_scale"]).max() <= TOL["dense"][0]
    assert np.abs(got["focal"] / sc.f_true - 1).max() <= 0.005


@pytest.mark.parametrize("name", [n for n, _ in CC.PLANTED])
def test_planted_edges_are_outliers(solved, name):
    sc, a, got, legs = solved[name]
    assert sc.planted.sum() == round(0.25 * len(sc.planted))
    assert (got["edge_state"][sc.planted] == 2).all() and (got["edge_state"][~sc.planted] == 1).all()
    assert got["counts"][6] == sc.planted.sum()
    r = got["edge_resid"]
    print(f"{name}: good edges end at |rho| <= {r[~sc.planted].max():.4f}, planted at >= {r[sc.planted].min():.4f}")
    assert r[~sc.planted].max() <= 0.05 < r[sc.planted].min()
    assert np.abs(got["focal"] / sc.f_true - 1).max() <= 0.05


@pytest.mark.parametrize("name", [n for n, _ in CC.SHARED])
def test_shared_cameras(solved, name):
    sc, a, got, legs = solved[name]
    G = len(np.unique(sc.camera_ids))
    assert got["focal_scale"].shape == (G,) and got["counts"][5] == G
    assert np.abs(got["focal"] / sc.f_true - 1).max() <= 0.05
    cal = calibrate_view_graph(sc.edge_image, sc.edge_F, sc.edge_weight, sc.n, sc.pp, sc.f0, camera_ids=sc.camera_ids)
    assert isinstance(cal, ViewGraphCalibration) and loftr_amd.ViewGraphCalibration is ViewGraphCalibration
    assert np.array_equal(cal.focal.numpy(), got["focal"]) and np.array_equal(cal.group.numpy(), a[5])
    for cid in np.unique(sc.camera_ids):
        assert len(np.unique(cal.focal.numpy()[sc.camera_ids == cid])) == 1
    assert cal.focal_ok.all() and cal.edge_ok.all() and cal.stats["n_groups"] == G and cal.stats["status_name"] == "converged"
    K = cal.K.numpy()
    assert np.array_equal(K[:, 0, 0], got["focal"]) and np.array_equal(K[:, 1, 1], got["focal"]) and np.array_equal(K[:, :2, 2], sc.pp)
    assert np.all(K[:, 2, 2] == 1) and np.all(K[:, 1, 0] == 0) and np.all(K[:, 0, 1] == 0) and np.all(K[:, 2, :2] == 0)
    host = cal.to_host()
    assert set(host) == set(ViewGraphCalibration.FIELDS) | {"stats"}


@pytest.mark.parametrize("seed", CC.DEGENERATE_SEEDS)
def test_the_prior_holds_the_degenerate_ring(seed):
    """optical axes through one point: the focals are not determined by F; the prior keeps them at the start, which is 10 % off"""
    sc = CC.ring(seed, n=12, k=3, noise=0.5, degenerate=True, start=0.1)
    a = CC.raw_args(sc)
    start = np.abs(sc.f0 / sc.f_true - 1).max()
    with_prior = np.abs(ops_calib.calibrate_view_graph_host(*a)["focal"] / sc.f_true - 1).max()
    without = np.abs(ops_calib.calibrate_view_graph_host(*a, prior_weight=0.0)["focal"] / sc.f_true - 1).max()
    print(f"seed {seed}: start {start:.4f}, default prior {with_prior:.4f}, no prior {without:.4f}")
    assert with_prior <= start < without


def test_bound_rejections_are_counted(solved):
    sc, a, _, _ = solved["ring12"]
    got = ops_calib.calibrate_view_graph_host(*a, bound_lo=0.9, bound_hi=1.1)        # the truth needs scales of 0.5 to 0.9
    want = CO.calibrate(*a[:6], 12, solver="pcg", bound_lo=0.9, bound_hi=1.1)
    assert got["counts"].tolist() == want["counts"].tolist() and got["counts"][8] > 0
    assert (got["focal_scale"] > 0.9).all() and (got["focal_scale"] < 1.1).all()
    assert got["counts"][0] >= got["counts"][2] + got["counts"][8]         # a trial outside the bounds is never accepted
    assert np.abs(got["focal_scale"] - want["focal_scale"]).max() <= TOL["pcg"][0]


def test_held_groups_and_images_without_edges(solved):
    sc, a, base, _ = solved["hub"]
    # the hub group has 13 images, the three others one each: 6 valid edge ends apiece
    got = ops_calib.calibrate_view_graph_host(*a, min_edges=7)
    assert got["group_state"].tolist() == [2, 1, 1, 1] and got["counts"][5] == 1
    assert np.all(got["focal_scale"][1:] == 1.0) and np.array_equal(got["focal"][13:], sc.f0[13:]) and got["focal_scale"][0] != 1.0
    got = ops_calib.calibrate_view_graph_host(*a, min_edges=1000)
    assert (got["group_state"] == 1).all() and got["counts"][7] == 3 and got["counts"][0] == 0 and np.array_equal(got["focal"], sc.f0)
    assert got["counts"][4] == len(a[0]) and (got["edge_state"] > 0).all() and got["info"][0] == got["info"][1] > 0
    # an image without edges: one more image, its own group
    sc2, a2, base2, _ = solved["ring12"]
    b = [a2[0], a2[1], a2[2], np.r_[a2[3], [[500.0, 375.0]]], np.r_[a2[4], 900.0], np.r_[a2[5], 12].astype(np.int32), np.r_[a2[6], a2[6][-1]], a2[7]]
    got = ops_calib.calibrate_view_graph_host(*b)
    assert got["group_state"].tolist() == [2] * 12 + [0] and got["focal"][12] == 900.0 and got["focal_scale"][12] == 1.0
    assert np.array_equal(got["focal"][:12], base2["focal"]) and got["counts"].tolist() == base2["counts"].tolist()


def test_max_iters_zero_and_no_edges(solved):
    sc, a, _, legs = solved["ring12"]
    got = ops_calib.calibrate_view_graph_host(*a, max_iters=0)
    want = CO.calibrate(*a[:6], 12, solver="pcg", max_iters=0)
    assert got["counts"].tolist() == want["counts"].tolist() and got["counts"][0] == 0 and got["counts"][7] == 1
    assert np.all(got["focal_scale"] == 1.0) and np.array_equal(got["focal"], sc.f0)
    assert np.abs(got["edge_resid"] - want["edge_resid"]).max() <= TOL["pcg"][1]              # the residuals of the start values
    assert got["counts"][6] == (got["edge_resid"] > 0.05).sum() > len(a[0]) // 2 and got["info"][0] == got["info"][1]
    none = [np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)), np.zeros(0, np.int32), a[3], a[4], a[5], np.zeros(13, np.int64), np.zeros(0, np.int32)]
    got = ops_calib.calibrate_view_graph_host(*none)
    assert got["counts"].tolist() == [0] * 7 + [3] + [0] * 8 and np.array_equal(got["focal"], sc.f0) and not got["group_state"].any()


def test_invalid_edges_duplicates_and_two_components():
    sc = CC.ring(2, n=12, k=3, noise=0.5)
    base = calibrate_view_graph(sc.edge_image, sc.edge_F, sc.edge_weight, sc.n, sc.pp, sc.f0)
    # invalid edges: zero weight, negative weight, NaN, infinity, a zero matrix -> state 0, and the result is that of the list without them
    ei, F, w = (np.concatenate([x, x[:5]]) for x in (sc.edge_image, sc.edge_F, sc.edge_weight))
    E = len(sc.edge_F)
    w[E], w[E + 1] = 0, -3
    F[E + 2, 1, 1], F[E + 3, 0, 2], F[E + 4] = np.nan, np.inf, 0.0
    cal = calibrate_view_graph(ei, F, w, sc.n, sc.pp, sc.f0)
    assert cal.edge_state[E:].tolist() == [0] * 5 and not cal.edge_resid[E:].any() and not cal.edge_ok[E:].any()
    assert cal.stats["n_valid_edges"] == E and cal.stats["n_trials"] == base.stats["n_trials"]
    assert np.abs(cal.focal_scale.numpy() - base.focal_scale.numpy()).max() <= TOL["dense"][0]
    # duplicates count twice: the same minimum when every edge is doubled (the prior's relative weight halves)
    cal = calibrate_view_graph(np.r_[sc.edge_image, sc.edge_image], np.r_[sc.edge_F, sc.edge_F], np.r_[sc.edge_weight, sc.edge_weight], sc.n, sc.pp,
                               sc.f0, prior_weight=2e-3)
    assert cal.stats["n_valid_edges"] == 2 * E and np.abs(cal.focal_scale.numpy() - base.focal_scale.numpy()).max() <= 1e-6
    assert np.array_equal(cal.edge_resid[:E].numpy(), cal.edge_resid[E:].numpy())
    # two components: the rings of images 0..11 and 12..23 share no edge
    s2 = CC.ring(3, n=12, k=3, noise=0.5)
    cal = calibrate_view_graph(np.r_[sc.edge_image, s2.edge_image + 12], np.r_[sc.edge_F, s2.edge_F], np.r_[sc.edge_weight, s2.edge_weight], 24,
                               np.r_[sc.pp, s2.pp], np.r_[sc.f0, s2.f0])
    assert cal.focal_ok.all() and np.abs(cal.focal.numpy() / np.r_[sc.f_true, s2.f_true] - 1).max() <= 0.05


def test_renumbering_the_edges(solved):
    sc, a, base, _ = solved["ring20_noise1"]
    perm = np.random.default_rng(0).permutation(len(sc.edge_F))
    cal = calibrate_view_graph(sc.edge_image[perm], sc.edge_F[perm], sc.edge_weight[perm], sc.n, sc.pp, sc.f0)
    # another order of the sums: the same trials, and a result that differs by what ftol leaves at the most
    assert cal.stats["n_trials"] == base["counts"][0] and np.array_equal(cal.edge_state.numpy(), base["edge_state"][perm])
    assert np.abs(cal.focal_scale.numpy() - base["focal_scale"]).max() <= TOL["dense"][0]
    assert np.abs(cal.edge_resid.numpy() - base["edge_resid"][perm]).max() <= TOL["dense"][1]
    # an edge stored the other way round is the same constraint: x_a^T F^T x_b = 0
    flip = np.arange(len(sc.edge_F)) % 2 == 0
    ei, F = sc.edge_image.copy(), sc.edge_F.copy()
    ei[flip], F[flip] = ei[flip][:, ::-1], F[flip].transpose(0, 2, 1)
    cal = calibrate_view_graph(ei, F, sc.edge_weight, sc.n, sc.pp, sc.f0)
    assert np.abs(cal.focal_scale.numpy() - base["focal_scale"]).max() <= TOL["dense"][0]


def test_error_bits_leave_every_other_output_zero(solved):
    sc, a, _, _ = solved["small"]

    def bits(i, edit, **kw):
        b = [x.copy() for x in a]
        edit(b[i])
        out = ops_calib.calibrate_view_graph_host(*b, **kw)
        for k, v in out.items():
            if k != "counts":
                assert not v.any(), k
        assert out["counts"][0] == 0 and not out["counts"][2:].any()
        return int(out["counts"][1])

    def put(idx, v):
        def edit(x):
            x[idx] = v
        return edit

    assert bits(0, put((3, 1), 5)) & 1 and bits(0, put((3, 0), -1)) & 1
    assert bits(0, put((2, slice(None)), 2)) == 1 | 4                      # a == b: the edge's second end sits in the wrong list too
    assert bits(5, put(2, 5)) & 2 and bits(5, put(0, -1)) & 2
    assert bits(7, lambda x: x.__setitem__(slice(0, 2), x[1::-1].copy())) == 4                 # two slots of one list swapped
    assert bits(7, put(3, 2 * len(a[0]))) == 4 and bits(7, put(3, -1)) == 4
    assert bits(6, put(2, a[6][2] + 1)) == 4 and bits(6, put(0, 1)) == 4 and bits(6, put(-1, a[6][-1] - 1)) == 4
    assert bits(4, put(1, 0.0)) == 8 and bits(4, put(1, -700.0)) == 8 and bits(4, put(4, np.nan)) == 8 and bits(4, put(0, np.inf)) == 8
    assert bits(3, put((2, 1), np.nan)) == 8 and bits(3, put((0, 0), -np.inf)) == 8
    assert bits(4, put(1, -1.0), max_iters=0) == 8


def test_every_value_error():
    sc = CC.small()
    args = lambda **over: {**dict(edge_image=sc.edge_image, edge_F=sc.edge_F, edge_weight=sc.edge_weight, n_images=sc.n,
                                  principal_point=sc.pp, f0=sc.f0), **over}
    assert calibrate_view_graph(**args()).stats["status_name"] == "converged"
    assert calibrate_view_graph(**args(principal_point=(500.0, 375.0), f0=1200.0)).stats["n_trials"] > 0       # one pair, one number
    bad = sc.edge_image.copy()
    bad[1, 0] = sc.n
    same = sc.edge_image.copy()
    same[1] = 3
    neg = sc.f0.copy()
    neg[2] = -1.0
    nanpp = sc.pp.copy()
    nanpp[0, 0] = np.nan
    for over, match in ((dict(edge_image=bad), "edge image outside"), (dict(edge_image=same), "edge image outside|to itself"),
                        (dict(f0=neg), "f0 must be finite and positive"), (dict(principal_point=nanpp), "principal_point finite"),
                        (dict(f0=0.0), "f0 must be finite"), (dict(n_images=0), "n_images must be an integer >= 1"),
                        (dict(n_images=2.0), "n_images must be"), (dict(edge_image=sc.edge_image.astype(np.float32)), "must hold integers"),
                        (dict(edge_weight=sc.edge_weight.astype(np.float64)), "must hold integers"),
                        (dict(edge_F=sc.edge_F[:-1]), "expected edge_image"), (dict(edge_weight=sc.edge_weight[:-1]), "expected edge_image"),
                        (dict(f0=sc.f0[:-1]), "expected principal_point"), (dict(principal_point=sc.pp[:-1]), "expected principal_point"),
                        (dict(camera_ids=np.zeros(sc.n - 1, np.int64)), "expected camera_ids"), (dict(camera_ids=np.array([0, 0, -1, 2, 2])), "non-negative"),
                        (dict(camera_ids=np.zeros(sc.n)), "must hold integers"),
                        (dict(loss=0.0), "loss must be > 0"), (dict(loss=float("nan")), "loss must be a finite number"), (dict(max_resid=-1.0), "max_resid"),
                        (dict(prior_weight=-1e-3), "prior_weight"), (dict(weight_cap=0), "weight_cap must be an integer >= 1"),
                        (dict(weight_cap=10.0), "weight_cap must be an integer"), (dict(bound_lo=0.0), "bounds"), (dict(bound_lo=1.0), "bounds"),
                        (dict(bound_hi=1.0), "bounds"), (dict(bound_hi=float("inf")), "bound_hi must be a finite number"),
                        (dict(min_edges=-1), "min_edges"), (dict(max_iters=-1), "max_iters"), (dict(max_iters=True), "max_iters"),
                        (dict(max_iters=(1 << 16) + 1), "at most"), (dict(pcg_iters=1.5), "pcg_iters"), (dict(pcg_tol=1.0), "pcg_tol"),
                        (dict(ftol=-1.0), "ftol")):
        with pytest.raises(ValueError, match=match):
            calibrate_view_graph(**args(**over))
    with pytest.raises(TypeError, match="unknown parameter"):
        calibrate_view_graph(**args(huber=0.1))
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops_calib.calibrate_view_graph_host(*[torch.from_numpy(x) for x in CC.raw_args(sc)])
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):           # the kernels take GPU tensors only: no fallback
        ops_calib.calibrate_view_graph(*[torch.from_numpy(x) for x in CC.raw_args(sc)])
    ids = np.array([9, 4, 9, 4, 1 << 40])
    cal = calibrate_view_graph(**args(camera_ids=ids))                    # any non-negative integers, compacted by first appearance
    assert cal.group.tolist() == [0, 1, 0, 1, 2] and cal.focal_scale.shape == (3,)
    cal_t = calibrate_view_graph(**args(camera_ids=torch.from_numpy(ids), edge_F=torch.from_numpy(sc.edge_F)))
    assert torch.equal(cal.focal, cal_t.focal)


def test_focal_errors():
    K = np.tile(np.diag([800.0, 820.0, 1.0]), (3, 1, 1))
    e = evaluation.focal_errors(np.array([810.0, 405.0, 1620.0]), K)
    assert np.allclose(e, [0.0, 0.5, 1.0]) and np.allclose(evaluation.focal_errors(torch.from_numpy(K), K), 0.0)
    with pytest.raises(ValueError, match="expected focal"):
        evaluation.focal_errors(np.ones(2), K)


# ---- end to end: an atlas without intrinsics ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def atlas():
    return CC.atlas_scene("cpu")


def test_pairwise_fundamentals_and_calibrate(atlas):
    sfm, sc = atlas
    assert sc.n == 8 and sfm.track_len.numel() >= 150 and sfm.cell_px == 2.0
    F, ninl = sfm.pairwise_fundamentals()
    R = sfm.row_images.shape[0]
    assert tuple(F.shape) == (R, 3, 3) and F.dtype == torch.float32 and ninl.dtype == torch.int64 and (ninl > 100).all()
    assert torch.allclose(torch.linalg.matrix_norm(F.double()), torch.ones(R, dtype=torch.float64), atol=1e-6)
    cal = sfm.calibrate()
    assert cal.stats["n_edges"] == R and cal.edge_ok.all() and cal.focal_ok.all() and cal.stats["status_name"] == "converged"
    assert np.array_equal(cal.K[:, :2, 2].numpy(), np.tile([CC.W / 2, CC.H / 2], (8, 1)))
    start = np.median(evaluation.focal_errors(np.full(8, 1.2 * CC.W), sc.K_true))
    after = np.median(evaluation.focal_errors(cal.focal, sc.K_true))
    print(f"median focal error: start {start:.4f}, after calibration alone {after:.4f}")
    assert after < start
    # the explicit form, and shared cameras
    same = sfm.calibrate(f0=1.2 * CC.W, principal_point=(CC.W / 2, CC.H / 2))
    assert torch.equal(same.focal, cal.focal)
    one = sfm.calibrate(camera_ids=np.zeros(8, np.int64))
    assert one.focal_scale.shape == (1,) and len(torch.unique(one.focal)) == 1
    # a row without a model is an invalid edge
    fields = {k: getattr(sfm, k) for k in sfm.FIELDS}
    ro = sfm.row_offsets.clone()
    cut = int(ro[1] - ro[0]) - 3
    keep = torch.ones(sfm.matches.shape[0], dtype=torch.bool)
    keep[3:int(ro[1])] = False
    ro[1:] -= cut
    fields.update(matches=sfm.matches[keep], match_conf=sfm.match_conf[keep], row_offsets=ro)
    few = loftr_amd.SfmResult(dict(sfm.stats), **fields)
    few.image_hw, few.cell_px = sfm.image_hw, sfm.cell_px
    F2, n2 = few.pairwise_fundamentals()
    assert n2[0] == -1 and not F2[0].any() and torch.equal(F2[1:], F[1:])
    c2 = few.calibrate()
    assert c2.edge_state[0] == 0 and c2.stats["n_valid_edges"] == R - 1
    # refused: a refined view; no image size
    few.is_refined = True
    with pytest.raises(ValueError, match="refined view"):
        few.calibrate()
    few.is_refined, few.image_hw = False, None
    with pytest.raises(ValueError, match="image_hw"):
        few.calibrate()
    assert few.calibrate(f0=1200.0, principal_point=(500.0, 375.0)).stats["n_valid_edges"] == R - 1


def test_reconstruct_uncalibrated_against_the_yardstick(atlas):
    """Figures (profiles/calibration_accuracy.txt): uncalibrated focal 6.16e-3, centre 2.45e-2; yardstick focal 5.98e-3, centre 2.46e-2."""
    sfm, sc = atlas
    rec = sfm.reconstruct_uncalibrated()
    ref = sfm.reconstruct(sc.K_true, ba={"refine_focal": True})             # the yardstick
    assert bool(rec.posed.all()) and bool(ref.posed.all())
    assert isinstance(rec.calibration, ViewGraphCalibration) and rec.stats["calibration"] is rec.calibration.stats and ref.calibration is None
    (fu, cu), (fy, cy) = CC.reconstruction_errors(rec, sc), CC.reconstruction_errors(ref, sc)
    print(f"uncalibrated: focal {fu:.3e}, centre {cu:.3e}; yardstick: focal {fy:.3e}, centre {cy:.3e}")
    assert fu <= fy + MARGIN_FOCAL and cu <= cy + MARGIN_CENTRE
    assert not torch.equal(rec.K, rec.calibration.K)                        # the bundle adjustment refined what the calibration left
    glob = sfm.reconstruct_uncalibrated(global_=True, camera_ids=np.arange(8))
    assert bool(glob.posed.all()) and glob.positions is not None and glob.calibration is not None
    fg, cg = CC.reconstruction_errors(glob, sc)
    print(f"global: focal {fg:.3e}, centre {cg:.3e}")
    assert fg <= fy + MARGIN_FOCAL and cg <= cy + MARGIN_CENTRE


def test_the_analytic_jacobian_against_central_differences():
    """The derivative of rule 4 as the oracle writes it (the host routine agrees with that oracle to rounding) against central
    differences of rho itself.  Step 1e-5 on scales near 1: the truncation error is about h^2 |rho'''| / 6 = 2e-11 |rho'''| and the
    rounding error about eps |rho| / h = 2e-11, and the third derivatives of rho by a scale are O(10) at the most (rho is a ratio of
    polynomials of degree 6 in the scales with |rho| <= 1), so 1e-8 leaves two orders of margin over both."""
    sc = CC.ring(2, n=12, k=3, noise=0.5)
    a = CC.raw_args(sc)
    ei = a[0].astype(np.int64)
    Fp = np.stack([CO.centred(a[1][e], a[3][ei[e, 0]], a[3][ei[e, 1]]) for e in range(len(ei))])
    rng = np.random.default_rng(0)
    ma, mb = rng.uniform(0.5, 1.5, len(ei)), rng.uniform(0.5, 1.5, len(ei))
    fa, fb = a[4][ei[:, 0]], a[4][ei[:, 1]]
    rho = lambda x, y: CO.rho_and_jacobian(CO.essential(Fp, fa * x, fb * y), x, y)[0]
    _, ja, jb = CO.rho_and_jacobian(CO.essential(Fp, fa * ma, fb * mb), ma, mb)
    h = 1e-5
    da = np.abs((rho(ma + h, mb) - rho(ma - h, mb)) / (2 * h) - ja).max()
    db = np.abs((rho(ma, mb + h) - rho(ma, mb - h)) / (2 * h) - jb).max()
    print(f"central differences: side a {da:.2e}, side b {db:.2e}; largest |j| {max(np.abs(ja).max(), np.abs(jb).max()):.2f}")
    assert da <= 1e-8 and db <= 1e-8
    s = np.linalg.svd(CO.essential(Fp, fa * ma, fb * mb), compute_uv=False)       # |rho| is the singular-value form
    assert np.abs(np.sqrt((rho(ma, mb) ** 2).sum(1)) - (s[:, 0] ** 2 - s[:, 1] ** 2) / (s[:, 0] ** 2 + s[:, 1] ** 2)).max() <= 1e-12
