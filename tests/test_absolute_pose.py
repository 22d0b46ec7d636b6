"""Absolute pose from 2D-3D matches, host side (csrc/absolute_pose.hip: loftr_p3p, loftr_estimate_absolute_pose;
evaluation.estimate_absolute_pose_native) against the float64 numpy oracle of tests/_absolute_pose_oracle.py, and the oracle's lifting
arithmetic against the reference's own warp_kpts (tests/golden/lift_warp.npz).  CPU only; parity against OpenCV's solvePnPRansac stays
unpinned (OpenCV is not available to this project)."""
import ctypes as C
import os

import numpy as np
import pytest

from loftr_amd import _lib, build as build_mod, evaluation as EV
import _absolute_pose_oracle as O

K = O.K_DEFAULT
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lift_warp.npz")


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def _p3p(lib, X, f):
    X, f = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(f, np.float64)
    R, t, n = np.zeros((4, 9)), np.zeros((4, 3)), C.c_int(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.loftr_p3p(ptr(X), ptr(f), ptr(R), ptr(t), C.byref(n)) == 0
    return R[:n.value].reshape(-1, 3, 3), t[:n.value]


def _bearings(px):
    f = np.c_[(px - K[:2, 2]) / np.array([K[0, 0], K[1, 1]]), np.ones(len(px))]
    return f / np.linalg.norm(f, axis=1, keepdims=True)


def _exact_problem(rng):
    """Three float64 world points (not rounded to float32) whose image triangle has an area of at least 2 500 px^2."""
    while True:
        sc = O.make_scene(rng, 3)
        px = np.c_[rng.uniform(20, 620, 3), rng.uniform(20, 460, 3)]
        if abs((px[1, 0] - px[0, 0]) * (px[2, 1] - px[0, 1]) - (px[1, 1] - px[0, 1]) * (px[2, 0] - px[0, 0])) / 2 < 2500:
            continue
        Xc = np.c_[(px - K[:2, 2]) / 525.0, np.ones(3)] * rng.uniform(2, 8, 3)[:, None]
        X = (Xc - sc["t"]) @ sc["R"]
        return X, O.project(K, sc["R"], sc["t"], X)[0], sc["R"], sc["t"]


def test_p3p_recovers_the_pose_on_exact_problems(lib):
    """40 exact problems: the true (R, t) is among the solutions to 1e-6 (the bar of test_pose.py / test_geometry.py for their minimal
    solvers), and every returned solution reprojects its three points to 1e-6 px with positive depth.  Measured over 2 000 such
    problems: worst pose error 1.6e-11, worst reprojection 3.6e-11 px."""
    rng = np.random.default_rng(40)
    for _ in range(40):
        X, px, R, t = _exact_problem(rng)
        Rs, ts = _p3p(lib, X, _bearings(px))
        assert 1 <= len(Rs) <= 4
        err = min(max(np.abs(Ri - R).max(), np.abs(ti - t).max()) for Ri, ti in zip(Rs, ts))
        assert err <= 1e-6, err
        for Ri, ti in zip(Rs, ts):
            assert np.abs(Ri @ Ri.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(Ri) > 0
            p, z = O.project(K, Ri, ti, X)
            assert (z > 0).all() and np.abs(p - px).max() <= 1e-6, (np.abs(p - px).max(), z)


def test_p3p_degenerate_samples_give_no_solution(lib):
    rng = np.random.default_rng(41)
    X, px, R, t = _exact_problem(rng)
    f = _bearings(px)
    line = np.stack([X[0], X[0] + 0.4 * (X[1] - X[0]), X[1]])                        # collinear world points
    assert len(_p3p(lib, line, f)[0]) == 0
    assert len(_p3p(lib, np.stack([X[0], X[0], X[1]]), f)[0]) == 0                    # two coincident world points
    assert len(_p3p(lib, X, np.stack([f[0], f[0], f[2]]))[0]) == 0                    # coincident bearings
    assert len(_p3p(lib, X, np.stack([f[0], f[1], f[1]]))[0]) == 0
    assert len(_p3p(lib, 1e6 * line, f)[0]) == 0 and len(_p3p(lib, 1e6 * X, f)[0]) >= 1   # the rule is relative
    assert lib.loftr_p3p(None, None, None, None, None) == -1


@pytest.mark.parametrize("seed", [0, 11])
def test_noise_free_scene_with_outliers_gives_exactly_the_true_inliers(seed):
    sc = O.make_scene(np.random.default_rng(50), 400, 0.0, 0.4)
    R, t, mask = EV.estimate_absolute_pose_native(sc["X"], sc["kpts"], sc["K"], 3.0, 0.999, seed)
    assert np.array_equal(mask, ~sc["is_outlier"])
    assert O.rotation_error_deg(R, sc["R"]) <= 1e-3 and np.abs(t - sc["t"]).max() <= 1e-4


def _rms_to_clean(sc, R, t):
    inl = ~sc["is_outlier"]
    return float(np.sqrt(np.mean(np.sum((O.project(K, R, t, sc["X"][inl])[0] - sc["clean"][inl]) ** 2, axis=1))))


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("outliers", [0.0, 0.4])
@pytest.mark.parametrize("n", [300, 2000])
def test_noisy_scenes_are_fitted_as_well_as_the_oracle_fits_the_true_inliers(n, outliers, planar):
    """0.5 px noise, thresh_px = 3.0 (6 sigma).  Metric: the RMS distance, over the true inliers, between the estimate's projections
    and the noise-free true projections; bar: at most 2 x the same metric of the oracle's Levenberg-Marquardt fit on the true inliers.
    Measured ratios (tools/micro/absolute_pose_accuracy.py -> profiles/absolute_pose_accuracy.txt, 200 scenes): 0.9997-1.0003 -- the
    final inlier set is the true one, and five Gauss-Newton steps reach the least-squares optimum the oracle finds.  The threshold stays
    at 6 sigma: at 2.0 px the adoption rule can reject the final fit (ratios up to 2.35 measured there)."""
    rng = np.random.default_rng(60 + n + int(10 * outliers) + planar)
    for seed in (0, 1, 2):
        sc = O.make_scene(rng, n, 0.5, outliers, planar)
        R, t, mask = EV.estimate_absolute_pose_native(sc["X"], sc["kpts"], sc["K"], 3.0, 0.999, seed)
        inl = ~sc["is_outlier"]
        Ro, to = O.fit_pose(K, sc["X"][inl], sc["kpts"][inl], sc["R"], sc["t"])
        ratio = _rms_to_clean(sc, R, t) / _rms_to_clean(sc, Ro, to)
        print(f"n {n} outliers {outliers} planar {planar} seed {seed}: ratio {ratio:.4f}, {mask.sum()} inliers of {inl.sum()} true")
        assert ratio <= 2.0, ratio
        assert not mask[sc["is_outlier"]].any()


def test_too_few_matches_and_the_minimal_case():
    sc = O.make_scene(np.random.default_rng(70), 3)
    for m in (0, 2):
        assert EV.estimate_absolute_pose_native(sc["X"][:m], sc["kpts"][:m], sc["K"]) is None
    R, t, mask = EV.estimate_absolute_pose_native(sc["X"], sc["kpts"], sc["K"])
    assert mask.tolist() == [True, True, True]
    col = O.make_collinear_scene()
    assert EV.estimate_absolute_pose_native(col["X"], col["kpts"], col["K"]) is None   # every sample is degenerate


def test_near_planar_scene_recovers_the_true_pose():
    """The case the five-point estimator cannot do (a plane is degenerate for the essential matrix)."""
    sc = O.make_scene(np.random.default_rng(80), 800, 0.5, 0.3, planar=True)
    R, t, mask = EV.estimate_absolute_pose_native(sc["X"], sc["kpts"], sc["K"], 3.0, 0.999, 0)
    inl = ~sc["is_outlier"]
    Ro, to = O.fit_pose(K, sc["X"][inl], sc["kpts"][inl], sc["R"], sc["t"])
    assert O.rotation_error_deg(R, sc["R"]) <= 2 * O.rotation_error_deg(Ro, sc["R"]) + 1e-3
    assert np.linalg.norm(R.T @ t - sc["R"].T @ sc["t"]) <= 2 * np.linalg.norm(Ro.T @ to - sc["R"].T @ sc["t"]) + 1e-3


def test_error_and_recall_helpers():
    R, t = O.rot([0, 0, 1.0], np.radians(3.0)), np.array([0.1, 0.0, 0.0])
    T = np.eye(4)
    r_err, c_err = EV.absolute_pose_error(T, R, t)
    assert abs(r_err - 3.0) <= 1e-9 and abs(c_err - 0.1) <= 1e-12
    assert EV.absolute_pose_error(T[:3], np.eye(3), np.zeros(3)) == (0.0, 0.0)
    rec = EV.localization_recall([0.1, 0.4, 3.0, np.inf], [1.0, 4.0, 9.0, np.inf])
    assert rec == {"recall@0.25/2": 0.25, "recall@0.5/5": 0.5, "recall@5/10": 0.75}


def test_lifting_oracle_is_pinned_to_the_reference_warp():
    """The oracle's float32 lift -> T_0to1 -> K1 projection against the reference's float32 w_kpts0 on the points with depth.
    Tolerance: 2 x the reference's own float32-vs-float64 distance, floored at one float32 ulp of a 640 px coordinate (2^-14)."""
    g = np.load(GOLDEN)
    N, L = g["kpts0"].shape[:2]
    assert g["depth0"].shape == (N, 60, 80) and 0 < (~g["nonzero"]).sum() < N * L and os.path.getsize(GOLDEN) < 100_000
    frac = g["kpts0"] - np.floor(g["kpts0"])
    assert (frac == 0.5).sum() >= 2 * 24 * N - 8                                       # exact halves are in the fixture
    bids = np.repeat(np.arange(N), L)
    X, valid = O.lift(g["kpts0"].reshape(-1, 2), bids, g["depth0"], g["K0"])
    assert np.array_equal(valid, g["nonzero"].reshape(-1))
    f = np.float32
    T, K1 = g["T_0to1"][bids], g["K1"][bids]
    Y = np.einsum("nij,nj->ni", T[:, :3, :3], X).astype(f) + T[:, :3, 3]
    h = np.einsum("nij,nj->ni", K1, Y).astype(f)
    w = h[:, :2] / (h[:, 2:] + f(1e-4))
    ref32, ref64 = g["w_kpts0_f32"].reshape(-1, 2)[valid], g["w_kpts0_f64"].reshape(-1, 2)[valid]
    tol = max(2 * np.abs(ref32.astype(np.float64) - ref64).max(), 2.0 ** -14)
    err = np.abs(w[valid].astype(np.float64) - ref32).max()
    print(f"lift vs reference fp32: {err:.3e} px, tolerance {tol:.3e}")
    assert err <= tol, (err, tol)
    assert not X[~valid].any()
