"""Batched pose estimation on the GPU (csrc/pose_gpu.hip, ops.estimate_poses): for every pair of a batch, the result of the host
estimator loftr_estimate_pose (evaluation.estimate_pose_native) with the same seed -- same n_inliers, same inlier mask, R and t
equal after the float32 rounding.  The host estimator is the reference here; parity against OpenCV stays unpinned."""
import os

import numpy as np
import pytest
import torch

from loftr_amd import _lib, evaluation as EV, ops
from _scenes import make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THR, CONF = 0.5, 0.99999


def _rot(axis, ang):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def _pair(rng, n, noise_px, outliers, t_scale=1.0):
    """A test_pose-style two-view pair with n matches (noise on both images, outliers replace image-1 points)."""
    K0 = np.array([[580.0, 0, 320], [0, 585.0, 240], [0, 0, 1]])
    K1 = np.array([[575.0, 0, 318], [0, 578.0, 243], [0, 0, 1]])
    R = _rot(rng.standard_normal(3), 0.1 + 0.4 * rng.random())
    t = rng.standard_normal(3)
    t *= t_scale / np.linalg.norm(t)
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)]
    Y = X @ R.T + t
    p0 = (X / X[:, 2:]) @ K0.T
    p1 = (Y / Y[:, 2:]) @ K1.T
    p0, p1 = p0[:, :2] + noise_px * rng.standard_normal((n, 2)), p1[:, :2] + noise_px * rng.standard_normal((n, 2))
    k = int(outliers * n)
    if k:
        sel = rng.choice(n, k, replace=False)
        p1[sel] = np.c_[rng.uniform(0, 640, k), rng.uniform(0, 480, k)]
    return p0.astype(np.float32), p1.astype(np.float32), K0.astype(np.float32), K1.astype(np.float32)


def _degenerate(rng):
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]], np.float32)
    same = np.full((50, 2), 200.0, np.float32)                                       # all points equal
    s = rng.uniform(0, 1, 60)
    line0 = np.c_[100 + 400 * s, 80 + 300 * s].astype(np.float32)                     # collinear in both images
    line1 = np.c_[120 + 380 * s, 90 + 290 * s + rng.normal(0, 0.2, 60)].astype(np.float32)
    rot = _pair(rng, 300, 0.3, 0.2, t_scale=0.0)                                      # pure rotation (t = 0)
    return [(same, same.copy(), K, K), (line0, line1, K, K), rot]


def _batch(pairs):
    """Stack per-pair (p0, p1, K0, K1) into the matcher's layout (m_bids grouped by ascending pair)."""
    return dict(mkpts0_f=np.concatenate([p[0] for p in pairs]).reshape(-1, 2), mkpts1_f=np.concatenate([p[1] for p in pairs]).reshape(-1, 2),
                m_bids=np.concatenate([np.full(len(p[0]), b, np.int64) for b, p in enumerate(pairs)]),
                K0=np.stack([p[2] for p in pairs]), K1=np.stack([p[3] for p in pairs]))


def _grid():
    rng = np.random.default_rng(2024)
    pairs = []
    for n in (0, 4, 5, 6, 37, 400, 2000, 8000):
        for noise in (0.0, 0.3, 1.0):
            for out in (0.0, 0.3, 0.6):
                if n == 8000 and (noise, out) not in ((0.0, 0.0), (0.3, 0.3), (1.0, 0.6)):
                    continue                                                          # (host time: three pairs of 8 000 are enough)
                pairs.append(_pair(rng, n, noise, out))
    pairs += _degenerate(rng)
    sc = make_scene(77, [300, 1200, 5, 0, 900], noise_px=0.5, outlier_frac=0.3)
    for b in range(5):
        m = sc["m_bids"] == b
        pairs.append((sc["mkpts0_f"][m], sc["mkpts1_f"][m], sc["K0"][b], sc["K1"][b]))
    return pairs


def _on_gpu(batch, seed=0):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in batch.items()}
    return ops.estimate_poses(t["mkpts0_f"], t["mkpts1_f"], t["m_bids"], t["K0"], t["K1"], THR, CONF, seed)


def _ransac_fraction(p0, p1, K0, K1, R, t):
    """Fraction of the matches within the threshold of E = [t]x R (the Sampson test of pose.hip, in numpy)."""
    q0 = (p0.astype(np.float64) - K0[:2, 2]) / [K0[0, 0], K0[1, 1]]
    q1 = (p1.astype(np.float64) - K1[:2, 2]) / [K1[0, 0], K1[1, 1]]
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    h0, h1 = np.c_[q0, np.ones(len(q0))], np.c_[q1, np.ones(len(q1))]
    l, m = h0 @ E.T, h1 @ E
    r = np.sum(h1 * l, 1)
    thr = THR / np.mean([K0[0, 0], K1[1, 1], K0[0, 0], K1[1, 1]])
    return float(np.mean(r * r < thr * thr * (l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2)))


def _compare(pairs, got, seed, host=None):
    """The batched result against the host estimator's, pair by pair (host: its results for `seed` where they are at hand)."""
    R, t, inl, n = (x.cpu().numpy() for x in got)
    bids = np.concatenate([np.full(len(p[0]), b) for b, p in enumerate(pairs)])
    stats = {"early": 0, "capped": 0, "none": 0}
    for b, (p0, p1, K0, K1) in enumerate(pairs):
        ref = host[b] if host is not None else EV.estimate_pose_native(p0, p1, K0, K1, THR, conf=CONF, seed=seed)
        mask = inl[bids == b]
        if ref is None:
            assert n[b] == -1 and not mask.any() and not R[b].any() and not t[b].any(), (b, n[b])
            stats["none"] += 1
            continue
        Rh, th, mh = ref
        assert n[b] == mh.sum(), (b, n[b], mh.sum())
        assert np.array_equal(mask, mh), (b, np.flatnonzero(mask != mh)[:10])
        assert np.abs(R[b].astype(np.float64) - Rh).max() <= 1e-6 and np.abs(t[b].astype(np.float64) - th).max() <= 1e-6, b
        # the host loop stopped early if at least 90 % of the matches are RANSAC inliers (>= the cheirality inliers):
        # (0.9^5 -> at most 13 iterations); it ran all 1000 if fewer than ~41 % are (here: < 30 % for E = [t]x R)
        stats["early"] += mh.mean() >= 0.9
        stats["capped"] += _ransac_fraction(p0, p1, K0, K1, Rh, th) < 0.3
    return stats


@pytest.fixture(scope="module")
def grid():
    return _grid()


@pytest.mark.parametrize("seed", [0, 11])
def test_identical_to_the_host_estimator_on_a_ragged_batch(grid, seed):
    got = _on_gpu(_batch(grid), seed)
    stats = _compare(grid, got, seed)
    assert stats["early"] >= 3 and stats["capped"] >= 3 and stats["none"] >= 4, stats


def test_repeat_calls_are_bit_identical_and_inputs_untouched(grid):
    batch = _batch(grid[40:])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in batch.items()}
    before = {k: v.clone() for k, v in t.items()}
    a = ops.estimate_poses(t["mkpts0_f"], t["mkpts1_f"], t["m_bids"], t["K0"], t["K1"], THR, CONF, 3)
    b = ops.estimate_poses(t["mkpts0_f"], t["mkpts1_f"], t["m_bids"], t["K0"], t["K1"], THR, CONF, 3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for k in t:
        assert torch.equal(t[k], before[k]), k
    assert a[0].shape == (len(grid) - 40, 3, 3) and a[1].shape == (len(grid) - 40, 3) and a[2].dtype == torch.bool
    assert a[3].dtype == torch.int64 and a[2].shape == t["m_bids"].shape


def test_refusals(grid):
    batch = _batch(grid[60:66])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in batch.items()}
    P = t["K0"].shape[0]
    call = lambda **o: ops.estimate_poses(*[o.get(k, t[k]) for k in ("mkpts0_f", "mkpts1_f", "m_bids", "K0", "K1")], THR, CONF)
    with pytest.raises(_lib.LoftrHipError):
        call(mkpts0_f=t["mkpts0_f"].cpu())
    with pytest.raises(_lib.LoftrHipError):
        call(K1=t["K1"].cpu())
    with pytest.raises(_lib.LoftrHipError):
        call(m_bids=t["m_bids"].flip(0))                                         # not grouped by ascending pair
    bad = t["m_bids"].clone(); bad[-1] = P                                        # out of range
    with pytest.raises(_lib.LoftrHipError):
        call(m_bids=bad)
    bad = t["m_bids"].clone(); bad[0] = -1
    with pytest.raises(_lib.LoftrHipError):
        call(m_bids=bad)
    with pytest.raises(_lib.LoftrHipError):
        call(mkpts0_f=t["mkpts0_f"].reshape(-1))                                  # wrong shapes
    with pytest.raises(_lib.LoftrHipError):
        call(K0=t["K0"][:-1])
    with pytest.raises(_lib.LoftrHipError):
        call(m_bids=t["m_bids"][:-1])
    R, tt, inl, n = call()                                                        # still fine after the refusals
    assert n.shape == (P,)


def test_empty_batch_and_no_matches():
    K = torch.eye(3, device=DEV).reshape(1, 3, 3).repeat(3, 1, 1)
    z = torch.zeros(0, 2, device=DEV)
    R, t, inl, n = ops.estimate_poses(z, z, torch.zeros(0, dtype=torch.int64, device=DEV), K, K, THR, CONF)
    assert n.tolist() == [-1, -1, -1] and inl.shape == (0,) and not R.any()


def _data(batch):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in batch.items()}


def _same_pose_errors(d0, d1):
    assert d0["R_errs"] == d1["R_errs"] and d0["t_errs"] == d1["t_errs"]
    assert len(d0["inliers"]) == len(d1["inliers"]) and all(np.array_equal(a, b) for a, b in zip(d0["inliers"], d1["inliers"]))
    assert all(a.dtype == b.dtype for a, b in zip(d0["inliers"], d1["inliers"]))


@pytest.mark.parametrize("case", ["a", "b", "c", "scene"])
def test_compute_pose_errors_native_gpu_equals_native(case):
    try:
        import cv2  # noqa: F401
        pytest.skip("OpenCV present: on_missing does not apply")
    except ImportError:
        pass
    if case == "scene":
        data = _data(make_scene(5, [500, 0, 3, 1500, 800, 6], noise_px=0.5, outlier_frac=0.3))
    else:
        npz = np.load(os.path.join(GOLD, "metrics_epi.npz"))
        data = _data({k: npz[f"{case}_{k}"] for k in ("mkpts0_f", "mkpts1_f", "m_bids", "T_0to1", "K0", "K1")})
    d_host, d_gpu, d_explicit = dict(data), dict(data), dict(data)
    EV.compute_pose_errors(d_host, on_missing="native")
    EV._WARNED_NATIVE.clear()
    with pytest.warns(UserWarning, match="parity"):
        EV.compute_pose_errors(d_gpu, on_missing="native_gpu")
    EV.compute_pose_errors(d_explicit, estimator=EV.estimate_pose_native_gpu)
    assert d_gpu["pose_estimator"] == d_explicit["pose_estimator"] == "estimate_pose_native_gpu"
    _same_pose_errors(d_host, d_gpu)
    _same_pose_errors(d_host, d_explicit)


def test_per_pair_form_matches_the_host_estimator(grid):
    for p0, p1, K0, K1 in grid[18:27] + grid[-3:]:
        ref, got = EV.estimate_pose_native(p0, p1, K0, K1, THR, CONF, seed=4), EV.estimate_pose_native_gpu(p0, p1, K0, K1, THR, CONF, seed=4)
        assert (ref is None) == (got is None)
        if ref is not None:
            assert np.array_equal(ref[2], got[2]) and np.abs(ref[0] - got[0]).max() <= 1e-6 and np.abs(ref[1] - got[1]).max() <= 1e-6


def test_test_step_on_a_real_forward_gives_identical_pose_errors():
    """evaluation.test_step on the 8-pair bench forward (e2e_batch8 inputs) with synthetic intrinsics / poses: the same pose errors and
    inlier masks with the host estimator and with the GPU one."""
    from test_e2e_golden import _bench_data, build_model, load
    rc, img0, img1, g = load("e2e_batch8")
    model = build_model(rc, 0.0, DEV)
    sc = make_scene(8, [1] * 8)
    out = {}
    for how in ("native", "native_gpu"):
        data = _bench_data(g, img0, img1, DEV)
        data.update({k: torch.from_numpy(sc[k]).to(DEV) for k in ("K0", "K1", "T_0to1")})
        out[how] = EV.test_step(model, data, dump=False, on_missing=how)["metrics"]
        assert data["mkpts0_f"].shape[0] > 100
    _same_pose_errors(out["native"], out["native_gpu"])
