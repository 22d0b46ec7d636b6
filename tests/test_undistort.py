"""Undistortion on the CPU: the host routine loftr_undistort_points_host, which DEFINES the result, and the distort routine of
the same text -- the round trip, a float64 reference, the points that must fail, the error bit and the empty call."""
import numpy as np
import pytest
import torch

import loftr_amd
from loftr_amd import _lib, build as build_mod, ops
import _undistort_cases as UC


@pytest.fixture(scope="module", autouse=True)
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def grid(i, k, R, steps=41):
    """Pinhole pixels of camera i on a grid of normalised points within radius R."""
    K, _ = UC.cameras()
    g = np.linspace(-R, R, steps)
    x = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    x = x[np.linalg.norm(x, axis=1) <= R]
    return (x @ K[i][:2, :2].T + K[i][:2, 2]).astype(np.float32), np.full(len(x), i, np.int32)


@pytest.mark.parametrize("i,k", list(enumerate(UC.KS)))
def test_round_trip_within_one_f32_ulp_of_a_coordinate(i, k):
    """undistort(distort(p)) against p.  The distorted pixel in between is rounded to f32, and the inverse map amplifies that rounding
    radially by 1 / (1 + 3 k r^2): 1 at the centre and unbounded at the fold of a barrel k.  The grid of a barrel k therefore stays
    where that factor is at most 1.25 (1 + 3 k r^2 >= 0.8: r <= 0.47 for k = -0.3, 0.75 for k = -0.12), well inside the monotone range;
    a pincushion k contracts and its grid goes to r = 1.6.  One ulp of a coordinate is the f32 spacing at the largest coordinate of
    the grid (555 to 1252 px here).  Measured: 1.0, 1.0, 0, 0.5, 0.5 ulp for k = -0.3, -0.12, 0, 0.08, 0.5."""
    K, ks = UC.cameras()
    R = min(1.6, np.sqrt(0.2 / (-3 * k))) if k < 0 else 1.6
    px, im = grid(i, k, R)
    d = ops.distort_points_host(px, im, K, ks)
    u = ops.undistort_points_host(d["xy"], im, K, ks)
    ulp = float(np.spacing(np.float32(np.abs(px).max())))
    err = np.abs(u["xy"].astype(np.float64) - px.astype(np.float64)).max() / ulp
    print(f"k = {k}: {len(px)} points to r = {R:.3f}, largest coordinate {np.abs(px).max():.1f}, round trip {err:.3f} ulp")
    assert d["ok"].all() and u["ok"].all() and u["counts"].tolist()[:3] == [len(px), 0, 0]
    assert err <= 1.0
    if k == 0:
        assert np.array_equal(d["xy"], u["xy"])                          # (both recompute the point through K)


@pytest.mark.parametrize("i,k", list(enumerate(UC.KS)))
def test_against_a_float64_newton_run_to_convergence(i, k):
    """The whole monotone range (to 0.97 of the fold of a barrel k, r = 1.6 else): the routine's result from the f32 distorted pixel
    against numpy's solution of the same equation from the same pixel, iterated until it stops moving.  Both read one input, so no
    rounding is amplified: what is left is the rounding of the output to f32, half an ulp of the coordinate, and the fp64 error of the
    solve (below 1e-9 px).  Twelve fixed iterations are therefore enough everywhere on this range."""
    K, ks = UC.cameras()
    px, im = grid(i, k, UC.monotone_radius(k, 0.97))
    d = ops.distort_points_host(px, im, K, ks)["xy"]
    u = ops.undistort_points_host(d, im, K, ks)
    y = (d[:, 1].astype(np.float64) - K[i, 1, 2]) / K[i, 1, 1]
    x = (d[:, 0].astype(np.float64) - K[i, 0, 2] - K[i, 0, 1] * y) / K[i, 0, 0]
    rd = np.hypot(x, y)
    r = rd.copy()
    for _ in range(200):
        r = r - (r * (1 + k * r * r) - rd) / (1 + 3 * k * r * r)
    m = 1 + k * r * r
    want = np.stack([K[i, 0, 0] * x / m + K[i, 0, 1] * y / m + K[i, 0, 2], K[i, 1, 1] * y / m + K[i, 1, 2]], 1)
    err = np.abs(u["xy"].astype(np.float64) - want)
    bound = 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 1e-9
    print(f"k = {k}: {len(px)} points, largest error {err.max():.3g} px, largest error / bound {(err / bound).max():.3f}")
    assert u["ok"].all() and (err <= bound).all()


def test_points_that_must_fail_are_nan_with_ok_zero():
    K, ks = UC.cameras()
    fold = 1 / np.sqrt(3 * 0.3)                                          # k = -0.3: r (1 + k r^2) peaks at r = 1.054 with r_d = 0.703
    rd = np.array([0.70, 0.71, 0.9, 2.0, 50.0])
    xy = np.stack([K[0, 0, 0] * rd + K[0, 0, 2], np.full(5, K[0, 1, 2])], 1).astype(np.float32)
    out = ops.undistort_points_host(xy, np.zeros(5, np.int32), K, ks)
    assert out["ok"].tolist() == [1, 0, 0, 0, 0] and np.isnan(out["xy"][1:]).all() and np.isfinite(out["xy"][0]).all()
    assert (out["xy"][0, 0] - K[0, 0, 2]) / K[0, 0, 0] < fold and out["counts"].tolist()[:3] == [1, 0, 4]
    assert np.array_equal(out["xy"][1:].view(np.uint32), np.full((4, 2), 0x7fc00000, np.uint32))     # one NaN, the same on both sides
    bad = np.array([[np.nan, 240], [320, np.inf], [-np.inf, 240], [320, 240]], np.float32)
    out = ops.undistort_points_host(bad, np.array([1, 1, 1, len(UC.KS)], np.int32), K, ks)       # the last: the camera with fx = 0
    assert out["ok"].tolist() == [0, 0, 0, 0] and np.isnan(out["xy"]).all()
    for edit in (lambda K, k: K.__setitem__((1, 1, 1), 0.0), lambda K, k: K.__setitem__((1, 0, 2), np.nan), lambda K, k: k.__setitem__(1, np.inf)):
        K2, k2 = K.copy(), ks.copy()
        edit(K2, k2)
        out = ops.undistort_points_host(np.array([[330, 250]], np.float32), np.array([1], np.int32), K2, k2)
        assert out["ok"].tolist() == [0] and np.isnan(out["xy"]).all()
    xy, ok = loftr_amd.undistort_points(torch.from_numpy(bad), torch.tensor([1, 1, 1, 2]), torch.from_numpy(K), torch.from_numpy(ks))
    assert ok.tolist() == [False, False, False, True] and ok.dtype == torch.bool and xy.dtype == torch.float32 and torch.isfinite(xy[3]).all()


def test_the_error_bit_and_the_empty_call():
    K, ks = UC.cameras()
    xy, image, _, _ = UC.batch(65)
    for at, bad in ((0, -1), (64, len(K))):
        im = image.copy()
        im[at] = bad
        out = ops.undistort_points_host(xy, im, K, ks)
        assert out["counts"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and not out["xy"].any() and not out["ok"].any()
        with pytest.raises(ValueError, match="image outside"):
            loftr_amd.undistort_points(xy, im, K, ks)
    with pytest.raises(ValueError, match="image must hold integers"):
        loftr_amd.undistort_points(xy, image.astype(np.float32), K, ks)
    out = ops.undistort_points_host(np.zeros((0, 2), np.float32), np.zeros(0, np.int32), K, ks)
    assert out["counts"].tolist() == [0] * 8 and out["xy"].shape == (0, 2) and out["ok"].shape == (0,)
    xy0, ok0 = loftr_amd.undistort_points(np.zeros((0, 2), np.float32), np.zeros(0, np.int64), K, ks)
    assert tuple(xy0.shape) == (0, 2) and tuple(ok0.shape) == (0,)
    with pytest.raises(ValueError, match="host routine only"):
        class Fake(torch.Tensor):
            @property
            def is_cuda(self):
                return True
        loftr_amd.distort_points(*[torch.from_numpy(a).as_subclass(Fake) for a in (xy, image, K, ks)])
