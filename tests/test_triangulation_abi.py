"""CPU checks of the triangulation entry points (csrc/triangulate.hip, csrc/triangulate_gpu.hip, added to ABI 25 without a bump): null
pointers, negative sizes, bad tracks and a short workspace are answered with the documented status before any device work; the ops
wrappers refuse what the kernels cannot take; a library without the entry points is refused."""
import ctypes
import os

import numpy as np
import pytest
import torch

from loftr_amd import _lib, build as build_mod

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_triangulate_tracks_host", "loftr_triangulation_pairs", "loftr_triangulate_tracks_workspace_bytes", "loftr_triangulate_tracks")


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def test_entry_points_are_exported_and_declared(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "loftr_hip.h")).read()
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert lib.loftr_hip_abi_version() == _lib.ABI_VERSION == 25
    assert build_mod.SOURCES.count("triangulate.hip") == 1 and build_mod.SOURCES.count("triangulate_gpu.hip") == 1
    assert "LOFTR_TRIANGULATE_STAGES 3" in header
    from loftr_amd import ops
    assert len(ops.TRI_STAGES) == 3 and len(ops.TRI_STATUS) == 5 and ops.TRI_COUNTS == 8


def test_a_library_without_the_triangulation_entry_points_is_refused(lib, monkeypatch):
    class Stale:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            if name in NAMES:
                raise AttributeError(name)
            return getattr(self._real, name)

    real = ctypes.CDLL(_lib.LIB_PATH)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Stale(real))
    with pytest.raises(_lib.LoftrHipError, match="loftr_triangulat.*rebuild"):
        _lib.load()


def _host_args(T=1, N=2, n=2):
    a = dict(offsets=np.array([0, N] if T == 1 else [0] * (T + 1), np.int64), T=T, obs_image=np.arange(N, dtype=np.int32) % max(n, 1),
             obs_xy=np.full((N, 2), 300, np.float32), N=N, K=np.tile(np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]), (n, 1, 1)),
             Tcw=np.tile(np.eye(4), (n, 1, 1)), n_images=n, thresh=4.0, cos_min=0.99,
             xyz=np.zeros((T, 3), np.float32), n_inliers=np.zeros(T, np.int32), rms=np.zeros(T, np.float32), tri_cos=np.zeros(T, np.float32),
             status=np.full(T, 9, np.uint8), obs_inlier=np.full(N, 9, np.uint8), counts=np.full(8, 7, np.int64))
    a["Tcw"][1:, 0, 3] = -1.0
    return a


def _call(f, a, **over):
    vals = {**a, **over}
    return f(*[v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v for v in vals.values()])


def test_host_routine_status_codes(lib):
    f = lib.loftr_triangulate_tracks_host
    a = _host_args()
    assert _call(f, a) == 0 and a["counts"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and a["status"].tolist() == [2] and not a["obs_inlier"].any()
    for name in ("offsets", "obs_image", "obs_xy", "K", "Tcw", "xyz", "n_inliers", "rms", "tri_cos", "status", "obs_inlier", "counts"):
        assert _call(f, a, **{name: None}) == BAD_ARG, name
    for name in ("T", "N", "n_images"):
        assert _call(f, a, **{name: -1}) == BAD_ARG, name
    assert _call(f, a, thresh=-1.0) == BAD_ARG and _call(f, a, thresh=float("nan")) == BAD_ARG
    assert _call(f, a, cos_min=1.5) == BAD_ARG and _call(f, a, cos_min=float("nan")) == BAD_ARG
    # obs_image out of range, offsets that descend / do not start at 0 / do not end at N
    for im in ([0, 2], [-1, 0]):
        assert _call(f, a, obs_image=np.array(im, np.int32)) == BAD_ARG, im
    assert _call(f, a, n_images=1) == BAD_ARG
    for off in ([1, 2], [0, 1], [0, 3]):
        assert _call(f, a, offsets=np.array(off, np.int64)) == BAD_ARG, off
    b = _host_args(T=3)
    assert _call(f, b, offsets=np.array([0, 2, 1, 2], np.int64)) == BAD_ARG
    assert _call(f, b, offsets=np.array([0, 2, 2, 2], np.int64)) == 0 and b["status"].tolist() == [2, 1, 1]
    # no track, no observation, no image: nothing is read
    c = _host_args()
    assert _call(f, c, T=0, N=0, n_images=0, obs_image=None, obs_xy=None, K=None, Tcw=None, xyz=None, n_inliers=None, rms=None, tri_cos=None,
                 status=None, obs_inlier=None, offsets=np.zeros(1, np.int64)) == 0 and not c["counts"].any()
    assert _call(f, c, T=0, offsets=np.zeros(1, np.int64)) == BAD_ARG                      # observations outside every track
    one = ctypes.c_void_p(1 << 20)                                                         # limits are answered before a pointer is read
    assert f(one, 2 ** 31, one, one, 2, one, one, 2, 4.0, 0.99, one, one, one, one, one, one, one) == UNSUPPORTED
    assert f(one, 1, one, one, 2 ** 31, one, one, 2, 4.0, 0.99, one, one, one, one, one, one, one) == UNSUPPORTED


def test_pairs_status_codes(lib):
    f = lib.loftr_triangulation_pairs
    buf, n = (ctypes.c_int * 128)(), ctypes.c_int(-1)
    assert f(5, ctypes.cast(buf, ctypes.c_void_p), ctypes.byref(n)) == 0 and n.value == 10
    assert f(5, None, ctypes.byref(n)) == BAD_ARG and f(5, ctypes.cast(buf, ctypes.c_void_p), None) == BAD_ARG
    assert f(-1, ctypes.cast(buf, ctypes.c_void_p), ctypes.byref(n)) == BAD_ARG


def test_kernel_entry_point_status_codes(lib):
    wsb, f, p = lib.loftr_triangulate_tracks_workspace_bytes, lib.loftr_triangulate_tracks, 1 << 20
    assert wsb(-1, 2, 2) == 0 and wsb(1, -1, 2) == 0 and wsb(1, 2, -1) == 0 and wsb(2 ** 31, 2, 2) == 0 and wsb(1, 2 ** 31, 2) == 0
    assert wsb(0, 0, 0) > 0 and wsb(10, 30, 100) >= 100 * 24 * 8 and wsb(10, 30, 1000) >= 1000 * 24 * 8
    ok = dict(offsets=p, T=10, obs_image=p, obs_xy=p, N=30, K=p, Tcw=p, n_images=100, thresh=4.0, cos_min=0.99, xyz=p, n_inliers=p, rms=p,
              tri_cos=p, status=p, obs_inlier=p, counts=p, group=0, ws=p, ws_bytes=wsb(10, 30, 100), stage_ms=None, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    assert call(ws_bytes=ok["ws_bytes"] - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    for name in ("offsets", "obs_image", "obs_xy", "K", "Tcw", "xyz", "n_inliers", "rms", "tri_cos", "status", "obs_inlier", "counts", "ws"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("T", "N", "n_images"):
        assert call(**{name: -1}) == BAD_ARG, name
    for g in (1, 4, 16, 32, 128, -8):
        assert call(group=g) == BAD_ARG, g
    assert call(thresh=-1.0) == BAD_ARG and call(cos_min=-1.5) == BAD_ARG and call(cos_min=float("nan")) == BAD_ARG
    assert call(T=0) == BAD_ARG                                                            # observations outside every track
    assert call(T=2 ** 31, ws_bytes=1 << 62) == UNSUPPORTED and call(N=2 ** 31, ws_bytes=1 << 62) == UNSUPPORTED


def test_ops_refuses_wrong_dtypes_shapes_and_devices(lib):
    from loftr_amd import ops
    a = _host_args()
    good = [a["offsets"], a["obs_image"], a["obs_xy"], a["K"], a["Tcw"]]
    assert ops.triangulate_tracks_host(*good, 4.0, 0.99)["status"].tolist() == [2]
    swaps = {0: good[0].astype(np.int32), 1: good[1].astype(np.int64), 2: good[2].astype(np.float64), 3: good[3].astype(np.float32),
             4: good[4].astype(np.float32)}
    for i, bad in swaps.items():
        with pytest.raises(_lib.LoftrHipError, match="must be"):
            ops.triangulate_tracks_host(*[bad if j == i else g for j, g in enumerate(good)], 4.0, 0.99)
    shapes = {0: good[0].reshape(1, 2), 1: good[1].reshape(2, 1), 2: good[2][:1], 3: good[3][:, :2], 4: good[4][:1]}
    for i, bad in shapes.items():
        with pytest.raises(_lib.LoftrHipError, match="must be|expected offsets"):
            ops.triangulate_tracks_host(*[bad if j == i else g for j, g in enumerate(good)], 4.0, 0.99)
    with pytest.raises(_lib.LoftrHipError, match="bad argument|BAD_ARG|status -1"):
        ops.triangulate_tracks_host(good[0], np.array([0, 5], np.int32), *good[2:], 4.0, 0.99)
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops.triangulate_tracks_host(*[torch.from_numpy(g) for g in good], 4.0, 0.99)
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):                            # the kernels take GPU tensors only
        ops.triangulate_tracks(*[torch.from_numpy(g) for g in good], 4.0, 0.99)
