"""CPU checks of the absolute-pose entry points (csrc/absolute_pose.hip, csrc/absolute_pose_gpu.hip, added to ABI 25 without a bump):
bad arguments and a short workspace return their status codes before any device work, an empty batch is a no-op success, the ops /
evaluation wrappers refuse what the kernels cannot take (CPU tensors, wrong dtypes or shapes) with no fallback, and a library without
the entry points is refused."""
import ctypes
import os

import numpy as np
import pytest
import torch

from loftr_amd import _lib, build as build_mod

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_estimate_absolute_pose", "loftr_p3p", "loftr_estimate_absolute_pose_batched",
         "loftr_estimate_absolute_pose_batched_workspace_bytes", "loftr_lift_keypoints")


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
    assert build_mod.SOURCES.count("absolute_pose.hip") == 1 and build_mod.SOURCES.count("absolute_pose_gpu.hip") == 1


def test_a_library_without_the_absolute_pose_entry_points_is_refused(lib, monkeypatch):
    """The entry points came without an ABI bump, so a stale library is caught by its missing symbol: a LoftrHipError that says to
    rebuild, not an AttributeError from ctypes."""
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
    with pytest.raises(_lib.LoftrHipError, match="loftr_estimate_absolute_pose.*rebuild"):
        _lib.load()


def _args(M=10, P=2, ws_bytes=None, ptr=1 << 20, **over):
    """Argument list of loftr_estimate_absolute_pose_batched with fake (never dereferenced) pointers."""
    a = dict(pts3d=ptr, kpts=ptr, bids=ptr, M=M, K=ptr, P=P, thr=3.0, conf=0.999, seed=0, R=ptr, t=ptr, inl=ptr, n=ptr, ws=ptr, ws_bytes=ws_bytes,
             stream=None)
    a.update(over)
    return list(a.values())


def test_workspace_bytes(lib):
    f = lib.loftr_estimate_absolute_pose_batched_workspace_bytes
    assert f(-1, 2) == 0 and f(10, -1) == 0
    assert f(0, 1) >= 4000 * (12 * 8 + 4 + 4) + 1000 * 3 * 4               # pose, count and work list of 4000 slots, samples
    assert f(2000, 1) - f(0, 1) >= 2000 * 65                               # 8 doubles + one byte per match
    assert f(100, 8) > 7 * f(100, 1)


def test_argument_checks(lib):
    f, need = lib.loftr_estimate_absolute_pose_batched, lib.loftr_estimate_absolute_pose_batched_workspace_bytes(10, 2)
    assert f(*_args(P=-1, ws_bytes=need)) == BAD_ARG
    assert f(*_args(M=-1, ws_bytes=need)) == BAD_ARG
    for name in ("pts3d", "kpts", "bids", "K", "R", "t", "inl", "n", "ws"):
        assert f(*_args(ws_bytes=need, **{name: None})) == BAD_ARG, name
    assert f(*_args(ws_bytes=need - 1)) == WORKSPACE
    assert f(*_args(ws_bytes=0)) == WORKSPACE
    assert f(*_args(M=0, P=0, ws_bytes=0)) == 0                                # nothing to do
    assert f(*_args(M=0, P=0, ws_bytes=0, pts3d=None, K=None, R=None, ws=None)) == 0
    assert f(*_args(M=5, P=0, ws_bytes=0)) == BAD_ARG                          # every pair id would be out of range
    assert f(*_args(M=0, P=2, ws_bytes=lib.loftr_estimate_absolute_pose_batched_workspace_bytes(0, 2) - 1, pts3d=None, kpts=None, bids=None,
                    inl=None)) == WORKSPACE
    assert f(*_args(M=1 << 31, ws_bytes=1 << 62)) == UNSUPPORTED
    assert f(*_args(M=10, P=(1 << 31) // 1000 + 1, ws_bytes=1 << 62)) == UNSUPPORTED


def test_lift_argument_checks(lib):
    f, p = lib.loftr_lift_keypoints, 1 << 20
    ok = dict(kpts=p, bids=p, M=10, depth=p, dh=60, dw=80, K=p, T=None, P=2, out=p, valid=p, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    for name in ("kpts", "bids", "depth", "K", "out", "valid"):
        assert call(**{name: None}) == BAD_ARG, name
    assert call(M=-1) == BAD_ARG and call(dh=-1) == BAD_ARG and call(dw=-1) == BAD_ARG and call(P=-1) == BAD_ARG and call(P=0) == BAD_ARG
    assert call(M=0) == 0 and call(M=0, kpts=None, depth=None, out=None, P=0) == 0


def test_host_estimator_argument_checks(lib):
    z, n = np.zeros(16, np.float32), ctypes.c_long(5)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    f = lib.loftr_estimate_absolute_pose
    assert f(None, None, 4, ptr(z), 3.0, 0.999, 0, ptr(z), ptr(z), None, ctypes.byref(n)) == BAD_ARG
    assert f(ptr(z), ptr(z), -1, ptr(z), 3.0, 0.999, 0, ptr(z), ptr(z), ptr(z), ctypes.byref(n)) == BAD_ARG
    R = np.ones(9, np.float32)
    assert f(None, None, 0, ptr(z), 3.0, 0.999, 0, ptr(R), ptr(z), None, ctypes.byref(n)) == 0 and n.value == -1 and not R.any()


def test_ops_refuses_cpu_tensors_wrong_dtypes_and_shapes():
    from loftr_amd import ops
    X, k, b, K = torch.zeros(6, 3), torch.zeros(6, 2), torch.zeros(6, dtype=torch.int64), torch.eye(3)[None]
    for args in ((X, k, b, K), (X.double(), k, b, K), (X, k, b.int(), K), (X, k, b, K.double()), (X.numpy(), k, b, K)):
        with pytest.raises(_lib.LoftrHipError):
            ops.estimate_absolute_poses(*args, 3.0, 0.999)
    d = torch.zeros(1, 60, 80)
    for args in ((k, b, d, K), (k.double(), b, d, K), (k, b.int(), d, K), (k, b, d.half(), K), (k, b, d, K, torch.eye(4)[None].double())):
        with pytest.raises(_lib.LoftrHipError):
            ops.lift_keypoints(*args)
    with pytest.raises(_lib.LoftrHipError, match="model"):
        ops.estimate_geometry(k, k, b, 1, "essential", 1.0, 0.999)                 # unchanged: the five-point path is estimate_poses


@pytest.mark.gpu
def test_ops_refuses_wrong_shapes_on_the_device():
    from loftr_amd import ops
    dev = "cuda:0"
    X, k, b, K = torch.zeros(6, 3, device=dev), torch.zeros(6, 2, device=dev), torch.zeros(6, dtype=torch.int64, device=dev), torch.eye(3, device=dev)[None]
    for args in ((X[:, :2], k, b, K), (X, k[:5], b, K), (X, k, b[:5], K), (X, k, b, K[0]), (X.reshape(-1), k, b, K)):
        with pytest.raises(_lib.LoftrHipError, match="expected pts3d"):
            ops.estimate_absolute_poses(*args, 3.0, 0.999)
    d = torch.zeros(1, 60, 80, device=dev)
    for args in ((k[:, :1], b, d, K), (k, b[:5], d, K), (k, b, d[0], K), (k, b, torch.zeros(2, 60, 80, device=dev), K), (k, b, d, K, torch.eye(4, device=dev))):
        with pytest.raises(_lib.LoftrHipError, match="expected kpts"):
            ops.lift_keypoints(*args)


def test_gpu_twin_returns_none_below_three_matches_without_a_gpu():
    from loftr_amd import evaluation as EV
    z3, z2 = np.zeros((2, 3), np.float32), np.zeros((2, 2), np.float32)
    assert EV.estimate_absolute_pose_native_gpu(z3, z2, np.eye(3)) is None and EV.estimate_absolute_pose_native(z3, z2, np.eye(3)) is None
    assert EV.estimate_absolute_pose_native_gpu(z3[:0], z2[:0], np.eye(3)) is None
