"""CPU checks of the batched pose entry point (csrc/pose_gpu.hip, added to ABI 25): bad arguments and a short workspace return
their status codes before any device work, an empty batch is a no-op success, the ops / evaluation wrappers refuse what the
kernels cannot take (CPU tensors, wrong dtypes or shapes) with no fallback, and a library without the entry point is refused."""
import ctypes

import numpy as np
import pytest
import torch

from loftr_amd import _lib, build as build_mod

BAD_ARG, WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def test_entry_points_are_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("loftr_estimate_pose_batched", "loftr_estimate_pose_batched_workspace_bytes"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name


def test_a_library_without_a_bound_entry_point_is_refused(lib, monkeypatch):
    """The entry points came without an ABI bump, so a stale library is caught by its missing symbol: a LoftrHipError that says
    to rebuild, not an AttributeError from ctypes."""
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.SIGNATURES, "loftr_not_exported", (ctypes.c_int, []))
    with pytest.raises(_lib.LoftrHipError, match="loftr_not_exported.*rebuild"):
        _lib.load()


def _args(M=10, P=2, ws_bytes=None, ptr=1 << 20, **over):
    """Argument list of loftr_estimate_pose_batched with fake (never dereferenced) pointers."""
    a = dict(k0=ptr, k1=ptr, bids=ptr, M=M, K0=ptr, K1=ptr, P=P, thr=0.5, conf=0.99999, seed=0, R=ptr, t=ptr, inl=ptr, n=ptr,
             ws=ptr, ws_bytes=ws_bytes, stream=None)
    a.update(over)
    return list(a.values())


def test_workspace_bytes(lib):
    f = lib.loftr_estimate_pose_batched_workspace_bytes
    assert f(-1, 2) == 0 and f(10, -1) == 0
    assert f(0, 1) >= 1000 * 10 * (9 * 8 + 4 + 4) + 1000 * 5 * 4        # E, counts and work list of 10 000 hypothesis slots, samples
    assert f(2000, 1) - f(0, 1) >= 2000 * 32                               # fp64 normalised points
    assert f(100, 8) > 7 * f(100, 1)


def test_argument_checks(lib):
    f, need = lib.loftr_estimate_pose_batched, lib.loftr_estimate_pose_batched_workspace_bytes(10, 2)
    assert f(*_args(P=-1, ws_bytes=need)) == BAD_ARG
    assert f(*_args(M=-1, ws_bytes=need)) == BAD_ARG
    for name in ("k0", "k1", "bids", "K0", "K1", "R", "t", "inl", "n", "ws"):
        assert f(*_args(ws_bytes=need, **{name: None})) == BAD_ARG, name
    assert f(*_args(ws_bytes=need - 1)) == WORKSPACE
    assert f(*_args(ws_bytes=0)) == WORKSPACE
    assert f(*_args(M=0, P=0, ws_bytes=0)) == 0                            # nothing to do
    assert f(*_args(M=0, P=0, ws_bytes=0, k0=None, K0=None, ws=None)) == 0
    assert f(*_args(M=5, P=0, ws_bytes=0)) == BAD_ARG                      # every pair id would be out of range
    assert f(*_args(M=0, P=2, ws_bytes=lib.loftr_estimate_pose_batched_workspace_bytes(0, 2) - 1, k0=None, bids=None, inl=None)) == WORKSPACE


def test_ops_refuses_cpu_tensors_and_wrong_dtypes():
    from loftr_amd import ops
    k = torch.zeros(6, 2)
    b = torch.zeros(6, dtype=torch.int64)
    K = torch.eye(3).reshape(1, 3, 3)
    with pytest.raises(_lib.LoftrHipError):
        ops.estimate_poses(k, k, b, K, K, 0.5, 0.99999)
    with pytest.raises(_lib.LoftrHipError):
        ops.estimate_poses(k.double(), k, b, K, K, 0.5, 0.99999)
    with pytest.raises(_lib.LoftrHipError):
        ops.estimate_poses(k, k, b.int(), K, K, 0.5, 0.99999)


def test_compute_pose_errors_names_native_gpu():
    from loftr_amd import evaluation as EV
    data = {"m_bids": torch.zeros(0, dtype=torch.int64), "mkpts0_f": torch.zeros(0, 2), "mkpts1_f": torch.zeros(0, 2),
            "K0": torch.zeros(0, 3, 3), "K1": torch.zeros(0, 3, 3), "T_0to1": torch.zeros(0, 4, 4)}
    with pytest.raises(ValueError, match="native_gpu"):
        EV.compute_pose_errors(dict(data), on_missing="gpu")
    assert EV.estimate_pose_native_gpu(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32), np.eye(3), np.eye(3), 0.5) is None
