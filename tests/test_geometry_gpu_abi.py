"""CPU checks of the batched geometry entry point (csrc/geometry_gpu.hip, added to ABI 25 without a bump): bad arguments and a short
workspace return their status codes before any device work, an empty batch is a no-op success, the ops / evaluation wrappers refuse what
the kernels cannot take (CPU tensors, wrong dtypes or shapes, unknown models) with no fallback, and a library without the entry points is
refused."""
import ctypes

import numpy as np
import pytest
import torch

from loftr_amd import _lib, build as build_mod

BAD_ARG, WORKSPACE = -1, -3
NAMES = ("loftr_estimate_geometry", "loftr_geometry_minimal", "loftr_estimate_geometry_batched", "loftr_estimate_geometry_batched_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def test_entry_points_are_exported_and_declared(lib):
    import os
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "loftr_hip.h")).read()
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert lib.loftr_hip_abi_version() == _lib.ABI_VERSION == 25
    assert build_mod.SOURCES.count("geometry.hip") == 1 and build_mod.SOURCES.count("geometry_gpu.hip") == 1


def test_a_library_without_the_geometry_entry_points_is_refused(lib, monkeypatch, tmp_path):
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
    with pytest.raises(_lib.LoftrHipError, match="loftr_estimate_geometry.*rebuild"):
        _lib.load()


def _args(M=10, P=2, model=1, ws_bytes=None, ptr=1 << 20, **over):
    """Argument list of loftr_estimate_geometry_batched with fake (never dereferenced) pointers."""
    a = dict(k0=ptr, k1=ptr, bids=ptr, M=M, P=P, model=model, thr=1.0, conf=0.999, seed=0, mat=ptr, inl=ptr, n=ptr, ws=ptr, ws_bytes=ws_bytes,
             stream=None)
    a.update(over)
    return list(a.values())


def test_workspace_bytes(lib):
    f = lib.loftr_estimate_geometry_batched_workspace_bytes
    assert f(-1, 2, 0) == 0 and f(10, -1, 0) == 0 and f(10, 2, 2) == 0 and f(10, 2, -1) == 0
    assert f(0, 1, 0) >= 1000 * (9 * 8 + 4 + 4) + 1000 * 4 * 4                # H: matrix, count and work list of 1000 slots, samples
    assert f(0, 1, 1) >= 3000 * (9 * 8 + 4 + 4) + 1000 * 7 * 4                # F: 3000 slots
    assert f(2000, 1, 0) - f(0, 1, 0) >= 2000 * 33                             # fp64 points + one byte per match
    assert f(100, 8, 1) > 7 * f(100, 1, 1)


def test_argument_checks(lib):
    f, need = lib.loftr_estimate_geometry_batched, lib.loftr_estimate_geometry_batched_workspace_bytes(10, 2, 1)
    assert f(*_args(P=-1, ws_bytes=need)) == BAD_ARG
    assert f(*_args(M=-1, ws_bytes=need)) == BAD_ARG
    assert f(*_args(model=2, ws_bytes=need)) == BAD_ARG and f(*_args(model=-1, ws_bytes=need)) == BAD_ARG
    for name in ("k0", "k1", "bids", "mat", "inl", "n", "ws"):
        assert f(*_args(ws_bytes=need, **{name: None})) == BAD_ARG, name
    assert f(*_args(ws_bytes=need - 1)) == WORKSPACE
    assert f(*_args(ws_bytes=0)) == WORKSPACE
    assert f(*_args(model=0, ws_bytes=lib.loftr_estimate_geometry_batched_workspace_bytes(10, 2, 0) - 1)) == WORKSPACE
    assert f(*_args(M=0, P=0, ws_bytes=0)) == 0                                # nothing to do
    assert f(*_args(M=0, P=0, ws_bytes=0, k0=None, mat=None, ws=None)) == 0
    assert f(*_args(M=5, P=0, ws_bytes=0)) == BAD_ARG                          # every pair id would be out of range
    assert f(*_args(M=0, P=2, ws_bytes=lib.loftr_estimate_geometry_batched_workspace_bytes(0, 2, 1) - 1, k0=None, bids=None, inl=None)) == WORKSPACE
    assert f(*_args(M=1 << 31, ws_bytes=1 << 62)) == -2                         # LOFTR_ERR_UNSUPPORTED


def test_ops_refuses_cpu_tensors_wrong_dtypes_and_models():
    from loftr_amd import ops
    k, b = torch.zeros(6, 2), torch.zeros(6, dtype=torch.int64)
    with pytest.raises(_lib.LoftrHipError):
        ops.estimate_geometry(k, k, b, 1, "homography", 3.0, 0.999)
    with pytest.raises(_lib.LoftrHipError):
        ops.estimate_geometry(k.double(), k, b, 1, "fundamental", 1.0, 0.999)
    with pytest.raises(_lib.LoftrHipError):
        ops.estimate_geometry(k, k, b.int(), 1, "fundamental", 1.0, 0.999)
    with pytest.raises(_lib.LoftrHipError, match="model"):
        ops.estimate_geometry(k, k, b, 1, "essential", 1.0, 0.999)


def test_gpu_twins_return_none_below_the_sample_size_without_a_gpu():
    from loftr_amd import evaluation as EV
    z = np.zeros((6, 2), np.float32)
    assert EV.estimate_homography_native_gpu(z[:3], z[:3]) is None and EV.estimate_fundamental_native_gpu(z, z) is None
    assert EV.estimate_homography_native(z[:3], z[:3]) is None and EV.estimate_fundamental_native(z, z) is None
