"""CPU checks of the similarity entry points (csrc/similarity.hip, csrc/similarity_gpu.hip, added to ABI 25 without a bump): the exports,
null pointers and bad counts return LOFTR_ERR_BAD_ARG before any device work, a short workspace its own code, an empty batch is a
no-op success, the ops wrappers refuse what the kernels cannot take (CPU tensors, wrong dtypes or shapes, mixed devices) with no
fallback, a library without the entry points is refused, and the README carries the number of entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

from loftr_amd import _lib, build as build_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_estimate_similarity", "loftr_similarity_minimal", "loftr_estimate_similarity_batched",
         "loftr_estimate_similarity_batched_workspace_bytes", "loftr_transform_model_host", "loftr_transform_model")


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def test_entry_points_are_exported_and_declared(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "loftr_hip.h")).read()
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert lib.loftr_hip_abi_version() == _lib.ABI_VERSION == 25 and "#define LOFTR_HIP_ABI_VERSION 25" in header
    assert build_mod.SOURCES.count("similarity.hip") == 1 and build_mod.SOURCES.count("similarity_gpu.hip") == 1
    assert f"{len(_lib.SIGNATURES)} entry points" in open(os.path.join(ROOT, "README.md")).read()
    import loftr_amd
    assert loftr_amd.Alignment is loftr_amd.alignment.Alignment and callable(loftr_amd.align_centres)


def test_a_library_without_the_similarity_entry_points_is_refused(lib, monkeypatch):
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
    with pytest.raises(_lib.LoftrHipError, match="loftr_estimate_similarity.*rebuild"):
        _lib.load()


def _args(M=10, P=2, ws_bytes=None, ptr=1 << 20, **over):
    """Argument list of loftr_estimate_similarity_batched with fake (never dereferenced) pointers."""
    a = dict(src=ptr, dst=ptr, bids=ptr, M=M, P=P, with_scale=1, thr=0.05, conf=0.999, seed=0, s=ptr, R=ptr, t=ptr, inl=ptr, n=ptr, ws=ptr,
             ws_bytes=ws_bytes, stream=None)
    a.update(over)
    return list(a.values())


def test_workspace_bytes(lib):
    f = lib.loftr_estimate_similarity_batched_workspace_bytes
    assert f(-1, 2) == 0 and f(10, -1) == 0
    assert f(0, 1) >= 1000 * (13 * 8 + 4 + 4) + 1000 * 3 * 4               # model, count and work list of 1000 slots, samples
    assert f(2000, 1) - f(0, 1) >= 2000 * 49                               # 6 doubles + one byte per correspondence
    assert f(100, 8) > 7 * f(100, 1)


def test_argument_checks(lib):
    f, need = lib.loftr_estimate_similarity_batched, lib.loftr_estimate_similarity_batched_workspace_bytes(10, 2)
    assert f(*_args(P=-1, ws_bytes=need)) == BAD_ARG
    assert f(*_args(M=-1, ws_bytes=need)) == BAD_ARG
    for name in ("src", "dst", "bids", "s", "R", "t", "inl", "n", "ws"):
        assert f(*_args(ws_bytes=need, **{name: None})) == BAD_ARG, name
    assert f(*_args(ws_bytes=need - 1)) == WORKSPACE
    assert f(*_args(ws_bytes=0)) == WORKSPACE
    assert f(*_args(M=0, P=0, ws_bytes=0)) == 0                                # nothing to do
    assert f(*_args(M=0, P=0, ws_bytes=0, src=None, s=None, R=None, ws=None)) == 0
    assert f(*_args(M=5, P=0, ws_bytes=0)) == BAD_ARG                          # every problem id would be out of range
    assert f(*_args(M=0, P=2, ws_bytes=lib.loftr_estimate_similarity_batched_workspace_bytes(0, 2) - 1, src=None, dst=None, bids=None,
                    inl=None)) == WORKSPACE
    assert f(*_args(M=1 << 31, ws_bytes=1 << 62)) == UNSUPPORTED
    assert f(*_args(M=10, P=(1 << 31) // 1000 + 1, ws_bytes=1 << 62)) == UNSUPPORTED


def test_transform_model_argument_checks(lib):
    p = 1 << 20
    ok = dict(xyz=p, N=10, T=p, posed=p, n=3, s=p, R=p, t=p, xyz_out=p, T_out=p, stream=None)
    call = lambda **over: lib.loftr_transform_model(*{**ok, **over}.values())
    for name in ("xyz", "T", "posed", "s", "R", "t", "xyz_out", "T_out"):
        assert call(**{name: None}) == BAD_ARG, name
    assert call(N=-1) == BAD_ARG and call(n=-1) == BAD_ARG
    z = np.zeros(16)
    q = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert call(N=0, n=0, xyz=None, T=None, posed=None, xyz_out=None, T_out=None, s=q(z), R=q(z), t=q(z)) == 0       # nothing to do, no launch
    host = lambda **over: lib.loftr_transform_model_host(*list({**ok, **over}.values())[:-1])
    for name in ("xyz", "T", "posed", "s", "R", "t", "xyz_out", "T_out"):
        assert host(**{name: None}) == BAD_ARG, name
    assert host(N=-1) == BAD_ARG and host(n=-1) == BAD_ARG
    assert host(N=0, n=0, xyz=None, T=None, posed=None, xyz_out=None, T_out=None, s=q(z), R=q(z), t=q(z)) == 0


def test_host_estimator_argument_checks(lib):
    z, n = np.zeros(16), ctypes.c_long(5)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    f = lib.loftr_estimate_similarity
    assert f(None, None, 4, 1, 0.05, 0.999, 0, ptr(z), ptr(z), ptr(z), None, ctypes.byref(n)) == BAD_ARG
    assert f(ptr(z), ptr(z), -1, 1, 0.05, 0.999, 0, ptr(z), ptr(z), ptr(z), ptr(z), ctypes.byref(n)) == BAD_ARG
    assert f(ptr(z), ptr(z), 4, 1, 0.05, 0.999, 0, None, ptr(z), ptr(z), ptr(z), ctypes.byref(n)) == BAD_ARG
    R, s = np.ones(9), np.ones(1)
    assert f(None, None, 0, 1, 0.05, 0.999, 0, ptr(s), ptr(R), ptr(z), None, ctypes.byref(n)) == 0 and n.value == -1 and not R.any() and not s.any()


def test_ops_refuses_cpu_tensors_wrong_dtypes_and_shapes():
    from loftr_amd import ops
    a, b = torch.zeros(6, 3, dtype=torch.float64), torch.zeros(6, dtype=torch.int64)
    for args in ((a, a, b), (a.float(), a, b), (a.half(), a, b), (a, a, b.int()), (a.numpy(), a, b)):
        with pytest.raises(_lib.LoftrHipError):
            ops.estimate_similarities(*args, 1)
    # transform_model: CPU tensors run the host routine, so the refusals are dtypes, shapes and mixed kinds
    xyz, T, posed = torch.zeros(4, 3), torch.eye(4, dtype=torch.float64).repeat(2, 1, 1), torch.ones(2, dtype=torch.bool)
    s, R, t = torch.ones(1, dtype=torch.float64), torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    out_xyz, out_T = ops.transform_model(xyz, T, posed, s, R, t)
    assert torch.equal(out_T, T) and torch.equal(out_xyz, xyz)
    for args in ((xyz.double(), T, posed, s, R, t), (xyz, T.float(), posed, s, R, t), (xyz, T, posed.long(), s, R, t), (xyz, T, posed, s.float(), R, t),
                 (xyz[:, :2], T, posed, s, R, t), (xyz, T, posed[:1], s, R, t), (xyz, T.numpy(), posed, s, R, t)):
        with pytest.raises(_lib.LoftrHipError):
            ops.transform_model(*args)


@pytest.mark.gpu
def test_ops_refuses_wrong_shapes_and_mixed_devices_on_the_device():
    from loftr_amd import alignment, ops
    dev = "cuda:0"
    a, b = torch.zeros(6, 3, dtype=torch.float64, device=dev), torch.zeros(6, dtype=torch.int64, device=dev)
    for args in ((a[:, :2], a, b), (a, a[:5], b), (a, a, b[:5]), (a.reshape(-1), a, b)):
        with pytest.raises(_lib.LoftrHipError, match="expected src"):
            ops.estimate_similarities(*args, 1)
    with pytest.raises(_lib.LoftrHipError):
        ops.estimate_similarities(a, a.cpu(), b, 1)
    xyz, T, posed = torch.zeros(4, 3, device=dev), torch.eye(4, dtype=torch.float64, device=dev).repeat(2, 1, 1), torch.ones(2, dtype=torch.bool, device=dev)
    s, R, t = torch.ones(1, dtype=torch.float64, device=dev), torch.eye(3, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)
    for args in ((xyz.cpu(), T, posed, s, R, t), (xyz, T, posed, s.cpu(), R, t), (xyz, T.cpu(), posed.cpu(), s, R, t)):
        with pytest.raises(_lib.LoftrHipError, match="different devices"):
            ops.transform_model(*args)
    with pytest.raises(_lib.LoftrHipError, match="mixed"):
        alignment.align_centres(T, posed.cpu(), torch.zeros(2, 3, dtype=torch.float64, device=dev), posed, 0.1)


def test_gpu_twin_returns_none_below_three_correspondences_without_a_gpu():
    from loftr_amd import evaluation as EV
    z = np.zeros((2, 3))
    assert EV.estimate_similarity_native_gpu(z, z) is None and EV.estimate_similarity_native(z, z) is None
    assert EV.estimate_similarity_native_gpu(z[:0], z[:0]) is None
