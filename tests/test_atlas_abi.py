"""CPU checks of the keypoint-atlas entry points (csrc/atlas.hip, csrc/atlas_gpu.hip, added to ABI 25 without a bump): null and
zero-size arguments, the workspace function and the status codes, all answered before any device work; the ops wrappers refuse what the
kernels cannot take; a library without the entry points is refused."""
import ctypes
import os

import numpy as np
import pytest
import torch

from loftr_amd import _lib, build as build_mod

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_atlas_host", "loftr_atlas_observe", "loftr_atlas_finalize_workspace_bytes", "loftr_atlas_finalize")
OUT_FIELDS = [n for n, _ in _lib.AtlasOut._fields_]


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
    assert build_mod.SOURCES.count("atlas.hip") == 1 and build_mod.SOURCES.count("atlas_gpu.hip") == 1
    assert "LOFTR_ATLAS_STAGES 7" in header
    from loftr_amd import ops
    assert len(ops.ATLAS_STAGES) == 7 and len(ops.ATLAS_REASONS) == 6


def test_a_library_without_the_atlas_entry_points_is_refused(lib, monkeypatch):
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
    with pytest.raises(_lib.LoftrHipError, match="loftr_atlas.*rebuild"):
        _lib.load()


def _host_out(M, R, n_images, cells):
    Kb = max(1, min(2 * M, cells))
    arr = {"kp_offsets": np.full(n_images + 1, 7, np.int64), "keypoints": np.zeros((Kb, 2), np.float32), "score": np.zeros(Kb, np.float32),
           "n_obs": np.zeros(Kb, np.int32), "row_offsets": np.full(R + 1, 7, np.int64), "matches": np.zeros((max(M, 1), 2), np.int32),
           "match_conf": np.zeros(max(M, 1), np.float32), "track_id": np.zeros(Kb, np.int32), "track_len": np.zeros(Kb, np.int32),
           "track_ok": np.zeros(Kb, np.uint8), "counts": np.full(16, 7, np.int64)}
    return arr, _lib.AtlasOut(**{k: v.ctypes.data_as(ctypes.c_void_p) for k, v in arr.items()})


def test_host_routine_status_codes(lib):
    f = lib.loftr_atlas_host
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    arr, out = _host_out(0, 0, 3, 75)
    # M == 0 and R == 0 succeed and leave zero counts and offsets
    assert f(None, None, None, None, None, 0, None, 0, 3, 5, 5, 0.5, 2, ctypes.byref(out)) == 0
    assert not arr["counts"].any() and not arr["kp_offsets"].any() and arr["row_offsets"].tolist() == [0]
    assert f(None, None, None, None, None, 0, None, 0, 0, 0, 0, 0.5, 2, ctypes.byref(out)) == 0
    # rows without matches
    arr, out = _host_out(0, 2, 3, 75)
    ri = np.array([[0, 1], [1, 2]], np.int32)
    assert f(None, None, None, None, None, 0, ptr(ri), 2, 3, 5, 5, 0.5, 2, ctypes.byref(out)) == 0 and arr["row_offsets"].tolist() == [0, 0, 0]
    assert f(None, None, None, None, None, 0, None, 2, 3, 5, 5, 0.5, 2, ctypes.byref(out)) == BAD_ARG            # rows need their images
    assert f(None, None, None, None, None, 0, ptr(ri), 2, 3, 5, 5, 0.5, 2, None) == BAD_ARG
    assert f(None, None, None, None, None, -1, ptr(ri), 2, 3, 5, 5, 0.5, 2, ctypes.byref(out)) == BAD_ARG
    assert f(None, None, None, None, None, 0, ptr(ri), -1, 3, 5, 5, 0.5, 2, ctypes.byref(out)) == BAD_ARG
    assert f(None, None, None, None, None, 0, ptr(ri), 2, 3, 5, 5, 0.5, 0, ctypes.byref(out)) == BAD_ARG         # min_track_len >= 1
    for bad in ([[0, 0], [1, 2]], [[0, 3], [1, 2]], [[-1, 1], [1, 2]]):                                            # a == b, ids out of range
        assert f(None, None, None, None, None, 0, ptr(np.array(bad, np.int32)), 2, 3, 5, 5, 0.5, 2, ctypes.byref(out)) == BAD_ARG
    # matches: null arrays, rows out of range or descending
    k, c = np.ones((2, 2), np.float32), np.ones(2, np.float32)
    arr, out = _host_out(2, 2, 3, 75)
    call = lambda rows, k0=k: f(None if k0 is None else ptr(k0), ptr(k), ptr(c), ptr(np.array(rows, np.int32)), None, 2, ptr(ri), 2, 3, 5, 5, 0.5, 2,
                                ctypes.byref(out))
    assert call([0, 1]) == 0 and arr["counts"][:3].tolist() == [3, 2, 1] and arr["counts"][4] == 2
    assert call([0, 1], None) == BAD_ARG and call([0, 2]) == BAD_ARG and call([-1, 0]) == BAD_ARG and call([1, 0]) == BAD_ARG
    one = ctypes.c_void_p(1 << 20)                                      # limits are answered before a pointer is read
    assert f(one, one, one, one, None, 2 ** 31 - 1, one, 2, 3, 5, 5, 0.5, 2, ctypes.byref(out)) == UNSUPPORTED
    assert f(one, one, one, one, None, 2, one, 2, 3, 1 << 16, 1 << 16, 0.5, 2, ctypes.byref(out)) == UNSUPPORTED     # 3 * 2^32 cells
    assert f(one, one, one, one, None, 2, one, 2, 3, 1, (1 << 24) + 1, 0.5, 2, ctypes.byref(out)) == UNSUPPORTED


def test_observe_status_codes(lib):
    f, p = lib.loftr_atlas_observe, 1 << 20
    ok = dict(k0=p, k1=p, conf=p, bids=p, mask=None, n=10, n_rows=2, match_base=0, row_base=0, row_images=p, n_images=3, gh=5, gw=5, inv=0.5,
              grid=p, obs_xy=p, obs_cell=p, m_conf=p, m_row=p, m_reason=p, status=p, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    assert call(n=0) == 0 and call(n=0, k0=None, grid=None, status=None, n_rows=0) == 0           # an empty chunk is a no-op
    for name in ("k0", "k1", "conf", "bids", "row_images", "grid", "obs_xy", "obs_cell", "m_conf", "m_row", "m_reason", "status"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("n", "n_rows", "match_base", "row_base", "n_images", "gh", "gw"):
        assert call(**{name: -1}) == BAD_ARG, name
    assert call(n_rows=0) == BAD_ARG and call(n_images=0) == BAD_ARG and call(gh=0) == BAD_ARG      # matches without rows / a grid
    assert call(match_base=2 ** 31 - 10) == UNSUPPORTED and call(gh=1 << 16, gw=1 << 16) == UNSUPPORTED
    assert call(row_base=1 << 30) == UNSUPPORTED


def test_finalize_workspace_and_status_codes(lib):
    wsb, f, p = lib.loftr_atlas_finalize_workspace_bytes, lib.loftr_atlas_finalize, 1 << 20
    assert wsb(-1, 3, 5, 5) == 0 and wsb(10, -1, 5, 5) == 0 and wsb(2 ** 31 - 1, 3, 5, 5) == 0 and wsb(10, 3, 1 << 16, 1 << 16) == 0
    assert wsb(0, 3, 5, 5) > 0                                                                    # the counts of an empty atlas still need the scan
    assert wsb(1000, 806, 240, 320) >= 16 * 4096 + 806 * 240 * 320 // 256 * 4                     # a table of >= 4 M slots, a count per block of cells
    a, b = wsb(100_000, 806, 240, 320), wsb(200_000, 806, 240, 320)
    assert 16 * (1 << 20) > b - a >= 16 * (1 << 19)                                                # the table doubles with the matches: 2^19 -> 2^20 slots
    out = _lib.AtlasOut(**{k: p for k in OUT_FIELDS})
    ok = dict(grid=p, obs_xy=p, obs_cell=p, m_conf=p, m_row=p, m_reason=p, M=10, R=2, n_images=3, gh=5, gw=5, min_track_len=2, status=p,
              out=ctypes.byref(out), ws=p, ws_bytes=wsb(10, 3, 5, 5), stage_ms=None, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    assert call(ws_bytes=ok["ws_bytes"] - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    for name in ("grid", "obs_xy", "obs_cell", "m_conf", "m_row", "m_reason", "out", "ws"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("M", "R", "n_images", "gh", "gw", "min_track_len"):
        assert call(**{name: -1}) == BAD_ARG, name
    assert call(min_track_len=0) == BAD_ARG and call(R=0) == BAD_ARG and call(n_images=0) == BAD_ARG           # matches without rows / a grid
    for name in OUT_FIELDS:
        assert call(out=ctypes.byref(_lib.AtlasOut(**{k: (None if k == name else p) for k in OUT_FIELDS}))) == BAD_ARG, name
    assert call(M=2 ** 31 - 1, ws_bytes=1 << 62) == UNSUPPORTED and call(gh=1 << 16, gw=1 << 16, ws_bytes=1 << 62) == UNSUPPORTED
    assert call(R=(1 << 30) + 1, ws_bytes=1 << 62) == UNSUPPORTED


def test_ops_refuses_cpu_tensors(lib):
    from loftr_amd import ops
    z = lambda n, dt: torch.zeros(n, dtype=dt)
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):
        ops.atlas_finalize(z(75, torch.int64), z(40, torch.float32), z(20, torch.int32), z(10, torch.float32), z(10, torch.int32), z(10, torch.uint8),
                           z(1, torch.int32), 10, 2, 3, 5, 5, 2)
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):
        ops.atlas_observe(torch.zeros(4, 2), torch.zeros(4, 2), torch.zeros(4), z(4, torch.int64), None, 1, 0, 0, z(2, torch.int32).reshape(1, 2), 3, 5, 5,
                          0.5, z(75, torch.int64), z(40, torch.float32), z(20, torch.int32), z(10, torch.float32), z(10, torch.int32),
                          z(10, torch.uint8), z(1, torch.int32))
    with pytest.raises(ValueError, match="agree on M"):
        ops.atlas_host(np.zeros((3, 2)), np.zeros((2, 2)), np.zeros(3), np.zeros(3), None, np.zeros((1, 2)), 3, 5, 5, 0.5, 2)
