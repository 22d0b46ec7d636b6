"""CPU checks of the track-splitting entry points (csrc/split.hip, csrc/split_gpu.hip, added to ABI 25 without a bump): null pointers,
negative sizes, a min_track_len below 1 and a short workspace are answered with the documented status before any device work; the
workspace query is 0 for sizes out of range; the ops wrappers refuse what the kernels cannot take; a library without the entry points
is refused; mixed devices are an error."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _split_cases as SC
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_split_tracks_host", "loftr_split_tracks_workspace_bytes", "loftr_split_tracks")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def test_entry_points_are_exported_and_declared(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "loftr_hip.h")).read()
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert lib.loftr_hip_abi_version() == _lib.ABI_VERSION == 25
    assert build_mod.SOURCES.count("split.hip") == 1 and build_mod.SOURCES.count("split_gpu.hip") == 1
    assert "LOFTR_SPLIT_STAGES(max_rounds) (3 + 4 * (max_rounds))" in header
    assert ops.SPLIT_COUNTS == 16 and len(ops.SPLIT_NAMES) == 11 and ops.SPLIT_STATES == ("ignored", "internal", "conflict", "open")
    assert [b for b, _ in ops.SPLIT_ERRORS] == [1, 2, 4, 8, 16]
    assert loftr_amd.split_tracks is not None and loftr_amd.Split.FIELDS == ("track_id_new", "track_len_new", "edge_state", "round_accepted")
    assert hasattr(loftr_amd.SfmResult, "split")
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme


def test_one_text_for_host_and_device():
    """the core header reuses the atlas's packing and is the only place of the rule's steps"""
    core = open(os.path.join(CSRC, "split_core.h")).read()
    assert '#include "atlas_core.h"' in core and "pack(" not in core.replace("atlas::pack(", "")
    for f in ("split.hip", "split_gpu.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "split_core.h"' in text and "atlas::pack(" in text and "shared_image(" in text and "splice(" in text, f
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))}
    for fn in ("shared_image", "splice", "check_edge", "edge_open"):
        defined = [f for f, text in sources.items() if f" {fn}(const " in text or f" {fn}(int* " in text]
        assert defined == ["split_core.h"], (fn, defined)


def test_a_library_without_the_entry_points_is_refused(lib, monkeypatch):
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
    with pytest.raises(_lib.LoftrHipError, match="loftr_split_tracks.*rebuild"):
        _lib.load()


def _host_args():
    e, c, im, tid, ok, n, min_len, rounds = SC.hand()[0][1]
    E, K, T = len(e), len(im), len(ok)
    return dict(edge_kp=e, edge_conf=c, E=E, kp_image=im, track_id=tid, K=K, track_ok=ok, T=T, n_images=n, min_track_len=min_len,
                max_rounds=rounds, track_id_new=np.full(K, -9, np.int32), track_len_new=np.full(K, -9, np.int32),
                edge_state=np.full(E, 9, np.uint8), round_accepted=np.full(rounds, -9, np.int32), counts=np.full(16, 7, np.int64))


def _call(f, a, **over):
    vals = {**a, **over}
    return f(*[v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v for v in vals.values()])


POINTERS = ("edge_kp", "edge_conf", "kp_image", "track_id", "track_ok", "track_id_new", "track_len_new", "edge_state", "round_accepted", "counts")


def test_host_routine_status_codes(lib):
    f = lib.loftr_split_tracks_host
    a = _host_args()
    assert _call(f, a) == 0
    assert a["counts"].tolist() == SC.hand()[0][2]["counts"] and a["track_id_new"].tolist() == [0, -1, 0] and a["track_len_new"].tolist() == [2, 0, 0]
    assert a["edge_state"].tolist() == [1, 2] and a["round_accepted"].tolist() == [1] + [0] * 31
    for name in POINTERS:
        assert _call(f, a, **{name: None}) == BAD_ARG, name
    for name in ("E", "K", "T", "n_images", "max_rounds"):
        assert _call(f, a, **{name: -1}) == BAD_ARG, name
    for v in (0, -1, -2 ** 31):
        assert _call(f, a, min_track_len=v) == BAD_ARG, v
    # nothing at all: no pointer but the counts is read
    none = {k: None for k in POINTERS if k != "counts"}
    assert _call(f, a, E=0, K=0, T=0, n_images=0, max_rounds=0, **none) == 0 and a["counts"].tolist() == [0] * 16
    # a bad table: BAD_ARG, the bits in counts[1] and nothing else written
    a = _host_args()
    bad = a["kp_image"][::-1].copy()
    assert _call(f, a, kp_image=bad) == BAD_ARG and a["counts"].tolist() == [0, 4] + [0] * 14
    assert (a["track_id_new"] == -9).all() and (a["edge_state"] == 9).all() and (a["round_accepted"] == -9).all()
    one = ctypes.c_void_p(1 << 20)                                                         # limits are answered before a pointer is read
    base = {k: one for k in POINTERS}
    base.update(E=1, K=2, T=1, n_images=2, min_track_len=2, max_rounds=4)
    lim = lambda **over: f(*[{**base, **over}[k] for k in a])
    assert lim(E=2 ** 31 - 1) == UNSUPPORTED and lim(K=2 ** 31) == UNSUPPORTED and lim(T=2 ** 31) == UNSUPPORTED and lim(max_rounds=2 ** 20) == UNSUPPORTED


def test_kernel_entry_point_status_codes(lib):
    wsb, f, p = lib.loftr_split_tracks_workspace_bytes, lib.loftr_split_tracks, 1 << 20
    assert wsb(-1, 2, 2, 2) == 0 and wsb(1, -1, 2, 2) == 0 and wsb(1, 2, -1, 2) == 0 and wsb(1, 2, 2, -1) == 0
    assert wsb(2 ** 31 - 1, 2, 2, 2) == 0 and wsb(1, 2 ** 31, 2, 2) == 0 and wsb(1, 2, 2 ** 31, 2) == 0 and wsb(1, 2, 2, 2 ** 20) == 0
    assert wsb(0, 0, 0, 0) > 0
    big = wsb(10 ** 6, 2 * 10 ** 6, 10 ** 5, 32)                                           # 24 bytes per keypoint, up to 5 per edge, 4 per track
    assert 24 * 2 * 10 ** 6 + 5 * 10 ** 6 + 4 * 10 ** 5 <= big < 24 * 2 * 10 ** 6 + 5 * 10 ** 6 + 4 * 10 ** 5 + 2 * 10 ** 5
    assert wsb(10 ** 6, 100, 10, 32) < 10 ** 6 + 64 * 1024                                # the accepted list is bounded by the keypoints
    ok = {k: p for k in POINTERS}
    ok.update(E=10, K=30, T=4, n_images=4, min_track_len=2, max_rounds=8)
    ok = {k: ok[k] for k in _host_args()}
    ok.update(ws=p, ws_bytes=wsb(10, 30, 4, 8), stage_ms=None, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    assert call(ws_bytes=ok["ws_bytes"] - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    for name in POINTERS + ("ws",):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("E", "K", "T", "n_images", "max_rounds"):
        assert call(**{name: -1}) == BAD_ARG, name
    assert call(min_track_len=0) == BAD_ARG
    huge = dict(ws_bytes=1 << 62)
    assert call(E=2 ** 31 - 1, **huge) == UNSUPPORTED and call(K=2 ** 31, **huge) == UNSUPPORTED and call(T=2 ** 31, **huge) == UNSUPPORTED
    assert call(max_rounds=2 ** 20, **huge) == UNSUPPORTED


def test_ops_refuses_wrong_dtypes_shapes_and_devices(lib):
    args = SC.hand()[0][1]
    good, tail = list(args[:5]), args[5:]
    assert ops.split_tracks_host(*good, *tail)["counts"][0] == 1
    swaps = {0: np.int64, 1: np.float64, 2: np.int64, 3: np.int64, 4: np.bool_}
    for i, dt in swaps.items():
        with pytest.raises(_lib.LoftrHipError, match="must be"):
            ops.split_tracks_host(*[g.astype(dt) if j == i else g for j, g in enumerate(good)], *tail)
    shapes = {0: good[0].reshape(-1), 1: good[1][:1], 3: good[3][:2], 2: good[2].reshape(1, -1)}
    for i, bad in shapes.items():
        with pytest.raises(_lib.LoftrHipError, match="must be|expected edge_kp"):
            ops.split_tracks_host(*[bad if j == i else g for j, g in enumerate(good)], *tail)
    with pytest.raises(_lib.LoftrHipError, match="expected edge_kp"):
        ops.split_tracks_host(np.zeros((2, 3), np.int32), *good[1:], *tail)
    for kw in ((2, 0, 32), (2, True, 32), (2, 2, -1), (2, 2, 1.5), (-1, 2, 32)):
        with pytest.raises(ValueError, match="must be an integer"):
            ops.split_tracks_host(*good, *kw)
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops.split_tracks_host(*[torch.from_numpy(g) for g in good], *tail)
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):                            # the kernels take GPU tensors only
        ops.split_tracks(*[torch.from_numpy(g) for g in good], *tail)


class _FakeGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: enough for the device check, which runs before any data is touched."""
    @property
    def is_cuda(self):
        return True


def test_mixed_devices_are_an_error(lib):
    args = SC.hand()[0][1]
    tensors = [torch.from_numpy(x) for x in args[:5]]
    for i in range(5):
        mixed = list(tensors)
        mixed[i] = tensors[i].as_subclass(_FakeGpu)
        with pytest.raises(_lib.LoftrHipError, match="GPU and CPU arguments mixed.*no silent fallback"):
            loftr_amd.split_tracks(*mixed, *args[5:])
