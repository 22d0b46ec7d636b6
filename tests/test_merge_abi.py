"""CPU checks of the track-merging entry points (csrc/merge.hip, csrc/merge_gpu.hip, added to ABI 25 without a bump): null pointers,
negative sizes, a reach or threshold out of range and a short workspace are answered with the documented status before any device work;
the workspace query is 0 for sizes out of range; the ops wrappers refuse what the kernels cannot take; a library without the entry
points is refused; mixed devices are an error."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _merge_cases as MC
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_merge_tracks_host", "loftr_merge_tracks_workspace_bytes", "loftr_merge_tracks")
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
    assert build_mod.SOURCES.count("merge.hip") == 1 and build_mod.SOURCES.count("merge_gpu.hip") == 1
    assert "LOFTR_MERGE_STAGES 5" in header and "LOFTR_MERGE_IMAGE_CHUNK 64" in header
    assert len(ops.MERGE_STAGES) == 5 and ops.MERGE_COUNTS == 8 == len(ops.MERGE_NAMES)
    assert loftr_amd.merge_tracks is not None and loftr_amd.Merge.FIELDS == ("row_into", "merge_r2", "merged", "kp_row_new")
    assert hasattr(loftr_amd.SfmResult, "merge")
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme


def test_one_text_for_host_and_device():
    """the core header includes completion's unchanged and is the only place of the rule; the two table kernels exist once"""
    core = open(os.path.join(CSRC, "merge_core.h")).read()
    assert '#include "complete_core.h"' in core and "#pragma clang fp contract(off)" in core
    for f in ("merge.hip", "merge_gpu.hip"):
        assert '#include "merge_core.h"' in open(os.path.join(CSRC, f)).read(), f
    defined = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip")) and "void complete_camera_kernel(" in open(os.path.join(CSRC, f)).read()]
    assert defined == ["complete_kernels.h"]
    for f in ("complete_gpu.hip", "merge_gpu.hip"):
        assert '#include "complete_kernels.h"' in open(os.path.join(CSRC, f)).read(), f


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
    with pytest.raises(_lib.LoftrHipError, match="loftr_merge_tracks.*rebuild"):
        _lib.load()


def _host_args():
    t, _ = MC.hand()
    gh, gw, inv = t["grid"]
    K, T = len(t["kp_row"]), len(t["status"])
    return dict(offsets=t["offsets"], T=T, obs_image=t["obs_image"], obs_xy=t["obs_xy"], obs_mask=t["obs_mask"], N=len(t["obs_image"]), xyz=t["xyz"],
                status=t["status"], kp_offsets=t["kp_offsets"], keypoints=t["keypoints"], kp_cell=t["kp_cell"], kp_row=t["kp_row"], K=K, Kmat=t["K"],
                T_cam_from_world=t["T_cam_from_world"], posed=t["posed"], n_images=len(t["posed"]), inv=inv, gh=gh, gw=gw, thresh_px=4.0, reach=2,
                row_into=np.full(T, -9, np.int32), merge_r2=np.full(T, -9, np.float32), kp_row_new=np.full(K, -9, np.int32),
                counts=np.full(8, 7, np.int64))


def _call(f, a, **over):
    vals = {**a, **over}
    return f(*[v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v for v in vals.values()])


POINTERS = ("offsets", "obs_image", "obs_xy", "obs_mask", "xyz", "status", "kp_offsets", "keypoints", "kp_cell", "kp_row", "Kmat", "T_cam_from_world",
            "posed", "row_into", "merge_r2", "kp_row_new", "counts")


def test_host_routine_status_codes(lib):
    f = lib.loftr_merge_tracks_host
    a = _host_args()
    assert _call(f, a) == 0
    assert a["counts"][[0, 1, 4, 5, 6, 7]].tolist() == [4, 0, 20, 18, 13, 5] and (a["kp_row_new"] != -9).all() and (a["row_into"] != -9).all()
    for name in POINTERS:
        assert _call(f, a, **{name: None}) == BAD_ARG, name
    for name in ("T", "N", "K", "n_images", "gh", "gw"):
        assert _call(f, a, **{name: -1}) == BAD_ARG, name
    for reach in (-1, 9, 2 ** 31 - 1, -2 ** 31):
        assert _call(f, a, reach=reach) == BAD_ARG, reach
    for reach in (0, 8):
        assert _call(f, a, reach=reach) == 0, reach
    for thr in (-1.0, float("nan"), float("inf")):
        assert _call(f, a, thresh_px=thr) == BAD_ARG, thr
    assert _call(f, a, thresh_px=0.0) == 0 and a["counts"][0] == 0
    # no row, no observation, no keypoint, no image: nothing is read
    none = {k: None for k in POINTERS if k not in ("offsets", "kp_offsets", "counts")}
    zero = np.zeros(1, np.int64)
    assert _call(f, a, T=0, N=0, K=0, n_images=0, offsets=zero, kp_offsets=zero, **none) == 0 and a["counts"].tolist() == [0] * 8
    assert _call(f, a, T=0, offsets=zero) == BAD_ARG                                      # observations outside every row
    assert _call(f, a, n_images=0, kp_offsets=zero) == BAD_ARG                            # keypoints outside every image
    one = ctypes.c_void_p(1 << 20)                                                         # limits are answered before a pointer is read
    base = {k: one for k in POINTERS}
    base.update(T=1, N=2, K=4, n_images=2, inv=0.5, gh=10, gw=10, thresh_px=4.0, reach=2)
    lim = lambda **over: f(*[{**base, **over}[k] for k in a])
    assert lim(T=2 ** 31) == UNSUPPORTED and lim(N=2 ** 31) == UNSUPPORTED and lim(K=2 ** 31) == UNSUPPORTED
    assert lim(gw=2 ** 24 + 1) == UNSUPPORTED and lim(gh=2 ** 16, gw=2 ** 16) == UNSUPPORTED


def test_kernel_entry_point_status_codes(lib):
    wsb, f, p = lib.loftr_merge_tracks_workspace_bytes, lib.loftr_merge_tracks, 1 << 20
    assert wsb(-1, 2, 2, 2) == 0 and wsb(1, -1, 2, 2) == 0 and wsb(1, 2, -1, 2) == 0 and wsb(1, 2, 2, -1) == 0
    assert wsb(2 ** 31, 2, 2, 2) == 0 and wsb(1, 2 ** 31, 2, 2) == 0 and wsb(1, 2, 2 ** 31, 2) == 0
    assert wsb(0, 0, 0, 0) > 0 and wsb(5000, 30, 5, 10) >= 5000 * 8 + 10 * 192 and wsb(10, 30, 5, 1000) >= 1000 * 192
    assert wsb(5000, 30, 10 ** 6, 10) < 5000 * 8 + 10 * 192 + 1024                         # 192 bytes per image, 8 per row: nothing per keypoint
    ok = {k: p for k in POINTERS}
    ok.update(T=10, N=30, K=40, n_images=4, inv=0.5, gh=240, gw=320, thresh_px=4.0, reach=2)
    ok = {k: ok[k] for k in _host_args()}
    ok.update(ws=p, ws_bytes=wsb(10, 30, 40, 4), stage_ms=None, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    assert call(ws_bytes=ok["ws_bytes"] - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    for name in POINTERS + ("ws",):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("T", "N", "K", "n_images", "gh", "gw"):
        assert call(**{name: -1}) == BAD_ARG, name
    assert call(reach=-1) == BAD_ARG and call(reach=9) == BAD_ARG
    assert call(thresh_px=-0.5) == BAD_ARG and call(thresh_px=float("nan")) == BAD_ARG and call(thresh_px=float("inf")) == BAD_ARG
    assert call(T=0) == BAD_ARG and call(n_images=0) == BAD_ARG                            # observations / keypoints outside every row / image
    big = dict(ws_bytes=1 << 62)
    assert call(T=2 ** 31, **big) == UNSUPPORTED and call(N=2 ** 31, **big) == UNSUPPORTED and call(K=2 ** 31, **big) == UNSUPPORTED
    assert call(gw=2 ** 24 + 1, **big) == UNSUPPORTED and call(n_images=64 * 65535 + 1, **big) == UNSUPPORTED


def test_ops_refuses_wrong_dtypes_shapes_and_devices(lib):
    t, _ = MC.hand()
    good, tail = MC.args(t)[:13], MC.args(t)[13:]
    out = ops.merge_tracks_host(*good, *tail)
    assert out["counts"][1] == 0 and out["counts"][0] == 4
    swaps = {0: np.int32, 1: np.int64, 2: np.float64, 3: np.bool_, 4: np.float64, 5: np.bool_, 6: np.int32, 7: np.float64, 8: np.int64, 9: np.int64,
             10: np.float32, 11: np.float32, 12: np.bool_}
    for i, dt in swaps.items():
        with pytest.raises(_lib.LoftrHipError, match="must be"):
            ops.merge_tracks_host(*[g.astype(dt) if j == i else g for j, g in enumerate(good)], *tail)
    shapes = {0: good[0].reshape(1, -1), **{i: good[i][:3] for i in range(2, 13)}}
    for i, bad in shapes.items():
        with pytest.raises(_lib.LoftrHipError, match="must be|expected offsets"):
            ops.merge_tracks_host(*[bad if j == i else g for j, g in enumerate(good)], *tail)
    for reach in (9, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="reach must be an integer in"):
            ops.merge_tracks_host(*good, *tail[:4], reach)
    with pytest.raises(ValueError, match="thresh_px"):
        ops.merge_tracks_host(*good, *tail[:3], -1.0, 2)
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops.merge_tracks_host(*[torch.from_numpy(g) for g in good], *tail)
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):                            # the kernels take GPU tensors only
        ops.merge_tracks(*[torch.from_numpy(g) for g in good], *tail)


class _FakeGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: enough for the device check, which runs before any data is touched."""
    @property
    def is_cuda(self):
        return True


def test_mixed_devices_are_an_error(lib):
    t, _ = MC.hand()
    names = ("offsets", "obs_image", "obs_xy", "obs_mask", "kp_offsets", "keypoints", "kp_row", "xyz", "status", "K", "T_cam_from_world")
    args = [torch.from_numpy(t[k]) for k in names]
    kw = dict(image_hw=MC.CC.HW, cell_px=MC.CC.CELL)
    for i in (0, 2, 3, 5, 6, 8, 10):
        mixed = list(args)
        mixed[i] = args[i].as_subclass(_FakeGpu)
        with pytest.raises(_lib.LoftrHipError, match="GPU and CPU arguments mixed.*no silent fallback"):
            loftr_amd.merge_tracks(*mixed, **kw)
    with pytest.raises(_lib.LoftrHipError, match="posed: GPU"):
        loftr_amd.merge_tracks(*args, posed=torch.from_numpy(t["posed"]).as_subclass(_FakeGpu), **kw)
