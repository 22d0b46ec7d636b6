"""CPU checks of the rotation-averaging entry points (csrc/rotation.hip, csrc/rotation_gpu.hip, added to ABI 25 without a bump): the
exports; null pointers, negative sizes and parameters out of range are answered with the documented status before any device work; the
workspace query is 0 without images and for sizes out of range; the ops wrappers refuse what the kernels cannot take; a library
without the entry points is refused; the README carries the number of entry points."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _rotation_cases as RC
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_rotation_averaging_host", "loftr_rotation_averaging_workspace_bytes", "loftr_rotation_averaging")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
ARGS = ("edge_image", "edge_R", "edge_weight", "E", "n_images", "root", "adj_offsets", "adj_edge", "edge_use_in", "cycle_cos_half", "loss_chord",
        "max_chord", "step_tol", "max_iters", "pcg_iters", "pcg_tol", "R", "in_graph", "edge_state", "edge_chord", "support", "tree", "edge_use",
        "counts", "info")
POINTERS = ("edge_image", "edge_R", "edge_weight", "adj_offsets", "adj_edge", "edge_use_in", "R", "in_graph", "edge_state", "edge_chord", "support",
            "tree", "edge_use", "counts", "info")


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def test_entry_points_are_exported_and_declared(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "loftr_hip.h")).read()
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert lib.loftr_hip_abi_version() == _lib.ABI_VERSION == 25 and len(_lib.SIGNATURES) == 153
    assert build_mod.SOURCES.count("rotation.hip") == 1 and build_mod.SOURCES.count("rotation_gpu.hip") == 1
    assert f"#define LOFTR_ROTATION_STAGES {len(ops.ROTATION_STAGES)}" in header
    assert ops.ROTATION_COUNTS == 16 == len(ops.ROTATION_NAMES) and ops.ROTATION_STATES == ("invalid", "outside", "ok", "outlier")
    assert [b for b, _ in ops.ROTATION_ERRORS] == [1, 2, 4, 8]
    assert loftr_amd.average_rotations is not None
    assert loftr_amd.GlobalRotations.FIELDS == ("R", "in_graph", "edge_state", "edge_chord", "support", "tree", "edge_use")
    for m in ("rotation_averaging", "without_rows"):
        assert hasattr(loftr_amd.SfmResult, m)
    assert f"{len(_lib.SIGNATURES)} entry points" in open(os.path.join(ROOT, "README.md")).read()


def test_one_text_for_host_and_device():
    """the core header holds every per-item step, reuses §18's quaternion conversions unchanged and uses no trigonometry"""
    core = open(os.path.join(CSRC, "rotation_core.h")).read()
    assert "#pragma clang fp contract(off)" in core and "ba::quat_from_matrix(" in core and "ba::matrix_from_quat(" in core
    for fn in ("sin(", "cos(", "acos(", "asin(", "atan", "exp(", "pow("):
        assert fn not in core.replace("cos_half", ""), fn
    for f in ("rotation.hip", "rotation_gpu.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "rotation_core.h"' in text and "#pragma clang fp contract(off)" in text, f
        for step in ("edge_setup(", "node_check(", "support_slot(", "start_edge(", "edge_eval(", "node_rhs(", "node_Lp(", "node_update(",
                     "node_direction(", "node_apply(", "node_commit(", "feed(", "decide(", "edge_verdict(", "node_write(", "finish("):
            assert step in text, (f, step)
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))}
    for fn in ("support_slot", "start_edge", "edge_eval", "node_rhs", "edge_verdict"):
        assert [f for f, text in sources.items() if f" {fn}(const P& p" in text] == ["rotation_core.h"], fn


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
    with pytest.raises(_lib.LoftrHipError, match="loftr_rotation_averaging.*rebuild"):
        _lib.load()


def _host_args():
    sc = RC.make_scene("abi", 6, 2, 3)
    a = RC.ops_args(sc)
    E, n = a[0].shape[0], sc.n
    vals = dict(zip(ARGS[:16], [a[0], a[1], a[2], E, n, a[7], a[3], a[4], a[5], *a[8:]]))
    vals.update(R=np.full((n, 3, 3), 7.0), in_graph=np.full(n, 9, np.uint8), edge_state=np.full(E, 9, np.uint8), edge_chord=np.full(E, 7.0),
                support=np.full(E, -9, np.int32), tree=np.full(E, 9, np.uint8), edge_use=np.full(E, 9, np.uint8), counts=np.full(16, 7, np.int64),
                info=np.full(4, 7.0))
    assert tuple(vals) == ARGS
    return vals


def _call(f, a, **over):
    vals = {**a, **over}
    return f(*[v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v for v in vals.values()])


def test_host_routine_status_codes(lib):
    f = lib.loftr_rotation_averaging_host
    a = _host_args()
    assert _call(f, a) == 0
    assert a["counts"][0] == 6 and a["counts"][1] == 0 and a["counts"][14] == 0 and (a["edge_state"] == 2).all() and a["in_graph"].all()
    for name in POINTERS:
        assert _call(f, a, **{name: None}) == BAD_ARG, name
    for name in ("E", "n_images", "max_iters", "pcg_iters"):
        assert _call(f, a, **{name: -1}) == BAD_ARG, name
    for name, v in (("loss_chord", 0.0), ("loss_chord", -1.0), ("max_chord", -1e-3), ("step_tol", -1.0), ("pcg_tol", 1.0), ("pcg_tol", -0.1),
                    ("cycle_cos_half", math.nan), ("loss_chord", math.inf), ("max_chord", math.nan), ("step_tol", math.inf)):
        assert _call(f, a, **{name: v}) == BAD_ARG, (name, v)
    assert _call(f, a, n_images=0) == BAD_ARG                             # edges without images
    # nothing at all: only adj_offsets [1], counts and info are read or written
    none = {k: None for k in POINTERS if k not in ("counts", "info", "adj_offsets")}
    assert _call(f, a, E=0, n_images=0, root=-1, adj_offsets=np.zeros(1, np.int64), **none) == 0
    assert a["counts"].tolist() == [0] * 14 + [3, -1] and a["info"].tolist() == [0.0] * 4
    # a bad graph: BAD_ARG, the bits in counts[1] and nothing else written
    a = _host_args()
    assert _call(f, a, root=6) == BAD_ARG and a["counts"].tolist() == [0, 8] + [0] * 14
    assert (a["R"] == 7.0).all() and (a["edge_state"] == 9).all() and (a["support"] == -9).all() and (a["info"] == 7.0).all()
    one = ctypes.c_void_p(1 << 20)                                        # limits are answered before a pointer is read
    lim = lambda **over: f(*[{**{k: (one if k in POINTERS else v) for k, v in a.items()}, **over}[k] for k in ARGS])
    assert lim(E=2 ** 31 - 1) == UNSUPPORTED and lim(n_images=2 ** 30 + 1) == UNSUPPORTED
    assert lim(max_iters=2 ** 16 + 1) == UNSUPPORTED and lim(pcg_iters=2 ** 16 + 1) == UNSUPPORTED


def test_kernel_entry_point_status_codes(lib):
    wsb, f, p = lib.loftr_rotation_averaging_workspace_bytes, lib.loftr_rotation_averaging, 1 << 20
    assert wsb(0, 0) == 0 and wsb(-1, 4) == 0 and wsb(4, -1) == 0 and wsb(2 ** 31 - 1, 4) == 0 and wsb(4, 2 ** 30 + 1) == 0
    assert wsb(0, 1) > 0
    big = wsb(10 ** 6, 10 ** 5)                                            # about 90 bytes per edge and 190 per image
    assert 80 * 10 ** 6 + 180 * 10 ** 5 <= big <= 100 * 10 ** 6 + 200 * 10 ** 5
    a = _host_args()
    ok = {k: (p if k in POINTERS else v) for k, v in a.items()}
    ok.update(ws=p, ws_bytes=wsb(ok["E"], ok["n_images"]), stage_ms=None, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    assert call(ws_bytes=ok["ws_bytes"] - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    for name in POINTERS + ("ws",):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("E", "n_images", "max_iters", "pcg_iters"):
        assert call(**{name: -1}) == BAD_ARG, name
    assert call(loss_chord=0.0) == BAD_ARG and call(pcg_tol=1.0) == BAD_ARG and call(n_images=0) == BAD_ARG
    huge = dict(ws_bytes=1 << 62)
    assert call(E=2 ** 31 - 1, **huge) == UNSUPPORTED and call(n_images=2 ** 30 + 1, **huge) == UNSUPPORTED
    assert call(max_iters=2 ** 16 + 1, **huge) == UNSUPPORTED


def test_ops_refuses_wrong_dtypes_shapes_and_devices(lib):
    a = RC.ops_args(RC.make_scene("abi", 6, 2, 3))
    good, tail = a[:6], a[6:]
    assert ops.rotation_averaging_host(*good, *tail)["counts"][0] == 6
    swaps = {0: np.int64, 1: np.float32, 2: np.int64, 3: np.int32, 4: np.int64, 5: np.bool_}
    for i, dt in swaps.items():
        with pytest.raises(_lib.LoftrHipError, match="must be"):
            ops.rotation_averaging_host(*[g.astype(dt) if j == i else g for j, g in enumerate(good)], *tail)
    shapes = {0: good[0][:, :1], 1: good[1][:-1], 2: good[2][:-1], 3: good[3][:-1], 4: good[4][:-1], 5: good[5][:-1], }
    for i, bad in shapes.items():
        with pytest.raises(_lib.LoftrHipError, match="must be|expected edge_image"):
            ops.rotation_averaging_host(*[bad if j == i else g for j, g in enumerate(good)], *tail)
    for i, v in ((0, -1), (0, True), (1, 1.5), (6, -1), (7, 2.5)):
        t = list(tail)
        t[i] = v
        with pytest.raises(ValueError, match="must be an integer"):
            ops.rotation_averaging_host(*good, *t)
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops.rotation_averaging_host(*[torch.from_numpy(g) for g in good], *tail)
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):           # the kernels take GPU tensors only: no fallback
        ops.rotation_averaging(*[torch.from_numpy(g) for g in good], *tail)
