"""CPU checks of the model-lookup entry points (csrc/model_lookup.hip, csrc/model_lookup_gpu.hip, added to ABI 25 without a bump): null
pointers, negative sizes, the limits, bad rows and a short workspace are answered with the documented status before any device work;
the ops wrappers refuse what the kernels cannot take; a library without the entry points is refused."""
import ctypes
import os

import numpy as np
import pytest
import torch

from loftr_amd import _lib, build as build_mod
import _model_lookup_cases as MC
import _model_lookup_oracle as O

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_model_cells_host", "loftr_model_cells", "loftr_model_lookup_host", "loftr_model_lookup_workspace_bytes", "loftr_model_lookup")


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def test_entry_points_are_exported_declared_and_bound(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "loftr_hip.h")).read()
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert lib.loftr_hip_abi_version() == _lib.ABI_VERSION == 25 and "#define LOFTR_HIP_ABI_VERSION 25" in header
    assert build_mod.SOURCES.count("model_lookup.hip") == 1 and build_mod.SOURCES.count("model_lookup_gpu.hip") == 1
    assert "LOFTR_MODEL_LOOKUP_STAGES 3" in header
    from loftr_amd import ops
    assert len(ops.MODEL_STAGES) == 3 and len(ops.MODEL_REASONS) == 9 and ops.MODEL_COUNTS == 16
    assert [n[2:] for n in ops.MODEL_REASONS] == list(O.REASONS) and [b for b, _ in ops.MODEL_STATUS] == [1, 2, 4, 8, 16, 32]


def test_a_library_without_the_model_entry_points_is_refused(lib, monkeypatch):
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
    with pytest.raises(_lib.LoftrHipError, match="loftr_model_.*rebuild"):
        _lib.load()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _host_setup():
    """The hand-written case as the arguments of loftr_model_lookup_host."""
    case, *_ = MC.hand_case()
    m, q = case["model"], case["q"]
    inv, gh, gw = O.grid(m["image_hw"], m["cell_px"])
    M = len(q["conf"])
    arrays = dict(kp_offsets=m["kp_offsets"], kp_cell=np.array([5, 40, 100, 5], np.int32), kp_point=m["kp_point"], xyz=m["xyz"])
    out = dict(pts3d=np.zeros((M, 3), np.float32), kpts=np.zeros((M, 2), np.float32), q_ids=np.zeros(M, np.int64), match=np.zeros(M, np.int32),
               point=np.zeros(M, np.int32), conf=np.zeros(M, np.float32), q_offsets=np.zeros(3, np.int64), match_reason=np.zeros(M, np.uint8),
               counts=np.full(16, 7, np.int64))
    scal = dict(K=4, P=2, n_images=2, gh=gh, gw=gw, inv=float(inv))
    args = dict(kpts_db=q["kpts_db"], kpts_q=q["kpts_q"], conf=q["conf"], rows=q["rows"], mask=q["mask"], M=M, row_db=q["row_db"],
                row_query=q["row_query"], R=3, Q=2)
    return arrays, scal, out, args


def _call(f, arrays, scal, out, args, tail=(), model_none=False, out_none=False):
    md = _lib.Model(**{k: _ptr(v) for k, v in arrays.items()}, **scal)
    st = _lib.ModelLookupOut(**{k: _ptr(v) for k, v in out.items()})
    vals = [_ptr(v) if isinstance(v, np.ndarray) or v is None else v for v in args.values()]
    return f(None if model_none else ctypes.byref(md), *vals, None if out_none else ctypes.byref(st), *tail)


def test_host_routine_status_codes(lib):
    f = lib.loftr_model_lookup_host
    arrays, scal, out, args = _host_setup()
    assert _call(f, arrays, scal, out, args) == 0 and out["counts"][0] == 4 and out["counts"][3] == 0 and out["match"][:4].tolist() == [2, 12, 14, 15]
    assert _call(f, arrays, scal, out, dict(args, mask=None)) == 0 and out["counts"][4 + O.MASKED] == 0
    assert _call(f, arrays, scal, out, args, model_none=True) == BAD_ARG and _call(f, arrays, scal, out, args, out_none=True) == BAD_ARG
    for name in arrays:
        assert _call(f, dict(arrays, **{name: None}), scal, out, args) == BAD_ARG, name
    for name in out:
        assert _call(f, arrays, scal, dict(out, **{name: None}), args) == BAD_ARG, name
    for name in ("kpts_db", "kpts_q", "conf", "rows", "row_db", "row_query"):
        assert _call(f, arrays, scal, out, dict(args, **{name: None})) == BAD_ARG, name
    for name in ("M", "R", "Q"):
        assert _call(f, arrays, scal, out, dict(args, **{name: -1})) == BAD_ARG, name
    for name in ("K", "P", "n_images", "gh", "gw"):
        assert _call(f, arrays, dict(scal, **{name: -1}), out, args) == BAD_ARG, name
    # bad rows, queries, images; kp_offsets that do not start at 0, end at K and ascend
    edit = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]]).astype(a.dtype)
    for over in (dict(rows=edit(args["rows"], 15, 3)), dict(rows=edit(args["rows"], 0, -1)), dict(rows=edit(args["rows"], 5, 1)),
                 dict(row_query=np.array([0, 0, 2], np.int32)), dict(row_query=np.array([1, 0, 1], np.int32)),
                 dict(row_db=np.array([0, 2, 0], np.int32)), dict(row_db=np.array([-1, 0, 0], np.int32)), dict(Q=1), dict(R=2)):
        assert _call(f, arrays, scal, out, dict(args, **over)) == BAD_ARG, over
    for off in ([1, 3, 4], [0, 3, 5], [0, 5, 4]):
        assert _call(f, dict(arrays, kp_offsets=np.array(off, np.int64)), scal, out, args) == BAD_ARG, off
    # nothing to do: nothing is read
    none = dict(kpts_db=None, kpts_q=None, conf=None, rows=None, mask=None, M=0, row_db=None, row_query=None, R=0, Q=0)
    bare = {k: (out[k] if k in ("q_offsets", "counts") else None) for k in out}
    assert _call(f, arrays, scal, bare, none) == 0 and not out["counts"].any()
    # the limits are answered before a data pointer is read
    one = np.zeros(1, np.int64)
    wild = {k: one for k in arrays}
    for over in (dict(M=2 ** 31 - 1), dict(R=2 ** 31), dict(Q=2 ** 31)):
        assert _call(f, wild, scal, {k: one for k in out}, dict({k: (one if isinstance(v, np.ndarray) else v) for k, v in args.items()}, **over)) == UNSUPPORTED, over
    for over in (dict(P=2 ** 31), dict(K=2 ** 31), dict(gw=(1 << 24) + 1), dict(gh=1 << 16, gw=1 << 16)):
        assert _call(f, wild, dict(scal, **over), {k: one for k in out}, {k: (one if isinstance(v, np.ndarray) else v) for k, v in args.items()}) == UNSUPPORTED, over


def test_model_cells_status_codes(lib):
    case, *_ = MC.hand_case()
    m = case["model"]
    inv, gh, gw = O.grid(m["image_hw"], m["cell_px"])
    cell, status = np.zeros(4, np.int32), ctypes.c_int(-1)
    ok = dict(kp_offsets=_ptr(m["kp_offsets"]), n_images=2, keypoints=_ptr(m["keypoints"]), kp_point=_ptr(m["kp_point"]), K=4, P=2, gh=gh, gw=gw,
              inv=float(inv), kp_cell=_ptr(cell), status=ctypes.cast(ctypes.byref(status), ctypes.c_void_p))
    host = lambda **over: lib.loftr_model_cells_host(*{**ok, **over}.values())
    dev = lambda **over: lib.loftr_model_cells(*{**ok, **over}.values(), None)
    assert host() == 0 and status.value == 0 and cell.tolist() == [5, 40, 100, 5]
    assert host(P=1) == 0 and status.value == 32
    for f in (host, dev):                                                                # the kernel entry answers these before any device work
        for name in ("kp_offsets", "keypoints", "kp_point", "kp_cell", "status"):
            assert f(**{name: None}) == BAD_ARG, name
        for name in ("n_images", "K", "P", "gh", "gw"):
            assert f(**{name: -1}) == BAD_ARG, name
        assert f(K=2 ** 31) == UNSUPPORTED and f(P=2 ** 31) == UNSUPPORTED and f(gw=(1 << 24) + 1) == UNSUPPORTED
        assert f(gh=1 << 16, gw=1 << 16) == UNSUPPORTED
    assert host(kp_offsets=_ptr(np.array([0, 3, 5], np.int64))) == BAD_ARG and host(kp_offsets=_ptr(np.array([0, 5, 4], np.int64))) == BAD_ARG
    assert host(K=0, keypoints=None, kp_point=None, kp_cell=None, kp_offsets=_ptr(np.zeros(3, np.int64))) == 0 and status.value == 0


def test_kernel_entry_point_status_codes(lib):
    wsb, f = lib.loftr_model_lookup_workspace_bytes, lib.loftr_model_lookup
    assert wsb(-1, 2) == 0 and wsb(2, -1) == 0 and wsb(2 ** 31 - 1, 2) == 0 and wsb(2, 2 ** 31) == 0
    assert wsb(0, 0) > 0 and wsb(1000, 10) >= 2048 * 16 + 1000 * 8 + 10 * 4 and wsb(1000, 10 ** 6) >= wsb(1000, 10) + 4 * (10 ** 6 - 10)
    p = 1 << 20                                                                          # never read: every answer comes before device work
    arrays = dict(kp_offsets=p, kp_cell=p, kp_point=p, xyz=p)
    scal = dict(K=4, P=2, n_images=2, gh=19, gw=27, inv=0.5)
    out = {k: p for k, _ in _lib.ModelLookupOut._fields_}
    args = dict(kpts_db=p, kpts_q=p, conf=p, rows=p, mask=p, M=16, row_db=p, row_query=p, R=3, Q=2)

    def call(arrays=arrays, scal=scal, out=out, ws=p, ws_bytes=wsb(16, 2), **over):
        md, st = _lib.Model(**arrays, **scal), _lib.ModelLookupOut(**out)
        return f(ctypes.byref(md), *{**args, **over}.values(), ctypes.byref(st), ws, ws_bytes, None, None)

    assert call(ws_bytes=wsb(16, 2) - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE and call(ws=None) == BAD_ARG
    for name in arrays:
        assert call(arrays=dict(arrays, **{name: None})) == BAD_ARG, name
    for name in out:
        assert call(out=dict(out, **{name: None})) == BAD_ARG, name
    for name in ("kpts_db", "kpts_q", "conf", "rows", "row_db", "row_query"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("M", "R", "Q"):
        assert call(**{name: -1}) == BAD_ARG, name
    for name in ("K", "P", "n_images", "gh", "gw"):
        assert call(scal=dict(scal, **{name: -1})) == BAD_ARG, name
    big = 1 << 62
    assert call(M=2 ** 31 - 1, ws_bytes=big) == UNSUPPORTED and call(R=2 ** 31, ws_bytes=big) == UNSUPPORTED and call(Q=2 ** 31, ws_bytes=big) == UNSUPPORTED
    assert call(scal=dict(scal, P=2 ** 31)) == UNSUPPORTED and call(scal=dict(scal, K=2 ** 31)) == UNSUPPORTED
    assert call(scal=dict(scal, gw=(1 << 24) + 1)) == UNSUPPORTED
    md, st = _lib.Model(**arrays, **scal), _lib.ModelLookupOut(**out)
    assert f(None, *args.values(), ctypes.byref(st), p, big, None, None) == BAD_ARG and f(ctypes.byref(md), *args.values(), None, p, big, None, None) == BAD_ARG


def test_ops_refuses_wrong_dtypes_shapes_and_devices(lib):
    from loftr_amd import ops
    case, *_ = MC.hand_case()
    m, q = case["model"], case["q"]
    inv, gh, gw = O.grid(m["image_hw"], m["cell_px"])
    cell = np.array([5, 40, 100, 5], np.int32)
    good = [m["kp_offsets"], cell, m["kp_point"], m["xyz"], gh, gw, float(inv), q["kpts_db"], q["kpts_q"], q["conf"], q["rows"], q["mask"],
            q["row_db"], q["row_query"], 2]
    assert ops.model_lookup_host(*good)["counts"][0] == 4
    swap = lambda i, v: [v if j == i else g for j, g in enumerate(good)]
    for i, bad in ((0, good[0].astype(np.int32)), (1, cell.astype(np.int64)), (2, good[2].astype(np.int64)), (3, good[3].astype(np.float64)),
                   (7, good[7].astype(np.float64)), (8, good[8].astype(np.float64)), (9, good[9].astype(np.float64)), (10, good[10].astype(np.int64)),
                   (11, good[11].astype(bool)), (12, good[12].astype(np.int64)), (13, good[13].astype(np.int64))):
        with pytest.raises(_lib.LoftrHipError, match="must be"):
            ops.model_lookup_host(*swap(i, bad))
    for i, bad in ((0, good[0].reshape(1, 3)), (1, cell[:3]), (2, good[2][:3]), (3, good[3][:, :2]), (7, good[7][:5]), (8, good[8].reshape(-1)),
                   (9, good[9][:5]), (10, good[10][:5]), (11, good[11][:5]), (13, good[13][:2])):
        with pytest.raises(_lib.LoftrHipError, match="must be|expected k"):
            ops.model_lookup_host(*swap(i, bad))
    with pytest.raises(_lib.LoftrHipError, match="Q must be"):
        ops.model_lookup_host(*swap(14, -1))
    with pytest.raises(_lib.LoftrHipError, match="status -1"):
        ops.model_lookup_host(*swap(14, 1))
    t = lambda a: torch.from_numpy(a) if isinstance(a, np.ndarray) else a
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops.model_lookup_host(*[t(g) for g in good])
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):                            # the kernels take GPU tensors only
        ops.model_lookup(*[t(g) for g in good])
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):
        ops.model_cells(t(m["kp_offsets"]), t(m["keypoints"]), t(m["kp_point"]), 2, gh, gw, float(inv))
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops.model_cells_host(t(m["kp_offsets"]), t(m["keypoints"]), t(m["kp_point"]), 2, gh, gw, float(inv))
    with pytest.raises(_lib.LoftrHipError, match="must be"):
        ops.model_cells_host(m["kp_offsets"], m["keypoints"].astype(np.float64), m["kp_point"], 2, gh, gw, float(inv))
    with pytest.raises(_lib.LoftrHipError, match="expected keypoints"):
        ops.model_cells_host(m["kp_offsets"], m["keypoints"], m["kp_point"][:3], 2, gh, gw, float(inv))
