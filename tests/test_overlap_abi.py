"""CPU checks of the view-overlap entry points (csrc/overlap.hip, csrc/overlap_gpu.hip, added to ABI 25 without a bump): the exports;
null pointers, negative sizes, parameters out of range and a short workspace are answered with the documented status before any device
work; the workspace query is 0 for sizes out of range; ops.view_overlap refuses what the routines cannot take; mixed devices are an
error; a library without the entry points is refused."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _overlap_cases as OC
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_view_overlap_host", "loftr_view_overlap_workspace_bytes", "loftr_view_overlap")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


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
    assert build_mod.SOURCES.count("overlap.hip") == 1 and build_mod.SOURCES.count("overlap_gpu.hip") == 1
    assert "LOFTR_OVERLAP_STAGES 3" in header and "LOFTR_OVERLAP_TILE 256" in header
    assert len(ops.OVERLAP_STAGES) == 3 and ops.OVERLAP_COUNTS == 8 and ops.OVERLAP_NAMES[1] == "error_bits"
    assert [b for b, _ in ops.OVERLAP_ERRORS] == [1, 2]
    assert loftr_amd.view_overlap is not None and loftr_amd.Overlap.FIELDS == ("overlap", "n_vis")
    assert loftr_amd.select_pairs is not None and loftr_amd.select_database is not None
    assert hasattr(loftr_amd.Reconstruction, "propose_pairs") and hasattr(loftr_amd.LocalizationModel, "propose_for_poses")
    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
    core = open(os.path.join(csrc, "overlap_core.h")).read()
    assert '#include "triangulate_core.h"' in core and "#pragma clang fp contract(off)" in core
    for src in ("overlap.hip", "overlap_gpu.hip"):                                       # both sides compile the one text
        assert '#include "overlap_core.h"' in open(os.path.join(csrc, src)).read()
    assert f"{len(_lib.SIGNATURES)} entry points" in open(os.path.join(ROOT, "README.md")).read()


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
    with pytest.raises(_lib.LoftrHipError, match="loftr_view_overlap.*rebuild"):
        _lib.load()


def _host_args():
    c = OC.scene_a()
    n, m = len(c["src_ok"]), len(c["tgt_ok"])
    return dict(vis_offsets=c["vis_offsets"], vis_point=c["vis_point"], V=len(c["vis_point"]), xyz=c["xyz"], point_ok=c["point_ok"], T=len(c["xyz"]),
                K_src=c["K_src"], T_src=c["T_src"], src_ok=c["src_ok"], n=n, K_tgt=c["K_tgt"], T_tgt=c["T_tgt"], tgt_ok=c["tgt_ok"],
                tgt_hw=c["tgt_hw"], m=m, border_px=c["border"], cos_min=c["cos_min"], max_scale2=c["max_scale2"],
                overlap=np.full((n, m), 9, np.int32), n_vis=np.full(n, 9, np.int32), counts=np.full(8, 7, np.int64))


def _call(f, a, **over):
    vals = {**a, **over}
    return f(*[v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v for v in vals.values()])


def test_host_routine_status_codes(lib):
    f = lib.loftr_view_overlap_host
    a = _host_args()
    assert _call(f, a) == 0
    assert a["counts"][1] == 0 and a["counts"][2] == 5 and a["counts"][5:].tolist() == [0, 0, 0] and (a["overlap"] != 9).all() and (a["n_vis"] != 9).all()
    for name in ("vis_offsets", "vis_point", "xyz", "point_ok", "K_src", "T_src", "src_ok", "K_tgt", "T_tgt", "tgt_ok", "tgt_hw", "overlap", "n_vis",
                 "counts"):
        assert _call(f, a, **{name: None}) == BAD_ARG, name
    for name in ("V", "T", "n", "m"):
        assert _call(f, a, **{name: -1}) == BAD_ARG, name
    for over in (dict(border_px=-1.0), dict(border_px=NAN), dict(border_px=INF), dict(cos_min=1.5), dict(cos_min=-1.5), dict(cos_min=NAN),
                 dict(max_scale2=0.99), dict(max_scale2=NAN), dict(max_scale2=-INF)):
        assert _call(f, a, **over) == BAD_ARG, over
    for over in (dict(border_px=0.0), dict(cos_min=1.0), dict(cos_min=-1.0), dict(max_scale2=1.0), dict(max_scale2=INF)):
        assert _call(f, a, **over) == 0, over
    # no source, no target, no entry, no point: nothing is read
    none = {k: None for k in ("vis_offsets", "vis_point", "xyz", "point_ok", "K_src", "T_src", "src_ok", "K_tgt", "T_tgt", "tgt_ok", "tgt_hw",
                              "overlap", "n_vis")}
    assert _call(f, a, V=0, T=0, n=0, m=0, **none) == 0 and a["counts"].tolist() == [0] * 8
    assert _call(f, a, n=0) == BAD_ARG                                                     # entries outside every list
    one = ctypes.c_void_p(1 << 20)                                                         # limits are answered before a pointer is read
    lim = lambda **over: f(*{**dict(vis_offsets=one, vis_point=one, V=4, xyz=one, point_ok=one, T=4, K_src=one, T_src=one, src_ok=one, n=2, K_tgt=one,
                                    T_tgt=one, tgt_ok=one, tgt_hw=one, m=2, border_px=0.0, cos_min=0.5, max_scale2=4.0, overlap=one, n_vis=one,
                                    counts=one), **over}.values())
    assert lim(V=2 ** 31) == UNSUPPORTED and lim(T=2 ** 31) == UNSUPPORTED and lim(n=2 ** 16, m=2 ** 15 + 1) == UNSUPPORTED


def test_kernel_entry_point_status_codes(lib):
    wsb, f, p = lib.loftr_view_overlap_workspace_bytes, lib.loftr_view_overlap, 1 << 20
    assert wsb(-1, 2) == 0 and wsb(2, -1) == 0 and wsb(2 ** 16, 2 ** 15 + 1) == 0
    assert wsb(0, 0) > 0 and wsb(806, 806) >= 2 * 806 * 224 and wsb(2 ** 16, 2 ** 15) > 0
    ok = dict(vis_offsets=p, vis_point=p, V=30, xyz=p, point_ok=p, T=10, K_src=p, T_src=p, src_ok=p, n=4, K_tgt=p, T_tgt=p, tgt_ok=p, tgt_hw=p, m=3,
              border_px=0.0, cos_min=0.5, max_scale2=4.0, overlap=p, n_vis=p, counts=p, ws=p, ws_bytes=wsb(4, 3), stage_ms=None, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    assert call(ws_bytes=ok["ws_bytes"] - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    for name in ("vis_offsets", "vis_point", "xyz", "point_ok", "K_src", "T_src", "src_ok", "K_tgt", "T_tgt", "tgt_ok", "tgt_hw", "overlap", "n_vis",
                 "counts", "ws"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("V", "T", "n", "m"):
        assert call(**{name: -1}) == BAD_ARG, name
    for over in (dict(border_px=-0.5), dict(border_px=NAN), dict(border_px=INF), dict(cos_min=1.01), dict(cos_min=NAN), dict(max_scale2=0.5),
                 dict(max_scale2=NAN)):
        assert call(**over) == BAD_ARG, over
    assert call(n=0) == BAD_ARG                                                            # entries outside every list
    big = dict(ws_bytes=1 << 62)
    assert call(V=2 ** 31, **big) == UNSUPPORTED and call(T=2 ** 31, **big) == UNSUPPORTED
    assert call(n=2 ** 16, m=2 ** 15 + 1, **big) == UNSUPPORTED and call(n=1, m=256 * 65535 + 1, **big) == UNSUPPORTED


def test_ops_refuses_wrong_dtypes_shapes_and_parameters(lib):
    good = OC.tensors(OC.scene_a())
    out = ops.view_overlap(*good)
    assert out["counts"][1] == 0 and out["overlap"].dtype == torch.int32 and out["n_vis"].dtype == torch.int32 and out["counts"].dtype == torch.int64
    swaps = {0: torch.int32, 1: torch.int64, 2: torch.float64, 3: torch.bool, 4: torch.float32, 5: torch.float32, 6: torch.bool, 7: torch.float32,
             8: torch.float32, 9: torch.int32, 10: torch.float32}
    for i, dt in swaps.items():
        with pytest.raises(_lib.LoftrHipError, match="must be"):
            ops.view_overlap(*[g.to(dt) if j == i else g for j, g in enumerate(good)])
    shapes = {0: good[0].reshape(1, -1), 2: good[2][:, :2], 3: good[3][:3], 4: good[4].reshape(-1, 3, 3), 5: good[5][:3], 6: good[6][:3], 8: good[8][:3],
              9: good[9][:3], 10: good[10][:3]}
    for i, bad in shapes.items():
        with pytest.raises(_lib.LoftrHipError, match="must be|expected vis_offsets"):
            ops.view_overlap(*[bad if j == i else g for j, g in enumerate(good)])
    with pytest.raises(_lib.LoftrHipError, match="must be a tensor"):
        ops.view_overlap(good[0].numpy(), *good[1:])
    for i, bad in ((11, -1.0), (11, NAN), (11, INF), (12, 1.5), (12, NAN), (13, 0.5), (13, NAN)):
        with pytest.raises(ValueError, match="border_px must be finite"):
            ops.view_overlap(*[bad if j == i else g for j, g in enumerate(good)])
    with pytest.raises(ValueError, match="entries without a source"):
        ops.view_overlap(torch.zeros(1, dtype=torch.int64), good[1], good[2], good[3], *[g[:0] for g in good[4:7]], *good[7:])
    n, m = 2 ** 16, 2 ** 15 + 1                                                            # refused from the shapes alone: there is no sparse output
    f64, u8 = torch.zeros((1, 1), dtype=torch.float64), torch.zeros(1, dtype=torch.uint8)
    with pytest.raises(ValueError, match="beyond the supported 2\\^31"):
        ops.view_overlap(torch.zeros(1, dtype=torch.int64).expand(n + 1), good[1][:0], good[2], good[3], f64.expand(n, 9), f64.expand(n, 16),
                         u8.expand(n), f64.expand(m, 9), f64.expand(m, 16), u8.expand(m), f64.expand(m, 2), 0.0, 0.5, 4.0)


class _FakeGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: enough for the device check, which runs before any data is touched."""
    @property
    def is_cuda(self):
        return True


def test_mixed_devices_are_an_error(lib):
    good = OC.tensors(OC.scene_a())
    for i in (0, 2, 5, 10):
        mixed = list(good)
        mixed[i] = good[i].as_subclass(_FakeGpu)
        with pytest.raises(_lib.LoftrHipError, match="GPU and CPU arguments mixed.*no silent fallback"):
            ops.view_overlap(*mixed)
        with pytest.raises(_lib.LoftrHipError, match="GPU and CPU arguments mixed.*no silent fallback"):
            loftr_amd.view_overlap(*mixed[:11])
