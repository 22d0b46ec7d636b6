"""CPU checks of the third shared library, libloftr_calib.so (include/loftr_calib.h; csrc/calib.hip, csrc/calib_gpu.hip): its exports
are exactly its header's; its binding matches; the first two libraries, their bindings and their ABI versions are as before; every
per-item step of view-graph calibration is one text for host and device; null pointers, negative sizes and parameters out of range
are answered with the documented status before any device work; a stale library is refused; the README names all three libraries."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _calibration_cases as CC
import loftr_amd
from loftr_amd import _lib, _lib_calib, _lib_global, build as build_mod, ops_calib

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_calib_abi_version", "loftr_calibrate_view_graph_host", "loftr_calibrate_view_graph_workspace_bytes",
         "loftr_calibrate_view_graph")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "loftr_amd", "csrc")
ARGS = ("edge_image", "edge_F", "edge_weight", "E", "pp", "f0", "group", "n_images", "n_groups", "grp_offsets", "grp_inc", "loss", "max_resid",
        "prior_weight", "weight_cap", "bound_lo", "bound_hi", "min_edges", "max_iters", "pcg_iters", "pcg_tol", "ftol", "focal_scale", "focal",
        "edge_resid", "edge_state", "group_state", "counts", "info")
POINTERS = ("edge_image", "edge_F", "edge_weight", "pp", "f0", "group", "grp_offsets", "grp_inc", "focal_scale", "focal", "edge_resid",
            "edge_state", "group_state", "counts", "info")


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib_calib.load()


def _header():
    return open(os.path.join(ROOT, "include", "loftr_calib.h")).read()


def _declared():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(loftr_[a-z0-9_]+)\s*\(", src)))


def test_entry_points_are_exported_and_declared(lib):
    raw = ctypes.CDLL(_lib_calib.LIB_PATH)
    header = _header()
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib_calib.SIGNATURES and name + "(" in header, name
    assert "#define LOFTR_CALIB_ABI_VERSION 1" in header and lib.loftr_calib_abi_version() == _lib_calib.ABI_VERSION == 1
    assert f"#define LOFTR_CALIB_STAGES {len(ops_calib.CALIB_STAGES)}" in header and ops_calib.CALIB_STAGES == ("check", "setup", "refine", "write")
    assert build_mod.CALIB_SOURCES == ["calib.hip", "calib_gpu.hip"] and build_mod.CALIB_LIB_PATH == _lib_calib.LIB_PATH
    assert not set(build_mod.CALIB_SOURCES) & set(build_mod.SOURCES + build_mod.GLOBAL_SOURCES)
    assert ops_calib.CALIB_COUNTS == 16 and [b for b, _ in ops_calib.CALIB_ERRORS] == [1, 2, 4, 8] and len(ops_calib.CALIB_NAMES) == 9
    assert len(ops_calib.CALIB_INFO) == 4 and len(ops_calib.CALIB_EDGE_STATES) == 3 and len(ops_calib.CALIB_GROUP_STATES) == 3
    assert ops_calib.CALIB_DEFAULTS == dict(loss=0.05, max_resid=0.05, prior_weight=1e-3, weight_cap=100, bound_lo=0.2, bound_hi=5.0, min_edges=1,
                                            max_iters=50, pcg_iters=30, pcg_tol=1e-2, ftol=1e-9)
    assert loftr_amd.ViewGraphCalibration.FIELDS[:5] == ("focal_scale", "focal", "edge_resid", "edge_state", "group_state")
    assert callable(loftr_amd.calibrate_view_graph)
    for m in ("pairwise_fundamentals", "calibrate", "reconstruct_uncalibrated"):
        assert hasattr(loftr_amd.SfmResult, m)
    doc = loftr_amd.calibrate_view_graph.__doc__ + loftr_amd.calibration.__doc__
    assert "UNVALIDATED" in doc and "UNVALIDATED" in header


def test_third_library_exports_exactly_its_header(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib_calib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    got = sorted({ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()})
    assert got == _declared() == sorted(NAMES) == sorted(_lib_calib.SIGNATURES)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)                  # the binding's argument counts against the declarations
    for name, (_, args) in _lib_calib.SIGNATURES.items():
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1).strip()
        assert len(args) == (0 if params == "void" else params.count(",") + 1), name
    assert len(_lib_calib.SIGNATURES["loftr_calibrate_view_graph_host"][1]) == len(ARGS)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _lib_calib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "loftr_" not in undefined                                       # it links no object of the other two libraries


def test_the_first_two_libraries_are_as_before():
    build_mod.build(verbose=False)
    lib1, lib2 = _lib.load(), _lib_global.load()
    assert lib1.loftr_hip_abi_version() == _lib.ABI_VERSION == 25 and len(_lib.SIGNATURES) == 153
    assert lib2.loftr_global_abi_version() == _lib_global.ABI_VERSION == 1 and len(_lib_global.SIGNATURES) == 4
    assert not any("calib" in name for name in list(_lib.SIGNATURES) + list(_lib_global.SIGNATURES))
    for path in (_lib.LIB_PATH, _lib_global.LIB_PATH):
        raw = ctypes.CDLL(path)
        assert not any(hasattr(raw, name) for name in NAMES)
    assert build_mod.GLOBAL_SOURCES == ["position.hip", "position_gpu.hip"] and "calib" not in "".join(build_mod.SOURCES + build_mod.GLOBAL_SOURCES)
    assert build_mod.build(verbose=False) == build_mod.LIB_PATH == _lib.LIB_PATH          # build() still returns the first library's path
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "153 entry points" in readme and "libloftr_global.so" in readme and "include/loftr_global.h" in readme
    assert "libloftr_calib.so" in readme and "include/loftr_calib.h" in readme


def test_staleness_lists():
    """the third library is stale against its own files only; its files are not in the first library's scan"""
    inc = os.path.join(ROOT, "include")
    newest = lambda files: max(os.path.getmtime(f) for f in files)
    own = [os.path.join(CSRC, f) for f in ("calib.hip", "calib_gpu.hip", "calib_core.h", "bundle_core.h", "tracks_core.h", "common.h", "stage_timer.h")]
    assert build_mod._deps_mtime(build_mod.CALIB_SOURCES) == newest(own + [os.path.join(inc, "loftr_calib.h"), os.path.join(inc, "loftr_hip.h")])
    first = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip")) and not f.startswith(("calib", "position"))]
    assert build_mod._deps_mtime(build_mod.SOURCES) == newest(first + [os.path.join(inc, "loftr_hip.h")])
    assert set(build_mod.CALIB_ONLY) == {"calib.hip", "calib_gpu.hip", "calib_core.h"}


STEPS = ("vg_edge_check(", "vg_image_check(", "vg_group_check(", "vg_slot_check(", "vg_edge_setup(", "vg_group_setup(", "vg_edge_eval(",
         "vg_group_eval(", "vg_edge_linearise(", "vg_term_setup(", "vg_group_finish_setup(", "vg_term_Ap(", "vg_group_finish_Ap(",
         "vg_group_update(", "vg_group_direction(", "vg_group_apply(", "vg_group_commit(", "vg_ctrl_init(", "vg_feed(", "vg_accept(",
         "vg_edge_write(", "vg_image_write(", "vg_group_write(", "vg_finish(", "vg_check_args(", "vg_problem(")


def test_one_text_for_host_and_device():
    """the core header holds every per-item step, and uses no function beyond sqrt"""
    core = open(os.path.join(CSRC, "calib_core.h")).read()
    assert "#pragma clang fp contract(off)" in core and "ba::kLambda0" in core and "tracks::span(" in core and "tracks::carve(" in core
    for fn in ("sin(", "cos(", "acos(", "asin(", "atan", "exp(", "pow(", "fma(", "log(", "cbrt(", "hypot(", "fabs(", "fmin(", "fmax("):
        assert fn not in core, fn
    called = set(re.findall(r"\b([a-z_0-9]+)\(", re.sub(r"//[^\n]*", "", core)))
    assert called & {"sqrt", "sin", "cos", "tan", "exp", "log", "pow", "fma", "cbrt", "hypot", "rsqrt", "floor", "ceil", "round"} == {"sqrt"}
    defined = set(re.findall(r"VG_HD [a-z_ ]*?\b(vg_[A-Za-z_0-9]+)\(", core)) | set(re.findall(r"inline [A-Za-z_ ]*?\b(vg_[A-Za-z_0-9]+)\(", core))
    assert {s[:-1] for s in STEPS} <= defined
    for f in ("calib.hip", "calib_gpu.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "calib_core.h"' in text and "#pragma clang fp contract(off)" in text, f
        for step in STEPS:
            assert step in text, (f, step)
    # every step has a name of its own: no other file of csrc/ defines or calls it, and the names other tests pin stay where they were
    others = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip")) and not f.startswith("calib")}
    assert not [f for f, text in others.items() if "vg_" in text or "calib_core.h" in text]
    mine = "".join(open(os.path.join(CSRC, f)).read() for f in ("calib_core.h", "calib.hip", "calib_gpu.hip"))
    for fn in ("edge_eval(const P& p", "start_edge", "node_rhs", "support_slot", "edge_verdict", "start_tree_edge", "obs_bearing", "cam_term_setup"):
        assert f" {fn}" not in mine, fn
    gpu = open(os.path.join(CSRC, "calib_gpu.hip")).read()
    assert "hipGraph" not in gpu and "cooperative" not in gpu and "atomicAdd(double" not in gpu and "__shfl_down" in gpu and "__ballot" in gpu


def test_a_stale_third_library_is_refused(lib, monkeypatch):
    class Stale:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            if name == "loftr_calibrate_view_graph":
                raise AttributeError(name)
            return getattr(self._real, name)

    real = ctypes.CDLL(_lib_calib.LIB_PATH)
    monkeypatch.setattr(_lib_calib, "_lib", None)
    monkeypatch.setattr(_lib_calib.C, "CDLL", lambda path: Stale(real))
    with pytest.raises(_lib.LoftrHipError, match="loftr_calibrate_view_graph.*predates this binding.*rebuild"):
        _lib_calib.load()
    monkeypatch.setattr(_lib_calib, "LIB_PATH", os.path.join(ROOT, "loftr_amd", "no_such_library.so"))
    with pytest.raises(_lib.LoftrHipError, match="not found: the HIP extension is not built"):
        _lib_calib.load()


def _host_args():
    sc = CC.small()
    a = CC.raw_args(sc)
    E, n, G = len(a[0]), sc.n, len(a[6]) - 1
    vals = dict(zip(ARGS[:22], [a[0], a[1], a[2], E, a[3], a[4], a[5], n, G, a[6], a[7], 0.05, 0.05, 1e-3, 100, 0.2, 5.0, 1, 3, 4, 1e-2, 1e-9]))
    vals.update(focal_scale=np.full(G, 7.0), focal=np.full(n, 7.0), edge_resid=np.full(E, 7.0), edge_state=np.full(E, 9, np.uint8),
                group_state=np.full(G, 9, np.uint8), counts=np.full(16, 7, np.int64), info=np.full(4, 7.0))
    assert tuple(vals) == ARGS
    return vals


def _call(f, a, **over):
    vals = {**a, **over}
    return f(*[v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v for v in vals.values()])


def test_host_routine_status_codes(lib):
    f = lib.loftr_calibrate_view_graph_host
    a = _host_args()
    assert _call(f, a) == 0
    assert a["counts"][0] == 3 and a["counts"][1] == 0 and a["counts"][4] == 10 and a["counts"][5] == 5 and a["group_state"].tolist() == [2] * 5
    for name in POINTERS:
        assert _call(f, a, **{name: None}) == BAD_ARG, name
    for name in ("E", "n_images", "n_groups", "weight_cap", "min_edges", "max_iters", "pcg_iters"):
        assert _call(f, a, **{name: -1}) == BAD_ARG, name
    for name, v in (("loss", 0.0), ("loss", -1.0), ("loss", math.nan), ("loss", math.inf), ("max_resid", -1.0), ("max_resid", math.nan),
                    ("prior_weight", -1.0), ("prior_weight", math.inf), ("weight_cap", 0), ("bound_lo", 0.0), ("bound_lo", 1.0), ("bound_lo", math.nan),
                    ("bound_hi", 1.0), ("bound_hi", math.inf), ("bound_hi", math.nan), ("pcg_tol", 1.0), ("pcg_tol", -0.1), ("ftol", -1.0),
                    ("ftol", math.nan)):
        assert _call(f, a, **{name: v}) == BAD_ARG, (name, v)
    assert _call(f, a, n_images=0) == BAD_ARG and _call(f, a, n_groups=0) == BAD_ARG and _call(f, a, n_groups=6) == BAD_ARG
    # a bad input: BAD_ARG, the bits in counts[1] and every other output zero
    a = _host_args()
    f0 = a["f0"].copy()
    f0[2] = -1.0
    assert _call(f, a, f0=f0) == BAD_ARG and a["counts"].tolist() == [0, 8] + [0] * 14
    assert not any(a[k].any() for k in ("focal_scale", "focal", "edge_resid", "edge_state", "group_state", "info"))
    # no edges: the edge pointers may be null
    a = _host_args()
    none = dict(E=0, edge_image=None, edge_F=None, edge_weight=None, grp_inc=None, edge_resid=None, edge_state=None, grp_offsets=np.zeros(6, np.int64))
    assert _call(f, a, **none) == 0 and a["counts"].tolist() == [0] * 7 + [3] + [0] * 8 and np.array_equal(a["focal"], a["f0"])
    one = ctypes.c_void_p(1 << 20)                                        # limits are answered before a pointer is read
    lim = lambda **over: f(*[{**{k: (one if k in POINTERS else v) for k, v in a.items()}, **over}[k] for k in ARGS])
    assert lim(E=2 ** 30) == UNSUPPORTED and lim(n_images=2 ** 30 + 1, n_groups=7) == UNSUPPORTED
    assert lim(max_iters=2 ** 16 + 1) == UNSUPPORTED and lim(pcg_iters=2 ** 16 + 1) == UNSUPPORTED


def test_kernel_entry_point_status_codes(lib):
    wsb, f, p = lib.loftr_calibrate_view_graph_workspace_bytes, lib.loftr_calibrate_view_graph, 1 << 20
    assert wsb(-1, 2, 2) == 0 and wsb(4, 0, 1) == 0 and wsb(4, 2, 0) == 0 and wsb(4, 2, 3) == 0 and wsb(2 ** 30, 2, 2) == 0
    assert wsb(4, 2 ** 30 + 1, 2) == 0 and wsb(0, 1, 1) > 0
    big = wsb(10 ** 6, 10 ** 5, 10 ** 5)                                   # about 130 bytes per edge and 90 per group
    assert 128 * 10 ** 6 + 85 * 10 ** 5 <= big <= 136 * 10 ** 6 + 100 * 10 ** 5
    a = _host_args()
    ok = {k: (p if k in POINTERS else v) for k, v in a.items()}
    ok.update(ws=p, ws_bytes=wsb(ok["E"], ok["n_images"], ok["n_groups"]), stage_ms=None, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    assert call(ws_bytes=ok["ws_bytes"] - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    for name in POINTERS + ("ws",):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("E", "n_images", "n_groups", "weight_cap", "min_edges", "max_iters", "pcg_iters"):
        assert call(**{name: -1}) == BAD_ARG, name
    assert call(loss=0.0) == BAD_ARG and call(pcg_tol=1.0) == BAD_ARG and call(bound_lo=1.5) == BAD_ARG and call(n_groups=6) == BAD_ARG
    huge = dict(ws_bytes=1 << 62)
    assert call(E=2 ** 30, **huge) == UNSUPPORTED and call(n_images=2 ** 30 + 1, **huge) == UNSUPPORTED
    assert call(max_iters=2 ** 16 + 1, **huge) == UNSUPPORTED


def test_ops_refuses_wrong_dtypes_shapes_and_devices(lib):
    good = CC.raw_args(CC.small())
    assert ops_calib.calibrate_view_graph_host(*good, max_iters=2)["counts"][0] == 2
    swaps = {0: np.int64, 1: np.float32, 2: np.int64, 3: np.float32, 4: np.float32, 5: np.int64, 6: np.int32, 7: np.int64}
    for i, dt in swaps.items():
        with pytest.raises(_lib.LoftrHipError, match="must be"):
            ops_calib.calibrate_view_graph_host(*[g.astype(dt) if j == i else g for j, g in enumerate(good)])
    for i in (1, 2, 3, 5, 7):
        with pytest.raises(_lib.LoftrHipError, match="must be|expected edge_image"):
            ops_calib.calibrate_view_graph_host(*[g[:-1] if j == i else g for j, g in enumerate(good)])
    for kw in (dict(max_iters=-1), dict(pcg_iters=True), dict(min_edges=1.5), dict(weight_cap=0)):
        with pytest.raises(ValueError, match="must be an integer"):
            ops_calib.calibrate_view_graph_host(*good, **kw)
    with pytest.raises(TypeError, match="unknown parameter"):
        ops_calib.calibrate_view_graph_host(*good, huber=1.0)
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops_calib.calibrate_view_graph_host(*[torch.from_numpy(g) for g in good])
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):           # the kernels take GPU tensors only: no fallback
        ops_calib.calibrate_view_graph(*[torch.from_numpy(g) for g in good])
