"""CPU checks of the second shared library, libloftr_global.so (include/loftr_global.h; csrc/position.hip, csrc/position_gpu.hip): its
exports are exactly its header's; its binding matches; the first library, its binding and its ABI version are as before; every
per-item step of global positioning is one text for host and device; null pointers, negative sizes and parameters out of range are
answered with the documented status before any device work; a stale library is refused; the README names both libraries."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _position_cases as PC
import loftr_amd
from loftr_amd import _lib, _lib_global, _tracks, build as build_mod, ops_global

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_global_abi_version", "loftr_global_positions_host", "loftr_global_positions_workspace_bytes", "loftr_global_positions")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "loftr_amd", "csrc")
ARGS = ("offsets", "T", "obs_image", "obs_xy", "N", "cam_offsets", "cam_obs", "K", "R", "in_graph", "n_images", "root", "tree_image", "tree_t",
        "Et", "huber", "max_iters", "pcg_iters", "pcg_tol", "ftol", "min_cam_obs", "centres", "xyz", "depth_scale", "obs_state", "cam_state",
        "point_active", "counts", "info")
POINTERS = ("offsets", "obs_image", "obs_xy", "cam_offsets", "cam_obs", "K", "R", "in_graph", "tree_image", "tree_t", "centres", "xyz",
            "depth_scale", "obs_state", "cam_state", "point_active", "counts", "info")


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib_global.load()


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loftr_global.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(loftr_[a-z0-9_]+)\s*\(", src)))


def test_entry_points_are_exported_and_declared(lib):
    raw = ctypes.CDLL(_lib_global.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "loftr_global.h")).read()
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib_global.SIGNATURES and name + "(" in header, name
    assert "#define LOFTR_GLOBAL_ABI_VERSION 1" in header and lib.loftr_global_abi_version() == _lib_global.ABI_VERSION == 1
    assert f"#define LOFTR_POSITION_STAGES {len(ops_global.POSITION_STAGES)}" in header
    assert build_mod.GLOBAL_SOURCES == ["position.hip", "position_gpu.hip"] and build_mod.GLOBAL_LIB_PATH == _lib_global.LIB_PATH
    assert not set(build_mod.GLOBAL_SOURCES) & set(build_mod.SOURCES)
    assert ops_global.POSITION_COUNTS == 16 and [b for b, _ in ops_global.POSITION_ERRORS] == [1, 2, 4, 8, 16]
    assert loftr_amd.GlobalPositions.FIELDS[:6] == ("centres", "xyz", "depth_scale", "obs_state", "cam_state", "point_active")
    for m in ("global_positions", "reconstruct_global"):
        assert hasattr(loftr_amd.SfmResult, m)


def test_second_library_exports_exactly_its_header(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib_global.LIB_PATH], capture_output=True, text=True, check=True).stdout
    got = sorted({ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()})
    assert got == _declared() == sorted(NAMES) == sorted(_lib_global.SIGNATURES)
    # the binding's argument counts against the header's declarations
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loftr_global.h")).read(), flags=re.S)
    for name, (_, args) in _lib_global.SIGNATURES.items():
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1).strip()
        assert len(args) == (0 if params == "void" else params.count(",") + 1), name
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _lib_global.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "loftr_" not in undefined                                       # it links no object of the first library


def test_first_library_is_as_before():
    build_mod.build(verbose=False)
    lib1 = _lib.load()
    assert lib1.loftr_hip_abi_version() == _lib.ABI_VERSION == 25 and len(_lib.SIGNATURES) == 153
    assert not any(name.startswith("loftr_global") for name in _lib.SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert not any(hasattr(raw, name) for name in NAMES)
    assert "position.hip" not in build_mod.SOURCES and "position_gpu.hip" not in build_mod.SOURCES
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "153 entry points" in readme and "libloftr_global.so" in readme and "include/loftr_global.h" in readme


STEPS = ("track_check(", "cam_check(", "tree_check(", "start_tree_edge(", "tree_claim(", "tree_verify(", "obs_bearing(", "track_setup(", "cam_setup(",
         "point_start(", "obs_eval(", "obs_linearise(", "point_factor(", "point_u(", "cam_term_setup(", "cam_finish_setup(", "cam_term_Sp(",
         "cam_finish_Sp(", "cam_update(", "cam_direction(", "cam_apply(", "point_apply(", "obs_apply(", "cam_commit(", "point_commit(",
         "obs_commit(", "feed(", "accept(", "obs_write(", "track_write(", "cam_write(", "finish(")


def test_one_text_for_host_and_device():
    """the core header holds every per-item step and uses no function beyond sqrt"""
    core = open(os.path.join(CSRC, "position_core.h")).read()
    assert "#pragma clang fp contract(off)" in core and "ba::kLambda0" in core and "tracks::group_slot(" in core
    for fn in ("sin(", "cos(", "acos(", "asin(", "atan", "exp(", "pow(", "fma("):
        assert fn not in core, fn
    for f in ("position.hip", "position_gpu.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "position_core.h"' in text and "#pragma clang fp contract(off)" in text, f
        for step in STEPS:
            assert step in text, (f, step)
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))}
    for step in STEPS:
        fn = step[:-1]
        if fn in ("feed", "accept", "finish", "cam_check", "track_check", "track_setup", "cam_setup", "track_write", "cam_write",
                  "cam_update", "cam_apply", "cam_commit"):                                       # (names other stages use as well)
            continue
        assert [f for f, text in sources.items() if re.search(rf"\b{fn}\(const P& p", text)] == ["position_core.h"], fn
    gpu = sources["position_gpu.hip"]
    assert "hipGraph" not in gpu and "cooperative" not in gpu and "atomicAdd(double" not in gpu
    assert "position" not in "".join(build_mod.SOURCES)


def test_a_stale_second_library_is_refused(lib, monkeypatch):
    class Stale:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            if name == "loftr_global_positions":
                raise AttributeError(name)
            return getattr(self._real, name)

    real = ctypes.CDLL(_lib_global.LIB_PATH)
    monkeypatch.setattr(_lib_global, "_lib", None)
    monkeypatch.setattr(_lib_global.C, "CDLL", lambda path: Stale(real))
    with pytest.raises(_lib.LoftrHipError, match="loftr_global_positions.*predates this binding.*rebuild"):
        _lib_global.load()
    monkeypatch.setattr(_lib_global, "LIB_PATH", os.path.join(ROOT, "loftr_amd", "no_such_library.so"))
    with pytest.raises(_lib.LoftrHipError, match="not found: the HIP extension is not built"):
        _lib_global.load()


def _host_args():
    sc = PC.small()
    cam_offsets, cam_obs = _tracks.group_by_image(sc.obs_image, sc.n)
    T, N, n, Et = len(sc.offsets) - 1, len(sc.obs_image), sc.n, len(sc.tree_image)
    vals = dict(zip(ARGS[:21], [sc.offsets, T, sc.obs_image, sc.obs_xy, N, cam_offsets, cam_obs, sc.K, sc.R, sc.in_graph, n, sc.root,
                                sc.tree_image, np.ascontiguousarray(sc.tree_t), Et, 0.1, 3, 4, 1e-2, 1e-7, 8]))
    vals.update(centres=np.full((n, 3), 7.0), xyz=np.full((T, 3), 7.0, np.float32), depth_scale=np.full(N, 7.0), obs_state=np.full(N, 9, np.uint8),
                cam_state=np.full(n, 9, np.uint8), point_active=np.full(T, 9, np.uint8), counts=np.full(16, 7, np.int64), info=np.full(4, 7.0))
    assert tuple(vals) == ARGS
    return vals


def _call(f, a, **over):
    vals = {**a, **over}
    return f(*[v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v for v in vals.values()])


def test_host_routine_status_codes(lib):
    f = lib.loftr_global_positions_host
    a = _host_args()
    assert _call(f, a) == 0
    assert a["counts"][0] == 3 and a["counts"][1] == 0 and a["counts"][6] == 4 and a["cam_state"].tolist() == [3, 2, 2, 2, 2]
    for name in POINTERS:
        assert _call(f, a, **{name: None}) == BAD_ARG, name
    for name in ("T", "N", "Et", "n_images", "max_iters", "pcg_iters", "min_cam_obs"):
        assert _call(f, a, **{name: -1}) == BAD_ARG, name
    for name, v in (("huber", -1.0), ("huber", math.nan), ("huber", math.inf), ("pcg_tol", 1.0), ("pcg_tol", -0.1), ("ftol", -1.0), ("ftol", math.nan)):
        assert _call(f, a, **{name: v}) == BAD_ARG, (name, v)
    assert _call(f, a, n_images=0) == BAD_ARG and _call(f, a, T=0) == BAD_ARG                 # observations without tracks
    # a bad input: BAD_ARG, the bits in counts[1] and every other output zero
    a = _host_args()
    assert _call(f, a, root=5) == BAD_ARG and a["counts"].tolist() == [0, 8] + [0] * 14
    assert not a["centres"].any() and not a["xyz"].any() and not a["obs_state"].any() and not a["cam_state"].any() and not a["info"].any()
    one = ctypes.c_void_p(1 << 20)                                        # limits are answered before a pointer is read
    lim = lambda **over: f(*[{**{k: (one if k in POINTERS else v) for k, v in a.items()}, **over}[k] for k in ARGS])
    assert lim(N=2 ** 31) == UNSUPPORTED and lim(T=2 ** 31) == UNSUPPORTED and lim(Et=2 ** 31) == UNSUPPORTED
    assert lim(n_images=2 ** 30 + 1) == UNSUPPORTED and lim(max_iters=2 ** 16 + 1) == UNSUPPORTED and lim(pcg_iters=2 ** 16 + 1) == UNSUPPORTED


def test_kernel_entry_point_status_codes(lib):
    wsb, f, p = lib.loftr_global_positions_workspace_bytes, lib.loftr_global_positions, 1 << 20
    assert wsb(4, 8, 0, 1) == 0 and wsb(-1, 8, 2, 1) == 0 and wsb(4, -1, 2, 1) == 0 and wsb(4, 8, 2, -1) == 0 and wsb(4, 2 ** 31, 2, 1) == 0
    assert wsb(0, 0, 1, 0) > 0
    big = wsb(10 ** 5, 10 ** 6, 10 ** 4, 10 ** 4)                          # about 130 bytes per observation, 170 per point, 300 per image
    assert 120 * 10 ** 6 + 160 * 10 ** 5 + 280 * 10 ** 4 <= big <= 140 * 10 ** 6 + 180 * 10 ** 5 + 340 * 10 ** 4
    a = _host_args()
    ok = {k: (p if k in POINTERS else v) for k, v in a.items()}
    ok.update(ws=p, ws_bytes=wsb(ok["T"], ok["N"], ok["n_images"], ok["Et"]), stage_ms=None, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    assert call(ws_bytes=ok["ws_bytes"] - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    for name in POINTERS + ("ws",):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("T", "N", "Et", "n_images", "max_iters", "pcg_iters", "min_cam_obs"):
        assert call(**{name: -1}) == BAD_ARG, name
    assert call(huber=-1.0) == BAD_ARG and call(pcg_tol=1.0) == BAD_ARG and call(n_images=0) == BAD_ARG
    huge = dict(ws_bytes=1 << 62)
    assert call(N=2 ** 31, **huge) == UNSUPPORTED and call(n_images=2 ** 30 + 1, **huge) == UNSUPPORTED
    assert call(max_iters=2 ** 16 + 1, **huge) == UNSUPPORTED


def test_ops_refuses_wrong_dtypes_shapes_and_devices(lib):
    v = _host_args()
    good = [v[k] for k in ("offsets", "obs_image", "obs_xy", "cam_offsets", "cam_obs", "K", "R", "in_graph", "tree_image", "tree_t")]
    assert ops_global.global_positions_host(*good, 0, max_iters=2)["counts"][0] == 2
    swaps = {0: np.int32, 1: np.int64, 2: np.float64, 3: np.int32, 4: np.int64, 5: np.float32, 6: np.float32, 7: np.bool_, 8: np.int64, 9: np.float32}
    for i, dt in swaps.items():
        with pytest.raises(_lib.LoftrHipError, match="must be"):
            ops_global.global_positions_host(*[g.astype(dt) if j == i else g for j, g in enumerate(good)], 0)
    for i in (2, 3, 4, 5, 6, 9):
        with pytest.raises(_lib.LoftrHipError, match="must be|expected offsets"):
            ops_global.global_positions_host(*[g[:-1] if j == i else g for j, g in enumerate(good)], 0)
    for kw in (dict(max_iters=-1), dict(pcg_iters=True), dict(min_cam_obs=1.5)):
        with pytest.raises(ValueError, match="must be an integer"):
            ops_global.global_positions_host(*good, 0, **kw)
    with pytest.raises(ValueError, match="must be an integer"):
        ops_global.global_positions_host(*good, 0.5)
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops_global.global_positions_host(*[torch.from_numpy(g) for g in good], 0)
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):           # the kernels take GPU tensors only: no fallback
        ops_global.global_positions(*[torch.from_numpy(g) for g in good], 0)
