"""CPU checks of the radial entry points (csrc/bundle.hip, csrc/bundle_gpu.hip, csrc/undistort.hip, csrc/undistort_gpu.hip; DESIGN §18.4;
added to ABI 25 without a bump): the exports, null pointers, negative sizes, bad parameters and a short workspace are answered with the
documented status before any device work; the workspace query; the ops wrappers refuse what the kernels cannot take; a library without the
entry points is refused; mixed devices are an error; the README carries the number of entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _bundle_cases as BC
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_bundle_adjust_radial_host", "loftr_bundle_adjust_radial_workspace_bytes", "loftr_bundle_adjust_radial",
         "loftr_undistort_points_host", "loftr_undistort_points", "loftr_distort_points_host")


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def test_entry_points_are_exported_and_declared(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "loftr_hip.h")).read()
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert lib.loftr_hip_abi_version() == _lib.ABI_VERSION == 25
    host, dev, shared = (_lib.SIGNATURES[n][1] for n in (NAMES[0], NAMES[2], "loftr_bundle_adjust_shared_host"))
    assert len(host) == len(shared) + 7 and dev == host + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert ops.BUNDLE_COUNTS == 16 and ops.UNDISTORT_COUNTS == 8 and [b for b, _ in ops.UNDISTORT_ERRORS] == [1]
    assert f"{len(_lib.SIGNATURES)} entry points" in open(os.path.join(root, "README.md")).read()
    assert loftr_amd.undistort_points is not None and loftr_amd.distort_points is not None


def test_a_library_without_the_radial_entry_points_is_refused(lib, monkeypatch):
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
    with pytest.raises(_lib.LoftrHipError, match="loftr_bundle_adjust_radial.*rebuild"):
        _lib.load()


def _host_args():
    """Three cameras one unit apart, two tracks of three observations each; camera 0 keeps its pose; cameras 0 and 2 are one body."""
    K = np.tile(np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]), (3, 1, 1))
    Tcw = np.tile(np.eye(4), (3, 1, 1))
    Tcw[1, 0, 3], Tcw[2, 0, 3] = -1.0, -2.0
    return dict(offsets=np.array([0, 3, 6], np.int64), T=2, obs_image=np.array([0, 1, 2, 0, 1, 2], np.int32),
                obs_xy=np.array([[382.5, 271.25], [257.5, 271.25], [132.5, 271.25], [320, 240], [195, 240], [70, 240]], np.float32),
                obs_mask=np.ones(6, np.uint8), N=6, xyz=np.array([[0.5, 0.25, 4.0], [0, 0, 4.1]], np.float32), K=K, Tcw=Tcw,
                fixed=np.array([1, 0, 0], np.uint8), refine=np.array([1, 1, 1], np.uint8), n_images=3, cam_offsets=np.array([0, 2, 4, 6], np.int64),
                cam_obs=np.array([0, 3, 1, 4, 2, 5], np.int32), cam_group=np.array([0, 1, 0], np.int32), group_offsets=np.array([0, 2, 3], np.int64),
                group_cams=np.array([0, 2, 1], np.int32), G=2, radial=np.array([0.0, 0.01, 0.0]), refine_radial=np.array([1, 1, 0], np.uint8),
                huber=0.0, max_iters=5, pcg_iters=10, pcg_tol=1e-2, ftol=1e-9, min_focal_obs=2, focal_lo=0.5, focal_hi=2.0, radial_lo=-1.0,
                radial_hi=1.0, T_out=np.zeros((3, 4, 4)), xyz_out=np.zeros((2, 3), np.float32), obs_active=np.full(6, 9, np.uint8),
                cam_free=np.full(3, 9, np.uint8), point_active=np.full(2, 9, np.uint8), K_out=np.zeros((3, 3, 3)), cam_focal=np.full(3, 9, np.uint8),
                group_focal=np.full(2, 9, np.uint8), radial_out=np.full(3, 9.0), cam_radial=np.full(3, 9, np.uint8),
                group_radial=np.full(2, 9, np.uint8), counts=np.full(16, 7, np.int64))


def _call(f, a, **over):
    vals = {**a, **over}
    return f(*[v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v for v in vals.values()])


POINTERS = ("offsets", "obs_image", "obs_xy", "obs_mask", "xyz", "K", "Tcw", "fixed", "refine", "cam_offsets", "cam_obs", "cam_group",
            "group_offsets", "group_cams", "radial", "refine_radial", "T_out", "xyz_out", "obs_active", "cam_free", "point_active", "K_out",
            "cam_focal", "group_focal", "radial_out", "cam_radial", "group_radial", "counts")


def test_host_routine_status_codes(lib):
    f = lib.loftr_bundle_adjust_radial_host
    a = _host_args()
    assert _call(f, a) == 0
    c = a["counts"].tolist()
    assert c[0] in (0, 1, 2) and c[1] == 0 and c[5:8] == [6, 2, 2] and c[13:] == [3, 2, 2]
    assert a["cam_focal"].tolist() == [1, 1, 1] and a["group_focal"].tolist() == [1, 1]
    # body 0 = images 0 and 2: only image 0 is flagged, its two observations reach min_focal_obs = 2; body 1 = image 1 likewise
    assert a["cam_radial"].tolist() == [1, 1, 0] and a["group_radial"].tolist() == [1, 1]
    assert np.array_equal(a["radial_out"][2:].view(np.uint64), a["radial"][2:].view(np.uint64)) and np.isfinite(a["radial_out"]).all()
    assert np.array_equal(a["T_out"][0].view(np.uint64), a["Tcw"][0].view(np.uint64))
    b = _host_args()
    assert _call(f, b, min_focal_obs=3) == 0                                               # body 0 holds 4 observations, 2 of them flagged for radial
    assert b["group_focal"].tolist() == [1, 0] and b["group_radial"].tolist() == [0, 0] and b["cam_radial"].tolist() == [0, 0, 0]
    assert b["counts"][13:].tolist() == [2, 1, 0] and np.array_equal(b["radial_out"].view(np.uint64), b["radial"].view(np.uint64))
    for name in POINTERS:
        assert _call(f, a, **{name: None}) == BAD_ARG, name
    for name in ("T", "N", "n_images", "G"):
        assert _call(f, a, **{name: -1}) == BAD_ARG, name
    for over in (dict(G=0), dict(G=4), dict(huber=-1.0), dict(max_iters=1001), dict(pcg_iters=0), dict(pcg_tol=1.0), dict(ftol=-1.0),
                 dict(min_focal_obs=0), dict(focal_lo=1.0), dict(focal_hi=float("inf")), dict(radial_lo=float("nan")), dict(radial_hi=float("nan")),
                 dict(radial_lo=float("-inf")), dict(radial_hi=float("inf")), dict(radial_lo=0.5, radial_hi=-0.5)):
        assert _call(f, a, **over) == BAD_ARG, over
    assert _call(f, a, radial_lo=0.0, radial_hi=0.0) == 0                                  # an empty interval is a legal bound
    # the error bits
    assert _call(f, a, obs_image=np.array([0, 3, 2, 0, 1, 2], np.int32)) == BAD_ARG
    assert _call(f, a, offsets=np.array([0, 4, 3], np.int64)) == BAD_ARG
    assert _call(f, a, cam_obs=np.array([3, 0, 1, 4, 2, 5], np.int32)) == BAD_ARG
    assert _call(f, a, cam_group=np.array([0, 1, 1], np.int32)) == BAD_ARG and _call(f, a, group_cams=np.array([2, 0, 1], np.int32)) == BAD_ARG
    # no track, no observation, no image: nothing is read
    e = _host_args()
    none = {k: None for k in POINTERS if k not in ("offsets", "cam_offsets", "group_offsets", "counts")}
    zero = np.zeros(1, np.int64)
    assert _call(f, e, T=0, N=0, n_images=0, G=0, offsets=zero, cam_offsets=zero, group_offsets=zero, **none) == 0
    assert e["counts"].tolist()[:8] == [3, 0, 0, 0, 0, 0, 0, 0] and e["counts"][13:].tolist() == [0, 0, 0]
    one = ctypes.c_void_p(1 << 20)                                                         # limits are answered before a pointer is read
    rest = (one, one, 0.0, 5, 10, 1e-2, 1e-9, 1, 0.5, 2.0, -1.0, 1.0, one, one, one, one, one, one, one, one, one, one, one, one)
    assert f(one, 2 ** 31, one, one, one, 2, one, one, one, one, one, 2, one, one, one, one, one, 1, *rest) == UNSUPPORTED


def test_kernel_entry_point_status_codes_and_the_workspace_query(lib):
    wsb, f, p = lib.loftr_bundle_adjust_radial_workspace_bytes, lib.loftr_bundle_adjust_radial, 1 << 20
    assert wsb(-1, 2, 2) == 0 and wsb(1, -1, 2) == 0 and wsb(1, 2, -1) == 0 and wsb(2 ** 31, 2, 2) == 0 and wsb(1, 2 ** 31, 2) == 0
    shared = lib.loftr_bundle_adjust_shared_workspace_bytes
    assert wsb(0, 0, 0) > shared(0, 0, 0) and wsb(10, 30, 1024) > shared(10, 30, 1024)
    # per image beyond §18.2's: U 36 - 28 twice, eight 8-wide vectors instead of 7-wide ones (gc, x, r, zc, p, Sp: six), five group vectors a
    # second time, the group block and its factor (6 instead of 1), k and the group's step in both states
    per_image = 8 * (2 * 8 + 6 + 5 + 5 + 2 + 2)
    assert wsb(10, 30, 1024) - shared(10, 30, 1024) == 1024 * per_image + 256              # (and the radial counter)
    assert wsb(10, 30, 4) == wsb(10, 30, 4) and wsb(1000, 30, 10) > wsb(10, 30, 10)
    ok = dict(offsets=p, T=10, obs_image=p, obs_xy=p, obs_mask=p, N=30, xyz=p, K=p, Tcw=p, fixed=p, refine=p, n_images=4, cam_offsets=p, cam_obs=p,
              cam_group=p, group_offsets=p, group_cams=p, G=2, radial=p, refine_radial=p, huber=0.0, max_iters=5, pcg_iters=10, pcg_tol=1e-2,
              ftol=1e-9, min_focal_obs=20, focal_lo=0.5, focal_hi=2.0, radial_lo=-1.0, radial_hi=1.0, T_out=p, xyz_out=p, obs_active=p, cam_free=p,
              point_active=p, K_out=p, cam_focal=p, group_focal=p, radial_out=p, cam_radial=p, group_radial=p, counts=p, ws=p,
              ws_bytes=wsb(10, 30, 4), class_ms=None, class_launches=None, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    assert call(ws_bytes=ok["ws_bytes"] - 1) == WORKSPACE and call(ws_bytes=shared(10, 30, 4)) == WORKSPACE
    for name in POINTERS + ("ws",):
        assert call(**{name: None}) == BAD_ARG, name
    for over in (dict(T=-1), dict(G=0), dict(G=5), dict(huber=-1.0), dict(pcg_iters=0), dict(min_focal_obs=0), dict(focal_lo=1.0),
                 dict(radial_lo=float("nan")), dict(radial_hi=float("inf")), dict(radial_lo=1.0, radial_hi=-1.0)):
        assert call(**over) == BAD_ARG, over
    assert call(T=2 ** 31, ws_bytes=1 << 62) == UNSUPPORTED


def test_undistort_status_codes(lib):
    K, k = np.tile(np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]), (2, 1, 1)), np.array([-0.1, 0.1])
    xy, image = np.array([[330, 250], [100, 80], [320, 240]], np.float32), np.array([0, 1, 1], np.int32)
    out, ok, counts = np.full((3, 2), 9, np.float32), np.full(3, 9, np.uint8), np.full(8, 7, np.int64)
    ptr = lambda v: v.ctypes.data_as(ctypes.c_void_p) if v is not None else None
    for f in (lib.loftr_undistort_points_host, lib.loftr_distort_points_host):
        assert f(ptr(xy), ptr(image), 3, ptr(K), ptr(k), 2, ptr(out), ptr(ok), ptr(counts)) == 0
        assert counts.tolist() == [3, 0, 0, 0, 0, 0, 0, 0] and ok.tolist() == [1, 1, 1] and out[2].tolist() == [320.0, 240.0]
        args = [xy, image, 3, K, k, 2, out, ok, counts]
        for i in (0, 1, 3, 4, 6, 7, 8):
            bad = [None if j == i else (ptr(v) if isinstance(v, np.ndarray) else v) for j, v in enumerate(args)]
            assert f(*bad) == BAD_ARG, i
        assert f(ptr(xy), ptr(image), -1, ptr(K), ptr(k), 2, ptr(out), ptr(ok), ptr(counts)) == BAD_ARG
        assert f(ptr(xy), ptr(image), 3, ptr(K), ptr(k), -1, ptr(out), ptr(ok), ptr(counts)) == BAD_ARG
        assert f(None, None, 0, None, None, 0, None, None, ptr(counts)) == 0 and counts.tolist() == [0] * 8
    g = lib.loftr_undistort_points
    assert g(None, ptr(image), 3, ptr(K), ptr(k), 2, ptr(out), ptr(ok), ptr(counts), None) == BAD_ARG
    assert g(ptr(xy), ptr(image), 3, ptr(K), ptr(k), 2, ptr(out), ptr(ok), None, None) == BAD_ARG
    assert g(ptr(xy), ptr(image), -1, ptr(K), ptr(k), 2, ptr(out), ptr(ok), ptr(counts), None) == BAD_ARG


def _ops_args():
    a = _host_args()
    return [a[k] for k in ("offsets", "obs_image", "obs_xy", "obs_mask", "xyz", "K", "Tcw", "fixed", "cam_offsets", "cam_obs", "refine", "cam_group",
                           "group_offsets", "group_cams", "radial", "refine_radial")]


def test_ops_refuses_wrong_dtypes_shapes_and_devices(lib):
    good, par = _ops_args(), (0.0, 5, 10, 1e-2, 1e-9, 2, 0.5, 2.0, -1.0, 1.0)
    out = ops.bundle_adjust_radial_host(*good, *par)
    assert out["counts"][1] == 0 and out["cam_radial"].tolist() == [1, 1, 0] and out["group_radial"].tolist() == [1, 1] and out["counts"][15] == 2
    assert list(out) == ["T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active", "K", "cam_focal", "group_focal", "radial",
                         "cam_radial", "group_radial", "counts"]
    for i, dt in {14: np.float32, 15: np.bool_, 10: np.bool_, 12: np.int32}.items():
        with pytest.raises(_lib.LoftrHipError, match="must be"):
            ops.bundle_adjust_radial_host(*[g.astype(dt) if j == i else g for j, g in enumerate(good)], *par)
    for i, bad in {14: good[14][:2], 15: good[15][:1], 11: good[11][:2]}.items():
        with pytest.raises(_lib.LoftrHipError, match="must be|expected offsets"):
            ops.bundle_adjust_radial_host(*[bad if j == i else g for j, g in enumerate(good)], *par)
    for bad in ((float("nan"), 1.0), (-1.0, float("inf")), (0.5, -0.5), (True, 1.0)):
        with pytest.raises(ValueError, match="radial bounds must be finite"):
            ops.bundle_adjust_radial_host(*good, *par[:8], *bad)
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops.bundle_adjust_radial_host(*[torch.from_numpy(g) for g in good], *par)
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):                            # the kernels take GPU tensors only
        ops.bundle_adjust_radial(*[torch.from_numpy(g) for g in good], *par)
    K, k = good[5][:2], np.array([-0.1, 0.1])
    xy, image = np.array([[330, 250], [100, 80]], np.float32), np.array([0, 1], np.int32)
    assert ops.undistort_points_host(xy, image, K, k)["counts"].tolist()[:3] == [2, 0, 0]
    for bad in ((xy.astype(np.float64), image, K, k), (xy, image.astype(np.int64), K, k), (xy, image, K.astype(np.float32), k),
                (xy, image, K, k.astype(np.float32)), (xy[:, :1], image, K, k), (xy, image[:1], K, k), (xy, image, K, k[:1])):
        with pytest.raises(_lib.LoftrHipError, match="must be|expected xy"):
            ops.undistort_points_host(*bad)
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):
        ops.undistort_points(*[torch.from_numpy(x) for x in (xy, image, K, k)])
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops.undistort_points_host(*[torch.from_numpy(x) for x in (xy, image, K, k)])


class _FakeGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: enough for the device check, which runs before any data is touched."""
    @property
    def is_cuda(self):
        return True


def test_mixed_devices_are_an_error(lib):
    s = BC.scene_a()
    args = [torch.from_numpy(np.ascontiguousarray(a)) for a in BC.inputs(s)]
    mask, k = torch.ones(5, dtype=torch.bool), torch.zeros(5, dtype=torch.float64)
    for i in (0, 2, 5):
        mixed = list(args)
        mixed[i] = args[i].as_subclass(_FakeGpu)
        with pytest.raises(_lib.LoftrHipError, match="GPU and CPU arguments mixed.*no silent fallback"):
            loftr_amd.bundle_adjust(*mixed, refine_focal=True, refine_radial=True)
    with pytest.raises(ValueError, match="refine_radial is on the GPU.*no silent fallback"):
        loftr_amd.bundle_adjust(*args, refine_focal=True, refine_radial=mask.as_subclass(_FakeGpu))
    with pytest.raises(ValueError, match="radial is on the GPU.*no silent fallback"):
        loftr_amd.bundle_adjust(*args, refine_focal=True, refine_radial=True, radial=k.as_subclass(_FakeGpu))
    with pytest.raises(ValueError, match="radial is on the CPU.*no silent fallback"):
        loftr_amd.bundle_adjust(*[a.as_subclass(_FakeGpu) for a in args], refine_focal=True, refine_radial=True, radial=k)
    xy, image, K = torch.zeros(3, 2), torch.zeros(3, dtype=torch.int32), torch.eye(3, dtype=torch.float64).repeat(5, 1, 1)
    for i in range(4):
        u = [xy, image, K, k]
        u[i] = u[i].as_subclass(_FakeGpu)
        with pytest.raises(_lib.LoftrHipError, match="GPU and CPU arguments mixed.*no silent fallback"):
            loftr_amd.undistort_points(*u)
