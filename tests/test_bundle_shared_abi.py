"""CPU checks of the grouped-focal entry points (csrc/bundle.hip, csrc/bundle_gpu.hip; added to ABI 25 without a bump):
null pointers, negative sizes, bad parameters, bad groupings and a short workspace are answered with the documented status before any
device work; the ops wrappers refuse what the kernels cannot take; a library without the entry points is refused; mixed devices are an
error."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _bundle_cases as BC
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_bundle_adjust_shared_host", "loftr_bundle_adjust_shared_workspace_bytes", "loftr_bundle_adjust_shared")


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
    host, dev, focal = (_lib.SIGNATURES[n][1] for n in (NAMES[0], NAMES[2], "loftr_bundle_adjust_focal_host"))
    assert len(host) == len(focal) + 5 and dev == host + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert ops.BUNDLE_COUNTS == 16 and [b for b, _ in ops.BUNDLE_SHARED_ERRORS] == [1, 2, 4, 8] and ops.BUNDLE_SHARED_ERRORS[:3] == ops.BUNDLE_ERRORS
    assert ops.bundle_adjust_shared_host is not None and ops.bundle_adjust_shared is not None
    assert f"{len(_lib.SIGNATURES)} entry points" in open(os.path.join(root, "README.md")).read()


def test_a_library_without_the_shared_entry_points_is_refused(lib, monkeypatch):
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
    with pytest.raises(_lib.LoftrHipError, match="loftr_bundle_adjust_shared.*rebuild"):
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
                group_cams=np.array([0, 2, 1], np.int32), G=2, huber=0.0, max_iters=5, pcg_iters=10, pcg_tol=1e-2, ftol=1e-9, min_focal_obs=3,
                focal_lo=0.5, focal_hi=2.0, T_out=np.zeros((3, 4, 4)), xyz_out=np.zeros((2, 3), np.float32), obs_active=np.full(6, 9, np.uint8),
                cam_free=np.full(3, 9, np.uint8), point_active=np.full(2, 9, np.uint8), K_out=np.zeros((3, 3, 3)), cam_focal=np.full(3, 9, np.uint8),
                group_focal=np.full(2, 9, np.uint8), counts=np.full(16, 7, np.int64))


def _call(f, a, **over):
    vals = {**a, **over}
    return f(*[v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v for v in vals.values()])


def test_host_routine_status_codes(lib):
    f = lib.loftr_bundle_adjust_shared_host
    a = _host_args()
    assert _call(f, a) == 0
    c = a["counts"].tolist()
    assert c[0] in (0, 1, 2) and c[1] == 0 and c[5:8] == [6, 2, 2] and c[13:] == [2, 1, 0]
    assert a["obs_active"].tolist() == [1] * 6 and a["cam_free"].tolist() == [0, 1, 1] and a["point_active"].tolist() == [1, 1]
    assert a["cam_focal"].tolist() == [1, 0, 1] and a["group_focal"].tolist() == [1, 0] and np.isfinite(a["K_out"]).all()
    assert np.array_equal(a["K_out"][1].view(np.uint64), a["K"][1].view(np.uint64))                  # body 1 holds two observations: too few
    assert np.array_equal(a["T_out"][0].view(np.uint64), a["Tcw"][0].view(np.uint64))                # the fixed pose comes back bit for bit
    reals = a["counts"][8:13].view(np.float64)
    assert reals[1] <= reals[0] and np.isfinite(reals).all()
    b = _host_args()
    assert _call(f, b, min_focal_obs=5) == 0 and b["cam_focal"].tolist() == [0, 0, 0] and b["counts"][13:].tolist() == [0, 0, 0]
    assert np.array_equal(b["K_out"].view(np.uint64), b["K"].view(np.uint64))
    for name in ("offsets", "obs_image", "obs_xy", "obs_mask", "xyz", "K", "Tcw", "fixed", "refine", "cam_offsets", "cam_obs", "cam_group",
                 "group_offsets", "group_cams", "T_out", "xyz_out", "obs_active", "cam_free", "point_active", "K_out", "cam_focal", "group_focal",
                 "counts"):
        assert _call(f, a, **{name: None}) == BAD_ARG, name
    for name in ("T", "N", "n_images", "G"):
        assert _call(f, a, **{name: -1}) == BAD_ARG, name
    for over in (dict(G=0), dict(G=4), dict(huber=-1.0), dict(huber=float("nan")), dict(max_iters=-1), dict(max_iters=1001), dict(pcg_iters=0),
                 dict(pcg_iters=201), dict(pcg_tol=1.0), dict(pcg_tol=float("nan")), dict(ftol=-1.0), dict(ftol=float("nan")),
                 dict(min_focal_obs=0), dict(min_focal_obs=-1), dict(focal_lo=1.0), dict(focal_hi=1.0), dict(focal_lo=float("nan")),
                 dict(focal_hi=float("nan")), dict(focal_lo=float("-inf")), dict(focal_hi=float("inf")), dict(focal_lo=2.0, focal_hi=0.5)):
        assert _call(f, a, **over) == BAD_ARG, over
    # the four error bits
    assert _call(f, a, obs_image=np.array([0, 3, 2, 0, 1, 2], np.int32)) == BAD_ARG
    assert _call(f, a, offsets=np.array([0, 4, 3], np.int64)) == BAD_ARG
    assert _call(f, a, cam_obs=np.array([3, 0, 1, 4, 2, 5], np.int32)) == BAD_ARG and _call(f, a, cam_offsets=np.array([0, 1, 4, 6], np.int64)) == BAD_ARG
    i32, i64 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.int64))
    for over in (dict(cam_group=i32(0, 1, 1)), dict(cam_group=i32(0, 2, 0)), dict(cam_group=i32(0, -1, 0)), dict(group_cams=i32(2, 0, 1)),
                 dict(group_cams=i32(0, 3, 1)), dict(group_cams=i32(0, -1, 1)), dict(group_cams=i32(0, 0, 1)), dict(group_offsets=i64(0, 1, 3)),
                 dict(group_offsets=i64(0, 3, 3)), dict(group_offsets=i64(0, 0, 3)), dict(group_offsets=i64(1, 2, 3)), dict(group_offsets=i64(0, 2, 2)),
                 dict(group_offsets=i64(0, 1 << 40, 3)), dict(cam_group=i32(1, 0, 1), group_cams=i32(1, 0, 2), group_offsets=i64(0, 1, 3))):
        assert _call(f, a, **over) == BAD_ARG, over
    # no track, no observation, no image: nothing is read
    e = _host_args()
    none = {k: None for k in ("obs_image", "obs_xy", "obs_mask", "xyz", "K", "Tcw", "fixed", "refine", "cam_obs", "cam_group", "group_cams", "T_out",
                              "xyz_out", "obs_active", "cam_free", "point_active", "K_out", "cam_focal", "group_focal")}
    zero = np.zeros(1, np.int64)
    assert _call(f, e, T=0, N=0, n_images=0, G=0, offsets=zero, cam_offsets=zero, group_offsets=zero, **none) == 0
    assert e["counts"].tolist()[:8] == [3, 0, 0, 0, 0, 0, 0, 0] and e["counts"][13:].tolist() == [0, 0, 0]
    assert _call(f, e, T=0, offsets=zero) == BAD_ARG
    one = ctypes.c_void_p(1 << 20)                                                         # limits are answered before a pointer is read
    rest = (0.0, 5, 10, 1e-2, 1e-9, 1, 0.5, 2.0, one, one, one, one, one, one, one, one, one)
    assert f(one, 2 ** 31, one, one, one, 2, one, one, one, one, one, 2, one, one, one, one, one, 1, *rest) == UNSUPPORTED
    assert f(one, 1, one, one, one, 2 ** 31, one, one, one, one, one, 2, one, one, one, one, one, 1, *rest) == UNSUPPORTED


def test_kernel_entry_point_status_codes(lib):
    wsb, f, p = lib.loftr_bundle_adjust_shared_workspace_bytes, lib.loftr_bundle_adjust_shared, 1 << 20
    assert wsb(-1, 2, 2) == 0 and wsb(1, -1, 2) == 0 and wsb(1, 2, -1) == 0 and wsb(2 ** 31, 2, 2) == 0 and wsb(1, 2 ** 31, 2) == 0
    assert wsb(0, 0, 0) > 0 and wsb(1000, 30, 10) >= 1000 * 208 and wsb(10, 3000, 10) >= 3000 * 4
    focal = lib.loftr_bundle_adjust_focal_workspace_bytes
    per_image = 8 * (7 + 2) + 4                                                            # seven group vectors, the factor twice, a count
    assert wsb(10, 30, 1024) - focal(10, 30, 1024) == 1024 * per_image + 256               # (and the scalars of the groups' sums)
    ok = dict(offsets=p, T=10, obs_image=p, obs_xy=p, obs_mask=p, N=30, xyz=p, K=p, Tcw=p, fixed=p, refine=p, n_images=4, cam_offsets=p, cam_obs=p,
              cam_group=p, group_offsets=p, group_cams=p, G=2, huber=0.0, max_iters=5, pcg_iters=10, pcg_tol=1e-2, ftol=1e-9, min_focal_obs=20,
              focal_lo=0.5, focal_hi=2.0, T_out=p, xyz_out=p, obs_active=p, cam_free=p, point_active=p, K_out=p, cam_focal=p, group_focal=p,
              counts=p, ws=p, ws_bytes=wsb(10, 30, 4), class_ms=None, class_launches=None, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    assert call(ws_bytes=ok["ws_bytes"] - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    assert call(ws_bytes=focal(10, 30, 4)) == WORKSPACE                                    # the per-image workspace is too short
    for name in ("offsets", "obs_image", "obs_xy", "obs_mask", "xyz", "K", "Tcw", "fixed", "refine", "cam_offsets", "cam_obs", "cam_group",
                 "group_offsets", "group_cams", "T_out", "xyz_out", "obs_active", "cam_free", "point_active", "K_out", "cam_focal", "group_focal",
                 "counts", "ws"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("T", "N", "n_images", "G"):
        assert call(**{name: -1}) == BAD_ARG, name
    for over in (dict(G=0), dict(G=5), dict(huber=-1.0), dict(max_iters=1001), dict(pcg_iters=0), dict(pcg_tol=1.0), dict(ftol=float("inf")),
                 dict(min_focal_obs=0), dict(focal_lo=1.0), dict(focal_hi=1.0), dict(focal_lo=float("nan")), dict(focal_hi=float("inf"))):
        assert call(**over) == BAD_ARG, over
    assert call(T=0) == BAD_ARG and call(n_images=0) == BAD_ARG
    assert call(T=2 ** 31, ws_bytes=1 << 62) == UNSUPPORTED and call(N=2 ** 31, ws_bytes=1 << 62) == UNSUPPORTED


def _ops_args():
    a = _host_args()
    return [a[k] for k in ("offsets", "obs_image", "obs_xy", "obs_mask", "xyz", "K", "Tcw", "fixed", "cam_offsets", "cam_obs", "refine", "cam_group",
                           "group_offsets", "group_cams")]


def test_ops_refuses_wrong_dtypes_shapes_and_devices(lib):
    good, par = _ops_args(), (0.0, 5, 10, 1e-2, 1e-9, 3, 0.5, 2.0)
    out = ops.bundle_adjust_shared_host(*good, *par)
    assert out["counts"][1] == 0 and out["cam_focal"].tolist() == [1, 0, 1] and out["group_focal"].tolist() == [1, 0] and out["counts"][14] == 1
    assert list(out) == ["T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active", "K", "cam_focal", "group_focal", "counts"]
    swaps = {0: np.int32, 1: np.int64, 2: np.float64, 3: np.bool_, 4: np.float64, 5: np.float32, 6: np.float32, 7: np.bool_, 8: np.int32, 9: np.int64,
             10: np.bool_, 11: np.int64, 12: np.int32, 13: np.int64}
    for i, dt in swaps.items():
        with pytest.raises(_lib.LoftrHipError, match="must be"):
            ops.bundle_adjust_shared_host(*[g.astype(dt) if j == i else g for j, g in enumerate(good)], *par)
    shapes = {0: good[0].reshape(1, 3), 2: good[2][:3], 5: good[5][:, :2], 7: good[7][:1], 8: good[8][:2], 10: good[10][:1], 11: good[11][:2],
              12: np.zeros(1, np.int64), 13: good[13][:2], }
    for i, bad in shapes.items():
        with pytest.raises(_lib.LoftrHipError, match="must be|expected offsets"):
            ops.bundle_adjust_shared_host(*[bad if j == i else g for j, g in enumerate(good)], *par)
    with pytest.raises(_lib.LoftrHipError, match="expected offsets"):                      # more groups than images
        ops.bundle_adjust_shared_host(*[np.arange(5, dtype=np.int64) if j == 12 else g for j, g in enumerate(good)], *par)
    with pytest.raises(_lib.LoftrHipError, match="group the images by camera"):            # the host routine's own refusal names the rule
        ops.bundle_adjust_shared_host(*[np.array([2, 0, 1], np.int32) if j == 13 else g for j, g in enumerate(good)], *par)
    with pytest.raises(ValueError, match="huber_px and ftol must be"):
        ops.bundle_adjust_shared_host(*good, 0.0, 5, 0, 1e-2, 1e-9, 2, 0.5, 2.0)
    for bad in ((0, 0.5, 2.0), (2, 1.0, 2.0), (2, 0.5, 1.0), (2, float("nan"), 2.0), (2, 0.5, float("inf")), (True, 0.5, 2.0)):
        with pytest.raises(ValueError, match="min_focal_obs must be an integer >= 1"):
            ops.bundle_adjust_shared_host(*good, 0.0, 5, 10, 1e-2, 1e-9, *bad)
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops.bundle_adjust_shared_host(*[torch.from_numpy(g) for g in good], *par)
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):                            # the kernels take GPU tensors only
        ops.bundle_adjust_shared(*[torch.from_numpy(g) for g in good], *par)


class _FakeGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: enough for the device check, which runs before any data is touched."""
    @property
    def is_cuda(self):
        return True


def test_mixed_devices_are_an_error(lib):
    s = BC.scene_a()
    args = [torch.from_numpy(np.ascontiguousarray(a)) for a in BC.inputs(s)]
    ids = torch.zeros(5, dtype=torch.int64)
    for i in (0, 2, 4, 6):
        mixed = list(args)
        mixed[i] = args[i].as_subclass(_FakeGpu)
        with pytest.raises(_lib.LoftrHipError, match="GPU and CPU arguments mixed.*no silent fallback"):
            loftr_amd.bundle_adjust(*mixed, refine_focal=True, camera_ids=ids)
    with pytest.raises(ValueError, match="camera_ids is on the GPU.*no silent fallback"):
        loftr_amd.bundle_adjust(*args, refine_focal=True, camera_ids=ids.as_subclass(_FakeGpu))
    with pytest.raises(ValueError, match="camera_ids is on the CPU.*no silent fallback"):
        loftr_amd.bundle_adjust(*[a.as_subclass(_FakeGpu) for a in args], refine_focal=True, camera_ids=ids)
