"""CPU checks of the correspondence-table entry points (csrc/register.hip, csrc/register_gpu.hip, added to ABI 25 without a bump): null
pointers, negative sizes, min_corr < 4 and a short workspace are answered with the documented status before any device work; the ops
wrappers refuse what the kernels cannot take; a library without the entry points is refused; mixed devices are an error."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _bundle_cases as BC
import _registration_cases as RC
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ("loftr_register_corr_host", "loftr_register_corr_workspace_bytes", "loftr_register_corr")


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
    assert build_mod.SOURCES.count("register.hip") == 1 and build_mod.SOURCES.count("register_gpu.hip") == 1
    assert "LOFTR_REGISTER_STAGES 4" in header and "LOFTR_REGISTER_RANK_BLOCK 256" in header
    assert len(ops.REGISTER_STAGES) == 4 and ops.REGISTER_COUNTS == 8 and ops.REGISTER_RANK_BLOCK == RC.RANK_BLOCK == 256 and ops.REGISTER_MIN_CORR == 4
    assert [b for b, _ in ops.REGISTER_ERRORS] == [1, 2, 4]
    assert loftr_amd.register_images is not None and loftr_amd.reconstruct_tracks is not None and loftr_amd.Reconstruction is not None
    assert loftr_amd.Registration.FIELDS == ("T_cam_from_world", "registered", "posed", "n_corr", "n_inliers", "cand_image", "cand_offsets", "corr_xyz",
                                             "corr_xy", "corr_obs", "corr_inlier")
    core = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "register_core.h")).read()
    assert "_core.h\"" not in core                                      # self-contained: none of the other *_core.h


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
    with pytest.raises(_lib.LoftrHipError, match="loftr_register_corr.*rebuild"):
        _lib.load()


def _host_args():
    h = RC.hand()
    N, n = len(h["obs_image"]), len(h["posed"])
    return dict(offsets=h["offsets"], T=len(h["offsets"]) - 1, obs_image=h["obs_image"], obs_xy=h["obs_xy"], N=N, xyz=h["xyz"], status=h["status"],
                posed=h["posed"], n_images=n, cam_offsets=h["cam_offsets"], cam_obs=h["cam_obs"], min_corr=4, n_corr=np.full(n, 9, np.int32),
                cand_rank=np.full(n, 9, np.int32), cand_image=np.full(n, 9, np.int32), cand_offsets=np.full(n + 1, 9, np.int64),
                corr_xyz=np.zeros((N, 3), np.float32), corr_xy=np.zeros((N, 2), np.float32), corr_bid=np.full(N, 9, np.int64),
                corr_obs=np.full(N, 9, np.int32), counts=np.full(8, 7, np.int64))


def _call(f, a, **over):
    vals = {**a, **over}
    return f(*[v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v for v in vals.values()])


def test_host_routine_status_codes(lib):
    f = lib.loftr_register_corr_host
    a = _host_args()
    assert _call(f, a) == 0
    assert a["counts"].tolist() == [9, 2, 0, 4, 3, 12, 5, 0] and a["n_corr"].tolist() == [0, 4, 3, 5, 0, 0]
    assert a["cand_image"].tolist() == [1, 3, 9, 9, 9, 9] and a["cand_offsets"].tolist() == [0, 4, 9, 9, 9, 9, 9]     # rows past P are not written
    assert a["corr_bid"][:9].tolist() == [0] * 4 + [1] * 5 and (a["corr_bid"][9:] == 9).all() and (a["corr_obs"][9:] == 9).all()
    for name in ("offsets", "obs_image", "obs_xy", "xyz", "status", "posed", "cam_offsets", "cam_obs", "n_corr", "cand_rank", "cand_image", "cand_offsets",
                 "corr_xyz", "corr_xy", "corr_bid", "corr_obs", "counts"):
        assert _call(f, a, **{name: None}) == BAD_ARG, name
    for name in ("T", "N", "n_images"):
        assert _call(f, a, **{name: -1}) == BAD_ARG, name
    for m in (3, 0, -1, -2 ** 31):
        assert _call(f, a, min_corr=m) == BAD_ARG, m
    assert _call(f, a, min_corr=2 ** 31 - 1) == 0
    # no track, no observation, no image: nothing is read
    e = _host_args()
    none = {k: None for k in ("obs_image", "obs_xy", "xyz", "status", "posed", "cam_obs", "n_corr", "cand_rank", "cand_image", "corr_xyz", "corr_xy",
                              "corr_bid", "corr_obs")}
    assert _call(f, e, T=0, N=0, n_images=0, offsets=np.zeros(1, np.int64), cam_offsets=np.zeros(1, np.int64), **none) == 0
    assert e["counts"].tolist() == [0] * 8 and e["cand_offsets"][0] == 0
    assert _call(f, e, T=0, offsets=np.zeros(1, np.int64)) == BAD_ARG                      # observations outside every track
    assert _call(f, e, n_images=0, cam_offsets=np.zeros(1, np.int64)) == BAD_ARG           # ... outside every image
    one = ctypes.c_void_p(1 << 20)                                                         # limits are answered before a pointer is read
    outs = (one,) * 9
    assert f(one, 2 ** 31, one, one, 4, one, one, one, 2, one, one, 4, *outs) == UNSUPPORTED
    assert f(one, 1, one, one, 2 ** 31, one, one, one, 2, one, one, 4, *outs) == UNSUPPORTED


def test_kernel_entry_point_status_codes(lib):
    wsb, f, p = lib.loftr_register_corr_workspace_bytes, lib.loftr_register_corr, 1 << 20
    assert wsb(-1, 2, 2) == 0 and wsb(1, -1, 2) == 0 and wsb(1, 2, -1) == 0 and wsb(2 ** 31, 2, 2) == 0 and wsb(1, 2 ** 31, 2) == 0
    assert wsb(0, 0, 0) > 0 and wsb(10, 3000, 10) >= 3000 * 5 and wsb(10, 30, 1000) >= 1000 * 4
    ok = dict(offsets=p, T=10, obs_image=p, obs_xy=p, N=30, xyz=p, status=p, posed=p, n_images=4, cam_offsets=p, cam_obs=p, min_corr=4, n_corr=p,
              cand_rank=p, cand_image=p, cand_offsets=p, corr_xyz=p, corr_xy=p, corr_bid=p, corr_obs=p, counts=p, ws=p, ws_bytes=wsb(10, 30, 4),
              stage_ms=None, stream=None)
    call = lambda **over: f(*{**ok, **over}.values())
    assert call(ws_bytes=ok["ws_bytes"] - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    for name in ("offsets", "obs_image", "obs_xy", "xyz", "status", "posed", "cam_offsets", "cam_obs", "n_corr", "cand_rank", "cand_image", "cand_offsets",
                 "corr_xyz", "corr_xy", "corr_bid", "corr_obs", "counts", "ws"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("T", "N", "n_images"):
        assert call(**{name: -1}) == BAD_ARG, name
    assert call(min_corr=3) == BAD_ARG and call(min_corr=-5) == BAD_ARG
    assert call(T=0) == BAD_ARG and call(n_images=0) == BAD_ARG                            # observations outside every track / image
    assert call(T=2 ** 31, ws_bytes=1 << 62) == UNSUPPORTED and call(N=2 ** 31, ws_bytes=1 << 62) == UNSUPPORTED


def test_ops_refuses_wrong_dtypes_shapes_and_devices(lib):
    h = RC.hand()
    good = [h[k] for k in RC.NAMES]
    out = ops.register_corr_host(*good, 4)
    assert out["counts"][2] == 0 and out["counts"][1] == 2
    swaps = {0: np.int32, 1: np.int64, 2: np.float64, 3: np.float64, 4: np.bool_, 5: np.bool_, 6: np.int32, 7: np.int64}
    for i, dt in swaps.items():
        with pytest.raises(_lib.LoftrHipError, match="must be"):
            ops.register_corr_host(*[g.astype(dt) if j == i else g for j, g in enumerate(good)], 4)
    shapes = {0: good[0].reshape(1, -1), 2: good[2][:3], 3: good[3][:1], 4: good[4][:3], 6: good[6][:2], 7: good[7][:3]}
    for i, bad in shapes.items():
        with pytest.raises(_lib.LoftrHipError, match="must be|expected offsets"):
            ops.register_corr_host(*[bad if j == i else g for j, g in enumerate(good)], 4)
    for m in (3, 4.0, True, None):
        with pytest.raises(ValueError, match="min_corr must be an integer >= 4"):
            ops.register_corr_host(*good, m)
    with pytest.raises(_lib.LoftrHipError, match="numpy arrays"):
        ops.register_corr_host(*[torch.from_numpy(g) for g in good], 4)
    with pytest.raises(_lib.LoftrHipError, match="GPU tensor"):                            # the kernels take GPU tensors only
        ops.register_corr(*[torch.from_numpy(g) for g in good], 4)


class _FakeGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: enough for the device check, which runs before any data is touched."""
    @property
    def is_cuda(self):
        return True


def test_mixed_devices_are_an_error(lib):
    s = BC.scene_a()
    T = len(s["offsets"]) - 1
    args = [torch.from_numpy(np.ascontiguousarray(a)) for a in (s["offsets"], s["obs_image"], s["obs_xy"], s["xyz"], np.zeros(T, np.uint8), s["K"],
                                                                 s["T_true"], np.zeros(5, bool))]
    for i in (0, 2, 4, 5, 7):
        mixed = list(args)
        mixed[i] = args[i].as_subclass(_FakeGpu)
        with pytest.raises(_lib.LoftrHipError, match="GPU and CPU arguments mixed.*no silent fallback"):
            loftr_amd.register_images(*mixed, min_corr=4, min_inliers=4)
    with pytest.raises(_lib.LoftrHipError, match="posed: GPU"):
        loftr_amd.register_images(*args[:7], args[7].as_subclass(_FakeGpu), min_corr=4, min_inliers=4)
    with pytest.raises(_lib.LoftrHipError, match="GPU and CPU arguments mixed.*K: GPU"):
        loftr_amd.reconstruct_tracks(args[0], args[1], args[2], args[5].as_subclass(_FakeGpu), (0, 1, np.eye(3), np.ones(3)), min_corr=4, min_inliers=4)
