"""CPU checks of the entry points with position priors (csrc/bundle.hip, csrc/bundle_gpu.hip; added to ABI 25 without a
bump): exports, the ctypes and ops tables, a mode out of range, null prior pointers, what is ignored below a mode, the workspace size."""
import ctypes
import os

import numpy as np
import pytest

from loftr_amd import _lib, build as build_mod, ops

BAD_ARG, UNSUPPORTED = -1, -2
NAMES = ("loftr_bundle_adjust_prior_host", "loftr_bundle_adjust_prior_workspace_bytes", "loftr_bundle_adjust_prior")


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
    # the grouped pair's list plus prior_xyz, prior_sigma, prior_mask, mode and cam_prior
    assert len(host) == len(shared) + 5 and dev == host + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert host[18:22] == [ctypes.c_void_p] * 3 + [ctypes.c_int] and _lib.SIGNATURES[NAMES[1]][1] == [ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int]
    assert ops.BUNDLE_COUNTS == 16 and ops.BUNDLE_PRIOR_COUNTS == 24
    # the one mode table: the number of each mode in the prior pair; the radial mode takes no priors
    assert {call: row[4] for call, row in ops._BA_MODES.items()} == {"bundle_adjust": 0, "bundle_adjust_focal": 1, "bundle_adjust_shared": 2,
                                                                      "bundle_adjust_radial": None}
    assert [k for k, *_ in ops._BA_PRIOR_IN] == ["prior_xyz", "prior_sigma", "prior_mask"] and [k for k, *_ in ops._BA_PRIOR_OUT] == ["cam_prior"]
    assert ops.bundle_adjust_prior_host is not None and ops.bundle_adjust_prior is not None


def _host_args():
    """Three cameras one unit apart, two tracks of three observations each; camera 0 keeps its pose; cameras 0 and 2 are one body; every
    camera has a measured position 0.1 off its centre."""
    K = np.tile(np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]), (3, 1, 1))
    Tcw = np.tile(np.eye(4), (3, 1, 1))
    Tcw[1, 0, 3], Tcw[2, 0, 3] = -1.0, -2.0
    return dict(offsets=np.array([0, 3, 6], np.int64), T=2, obs_image=np.array([0, 1, 2, 0, 1, 2], np.int32),
                obs_xy=np.array([[382.5, 271.25], [257.5, 271.25], [132.5, 271.25], [320, 240], [195, 240], [70, 240]], np.float32),
                obs_mask=np.ones(6, np.uint8), N=6, xyz=np.array([[0.5, 0.25, 4.0], [0, 0, 4.1]], np.float32), K=K, Tcw=Tcw,
                fixed=np.array([1, 0, 0], np.uint8), refine=np.array([1, 1, 1], np.uint8), n_images=3, cam_offsets=np.array([0, 2, 4, 6], np.int64),
                cam_obs=np.array([0, 3, 1, 4, 2, 5], np.int32), cam_group=np.array([0, 1, 0], np.int32), group_offsets=np.array([0, 2, 3], np.int64),
                group_cams=np.array([0, 2, 1], np.int32), G=2, prior_xyz=np.array([[0.1, 0, 0], [1.1, 0, 0], [2.0, 0.1, 0]]),
                prior_sigma=np.full((3, 3), 0.05), prior_mask=np.ones(3, np.uint8), mode=2, huber=0.0, max_iters=5, pcg_iters=10, pcg_tol=1e-2,
                ftol=1e-9, min_focal_obs=3, focal_lo=0.5, focal_hi=2.0, T_out=np.zeros((3, 4, 4)), xyz_out=np.zeros((2, 3), np.float32),
                obs_active=np.full(6, 9, np.uint8), cam_free=np.full(3, 9, np.uint8), point_active=np.full(2, 9, np.uint8), K_out=np.zeros((3, 3, 3)),
                cam_focal=np.full(3, 9, np.uint8), group_focal=np.full(2, 9, np.uint8), cam_prior=np.full(3, 9, np.uint8),
                counts=np.full(24, 7, np.int64))


def _call(f, a, **over):
    vals = {**a, **over}
    return f(*[v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v for v in vals.values()])


FOCAL_ARGS = ("refine", "K_out", "cam_focal")
GROUP_ARGS = ("cam_group", "group_offsets", "group_cams", "group_focal")


def test_host_routine_status_codes(lib):
    f = lib.loftr_bundle_adjust_prior_host
    for mode in (0, 1, 2):
        a = _host_args()
        assert _call(f, a, mode=mode) == 0
        c = a["counts"].tolist()
        assert c[0] in (0, 1, 2) and c[1] == 0 and c[5:8] == [6, 2, 2] and c[16] == 2 and c[21:] == [0, 0, 0]
        assert a["cam_free"].tolist() == [0, 1, 1] and a["cam_prior"].tolist() == [0, 1, 1]          # the fixed camera has no prior
        reals = a["counts"][17:21].view(np.float64)
        # the two priors are 0.1 off: cost (0.1 / 0.05)^2 each, rms 0.1 (the centres are -(-1) and -(-2): exact)
        assert abs(reals[0] - 8.0) <= 1e-12 and abs(reals[2] - 0.1) <= 1e-15 and reals[1] < reals[0] and reals[3] < reals[2]
        assert np.array_equal(a["T_out"][0].view(np.uint64), a["Tcw"][0].view(np.uint64))
        # min_focal_obs = 3: no single image has three observations (mode 1), the body of images 0 and 2 has four (mode 2)
        assert c[13:16] == ([0, 0, 0], [0, 0, 0], [2, 1, 0])[mode]
        # what the mode does not use is ignored and may be null; what it uses may not
        ignored = (FOCAL_ARGS + GROUP_ARGS, GROUP_ARGS, ())[mode]
        b = _host_args()
        assert _call(f, b, mode=mode, **{k: None for k in ignored}, **({"G": -5, "min_focal_obs": 0} if mode == 0 else {})) == 0
        assert b["counts"].tolist() == c and b["T_out"].tobytes() == a["T_out"].tobytes()
        for name in set(FOCAL_ARGS + GROUP_ARGS) - set(ignored):
            assert _call(f, a, mode=mode, **{name: None}) == BAD_ARG, (mode, name)
        for name in ("prior_xyz", "prior_sigma", "prior_mask", "cam_prior", "counts", "offsets", "fixed", "T_out"):
            assert _call(f, a, mode=mode, **{name: None}) == BAD_ARG, (mode, name)
    a = _host_args()
    for mode in (-1, 3, 7):
        assert _call(f, a, mode=mode) == BAD_ARG, mode
    assert _call(f, a, max_iters=1001) == BAD_ARG and _call(f, a, huber=-1.0) == BAD_ARG and _call(f, a, T=-1) == BAD_ARG
    assert _call(f, a, obs_image=np.array([0, 3, 2, 0, 1, 2], np.int32)) == BAD_ARG                       # the error bits are the mode's
    # n_images = 0: the prior pointers may be null
    e = _host_args()
    e.update(T=0, N=0, n_images=0, G=0, offsets=np.zeros(1, np.int64), cam_offsets=np.zeros(1, np.int64), group_offsets=np.zeros(1, np.int64))
    assert _call(f, e, prior_xyz=None, prior_sigma=None, prior_mask=None, cam_prior=None) == 0
    assert e["counts"][0] == 3 and not e["counts"][1:12].any() and not e["counts"][13:].any()              # nothing to adjust; [12] is lambda


def test_device_entry_point_refuses_before_any_device_work(lib):
    f = lib.loftr_bundle_adjust_prior
    a = _host_args()
    tail = dict(ws=None, ws_bytes=0, class_ms=None, class_launches=None, stream=None)
    assert _call(f, {**a, **tail}) == BAD_ARG                                                           # no workspace
    ws = np.zeros(16, np.uint8)
    for mode in (-1, 3):
        assert _call(f, {**a, **tail}, mode=mode, ws=ws, ws_bytes=16) == BAD_ARG
    for name in ("prior_xyz", "prior_sigma", "prior_mask", "cam_prior"):
        assert _call(f, {**a, **tail}, ws=ws, ws_bytes=16, **{name: None}) == BAD_ARG, name
    assert _call(f, {**a, **tail}, ws=ws, ws_bytes=16) == -3                                            # LOFTR_ERR_WORKSPACE: too short


def test_workspace_bytes(lib):
    w = lib.loftr_bundle_adjust_prior_workspace_bytes
    base = (lib.loftr_bundle_adjust_workspace_bytes, lib.loftr_bundle_adjust_focal_workspace_bytes, lib.loftr_bundle_adjust_shared_workspace_bytes)
    for mode in (0, 1, 2):
        got, plain = w(1000, 5000, 100, mode), base[mode](1000, 5000, 100)
        assert plain < got <= plain + 16 * 100 + 3 * 256, (mode, got, plain)                           # two doubles per image and the scalars
        assert w(0, 0, 0, mode) > 0
        assert w(-1, 0, 0, mode) == 0 and w(0, -1, 0, mode) == 0 and w(0, 0, -1, mode) == 0 and w(1 << 40, 1 << 40, 1 << 30, mode) == 0
    assert w(1000, 5000, 100, -1) == 0 and w(1000, 5000, 100, 3) == 0


def test_ops_wrappers_refuse_what_the_routines_cannot_take(lib):
    a = _host_args()
    base = [a[k] for k in ("offsets", "obs_image", "obs_xy", "obs_mask", "xyz", "K", "Tcw", "fixed", "cam_offsets", "cam_obs")]
    groups, prior, params = [a[k] for k in ("cam_group", "group_offsets", "group_cams")], [a[k] for k in ("prior_xyz", "prior_sigma", "prior_mask")], (0.0, 5, 10, 1e-2, 1e-9)
    out = ops.bundle_adjust_prior_host(2, *base, a["refine"], *groups, *prior, *params, 3, 0.5, 2.0)
    assert out["counts"].shape == (24,) and out["cam_prior"].tolist() == [0, 1, 1] and list(out)[-2:] == ["cam_prior", "counts"]
    assert sorted(ops.bundle_adjust_prior_host(0, *base, None, None, None, None, *prior, *params)) == sorted(
        ["T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active", "cam_prior", "counts"])
    with pytest.raises(ValueError, match="mode must be 0"):
        ops.bundle_adjust_prior_host(3, *base, a["refine"], *groups, *prior, *params)
    for bad in ([prior[0].astype(np.float32), prior[1], prior[2]], [prior[0][:2], prior[1], prior[2]], [prior[0], prior[1][:, :2], prior[2]],
                [prior[0], prior[1], prior[2].astype(bool)], [prior[0], prior[1], prior[2][:2]]):
        with pytest.raises(_lib.LoftrHipError, match="prior_"):
            ops.bundle_adjust_prior_host(0, *base, None, None, None, None, *bad, *params)
    import torch
    with pytest.raises(_lib.LoftrHipError):                                                             # CPU tensors to the kernels: no fallback
        ops.bundle_adjust_prior(0, *[torch.from_numpy(x) for x in base], None, None, None, None, *[torch.from_numpy(x) for x in prior], *params)
