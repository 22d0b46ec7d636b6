"""GPU tests of the bundle adjustment (csrc/bundle_gpu.hip): the kernels against the defining host routine, bit for bit on
every output tensor and every count -- the seeded scenes, the Huber case, the hand-written cases, the sizes at which a kernel can go wrong
(a camera's list around 64 slots, free cameras around a wave, tracks around a block, a chunk of the ordered sum and beyond, a long track),
device-side error bits, a run whose launches are all skipped, and the atlas chain end to end."""
import numpy as np
import pytest
import torch

import loftr_amd
from loftr_amd import BundleResult, _lib, build as build_mod, ops
import _bundle_cases as BC
import _triangulation_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def _same(got, want, what):
    """torch.equal on every field (NaN positions compared by mask) and equal stats, the float ones bit for bit."""
    for k in BundleResult.FIELDS:
        g, w = getattr(got, k).cpu(), getattr(want, k)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype.is_floating_point:
            assert torch.equal(torch.isnan(g), torch.isnan(w)), (what, k, "NaN positions")
            g, w = torch.nan_to_num(g, nan=0.0), torch.nan_to_num(w, nan=0.0)
        assert torch.equal(g, w), (what, k, int((g != w).sum()))
    assert got.stats == want.stats, (what, got.stats, want.stats)


def both(s, **kw):
    """Scene s through the host routine and through the kernels; asserts equality -> the GPU result."""
    fixed = s.get("fixed")
    want = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=fixed, **kw)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in BC.inputs(s)]
    got = loftr_amd.bundle_adjust(*dev, fixed=None if fixed is None else torch.from_numpy(fixed).cuda(), **kw)
    assert got.xyz.is_cuda and got.T_cam_from_world.is_cuda
    _same(got, want, kw)
    return got


@pytest.mark.parametrize("name,kw", [("scene_a", {}), ("scene_b", {}), ("scene_huber", dict(huber_px=2.0, max_iters=40)),
                                     ("scene_huber", dict(max_iters=10))])
def test_scenes_equal_the_host_routine(lib, name, kw):
    got = both(getattr(BC, name)(), **kw)
    assert got.cost_after < 0.1 * got.cost_before and got.n_pcg > 0


def test_hand_written_cases(lib):
    s, n = BC.hand_problem()
    got = both(s)
    assert got.status == "converged" and got.cam_free.tolist() == [False, False, True, True, True, False, False, False]
    assert not got.point_active[n["single"]] and not got.point_active[n["nan_point"]] and not got.obs_active[n["behind_obs"]]
    e = BC.scene_a()
    every_fixed = dict(e, fixed=np.ones(5, bool))
    assert both(every_fixed).n_pcg == 0
    assert both(dict(e, fixed=None)).cam_free.tolist() == [False, True, True, True, True]
    assert both(dict(e, obs_mask=np.zeros_like(e["obs_mask"]))).status == "nothing_to_adjust"
    assert both(e, max_iters=0).status == "max_iters"
    empty = dict(e, offsets=np.zeros(1, np.int64), obs_image=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2), np.float32), obs_mask=np.zeros(0, bool),
                 xyz=np.zeros((0, 3), np.float32))
    assert both(empty).status == "nothing_to_adjust"                                       # T = 0, N = 0
    assert both(dict(empty, offsets=np.zeros(4, np.int64), xyz=e["xyz"][:3])).status == "nothing_to_adjust"      # N = 0


@pytest.mark.parametrize("slots", [63, 64, 65, 129])
def test_observations_in_one_camera_around_a_wave(lib, slots):
    got = both(BC.all_see_all(3, slots), max_iters=8)
    assert got.stats["n_free_cameras"] == 1 and got.stats["n_active_observations"] == 3 * slots and got.n_accepted >= 1


@pytest.mark.parametrize("n_free", [1, 63, 64, 65])
def test_free_cameras_around_a_wave(lib, n_free):
    got = both(BC.spread(n_free, max(40, 2 * n_free)), max_iters=8)
    assert got.stats["n_free_cameras"] == n_free and got.n_accepted >= 1 and got.n_pcg >= 1


@pytest.mark.parametrize("n_tracks", [1, 3, 37, 257, 4096, 4097])
def test_tracks_around_a_block_and_a_chunk(lib, n_tracks):
    got = both(BC.spread(2, n_tracks), max_iters=6)
    assert got.stats["n_active_points"] == n_tracks and got.n_accepted >= 1


def test_a_track_of_70_observations(lib):
    tracks = [list(range(2, 72))] + [sorted({0, 1, 2 + j % 70, 2 + (11 * j + 5) % 70}) for j in range(140)]
    got = both(BC.synthetic(72, tracks), max_iters=8)
    assert got.stats["n_free_cameras"] == 70 and got.point_active[0] and got.n_accepted >= 1


def test_rejected_trials_a_stall_and_a_camera_with_one_observation(lib):
    s = BC.all_see_all(4, 12, noise_px=0.0, rot_deg=0.0, centre_sigma=0.0, point_sigma=0.0)
    got = both(s, ftol=0.0, max_iters=60)                               # rounding-level cost: trials are rejected until lambda > 1e10
    assert got.status == "stalled" and got.n_accepted < got.n_iters < 60 and got.stats["lambda"] > 1e10
    lonely = BC.synthetic(4, [[0, 1, 2]] + [[0, 1, 3]] * 10 + [[0, 1]] * 3)              # camera 2: one observation, U of rank 2
    assert both(lonely, max_iters=40).cam_free.tolist() == [False, False, True, True]
    assert both(lonely, max_iters=40, huber_px=1.0).n_accepted >= 1


def test_device_side_error_bits_are_value_errors(lib):
    s = BC.scene_a()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    N = len(s["obs_image"])
    im = s["obs_image"].copy(); im[7] = 5
    neg = s["obs_image"].copy(); neg[0] = -1
    off = s["offsets"].copy(); off[3] = off[2] - 1
    for k, bad, msg in (("obs_image", im, "obs_image outside"), ("obs_image", neg, "obs_image outside"), ("offsets", off, "offsets must"),
                        ("offsets", np.r_[1, s["offsets"][1:]], "offsets must"), ("offsets", np.r_[s["offsets"][:-1], N - 1], "offsets must")):
        with pytest.raises(ValueError, match=msg + ".*found on the device"):
            loftr_amd.bundle_adjust(*[dev(bad if n == k else s[n]) for n in BC.ARGS])
    # the grouping by image is made by the wrapper; a wrong one goes through ops
    a = [s[k] for k in BC.ARGS]
    a[3] = a[3].astype(np.uint8)
    cam_obs = np.argsort(a[1], kind="stable").astype(np.int32)
    cam_offsets = np.zeros(6, np.int64)
    cam_offsets[1:] = np.cumsum(np.bincount(a[1], minlength=5))
    par = (0.0, 3, 5, 1e-2, 1e-9)
    run = lambda co, ob: ops.bundle_adjust(*[dev(x) for x in a], dev(s["fixed"].astype(np.uint8)), dev(co), dev(ob), *par)["counts"].cpu().tolist()
    assert run(cam_offsets, cam_obs)[1] == 0
    swapped = cam_obs.copy(); swapped[[0, 1]] = swapped[[1, 0]]
    outside = cam_obs.copy(); outside[3] = N
    below = cam_obs.copy(); below[3] = -1
    short = cam_offsets.copy(); short[1] -= 1
    late = cam_offsets.copy(); late[-1] = N + 1
    far = cam_offsets.copy(); far[2] = 1 << 40
    for co, ob in ((cam_offsets, swapped), (cam_offsets, outside), (cam_offsets, below), (short, cam_obs), (late, cam_obs), (far, cam_obs)):
        c = run(co, ob)
        assert c[1] == 4 and c[2] == 0, c                                # the bit is up and no trial ran


def test_a_run_that_stops_before_the_first_trial_skips_every_launch(lib):
    got = both(BC.exact_problem())
    assert got.status == "converged" and got.n_iters == 0 and got.cost_after == 0.0
    # ... and one that stops in its first trials
    s = BC.all_see_all(4, 12, noise_px=0.0, rot_deg=0.0, centre_sigma=0.0, point_sigma=0.0)
    got = both(s, ftol=0.9)
    assert got.status == "converged" and got.n_iters <= 2
    timings = {}
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in BC.inputs(s)]
    timed = loftr_amd.bundle_adjust(*dev, fixed=torch.from_numpy(s["fixed"]).cuda(), ftol=0.9, max_iters=3, pcg_iters=4, timings=timings)
    _same(timed, loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], ftol=0.9, max_iters=3, pcg_iters=4), "timed")
    assert set(timings) == set(ops.BUNDLE_CLASSES) and timings["accept"][2] == 3 and timings["track_half"][2] == 3 * (1 + 4)
    assert timings["osum"][2] == 2 + 3 * (1 + 2 * 4 + 2) and all(t[0] >= 0 and t[1] >= t[0] for t in timings.values())


def test_gpu_chain_equals_the_cpu_chain(lib):
    s, a = TC.sfm_scene(), BC.scene_a()
    out = {}
    for device in ("cpu", "cuda"):
        sfm = TC.run_atlas(device)
        pts1 = sfm.triangulate(s["K"], a["T_cam_from_world"])
        res = sfm.adjust(pts1, s["K"], a["T_cam_from_world"], fixed=a["fixed"])
        pts2 = sfm.triangulate(s["K"], res.T_cam_from_world)
        out[device] = (res, pts2)
    _same(out["cuda"][0], out["cpu"][0], "chain")
    assert out["cuda"][0].xyz.is_cuda and out["cuda"][1].stats == out["cpu"][1].stats
    assert torch.equal(out["cuda"][1].obs_inlier.cpu(), out["cpu"][1].obs_inlier)
    assert torch.equal(torch.nan_to_num(out["cuda"][1].xyz.cpu()), torch.nan_to_num(out["cpu"][1].xyz))
