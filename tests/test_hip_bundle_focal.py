"""GPU tests of the bundle adjustment with focal refinement (csrc/bundle_gpu.hip, the 7-wide camera block): the kernels
against the defining host routine, bit for bit on every output tensor (K and cam_focal included) and every count -- the detuned scenes,
the Huber case, a mixed mask, the bounds case, the hand-written and the exact problem, the sizes at which a kernel can go wrong (a
refining camera's list around 64 slots for the 35-accumulator sum, refining cameras around a wave, tracks around a block and a chunk of
the ordered sum, a long track), device-side error bits, a run whose launches are all skipped, and reconstruct_tracks end to end."""
import numpy as np
import pytest
import torch

import loftr_amd
from loftr_amd import _lib, build as build_mod, ops
import _bundle_cases as BC
import _bundle_focal_cases as FC

pytestmark = pytest.mark.gpu
FIELDS = ("T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active", "K", "cam_focal")


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def _same(got, want, what):
    """torch.equal on every field (NaN positions compared by mask) and equal stats, the float ones bit for bit."""
    assert got.FIELDS == want.FIELDS == FIELDS
    for k in FIELDS:
        g, w = getattr(got, k).cpu(), getattr(want, k)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype.is_floating_point:
            assert torch.equal(torch.isnan(g), torch.isnan(w)), (what, k, "NaN positions")
            g, w = torch.nan_to_num(g, nan=0.0), torch.nan_to_num(w, nan=0.0)
        assert torch.equal(g, w), (what, k, int((g != w).sum()))
    assert got.stats == want.stats, (what, got.stats, want.stats)


def both(s, refine_focal=True, min_focal_obs=1, **kw):
    """Scene s through the host routine and through the kernels; asserts equality -> the GPU result."""
    fixed = s.get("fixed")
    want = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=fixed, refine_focal=refine_focal, min_focal_obs=min_focal_obs, **kw)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in BC.inputs(s)]
    mask = refine_focal if refine_focal is True else torch.from_numpy(np.asarray(refine_focal)).cuda()
    got = loftr_amd.bundle_adjust(*dev, fixed=None if fixed is None else torch.from_numpy(fixed).cuda(), refine_focal=mask,
                                  min_focal_obs=min_focal_obs, **kw)
    assert got.xyz.is_cuda and got.K.is_cuda and got.cam_focal.is_cuda
    _same(got, want, kw)
    return got


@pytest.mark.parametrize("name,kw", [("scene_a", {}), ("scene_b", {}), ("scene_huber", dict(huber_px=2.0, max_iters=40))])
def test_detuned_scenes_equal_the_host_routine(lib, name, kw):
    got = both(FC.focal_case(name), min_focal_obs=20, **kw)
    assert got.cost_after < 0.1 * got.cost_before and got.n_pcg > 0 and got.stats["n_focal_cameras"] == got.stats["n_free_cameras"]


def test_mixed_mask_and_bounds(lib):
    s = FC.focal_case("scene_b")
    mask = np.zeros(12, bool)
    mask[[0, 3, 4, 7, 10]] = True
    got = both(s, refine_focal=mask)
    assert got.cam_focal.cpu().tolist() == (mask & ~s["fixed"]).tolist()
    assert torch.equal(got.K.cpu()[~got.cam_focal.cpu()], torch.from_numpy(s["K"])[~got.cam_focal.cpu()])
    assert both(s, min_focal_obs=65).stats["n_focal_cameras"] == 6                         # the lists hold 49-75 observations
    tight = both(s, focal_bounds=(0.97, 1.03), max_iters=12)
    assert tight.n_accepted < tight.n_iters and tight.stats["lambda"] > 1e-4
    one = both(s, focal_bounds=(0.97, 1.03), max_iters=1)
    assert one.n_accepted == 0 and torch.equal(one.K.cpu(), torch.from_numpy(s["K"]))


def test_hand_written_and_exact_problems(lib):
    s, n = BC.hand_problem()
    got = both(s)
    assert got.status == "converged" and got.cam_focal.tolist() == [False, False, True, True, True, False, False, False]
    assert not got.point_active[n["nan_point"]] and not got.obs_active[n["behind_obs"]] and float(got.K[n["bad_cam"], 0, 0]) == 0.0
    e = FC.focal_case("scene_a")
    assert both(dict(e, fixed=np.ones(5, bool))).stats["n_focal_cameras"] == 0
    assert both(dict(e, fixed=None)).cam_focal.tolist() == [False, True, True, True, True]
    assert both(dict(e, obs_mask=np.zeros_like(e["obs_mask"]))).status == "nothing_to_adjust"
    assert both(e, max_iters=0).status == "max_iters"
    empty = dict(e, offsets=np.zeros(1, np.int64), obs_image=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2), np.float32), obs_mask=np.zeros(0, bool),
                 xyz=np.zeros((0, 3), np.float32))
    assert both(empty).status == "nothing_to_adjust"                                       # T = 0, N = 0


@pytest.mark.parametrize("slots", [63, 64, 65, 129])
def test_observations_in_one_refining_camera_around_a_wave(lib, slots):
    got = both(FC.detune(BC.all_see_all(3, slots)), max_iters=8)
    assert got.stats["n_focal_cameras"] == 1 and got.stats["n_active_observations"] == 3 * slots and got.n_accepted >= 1
    assert float(got.K[2, 0, 0]) != float(FC.detune(BC.all_see_all(3, slots))["K"][2, 0, 0])


@pytest.mark.parametrize("n_free", [1, 63, 64, 65])
def test_refining_cameras_around_a_wave(lib, n_free):
    got = both(FC.detune(BC.spread(n_free, max(40, 2 * n_free))), max_iters=8)
    assert got.stats["n_focal_cameras"] == n_free and got.n_accepted >= 1 and got.n_pcg >= 1


@pytest.mark.parametrize("n_tracks", [1, 3, 257, 4097])
def test_tracks_around_a_block_and_a_chunk(lib, n_tracks):
    got = both(FC.detune(BC.spread(2, n_tracks)), max_iters=6)
    assert got.stats["n_active_points"] == n_tracks and got.n_accepted >= 1 and got.stats["n_focal_cameras"] == 2


def test_a_track_of_70_observations(lib):
    tracks = [list(range(2, 72))] + [sorted({0, 1, 2 + j % 70, 2 + (11 * j + 5) % 70}) for j in range(140)]
    got = both(FC.detune(BC.synthetic(72, tracks)), max_iters=8)
    assert got.stats["n_focal_cameras"] == 70 and got.point_active[0] and got.n_accepted >= 1


def test_device_side_error_bits_are_value_errors_and_nothing_is_written(lib):
    s = FC.focal_case("scene_a")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    N = len(s["obs_image"])
    im = s["obs_image"].copy(); im[7] = 5
    off = s["offsets"].copy(); off[3] = off[2] - 1
    for k, bad, msg in (("obs_image", im, "obs_image outside"), ("offsets", off, "offsets must"),
                        ("offsets", np.r_[s["offsets"][:-1], N - 1], "offsets must")):
        with pytest.raises(ValueError, match=msg + ".*found on the device"):
            loftr_amd.bundle_adjust(*[dev(bad if n == k else s[n]) for n in BC.ARGS], refine_focal=True)
    # the grouping by image is made by the wrapper; a wrong one goes through ops
    a = [s[k] for k in BC.ARGS]
    a[3] = a[3].astype(np.uint8)
    cam_obs = np.argsort(a[1], kind="stable").astype(np.int32)
    cam_offsets = np.zeros(6, np.int64)
    cam_offsets[1:] = np.cumsum(np.bincount(a[1], minlength=5))
    par = (0.0, 3, 5, 1e-2, 1e-9, 1, 0.5, 2.0)
    run = lambda co, ob: ops.bundle_adjust_focal(*[dev(x) for x in a], dev(s["fixed"].astype(np.uint8)), dev(co), dev(ob),
                                                 dev(np.ones(5, np.uint8)), *par)
    good = run(cam_offsets, cam_obs)
    assert good["counts"].cpu().tolist()[1] == 0 and good["counts"].cpu().tolist()[13] == 3
    swapped = cam_obs.copy(); swapped[[0, 1]] = swapped[[1, 0]]
    outside = cam_obs.copy(); outside[3] = N
    short = cam_offsets.copy(); short[1] -= 1
    far = cam_offsets.copy(); far[2] = 1 << 40
    for co, ob in ((cam_offsets, swapped), (cam_offsets, outside), (short, cam_obs), (far, cam_obs)):
        out = run(co, ob)
        c = out["counts"].cpu().tolist()
        assert c[1] == 4 and c[2] == 0, c                                # the bit is up and no trial ran
        assert torch.equal(out["K"].cpu(), torch.from_numpy(s["K"]))     # no focal was written: K holds the input's bits
        assert torch.equal(out["T_cam_from_world"].cpu(), torch.from_numpy(s["T_cam_from_world"]))


def test_a_run_that_stops_before_the_first_trial_skips_every_launch(lib):
    got = both(BC.exact_problem())
    assert got.status == "converged" and got.n_iters == 0 and got.cost_after == 0.0 and got.stats["n_focal_cameras"] == 2
    assert torch.equal(got.K.cpu(), torch.from_numpy(BC.exact_problem()["K"]))
    s = BC.all_see_all(4, 12, noise_px=0.0, rot_deg=0.0, centre_sigma=0.0, point_sigma=0.0)
    timings = {}
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in BC.inputs(s)]
    kw = dict(ftol=0.9, max_iters=3, pcg_iters=4, refine_focal=True, min_focal_obs=1)
    timed = loftr_amd.bundle_adjust(*dev, fixed=torch.from_numpy(s["fixed"]).cuda(), timings=timings, **kw)
    _same(timed, loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], **kw), "timed")
    assert timed.status == "converged" and timed.n_iters <= 2
    assert set(timings) == set(ops.BUNDLE_CLASSES) and timings["accept"][2] == 3 and timings["track_half"][2] == 3 * (1 + 4)      # §18's schedule
    assert timings["osum"][2] == 2 + 3 * (1 + 2 * 4 + 2) and all(t[0] >= 0 and t[1] >= t[0] for t in timings.values())


def test_gpu_reconstruction_equals_the_cpu_reconstruction(lib):
    s = FC.focal_case("scene_b")
    R = s["T_true"][1, :3, :3] @ s["T_true"][0, :3, :3].T
    t = s["T_true"][1, :3, 3] - R @ s["T_true"][0, :3, 3]
    out = {}
    for device in ("cpu", "cuda"):
        a = [torch.from_numpy(np.ascontiguousarray(s[k])).to(device) for k in ("offsets", "obs_image", "obs_xy", "K")]
        out[device] = loftr_amd.reconstruct_tracks(*a, (0, 1, R, t), ba={"refine_focal": True}, min_corr=6, min_inliers=6)
    cpu, gpu = out["cpu"], out["cuda"]
    _same(gpu.bundle, cpu.bundle, "reconstruction")
    assert gpu.K.is_cuda and torch.equal(gpu.K.cpu(), cpu.K) and torch.equal(gpu.posed.cpu(), cpu.posed) and cpu.posed.all()
    assert torch.equal(gpu.T_cam_from_world.cpu(), cpu.T_cam_from_world) and torch.equal(gpu.round_registered.cpu(), cpu.round_registered)
    assert gpu.points.stats == cpu.points.stats and torch.equal(torch.nan_to_num(gpu.points.xyz.cpu()), torch.nan_to_num(cpu.points.xyz))
