"""GPU tests of the bundle adjustment with one focal step per group of images (csrc/bundle_gpu.hip): the kernels against the
defining host routine, bit for bit on every output tensor (K, cam_focal and group_focal included) and every count -- the scenes of
tests/_bundle_shared_cases.py, the Huber case, a mixed mask, the bounds case, the hand-written and the exact problem, the sizes at which
a kernel can go wrong (a group's list around 64 members for the group sums, refining groups around a wave and past a chunk of the
ordered sum over groups, a carrying camera's list around 64 slots, tracks around a block and a chunk), groups that mix fixed-pose and
free members, known poses with an unknown focal, device-side error bits, a run whose launches are all skipped, and reconstruct_tracks."""
import numpy as np
import pytest
import torch

import loftr_amd
from loftr_amd import _lib, _tracks, build as build_mod, ops
import _bundle_cases as BC
import _bundle_shared_cases as SC

pytestmark = pytest.mark.gpu
FIELDS = ("T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active", "K", "cam_focal", "cam_group", "group_focal")


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


def both(s, ids=None, refine_focal=True, min_focal_obs=1, **kw):
    """Scene s through the host routine and through the kernels; asserts equality -> the GPU result."""
    fixed, ids = s.get("fixed"), np.asarray(s["camera_ids"] if ids is None else ids, np.int64)
    want = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=fixed, refine_focal=refine_focal, camera_ids=ids, min_focal_obs=min_focal_obs, **kw)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in BC.inputs(s)]
    mask = refine_focal if refine_focal is True else torch.from_numpy(np.asarray(refine_focal)).cuda()
    got = loftr_amd.bundle_adjust(*dev, fixed=None if fixed is None else torch.from_numpy(fixed).cuda(), refine_focal=mask,
                                  camera_ids=torch.from_numpy(ids).cuda(), min_focal_obs=min_focal_obs, **kw)
    assert got.xyz.is_cuda and got.K.is_cuda and got.cam_focal.is_cuda and got.cam_group.is_cuda and got.group_focal.is_cuda
    _same(got, want, kw)
    return got


def grouped(s, ids):
    """Scene s with one detuning factor per id."""
    return SC.detune_groups(s, ids)


@pytest.mark.parametrize("name,kw", [("one_a", {}), ("one_b", {}), ("bodies", {}), ("thin", {}), ("huber", dict(huber_px=2.0, max_iters=40))])
def test_scenes_equal_the_host_routine(lib, name, kw):
    got = both(SC.shared_case(name), min_focal_obs=20, **kw)
    assert got.cost_after < 0.1 * got.cost_before and got.n_pcg > 0 and got.cam_focal.all() and got.group_focal.all()
    assert got.stats["n_focal_groups"] == (1 if name.startswith("one") else 3)


def test_mixed_mask_bounds_and_thresholds(lib):
    s = SC.shared_case("bodies")
    mask = np.ones(12, bool)
    mask[[3, 4]] = False
    got = both(s, refine_focal=mask)
    assert got.cam_focal.cpu().tolist() == mask.tolist()
    assert torch.equal(got.K.cpu()[~mask], torch.from_numpy(s["K"])[~mask])
    thin = SC.shared_case("thin")
    assert both(thin, min_focal_obs=52).group_focal.cpu().tolist() == [True, True, False]      # the groups hold 94 / 76 / 51 observations
    assert both(thin, min_focal_obs=95).stats["n_focal_groups"] == 0
    tight = both(s, focal_bounds=(0.97, 1.03), max_iters=12)
    assert tight.n_accepted < tight.n_iters and tight.stats["lambda"] > 1e-4
    one = both(s, focal_bounds=(0.97, 1.03), max_iters=1)
    assert one.n_accepted == 0 and torch.equal(one.K.cpu(), torch.from_numpy(s["K"]))


def test_hand_written_and_exact_problems(lib):
    s, n = BC.hand_problem()
    got = both(s, ids=[0, 0, 1, 1, 1, 2, 2, 3])
    assert got.status == "converged" and got.cam_focal.tolist() == [True] * 5 + [False] * 3 and got.group_focal.tolist() == [True, True, False, False]
    assert not got.point_active[n["nan_point"]] and not got.obs_active[n["behind_obs"]] and float(got.K[n["bad_cam"], 0, 0]) == 0.0
    e = SC.shared_case("one_a")
    assert both(dict(e, fixed=None)).cam_free.tolist() == [False, True, True, True, True]
    assert both(dict(e, obs_mask=np.zeros_like(e["obs_mask"]))).status == "nothing_to_adjust"
    assert both(e, max_iters=0).status == "max_iters"
    empty = dict(e, offsets=np.zeros(1, np.int64), obs_image=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2), np.float32), obs_mask=np.zeros(0, bool),
                 xyz=np.zeros((0, 3), np.float32))
    assert both(empty).status == "nothing_to_adjust"                                       # T = 0, N = 0


@pytest.mark.parametrize("members", [1, 63, 64, 65, 129])
def test_members_of_one_group_around_a_wave(lib, members):
    """The group's osum64 edges: `members` cameras of 3 observations each in one group (the two fixed-pose ones among them when there is
    room), two more cameras in a second group."""
    n = members + 2
    ids = np.r_[np.zeros(members, np.int64), np.ones(2, np.int64)] if members > 1 else np.array([1, 1, 0], np.int64)
    s = grouped(BC.all_see_all(n, 3), ids)
    got = both(s, max_iters=6)
    assert got.stats["n_focal_groups"] == 2 and got.stats["n_focal_cameras"] == n and got.n_accepted >= 1 and got.n_pcg >= 1
    assert (got.K.cpu().numpy()[:, 0, 0] != s["K"][:, 0, 0]).all()


@pytest.mark.parametrize("groups", [1, 2, 64, 65])
def test_refining_groups_around_a_wave(lib, groups):
    n = 66
    s = grouped(BC.spread(n - 2, 140), np.arange(n) % groups)
    got = both(s, max_iters=6)
    assert got.stats["n_focal_groups"] == groups and got.stats["n_focal_cameras"] == n and got.n_accepted >= 1 and got.n_pcg >= 1


def test_4097_singleton_groups_pass_the_chunk_of_the_sum_over_groups(lib):
    n = 4097
    s = grouped(BC.spread(n - 2, 2 * n), np.arange(n)[::-1].copy())
    got = both(s, max_iters=3, pcg_iters=5)
    assert got.stats["n_focal_groups"] == n == got.stats["n_focal_cameras"] and got.n_pcg >= 1 and got.cam_group.cpu().tolist() == list(range(n))


def test_a_group_mixing_fixed_pose_and_free_members_and_known_poses(lib):
    s = SC.shared_case("bodies")
    fixed = s["fixed"] | (np.arange(12) % 4 == 3)                                          # images 0, 1, 3, 7, 11
    got = both(dict(s, fixed=fixed), min_focal_obs=20)
    assert got.cam_free.cpu().tolist() == (~fixed).tolist() and got.cam_focal.all()
    assert torch.equal(got.T_cam_from_world.cpu()[fixed], torch.from_numpy(s["T_cam_from_world"])[fixed])
    one = SC.shared_case("one_b")
    known = both(dict(one, T_cam_from_world=one["T_true"].copy(), fixed=np.ones(12, bool)), min_focal_obs=20)   # zero free cameras, one refining group
    assert known.stats["n_free_cameras"] == 0 and known.stats["n_focal_groups"] == 1 and known.n_pcg > 0 and known.status == "converged"
    assert known.cost_after < 0.01 * known.cost_before


@pytest.mark.parametrize("slots", [63, 64, 65, 129])
def test_observations_in_one_carrying_camera_around_a_wave(lib, slots):
    got = both(grouped(BC.all_see_all(3, slots), [0, 1, 0]), max_iters=8)
    assert got.stats["n_focal_cameras"] == 3 and got.stats["n_active_observations"] == 3 * slots and got.n_accepted >= 1


@pytest.mark.parametrize("n_tracks", [1, 3, 257, 4097])
def test_tracks_around_a_block_and_a_chunk(lib, n_tracks):
    got = both(grouped(BC.spread(2, n_tracks), [0, 1, 0, 1]), max_iters=6)
    assert got.stats["n_active_points"] == n_tracks and got.n_accepted >= 1 and got.stats["n_focal_groups"] == 2


def test_device_side_error_bits_are_value_errors_and_no_trial_runs(lib):
    s = SC.shared_case("one_a")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    im = s["obs_image"].copy(); im[7] = 5
    with pytest.raises(ValueError, match="obs_image outside.*found on the device"):
        loftr_amd.bundle_adjust(*[dev(im if n == "obs_image" else s[n]) for n in BC.ARGS], refine_focal=True, camera_ids=dev(s["camera_ids"]))
    with pytest.raises(ValueError, match="camera_ids must not be negative"):
        loftr_amd.bundle_adjust(*[dev(s[n]) for n in BC.ARGS], refine_focal=True, camera_ids=dev(np.array([0, 0, -2, 0, 0])))
    # the grouping by camera is made by the wrapper; a wrong one goes through ops
    a = [s[k] for k in BC.ARGS]
    a[3] = a[3].astype(np.uint8)
    by_image = _tracks.group_by_image(a[1], 5)
    ids = np.array([0, 1, 0, 1, 2], np.int64)
    group, offsets, cams = _tracks.group_by_camera(ids)
    assert group.tolist() == [0, 1, 0, 1, 2] and offsets.tolist() == [0, 2, 4, 5] and cams.tolist() == [0, 2, 1, 3, 4]
    par = (0.0, 3, 5, 1e-2, 1e-9, 1, 0.5, 2.0)
    run = lambda g, o, c: ops.bundle_adjust_shared(*[dev(x) for x in a], dev(s["fixed"].astype(np.uint8)), *[dev(x) for x in by_image],
                                                   dev(np.ones(5, np.uint8)), dev(g), dev(o), dev(c), *par)
    good = run(group, offsets, cams)["counts"].cpu().tolist()
    assert good[1] == 0 and good[13] == 5 and good[14] == 3
    edit = lambda arr, i, v: np.r_[arr[:i], np.array([v], arr.dtype), arr[i + 1:]]
    bad = ((edit(group, 2, 1), offsets, cams),                     # a member whose group is another
           (edit(group, 4, 3), offsets, cams), (edit(group, 4, -1), offsets, cams),        # a group outside [0, G)
           (group, offsets, cams[[1, 0, 2, 3, 4]]),                # descending within a group
           (group, offsets, edit(cams, 3, 5)), (group, offsets, edit(cams, 3, -1)),        # a member outside [0, n)
           (group, edit(offsets, 1, 1), cams), (group, edit(offsets, 1, 1 << 40), cams), (group, edit(offsets, 3, 4), cams),
           (group, edit(offsets, 1, 0), cams),                     # an empty group
           (np.array([1, 0, 1, 0, 2], np.int32), offsets, cams[[2, 3, 0, 1, 4]]))          # groups not in the order of their first members
    for g, o, c in bad:
        out = run(g, o, c)
        cnt = out["counts"].cpu().tolist()
        assert cnt[1] == 8 and cnt[2] == 0, (cnt, g, o, c)               # the bit is up and no trial ran
        assert torch.equal(out["T_cam_from_world"].cpu(), torch.from_numpy(s["T_cam_from_world"]))
    with pytest.raises(ValueError, match="cam_group / group_offsets / group_cams.*found on the device"):
        _tracks.raise_error_bits("bundle_adjust", 8, ops.BUNDLE_SHARED_ERRORS)


def test_a_run_that_stops_before_the_first_trial_skips_every_launch(lib):
    got = both(BC.exact_problem(), ids=[4, 4, 9, 9])
    assert got.status == "converged" and got.n_iters == 0 and got.cost_after == 0.0 and got.stats["n_focal_groups"] == 2
    assert torch.equal(got.K.cpu(), torch.from_numpy(BC.exact_problem()["K"]))
    s = BC.all_see_all(4, 12, noise_px=0.0, rot_deg=0.0, centre_sigma=0.0, point_sigma=0.0)
    timings = {}
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in BC.inputs(s)]
    kw = dict(ftol=0.9, max_iters=3, pcg_iters=4, refine_focal=True, min_focal_obs=1)
    timed = loftr_amd.bundle_adjust(*dev, fixed=torch.from_numpy(s["fixed"]).cuda(), camera_ids=torch.tensor([0, 0, 1, 1]).cuda(), timings=timings, **kw)
    _same(timed, loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], camera_ids=[0, 0, 1, 1], **kw), "timed")
    assert timed.status == "converged" and timed.n_iters <= 2
    assert set(timings) == set(ops.BUNDLE_CLASSES) and timings["accept"][2] == 3 and timings["track_half"][2] == 3 * (1 + 4)
    assert timings["camera_half"][2] == 2 * 3 * (1 + 4) and timings["setup"][2] == 5 and timings["linearise"][2] == 3 * 3
    assert timings["osum"][2] == 2 + 3 * (2 + 4 * 4 + 2) and all(t[0] >= 0 and t[1] >= t[0] for t in timings.values())      # a dot product is two sums


def test_gpu_reconstruction_equals_the_cpu_reconstruction(lib):
    s = SC.shared_case("one_b")
    R = s["T_true"][1, :3, :3] @ s["T_true"][0, :3, :3].T
    t = s["T_true"][1, :3, 3] - R @ s["T_true"][0, :3, 3]
    out = {}
    for device in ("cpu", "cuda"):
        a = [torch.from_numpy(np.ascontiguousarray(s[k])).to(device) for k in ("offsets", "obs_image", "obs_xy", "K")]
        ba = {"refine_focal": True, "camera_ids": torch.zeros(12, dtype=torch.int64, device=device)}
        out[device] = loftr_amd.reconstruct_tracks(*a, (0, 1, R, t), ba=ba, min_corr=6, min_inliers=6)
    cpu, gpu = out["cpu"], out["cuda"]
    _same(gpu.bundle, cpu.bundle, "reconstruction")
    assert gpu.K.is_cuda and torch.equal(gpu.K.cpu(), cpu.K) and torch.equal(gpu.posed.cpu(), cpu.posed) and cpu.posed.all()
    assert torch.equal(gpu.T_cam_from_world.cpu(), cpu.T_cam_from_world) and torch.equal(gpu.round_registered.cpu(), cpu.round_registered)
    assert gpu.points.stats == cpu.points.stats and torch.equal(torch.nan_to_num(gpu.points.xyz.cpu()), torch.nan_to_num(cpu.points.xyz))
