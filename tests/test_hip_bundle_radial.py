"""GPU tests of the bundle adjustment with one radial coefficient per group of images (csrc/bundle_gpu.hip): the kernels
against the defining host routine, bit for bit on every output tensor (K, radial, cam_radial and group_radial included) and every count --
the scenes of tests/_bundle_radial_cases.py, the Huber case, a mixed mask, the bounds case, the start at a cost of exactly 0, the sizes at
which a kernel can go wrong (a group's list around 64 members for the group sums, refining groups around a wave, a carrying camera's list
around 64 slots, tracks around a block), a group that mixes fixed-pose and free members, known poses with an unknown lens, a bad grouping's
error bit, a run whose launches are all skipped, and reconstruct_tracks."""
import numpy as np
import pytest
import torch

import loftr_amd
from loftr_amd import _lib, _tracks, build as build_mod, ops
import _bundle_cases as BC
import _bundle_radial_cases as RC
import _bundle_shared_cases as SC

pytestmark = pytest.mark.gpu
FIELDS = ("T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active", "K", "cam_focal", "cam_group", "group_focal", "radial",
          "cam_radial", "group_radial")
K_CYCLE = np.array([-0.10, 0.06, -0.04, 0.03])                                               # the lens of group g is K_CYCLE[g % 4]


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


def both(s, ids=None, refine_focal=True, refine_radial=True, min_focal_obs=1, **kw):
    """Scene s through the host routine and through the kernels; asserts equality -> the GPU result."""
    fixed, ids = s.get("fixed"), np.asarray(s["camera_ids"] if ids is None else ids, np.int64)
    start = s.get("radial")
    want = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=fixed, refine_focal=refine_focal, refine_radial=refine_radial, radial=start,
                                   camera_ids=ids, min_focal_obs=min_focal_obs, **kw)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in BC.inputs(s)]
    cu = lambda m: m if m is True or m is None else torch.from_numpy(np.asarray(m)).cuda()
    got = loftr_amd.bundle_adjust(*dev, fixed=None if fixed is None else torch.from_numpy(fixed).cuda(), refine_focal=cu(refine_focal),
                                  refine_radial=cu(refine_radial), radial=cu(start), camera_ids=torch.from_numpy(ids).cuda(),
                                  min_focal_obs=min_focal_obs, **kw)
    assert got.xyz.is_cuda and got.K.is_cuda and got.radial.is_cuda and got.cam_radial.is_cuda and got.group_radial.is_cuda
    _same(got, want, kw)
    return got


def lens(s, ids):
    """Scene s with one detuning factor and one lens per id, observed through it."""
    s = SC.detune_groups(s, ids)
    group = _tracks.group_by_camera(np.asarray(ids, np.int64))[0]
    return RC.distort_scene(s, K_CYCLE[group % 4])


@pytest.mark.parametrize("name,kw", [("one_a", {}), ("one_b", {}), ("bodies", {}), ("huber", dict(huber_px=2.0, max_iters=40))])
def test_scenes_equal_the_host_routine(lib, name, kw):
    s = RC.radial_case(name)
    got = both(s, min_focal_obs=20, **kw)
    assert got.cost_after < 0.1 * got.cost_before and got.n_pcg > 0 and got.cam_radial.all() and got.group_radial.all()
    assert got.stats["n_focal_groups"] == (1 if name.startswith("one") else 3) and got.stats["n_radial_cameras"] == len(s["K"])
    assert np.abs(got.radial.cpu().numpy() - s["k_true"]).max() < 0.01


def test_mixed_mask_bounds_and_a_start_at_cost_zero(lib):
    s = RC.radial_case("bodies")
    mask = np.ones(12, bool)
    mask[[3, 4]] = False
    got = both(s, refine_radial=mask)
    assert got.cam_radial.cpu().tolist() == mask.tolist() and got.cam_focal.all() and got.group_radial.all()
    assert torch.equal(got.radial.cpu()[~mask], torch.from_numpy(s["radial"])[~mask])
    tight = both(s, radial_bounds=(-0.01, 0.01), max_iters=12)
    assert tight.n_accepted < tight.n_iters and tight.radial.abs().max() <= 0.01
    one = both(s, radial_bounds=(-0.01, 0.01), max_iters=1)
    assert one.n_accepted == 0 and torch.equal(one.K.cpu(), torch.from_numpy(s["K"])) and torch.equal(one.radial.cpu(), torch.from_numpy(s["radial"]))
    nan = dict(s, radial=np.r_[np.nan, np.zeros(11)])
    bad = both(dict(nan, fixed=None))
    assert not bad.cam_radial[0] and not bad.cam_focal[0] and not bad.obs_active.cpu()[s["obs_image"] == 0].any()


@pytest.mark.parametrize("members", [1, 63, 64, 65, 129])
def test_members_of_one_group_around_a_wave(lib, members):
    """The group's osum64 edges: `members` cameras of 3 observations each in one group (the two fixed-pose ones among them when there is
    room), two more cameras in a second group."""
    n = members + 2
    ids = np.r_[np.zeros(members, np.int64), np.ones(2, np.int64)] if members > 1 else np.array([1, 1, 0], np.int64)
    s = lens(BC.all_see_all(n, 3), ids)
    got = both(s, max_iters=6)
    assert got.stats["n_focal_groups"] == 2 and got.stats["n_radial_cameras"] == n and got.n_accepted >= 1 and got.n_pcg >= 1
    assert (got.radial.cpu().numpy() != 0).all()


@pytest.mark.parametrize("groups", [1, 2, 64, 65])
def test_refining_groups_around_a_wave(lib, groups):
    n = 66
    s = lens(BC.spread(n - 2, 140), np.arange(n) % groups)
    got = both(s, max_iters=6)
    assert got.stats["n_focal_groups"] == groups and got.stats["n_radial_cameras"] == n and got.n_accepted >= 1 and got.n_pcg >= 1
    assert got.group_radial.all()


def test_a_group_mixing_fixed_pose_and_free_members_and_known_poses(lib):
    s = RC.radial_case("bodies")
    fixed = s["fixed"] | (np.arange(12) % 4 == 3)                                          # images 0, 1, 3, 7, 11
    got = both(dict(s, fixed=fixed), min_focal_obs=20)
    assert got.cam_free.cpu().tolist() == (~fixed).tolist() and got.cam_radial.all()
    assert torch.equal(got.T_cam_from_world.cpu()[fixed], torch.from_numpy(s["T_cam_from_world"])[fixed])
    one = RC.radial_case("one_b")
    known = both(dict(one, T_cam_from_world=one["T_true"].copy(), fixed=np.ones(12, bool)), min_focal_obs=20)   # zero free cameras, one refining group
    assert known.stats["n_free_cameras"] == 0 and known.stats["n_focal_groups"] == 1 and known.n_pcg > 0 and known.group_radial.all()
    assert known.cost_after < 0.01 * known.cost_before


@pytest.mark.parametrize("slots", [63, 64, 65])
def test_observations_in_one_carrying_camera_around_a_wave(lib, slots):
    got = both(lens(BC.all_see_all(3, slots), [0, 1, 0]), max_iters=8)
    assert got.stats["n_radial_cameras"] == 3 and got.stats["n_active_observations"] == 3 * slots and got.n_accepted >= 1


@pytest.mark.parametrize("n_tracks", [1, 3, 257])
def test_tracks_around_a_block(lib, n_tracks):
    got = both(lens(BC.spread(2, n_tracks), [0, 1, 0, 1]), max_iters=6)
    assert got.stats["n_active_points"] == n_tracks and got.n_accepted >= 1 and got.stats["n_focal_groups"] == 2


def test_a_bad_grouping_raises_its_error_bit_and_no_trial_runs(lib):
    s = RC.radial_case("one_a")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a = [s[k] for k in BC.ARGS]
    a[3] = a[3].astype(np.uint8)
    by_image = _tracks.group_by_image(a[1], 5)
    group, offsets, cams = _tracks.group_by_camera(np.array([0, 1, 0, 1, 2], np.int64))
    par = (0.0, 3, 5, 1e-2, 1e-9, 1, 0.5, 2.0, -1.0, 1.0)
    run = lambda g, o, c: ops.bundle_adjust_radial(*[dev(x) for x in a], dev(s["fixed"].astype(np.uint8)), *[dev(x) for x in by_image],
                                                   dev(np.ones(5, np.uint8)), dev(g), dev(o), dev(c), dev(np.zeros(5)), dev(np.ones(5, np.uint8)),
                                                   *par)
    good = run(group, offsets, cams)["counts"].cpu().tolist()
    assert good[1] == 0 and good[13] == 5 and good[14] == 3 and good[15] == 5
    edit = lambda arr, i, v: np.r_[arr[:i], np.array([v], arr.dtype), arr[i + 1:]]
    for g, o, c in ((edit(group, 2, 1), offsets, cams), (group, offsets, cams[[1, 0, 2, 3, 4]]), (group, offsets, edit(cams, 3, 5)),
                    (group, edit(offsets, 1, 0), cams)):
        out = run(g, o, c)
        cnt = out["counts"].cpu().tolist()
        assert cnt[1] == 8 and cnt[2] == 0, (cnt, g, o, c)                             # the bit is up and no trial ran
        assert torch.equal(out["T_cam_from_world"].cpu(), torch.from_numpy(s["T_cam_from_world"]))
        assert torch.equal(out["radial"].cpu(), torch.zeros(5, dtype=torch.float64))
    im = s["obs_image"].copy(); im[7] = 5
    with pytest.raises(ValueError, match="obs_image outside.*found on the device"):
        loftr_amd.bundle_adjust(*[dev(im if n == "obs_image" else s[n]) for n in BC.ARGS], refine_focal=True, refine_radial=True)


def test_a_run_that_stops_before_the_first_trial_skips_every_launch(lib):
    got = both(dict(BC.exact_problem(), radial=np.zeros(4)), ids=[4, 4, 9, 9])               # k = 0 leaves the exact projections exact
    assert got.status == "converged" and got.n_iters == 0 and got.cost_after == 0.0 and got.stats["n_radial_cameras"] == 4
    assert torch.equal(got.K.cpu(), torch.from_numpy(BC.exact_problem()["K"])) and torch.equal(got.radial.cpu(), torch.zeros(4, dtype=torch.float64))
    s = BC.all_see_all(4, 12, noise_px=0.0, rot_deg=0.0, centre_sigma=0.0, point_sigma=0.0)
    timings = {}
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in BC.inputs(s)]
    kw = dict(ftol=0.9, max_iters=3, pcg_iters=4, refine_focal=True, refine_radial=True, min_focal_obs=1)
    timed = loftr_amd.bundle_adjust(*dev, fixed=torch.from_numpy(s["fixed"]).cuda(), camera_ids=torch.tensor([0, 0, 1, 1]).cuda(), timings=timings, **kw)
    _same(timed, loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], camera_ids=[0, 0, 1, 1], **kw), "timed")
    assert timed.status == "converged" and timed.n_iters <= 2
    assert set(timings) == set(ops.BUNDLE_CLASSES) and timings["accept"][2] == 3 and timings["track_half"][2] == 3 * (1 + 4)
    assert timings["camera_half"][2] == 2 * 3 * (1 + 4) and timings["setup"][2] == 5 and timings["linearise"][2] == 3 * 3      # the schedule is §18.2's
    assert timings["osum"][2] == 2 + 3 * (2 + 4 * 4 + 2)


def test_singleton_groups_without_camera_ids(lib):
    s = RC.radial_case("one_a")
    want = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True, refine_radial=True)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in BC.inputs(s)]
    got = loftr_amd.bundle_adjust(*dev, fixed=torch.from_numpy(s["fixed"]).cuda(), refine_focal=True, refine_radial=True)
    _same(got, want, "singletons")
    assert got.cam_group.cpu().tolist() == list(range(5)) and got.stats["n_focal_groups"] == 5


def test_gpu_reconstruction_equals_the_cpu_reconstruction(lib):
    s = RC.radial_case("one_b")
    R = s["T_true"][1, :3, :3] @ s["T_true"][0, :3, :3].T
    t = s["T_true"][1, :3, 3] - R @ s["T_true"][0, :3, 3]
    out = {}
    for device in ("cpu", "cuda"):
        a = [torch.from_numpy(np.ascontiguousarray(s[k])).to(device) for k in ("offsets", "obs_image", "obs_xy", "K")]
        ba = {"refine_focal": True, "refine_radial": True, "camera_ids": torch.zeros(12, dtype=torch.int64, device=device)}
        out[device] = loftr_amd.reconstruct_tracks(*a, (0, 1, R, t), ba=ba, min_corr=6, min_inliers=6)
    cpu, gpu = out["cpu"], out["cuda"]
    _same(gpu.bundle, cpu.bundle, "reconstruction")
    assert gpu.K.is_cuda and torch.equal(gpu.K.cpu(), cpu.K) and torch.equal(gpu.posed.cpu(), cpu.posed) and cpu.posed.all()
    assert gpu.radial.is_cuda and torch.equal(gpu.radial.cpu(), cpu.radial)
    assert torch.equal(gpu.T_cam_from_world.cpu(), cpu.T_cam_from_world) and torch.equal(gpu.round_registered.cpu(), cpu.round_registered)
    assert gpu.points.stats == cpu.points.stats and torch.equal(torch.nan_to_num(gpu.points.xyz.cpu()), torch.nan_to_num(cpu.points.xyz))
