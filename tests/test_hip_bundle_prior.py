"""GPU tests of the bundle adjustment with position priors (csrc/bundle_gpu.hip): the kernels against the defining host
routine, bit for bit on every output tensor (cam_prior included) and every count -- the prior scenes of tests/_bundle_prior_cases.py in
the three modes, the sizes at which a kernel can go wrong (cameras with a prior around a wave and past a chunk of the ordered sum over
cameras, a camera's list around 64 slots, tracks around a block and a chunk), a mix of cameras with a prior, without and fixed, the
all-zero mask against the existing kernels, runs that stop before the first trial, and the align -> adjust -> triangulate chain."""
import numpy as np
import pytest
import torch

import loftr_amd
from loftr_amd import _lib, build as build_mod
import _bundle_cases as BC
import _bundle_prior_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def _same(got, want, what):
    """torch.equal on every field (NaN positions compared by mask) and equal stats, the float ones bit for bit."""
    assert got.FIELDS == want.FIELDS and got.FIELDS[-1] == "cam_prior"
    for k in want.FIELDS:
        g, w = getattr(got, k), getattr(want, k)
        assert g.is_cuda, (what, k)
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype.is_floating_point:
            assert torch.equal(torch.isnan(g), torch.isnan(w)), (what, k, "NaN positions")
            g, w = torch.nan_to_num(g, nan=0.0), torch.nan_to_num(w, nan=0.0)
        assert torch.equal(g, w), (what, k, int((g != w).sum()))
    assert got.stats.keys() == want.stats.keys()
    for k, v in want.stats.items():
        assert np.float64(got.stats[k]).tobytes() == np.float64(v).tobytes() if isinstance(v, float) else got.stats[k] == v, (what, k, got.stats[k], v)


def cuda(x):
    return x if x is None or isinstance(x, (bool, int, float)) else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def both(s, prior=True, **kw):
    """Scene s through the host routine and through the kernels; asserts equality -> the GPU result.  kw: keywords of bundle_adjust
    (arrays among them are moved to the device for the second call)."""
    if prior:
        kw = dict(PC.prior_kwargs(s), **kw)
    want = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s.get("fixed"), **kw)
    got = loftr_amd.bundle_adjust(*[cuda(a) for a in BC.inputs(s)], fixed=cuda(s.get("fixed")), **{k: cuda(v) for k, v in kw.items()})
    _same(got, want, sorted(kw))
    return got


@pytest.mark.parametrize("name", ["scene_a", "scene_b", "focal", "shared", "scaled"])
def test_scenes_equal_the_host_routine(lib, name):
    s = PC.prior_case(name)
    got = both(s, **PC.mode_kwargs(name, s))
    n = len(s["K"])
    assert got.status == "converged" and got.cost_after < 0.1 * got.cost_before and got.n_pcg > 0
    assert got.cam_prior.all() and got.stats["n_prior_cameras"] == n and got.stats["prior_rms_after"] < 0.5 * got.stats["prior_rms_before"]
    if name in ("focal", "shared"):
        assert got.cam_focal.all() and got.stats["n_focal_cameras"] == n


def test_huber_acts_on_the_observations_only(lib):
    s = PC.with_priors(BC.scene_huber())
    got = both(s, huber_px=2.0, max_iters=12)
    plain = both(s, max_iters=12)
    assert got.n_accepted >= 1 and got.cost_after < plain.cost_after and got.stats["prior_cost_before"] == plain.stats["prior_cost_before"]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_cameras_with_a_prior_around_a_wave(lib, count):
    s = PC.many_cameras(count, n_fixed=2)
    got = both(s, max_iters=6)
    assert got.stats["n_prior_cameras"] == count and got.cam_prior.cpu().tolist() == [False, False] + [True] * count
    assert got.n_accepted >= 1 and got.n_pcg >= 1 and got.stats["prior_cost_after"] < got.stats["prior_cost_before"]


def test_cameras_with_a_prior_past_a_chunk_of_the_ordered_sum(lib):
    s = PC.many_cameras(4097)
    got = both(s, max_iters=3, pcg_iters=10)
    assert got.stats["n_prior_cameras"] == 4097 and got.stats["n_free_cameras"] == 4097 and got.n_accepted >= 1


def test_a_mix_of_cameras_with_a_prior_without_and_fixed(lib):
    s = PC.many_cameras(40, n_plain=30, n_fixed=3)
    sigma = np.full((73, 3), PC.SIGMA)
    sigma[40, 1], sigma[50, 0] = np.nan, 0.0                             # two more switched off on the device
    prior = s["prior_xyz"].copy()
    prior[60, 2] = np.inf
    got = both(s, position_prior=prior, prior_sigma=sigma, max_iters=8)
    want = np.arange(73) >= 33
    want[[40, 50, 60]] = False
    assert got.cam_prior.cpu().tolist() == want.tolist() and got.stats["n_prior_cameras"] == 37 and got.stats["n_free_cameras"] == 70
    assert got.n_accepted >= 1
    fixed = s["fixed"]
    assert torch.equal(got.T_cam_from_world.cpu()[fixed], torch.from_numpy(s["T_cam_from_world"])[fixed])


@pytest.mark.parametrize("slots", [63, 64, 65])
def test_a_camera_with_a_prior_around_64_observations(lib, slots):
    got = both(PC.one_camera_many_obs(slots), max_iters=6)
    assert got.cam_prior.cpu().tolist() == [False, True] and got.stats["n_active_observations"] == 2 * slots and got.n_accepted >= 1


@pytest.mark.parametrize("tracks", [1, 257, 4097])
def test_tracks_around_a_block_and_a_chunk(lib, tracks):
    s = PC.with_priors(BC.all_see_all(3, tracks))
    got = both(s, max_iters=4, pcg_iters=10)
    assert got.stats["n_active_points"] == tracks and got.stats["n_prior_cameras"] == 3 and got.n_accepted >= 1


@pytest.mark.parametrize("name", ["scene_b", "focal", "shared"])
def test_an_all_zero_mask_equals_the_existing_kernels(lib, name):
    s = PC.prior_case(name)
    s = dict(s, fixed=(BC.scene_a() if name == "focal" else BC.scene_b())["fixed"])
    kw = {k: cuda(v) for k, v in PC.mode_kwargs(name, s).items()}
    dev = [cuda(a) for a in BC.inputs(s)]
    for huber in (0.0, 2.0):
        want = loftr_amd.bundle_adjust(*dev, fixed=cuda(s["fixed"]), huber_px=huber, **kw)
        got = loftr_amd.bundle_adjust(*dev, fixed=cuda(s["fixed"]), huber_px=huber, position_prior=cuda(s["prior_xyz"]), prior_sigma=0.02,
                                      prior_mask=torch.zeros(len(s["K"]), dtype=torch.bool, device="cuda"), **kw)
        assert got.FIELDS == want.FIELDS + ("cam_prior",) and not got.cam_prior.any()
        for k in want.FIELDS:
            g, w = getattr(got, k), getattr(want, k)
            assert g.dtype == w.dtype and torch.equal(torch.nan_to_num(g.double()), torch.nan_to_num(w.double())), (name, huber, k)
        for k, v in want.stats.items():
            assert np.float64(got.stats[k]).tobytes() == np.float64(v).tobytes() if isinstance(v, float) else got.stats[k] == v, (name, huber, k)


def test_runs_that_stop_before_the_first_trial(lib):
    s = PC.prior_case("scene_a")
    zero = both(s, max_iters=0)
    assert zero.status == "max_iters" and zero.n_iters == 0 and zero.stats["prior_cost_after"] == zero.stats["prior_cost_before"] > 0
    assert zero.stats["prior_rms_after"] == zero.stats["prior_rms_before"] > 0 and zero.cost_after == zero.cost_before
    none = both(dict(s, obs_mask=np.zeros_like(s["obs_mask"])))
    assert none.status == "nothing_to_adjust" and none.stats["n_prior_cameras"] == 0 and not none.cam_prior.any()
    empty = dict(s, offsets=np.zeros(1, np.int64), obs_image=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2), np.float32), obs_mask=np.zeros(0, bool),
                 xyz=np.zeros((0, 3), np.float32))
    assert both(empty).status == "nothing_to_adjust"                     # T = 0, N = 0: every camera osum has five +0 terms


def test_align_refine_chain_equals_the_cpu_chain(lib):
    _, rec_c, _, _, want, al_c = PC.refine_chain("cpu")
    _, rec_g, _, _, got, al_g = PC.refine_chain("cuda")
    assert torch.equal(al_g.inliers.cpu(), al_c.inliers) and got.T_cam_from_world.is_cuda and got.points.xyz.is_cuda
    same = lambda a, b: a.cpu().numpy().tobytes() == b.numpy().tobytes()
    assert same(rec_g.T_cam_from_world, rec_c.T_cam_from_world)
    assert same(got.T_cam_from_world, want.T_cam_from_world) and same(got.points.xyz, want.points.xyz) and same(got.K, want.K)
    assert torch.isnan(got.T_cam_from_world[4]).all()
    _same(got.bundle, want.bundle, "chain")
