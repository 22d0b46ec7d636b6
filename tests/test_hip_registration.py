"""GPU tests of image registration (csrc/register_gpu.hip): the kernels of the correspondence table against the defining host
routine, bit for bit on every output tensor and every count -- the seeded scenes, the hand-written cases, the sizes at which a kernel can
go wrong (an image's list around the ballot steps, images around a wave and around the block of reg_rank_kernel, tracks around a block, a
long track), no candidate at all, device-side error bits -- then register_images and the reconstruction chains, GPU against CPU."""
import numpy as np
import pytest
import torch

import loftr_amd
from loftr_amd import Registration, _lib, build as build_mod, ops
import _bundle_cases as BC
import _registration_cases as RC
import _triangulation_cases as TC

pytestmark = pytest.mark.gpu
B = RC.RANK_BLOCK                                                       # b: the images reg_rank_kernel takes per step
MIN_CORR = MIN_INLIERS = 6


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    assert ops.REGISTER_RANK_BLOCK == B
    return _lib.load()


def _equal(g, w, what):
    g, w = g.cpu(), torch.as_tensor(w)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    if g.dtype.is_floating_point:
        assert torch.equal(torch.isnan(g), torch.isnan(w)), (what, "NaN positions")
        g, w = torch.nan_to_num(g, nan=0.0), torch.nan_to_num(w, nan=0.0)
    assert torch.equal(g, w), (what, int((g != w).sum()))


def both(c, what):
    """Case c through the host routine and through the kernels; asserts equality of every output (rows past P / C are zero on both
    sides) -> the host result."""
    want = ops.register_corr_host(*RC.args(c))
    got = ops.register_corr(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in RC.args(c)[:-1]], c["min_corr"])
    assert sorted(got) == sorted(want) == sorted(RC.OUT)
    for k in RC.OUT:
        assert got[k].is_cuda
        _equal(got[k], want[k], (what, k))
    return want


@pytest.mark.parametrize("name", sorted(RC.scene_cases()))
def test_scenes_equal_the_host_routine(lib, name):
    want = both(RC.scene_cases()[name], name)
    assert want["counts"][1] >= 1 and want["counts"][0] >= 4


def test_hand_written_cases(lib):
    cases = RC.edge_cases()
    for name in sorted(cases):
        want = both(cases[name], name)
        if name in ("all_posed", "no_candidate", "T=0", "N=0", "n=0"):
            assert want["counts"][:2].tolist() == [0, 0], name          # P = 0
    assert both(cases["hand"], "hand")["counts"].tolist() == [9, 2, 0, 4, 3, 12, 5, 0]
    assert both(cases["min_corr_5"], "min_corr_5")["counts"][:2].tolist() == [5, 1]


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 129, 4097])
def test_a_list_around_the_ballot_steps(lib, k):
    want = both(RC.list_case(k), k)
    assert want["counts"][6] <= max(k, 9) and (k < 20 or want["counts"][1] == 2)


@pytest.mark.parametrize("n", [1, 63, 64, 65, B - 1, B, B + 1, 4097])
def test_images_around_a_wave_and_the_rank_block(lib, n):
    want = both(RC.images_case(n), n)
    assert n < 63 or 0 < want["counts"][1] < n


@pytest.mark.parametrize("T", [1, 3, 257, 4097])
def test_tracks_around_a_block(lib, T):
    both(RC.random_case(50 + T, 7, T, 9), T)


def test_a_long_track_and_many_images(lib):
    assert both(RC.long_track(), "long track")["counts"][1] >= 1
    both(RC.random_case(61, 700, 3000, 12, min_corr=30), "700 images")


@pytest.mark.parametrize("name,case,bit", RC.bad_inputs(), ids=[b[0] for b in RC.bad_inputs()])
def test_device_side_error_bits(lib, name, case, bit):
    got = ops.register_corr(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in RC.args(case)[:-1]], 4)
    counts = got["counts"].cpu().tolist()
    assert counts[2] & bit and counts[:2] == [0, 0] and counts[3:] == [0] * 5, (name, counts)
    for k in RC.OUT[:-1]:
        assert not got[k].any(), (name, k)                              # nothing written


def test_register_images_raises_on_device_side_errors(lib):
    s = BC.scene_a()
    T = len(s["offsets"]) - 1
    a = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (s["offsets"], s["obs_image"], s["obs_xy"], s["xyz"], np.zeros(T, np.uint8), s["K"],
                                                                     s["T_true"], np.zeros(5, bool))]
    bad = a[1].clone()
    bad[3] = 5
    with pytest.raises(ValueError, match=r"obs_image outside .* \(found on the device\)"):
        loftr_amd.register_images(a[0], bad, *a[2:], min_corr=4, min_inliers=4)
    off = a[0].clone()
    off[3] = off[2] - 1
    with pytest.raises(ValueError, match=r"offsets must start at 0.* \(found on the device\)"):
        loftr_amd.register_images(off, *a[1:], min_corr=4, min_inliers=4)


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def test_register_images_equals_the_cpu_call(lib):
    s = BC.scene_b()
    pts = loftr_amd.triangulate_tracks(s["offsets"], s["obs_image"], s["obs_xy"], s["K"], s["T_true"])
    posed = np.zeros(12, bool)
    posed[[0, 1, 4, 7]] = True
    T_in = s["T_true"].copy()
    T_in[~posed] = np.nan
    a = [s["offsets"], s["obs_image"], s["obs_xy"], pts.xyz.numpy(), pts.status.numpy(), s["K"], T_in, posed]
    for kw in (dict(min_corr=60, min_inliers=55, seed=3), dict(min_corr=4, min_inliers=70), dict(min_corr=500, min_inliers=4)):
        want = loftr_amd.register_images(*a, **kw)
        timings = []
        got = loftr_amd.register_images(*[_cuda(x) for x in a], timings=timings, **kw)
        for k in Registration.FIELDS:
            assert getattr(got, k).is_cuda
            _equal(getattr(got, k), getattr(want, k), (kw, k))
        assert got.stats == want.stats and [t[0] for t in timings] == list(ops.REGISTER_STAGES)
    assert want.stats["n_candidates"] == 0                              # the last one: P = 0, no estimator call


def test_reconstruct_tracks_equals_the_cpu_chain(lib):
    s = BC.scene_b()
    R = s["T_true"][1, :3, :3] @ s["T_true"][0, :3, :3].T
    t = s["T_true"][1, :3, 3] - R @ s["T_true"][0, :3, 3]
    a = [s["offsets"], s["obs_image"], s["obs_xy"], s["K"]]
    want = loftr_amd.reconstruct_tracks(*a, (0, 1, R, t), min_corr=MIN_CORR, min_inliers=MIN_INLIERS)
    got = loftr_amd.reconstruct_tracks(*[_cuda(x) for x in a], (0, 1, R, t), min_corr=MIN_CORR, min_inliers=MIN_INLIERS)
    assert want.posed.all() and got.T_cam_from_world.is_cuda and got.points.xyz.is_cuda
    for k in ("T_cam_from_world", "posed", "round_registered"):
        _equal(getattr(got, k), getattr(want, k), k)
    _equal(got.points.xyz, want.points.xyz, "xyz")
    assert got.stats == want.stats


def test_sfm_reconstruct_equals_the_cpu_chain(lib):
    s = TC.sfm_scene()
    want = TC.run_atlas("cpu").reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS)
    got = TC.run_atlas("cuda").reconstruct(torch.from_numpy(s["K"]).cuda(), min_corr=MIN_CORR, min_inliers=MIN_INLIERS)
    assert want.posed.all() and got.stats["init_row"] == want.stats["init_row"] and got.stats["pair_inliers"] == want.stats["pair_inliers"]
    for k in ("T_cam_from_world", "posed", "round_registered"):
        _equal(getattr(got, k), getattr(want, k), k)
    _equal(got.points.xyz, want.points.xyz, "xyz")
    _equal(got.points.offsets, want.points.offsets, "offsets")
