"""View-graph calibration on the GPU (csrc/calib_gpu.hip): every output of the kernels is bit for bit the host routine's,
at the wave and chunk edges of the edge count, of the image count and of one group's incidence list, with one camera for all images,
with invalid edges and held groups spread over those sizes, for every error bit, and through the chain of SfmResult.calibrate and
reconstruct_uncalibrated.  At the edge sizes the iteration limits are small so that the fixed launch schedule stays short."""
import numpy as np
import pytest
import torch

import _calibration_cases as CC
from loftr_amd import calibration, ops_calib

pytestmark = pytest.mark.gpu

SHORT = dict(max_iters=4, pcg_iters=6)


def both(a, **kw):
    """-> the host routine's outputs; asserts that the kernels give the same bytes in every output."""
    want = ops_calib.calibrate_view_graph_host(*a, **kw)
    got = ops_calib.calibrate_view_graph(*[torch.from_numpy(x).cuda() for x in a], **kw)
    torch.cuda.synchronize()
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])) and got[k].cpu().numpy().tobytes() == want[k].tobytes(), (k, kw)
    return want


@pytest.mark.parametrize("E", (1, 63, 64, 65, 4095, 4096, 4097))
def test_edge_counts_at_the_wave_and_chunk_edges(E):
    a = CC.synthetic(E, max(2, min(E + 1, 40)), seed=E)
    out = both(a, **SHORT)
    assert out["counts"][1] == 0 and out["counts"][4] == E and out["counts"][0] >= 1 and (out["group_state"] == 2).all()
    both(a, prior_weight=0.0, **SHORT)


@pytest.mark.parametrize("n,topology", ((2, "path"), (3, "path"), (64, "star"), (65, "path"), (1025, "path"), (1025, "star")))
def test_image_counts(n, topology):
    """1025 images: more groups than a block of group threads, more waves than a block of group waves; the star's hub list is 2048 long."""
    a = CC.synthetic(2 * (n - 1) if n > 2 else 3, n, seed=n, topology=topology)
    out = both(a, **SHORT)
    assert out["counts"][1] == 0 and out["counts"][5] == n and out["counts"][0] >= 1


@pytest.mark.parametrize("count", (1, 64, 65, 4097))
def test_one_incidence_list_at_the_wave_edges(count):
    a = CC.synthetic(count, min(count + 1, 30), seed=count, topology="star")
    assert a[6][1] - a[6][0] == count                                      # image 0 is on every edge
    out = both(a, **SHORT)
    assert out["counts"][1] == 0 and out["group_state"][0] == 2


@pytest.mark.parametrize("E", (1, 32, 33, 2049))
def test_one_camera_for_all_images(E):
    """G = 1: both ends of every edge lie in the one group, whose list has 2E = 2, 64, 66, 4098 entries."""
    a = CC.synthetic(E, min(E + 1, 20), seed=E, one_camera=True)
    assert len(a[6]) == 2 and a[6][1] == 2 * E
    out = both(a, **SHORT)
    assert out["counts"][1] == 0 and out["counts"][5] == 1 and out["focal_scale"].shape == (1,)


@pytest.mark.parametrize("name,kw", CC.GENERAL[:1] + CC.PLANTED[:1] + CC.SHARED, ids=lambda x: x if isinstance(x, str) else "")
def test_scenes_with_the_default_limits(name, kw):
    sc = CC.ring(**kw)
    out = both(CC.raw_args(sc))
    assert out["counts"][7] == 0 and np.abs(out["focal"] / sc.f_true - 1).max() <= 0.05


@pytest.mark.parametrize("pcg_iters", (0, 1))
def test_few_conjugate_gradient_iterations(pcg_iters):
    a = CC.raw_args(CC.small())
    out = both(a, max_iters=3, pcg_iters=pcg_iters)
    assert out["counts"][3] <= 3 * pcg_iters and out["counts"][0] == 3
    start = both(a, max_iters=0, pcg_iters=4)
    assert start["counts"][0] == 0 and start["info"][0] == start["info"][1] and (start["focal_scale"] == 1).all()


def test_a_bound_rejection():
    a = CC.raw_args(CC.ring(**dict(CC.GENERAL)["ring12"]))
    out = both(a, bound_lo=0.9, bound_hi=1.1, max_iters=12, pcg_iters=8)
    assert out["counts"][8] > 0 and (out["focal_scale"] > 0.9).all() and (out["focal_scale"] < 1.1).all()


LARGE = (("edges4097", lambda: CC.synthetic(4097, 40, seed=1)), ("images1025_path", lambda: CC.synthetic(2048, 1025, seed=2)),
         ("images1025_star", lambda: CC.synthetic(2048, 1025, seed=3, topology="star")),
         ("one_camera4098", lambda: CC.synthetic(2049, 20, seed=4, one_camera=True)))


@pytest.mark.parametrize("name,make", LARGE, ids=[c[0] for c in LARGE])
@pytest.mark.parametrize("min_edges", (1, 4))
def test_invalid_edges_and_held_groups_at_the_edge_sizes(name, make, min_edges):
    """weight 0 on every 7th edge, a NaN on every 11th: invalid edges sit in the middle and at the tail of waves and chunks, the counters
    run over many waves; min_edges = 4 holds the images of the 1025-image graphs that keep fewer valid edge ends."""
    a = CC.spoiled(make())
    out = both(a, min_edges=min_edges, **SHORT)
    E = len(a[0])
    bad = (np.arange(E) % 7 == 0) | (np.arange(E) % 11 == 0)
    assert out["counts"][1] == 0 and out["counts"][4] == E - bad.sum() and np.array_equal(out["edge_state"] == 0, bad)
    assert not out["edge_resid"][bad].any() and (out["edge_resid"][~bad] > 0).all()
    if min_edges == 4 and name.startswith("images1025"):
        assert (out["group_state"] == 1).any() and (out["focal_scale"][out["group_state"] == 1] == 1).all()
    start = both(a, min_edges=min_edges, max_iters=0, pcg_iters=4)
    assert start["counts"][0] == 0 and np.array_equal(start["group_state"], out["group_state"])
    both(a, min_edges=min_edges, max_iters=2, pcg_iters=1, prior_weight=0.0)


_SMALL_ERRORS = CC.error_cases(lambda: CC.raw_args(CC.small()))
_LARGE_ERRORS = CC.error_cases(lambda: CC.synthetic(4097, 40, seed=1))


@pytest.mark.parametrize("name,a,bit", _SMALL_ERRORS + _LARGE_ERRORS,
                         ids=[f"small-{c[0]}" for c in _SMALL_ERRORS] + [f"edges4097-{c[0]}" for c in _LARGE_ERRORS])
def test_error_bits(name, a, bit):
    out = both(a, **SHORT)
    assert out["counts"][1] & bit and out["counts"].sum() == out["counts"][1] and not any(out[k].any() for k in out if k != "counts")


def test_wrapper_and_timings():
    sc = CC.ring(**dict(CC.SHARED)["hub"])
    timings = []
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    got = calibration.calibrate_view_graph(dev(sc.edge_image), dev(sc.edge_F), dev(sc.edge_weight), sc.n, dev(sc.pp), dev(sc.f0),
                                           camera_ids=dev(sc.camera_ids), timings=timings, **SHORT)
    want = calibration.calibrate_view_graph(sc.edge_image, sc.edge_F, sc.edge_weight, sc.n, sc.pp, sc.f0, camera_ids=sc.camera_ids, **SHORT)
    assert [s for s, _ in timings] == list(ops_calib.CALIB_STAGES) and all(ms >= 0 for _, ms in timings)
    for k in calibration.ViewGraphCalibration.FIELDS:
        assert getattr(got, k).is_cuda and getattr(got, k).cpu().numpy().tobytes() == getattr(want, k).numpy().tobytes(), k
    assert got.stats == want.stats and torch.equal(got.edge_ok.cpu(), want.edge_ok) and torch.equal(got.focal_ok.cpu(), want.focal_ok)
    with pytest.raises(ValueError, match="edge image outside"):
        bad = sc.edge_image.copy()
        bad[0, 0] = sc.n
        calibration.calibrate_view_graph(dev(bad), dev(sc.edge_F), dev(sc.edge_weight), sc.n, dev(sc.pp), dev(sc.f0))
    with pytest.raises(Exception, match="GPU and CPU arguments mixed"):
        calibration.calibrate_view_graph(dev(sc.edge_image), sc.edge_F, dev(sc.edge_weight), sc.n, dev(sc.pp), dev(sc.f0))


def test_uncalibrated_chain_matches_the_cpu_chain():
    """Figures (profiles/calibration_accuracy.txt): uncalibrated focal 6.16e-3, centre 2.45e-2; yardstick focal 5.98e-3, centre 2.46e-2."""
    sfm_c, sc = CC.atlas_scene("cpu")
    sfm_g, _ = CC.atlas_scene("cuda")
    Fc, nc = sfm_c.pairwise_fundamentals()
    Fg, ng = sfm_g.pairwise_fundamentals()
    assert Fg.is_cuda and torch.equal(Fg.cpu(), Fc) and torch.equal(ng.cpu(), nc)
    cal_c, cal_g = sfm_c.calibrate(), sfm_g.calibrate()
    for k in calibration.ViewGraphCalibration.FIELDS:
        assert getattr(cal_g, k).is_cuda and getattr(cal_g, k).cpu().numpy().tobytes() == getattr(cal_c, k).numpy().tobytes(), k
    assert cal_g.stats == cal_c.stats
    cpu, gpu = sfm_c.reconstruct_uncalibrated(), sfm_g.reconstruct_uncalibrated()
    assert gpu.T_cam_from_world.is_cuda and gpu.calibration.focal.is_cuda and bool(gpu.posed.all())
    assert gpu.T_cam_from_world.cpu().numpy().tobytes() == cpu.T_cam_from_world.numpy().tobytes()          # the same poses bit for bit
    assert gpu.K.cpu().numpy().tobytes() == cpu.K.numpy().tobytes()
    ref = sfm_g.reconstruct(torch.from_numpy(sc.K_true).cuda(), ba={"refine_focal": True})                 # the yardstick, on the GPU
    (fu, cu), (fy, cy) = CC.reconstruction_errors(gpu, sc), CC.reconstruction_errors(ref, sc)
    print(f"uncalibrated: focal {fu:.3e}, centre {cu:.3e}; yardstick: focal {fy:.3e}, centre {cy:.3e}")
    assert fu <= fy + 2e-3 and cu <= cy + 2.5e-3                                                           # the recorded margins
