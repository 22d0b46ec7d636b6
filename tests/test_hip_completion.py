"""GPU tests of track completion: the kernels of csrc/complete_gpu.hip against the host routine, torch.equal on kp_row_new,
link_r2 (compared as int32) and the counts, on the split scene, the hand-written cases and tables sized for the edges of the kernels
(rows around a wave and a workgroup, images around a chunk of LOFTR_COMPLETE_IMAGE_CHUNK = 64, an image with 0 / 1 / 4097 keypoints, a
row of 70 observations, 4096 rows contending for one keypoint, reach 0 and 8 at the grid corners); the error bits raised on the device;
SfmResult.complete and SfmResult.reconstruct(complete=True) GPU against CPU on every field."""
import numpy as np
import pytest
import torch

import _completion_cases as CC
import loftr_amd
from loftr_amd import ops

pytestmark = pytest.mark.gpu
MIN_CORR = MIN_INLIERS = 6

SIZED = {
    "rows_1": dict(seed=2, n_points=1, rows_per_point=1, posed_rate=1.0), "images_1": dict(seed=2, n_images=1, posed_rate=1.0),      # (seeds with links)
    **{f"rows_{r}": dict(seed=10 + r, n_points=r, rows_per_point=1, posed_rate=1.0) for r in (63, 64, 65, 257)},
    **{f"images_{n}": dict(seed=20 + n, n_images=n, posed_rate=1.0) for n in (2, 63, 64, 65)},
    "keypoints_0_1_4097": dict(seed=31, n_images=5, kp_per_image={0: 0, 1: 1, 2: 4097}, posed_rate=1.0),
    "row_of_70": dict(seed=32, n_images=80, n_points=12, row_views=70, posed_rate=1.0),
    "random_a": dict(seed=1), "random_b": dict(seed=2),
}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def run_both(t, dev, reach=None, timings=None):
    a = CC.args(t, reach)
    host = ops.complete_tracks_host(*a)
    gpu = ops.complete_tracks(*[torch.from_numpy(x).to(dev) for x in a[:11]], *a[11:], timings=timings)
    return host, {k: v.cpu() for k, v in gpu.items()}


def same(gpu, host):
    assert torch.equal(gpu["counts"], torch.from_numpy(host["counts"])), (gpu["counts"].tolist(), host["counts"].tolist())
    assert torch.equal(gpu["kp_row_new"], torch.from_numpy(host["kp_row_new"]))
    assert torch.equal(gpu["link_r2"].view(torch.int32), torch.from_numpy(host["link_r2"]).view(torch.int32))


def test_split_scene(dev):
    t, expected, detached = CC.split_scene()
    timings = []
    host, gpu = run_both(t, dev, timings=timings)
    same(gpu, host)
    assert np.array_equal(gpu["kp_row_new"].numpy(), expected) and gpu["counts"][0] == detached.sum()
    assert [s for s, _ in timings] == list(ops.COMPLETE_STAGES) and all(ms >= 0 for _, ms in timings)


@pytest.mark.parametrize("reach", (0, 1, 2))
def test_hand_cases(dev, reach):
    t, notes = CC.hand()
    host, gpu = run_both(t, dev, reach)
    same(gpu, host)
    CC.check_hand(t, notes, {k: v.numpy() for k, v in gpu.items()}, reach)


def test_no_rows_no_keypoints_no_images(dev):
    for name, t in CC.empties().items():
        host, gpu = run_both(t, dev)
        same(gpu, host)


@pytest.mark.parametrize("name", sorted(SIZED))
def test_sized_tables(dev, name):
    t = CC.random_table(**SIZED[name])
    host, gpu = run_both(t, dev)
    same(gpu, host)
    if name == "keypoints_0_1_4097":
        assert np.diff(t["kp_offsets"])[:3].tolist() == [0, 1, 4097]
    if name == "row_of_70":
        assert t["offsets"][1] == 70
    assert host["counts"][0] > 0                                          # every table has links to get wrong
    if name.startswith("random"):
        assert host["counts"][0] > 10 and host["counts"][6] > 0 and host["counts"][7] > 0


def test_4096_rows_contend_for_one_keypoint(dev):
    t = CC.random_table(5, n_images=2, n_points=4096, rows_per_point=1, identical=True)
    host, gpu = run_both(t, dev)
    same(gpu, host)
    assert len(t["kp_row"]) == 1 and gpu["kp_row_new"].tolist() == [0] and gpu["counts"].tolist() == [1, 0, 4096, 4096, 4096, 4096, 4095, 0]


@pytest.mark.parametrize("reach", (0, 8))
def test_grid_corners(dev, reach):
    t = CC.corners(reach)
    host, gpu = run_both(t, dev)
    same(gpu, host)
    assert host["counts"][4] == 4 and host["counts"][0] >= 3


@pytest.mark.parametrize("bit", (1, 2, 4, 8))
def test_error_bits_raised_on_the_device(dev, bit):
    """the check kernel meets the bad value before anything is read through it; the link kernel then returns at once"""
    t = CC.bad_tables()[bit]
    a = CC.args(t)
    gpu = {k: v.cpu() for k, v in ops.complete_tracks(*[torch.from_numpy(x).to(dev) for x in a[:11]], *a[11:]).items()}
    assert gpu["counts"].tolist() == [0, bit, 0, 0, 0, 0, 0, 0]
    assert torch.equal(gpu["kp_row_new"], torch.from_numpy(t["kp_row"])) and torch.isnan(gpu["link_r2"]).all()
    kw = dict(offsets=t["offsets"], obs_image=t["obs_image"], kp_offsets=t["kp_offsets"], keypoints=t["keypoints"], kp_row=t["kp_row"], xyz=t["xyz"],
              status=t["status"], K=t["K"], T_cam_from_world=t["T_cam_from_world"], posed=t["posed"])
    with pytest.raises(ValueError, match="found on the device"):
        loftr_amd.complete_tracks(**{k: torch.from_numpy(v).to(dev) for k, v in kw.items()}, image_hw=CC.HW, cell_px=CC.CELL)


def _equal(a, b):
    a, b = a.cpu(), b.cpu()
    if a.is_floating_point():                                             # NaN-safe: the bits
        it = torch.int64 if a.element_size() == 8 else torch.int32
        return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))
    return torch.equal(a, b)


def test_sfm_complete_gpu_against_cpu(dev):
    (cpu, s, cut), (gpu, _, _) = CC.split_atlas("cpu"), CC.split_atlas("cuda")
    out = []
    for sfm in (cpu, gpu):
        pts = sfm.triangulate(s["K"], s["T"])
        sfm2, done = sfm.complete(pts, s["K"], s["T"])
        out.append((sfm2, done))
    (c2, cd), (g2, gd) = out
    assert gd.stats == cd.stats and cd.stats["n_links"] == int(cut.sum())
    assert g2.track_id.is_cuda and gd.kp_row_new.is_cuda
    for k in c2.FIELDS:
        assert _equal(getattr(g2, k), getattr(c2, k)), k
    for k in cd.FIELDS:
        assert _equal(getattr(gd, k), getattr(cd, k)), k


def test_reconstruct_complete_gpu_against_cpu(dev):
    (cpu, s, cut), (gpu, _, _) = CC.split_atlas("cpu"), CC.split_atlas("cuda")
    c = cpu.reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS, complete=True)
    g = gpu.reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS, complete=True)
    assert g.stats["completion"] == c.stats["completion"] and c.stats["completion"]["n_links"] == int(cut.sum())
    for k in ("T_cam_from_world", "posed", "round_registered", "K"):
        assert _equal(getattr(g, k), getattr(c, k)), k
    for k in loftr_amd.Points3D.FIELDS + ("offsets", "image", "keypoint"):
        assert _equal(getattr(g.points, k), getattr(c.points, k)), k
    for k in c.sfm.FIELDS:
        assert _equal(getattr(g.sfm, k), getattr(c.sfm, k)), k
    assert g.points.stats == c.points.stats and g.bundle.rms_px_after == c.bundle.rms_px_after
