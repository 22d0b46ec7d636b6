"""GPU tests of track merging: the kernels of csrc/merge_gpu.hip against the host routine, torch.equal on row_into, merge_r2
(compared as int32), kp_row_new and the counts, on the twin scene, the hand-written cases and tables sized for the edges of the kernels
(rows around a wave and a workgroup, images around a chunk of LOFTR_MERGE_IMAGE_CHUNK = 64, an image with 0 / 1 / 4097 keypoints, a row
of 70 observations merging with a row of 2, 512 rows all accepted against row 0 with equal scores over three chunks, reach 0 and 8 at the
grid corners); the error bits raised on the device; SfmResult.merge and SfmResult.reconstruct(merge=True) GPU against CPU on every
field."""
import numpy as np
import pytest
import torch

import _merge_cases as MC
import loftr_amd
from loftr_amd import ops

pytestmark = pytest.mark.gpu
MIN_CORR = MIN_INLIERS = 6

SIZED = {
    **{f"rows_{r}": dict(n_rows=r, n_images=7, seed=10 + r) for r in (1, 63, 64, 65, 257)},
    **{f"images_{n}": dict(n_rows=40, n_images=n, seed=20 + n) for n in (1, 2, 63, 64, 65)},
    "keypoints_0_1_4097": dict(n_rows=30, n_images=7, seed=31, views=(1, 2), kp_per_image={2: 4097}),
}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def run_both(t, dev, reach=None, timings=None):
    a = MC.args(t, reach)
    host = ops.merge_tracks_host(*a)
    gpu = ops.merge_tracks(*[torch.from_numpy(x).to(dev) for x in a[:13]], *a[13:], timings=timings)
    return host, {k: v.cpu() for k, v in gpu.items()}


def same(gpu, host):
    assert torch.equal(gpu["counts"], torch.from_numpy(host["counts"])), (gpu["counts"].tolist(), host["counts"].tolist())
    assert torch.equal(gpu["row_into"], torch.from_numpy(host["row_into"]))
    assert torch.equal(gpu["merge_r2"].view(torch.int32), torch.from_numpy(host["merge_r2"]).view(torch.int32))
    assert torch.equal(gpu["kp_row_new"], torch.from_numpy(host["kp_row_new"]))


def test_twin_scene(dev):
    t, row_into, kp_row_new, twins = MC.twin_scene()
    timings = []
    host, gpu = run_both(t, dev, timings=timings)
    same(gpu, host)
    MC.check_twins(t, {k: v.numpy() for k, v in gpu.items()}, row_into, kp_row_new, twins)
    assert [s for s, _ in timings] == list(ops.MERGE_STAGES) and all(ms >= 0 for _, ms in timings)


def test_hand_cases(dev):
    t, notes = MC.hand()
    host, gpu = run_both(t, dev)
    same(gpu, host)
    MC.check_hand(t, notes, {k: v.numpy() for k, v in gpu.items()})
    for reach in (0, 1, 8):
        same(*run_both(t, dev, reach)[::-1])


def test_no_rows_no_keypoints_no_images(dev):
    for name, t in MC.empties().items():
        host, gpu = run_both(t, dev)
        same(gpu, host)


@pytest.mark.parametrize("name", sorted(SIZED))
def test_sized_tables(dev, name):
    kw = dict(SIZED[name])
    if name == "keypoints_0_1_4097":                                       # image 0 emptied, image 1 cut down to one keypoint, image 2 filled up
        t = MC.sized(**kw)
        t = _drop_image_0_and_thin_image_1(t)
        assert np.diff(t["kp_offsets"])[:3].tolist() == [0, 1, 4097]
    else:
        t = MC.sized(**kw)
    host, gpu = run_both(t, dev)
    same(gpu, host)
    if name not in ("rows_1", "images_1"):                                 # (one row, or one image, meets nothing)
        assert host["counts"][0] > 0 and host["counts"][4] >= host["counts"][6] > host["counts"][0]
    else:
        assert host["counts"][2] > 0 and host["counts"][4] == 0


def _drop_image_0_and_thin_image_1(t):
    """the keypoints of image 0 are dropped and image 1 keeps its first keypoint only; the rows keep their observations (a keypoint per
    observation is the atlas's habit, not the rule's requirement)"""
    image = np.repeat(np.arange(len(t["posed"])), np.diff(t["kp_offsets"]))
    keep = (image > 1) | ((image == 1) & (np.arange(len(image)) == t["kp_offsets"][1]))
    out = dict(t)
    for k in ("keypoints", "kp_cell", "kp_row"):
        out[k] = np.ascontiguousarray(t[k][keep])
    out["kp_offsets"] = np.concatenate([[0], np.cumsum(np.bincount(image[keep], minlength=len(t["posed"])))]).astype(np.int64)
    return out


@pytest.mark.parametrize("seed", (1, 2))
def test_random_tables(dev, seed):
    t = MC.random_table(seed)
    host, gpu = run_both(t, dev)
    same(gpu, host)
    assert host["counts"][0] >= 3 and host["counts"][4] > host["counts"][5] > host["counts"][6]


def test_a_row_of_70_merges_with_a_row_of_2(dev):
    t = MC.long_and_short()
    host, gpu = run_both(t, dev)
    same(gpu, host)
    assert np.diff(t["offsets"]).tolist() == [70, 2] and gpu["row_into"].tolist() == [0, 0] and gpu["counts"][0] == 1


def test_512_rows_accepted_against_row_0_with_equal_scores(dev):
    t = MC.star()
    host, gpu = run_both(t, dev)
    same(gpu, host)
    assert len(t["posed"]) == 130 and (np.diff(t["kp_offsets"])[1:129] == 8).sum() >= 126
    assert gpu["counts"][0] == 1 and gpu["counts"][6] == 128 + 511 and gpu["row_into"][:3].tolist() == [0, 0, 2]
    assert torch.equal(gpu["row_into"][2:], torch.arange(2, 512, dtype=torch.int32))


@pytest.mark.parametrize("reach", (0, 8))
def test_grid_corners(dev, reach):
    t = MC.corners(reach)
    host, gpu = run_both(t, dev)
    same(gpu, host)
    assert host["counts"][0] == 4


@pytest.mark.parametrize("bit", (1, 2, 4, 8))
def test_error_bits_raised_on_the_device(dev, bit):
    """the check kernel meets the bad value before anything is read through it; the meet kernel then returns at once and the relabel
    kernel copies kp_row"""
    t = MC.bad_tables()[bit]
    a = MC.args(t)
    gpu = {k: v.cpu() for k, v in ops.merge_tracks(*[torch.from_numpy(x).to(dev) for x in a[:13]], *a[13:]).items()}
    assert gpu["counts"].tolist() == [0, bit, 0, 0, 0, 0, 0, 0]
    assert torch.equal(gpu["kp_row_new"], torch.from_numpy(t["kp_row"])) and torch.isnan(gpu["merge_r2"]).all()
    assert torch.equal(gpu["row_into"], torch.arange(len(t["status"]), dtype=torch.int32))
    kw = {k: t[k] for k in ("offsets", "obs_image", "obs_xy", "obs_mask", "kp_offsets", "keypoints", "kp_row", "xyz", "status", "K",
                            "T_cam_from_world", "posed")}
    with pytest.raises(ValueError, match="found on the device"):
        loftr_amd.merge_tracks(**{k: torch.from_numpy(v).to(dev) for k, v in kw.items()}, image_hw=MC.CC.HW, cell_px=MC.CC.CELL)


def _equal(a, b):
    a, b = a.cpu(), b.cpu()
    if a.is_floating_point():                                             # NaN-safe: the bits
        it = torch.int64 if a.element_size() == 8 else torch.int32
        return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))
    return torch.equal(a, b)


def test_sfm_merge_gpu_against_cpu(dev):
    (cpu, s, cut), (gpu, _, _) = MC.twin_atlas("cpu"), MC.twin_atlas("cuda")
    out = []
    for sfm in (cpu, gpu):
        pts = sfm.triangulate(s["K"], s["T"])
        out.append(sfm.merge(pts, s["K"], s["T"]))
    (c2, cd), (g2, gd) = out
    assert gd.stats == cd.stats and cd.stats["n_merges"] == int(cut.sum())
    assert g2.track_id.is_cuda and gd.kp_row_new.is_cuda
    for k in c2.FIELDS:
        assert _equal(getattr(g2, k), getattr(c2, k)), k
    for k in cd.FIELDS:
        assert _equal(getattr(gd, k), getattr(cd, k)), k


def test_reconstruct_merge_gpu_against_cpu(dev):
    (cpu, s, cut), (gpu, _, _) = MC.twin_atlas("cpu"), MC.twin_atlas("cuda")
    c = cpu.reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS, merge=True)
    g = gpu.reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS, merge=True)
    assert g.stats["merge"] == c.stats["merge"] and c.stats["merge"]["n_merges"] == int(cut.sum())
    for k in ("T_cam_from_world", "posed", "round_registered", "K"):
        assert _equal(getattr(g, k), getattr(c, k)), k
    for k in loftr_amd.Points3D.FIELDS + ("offsets", "image", "keypoint"):
        assert _equal(getattr(g.points, k), getattr(c.points, k)), k
    for k in c.sfm.FIELDS:
        assert _equal(getattr(g.sfm, k), getattr(c.sfm, k)), k
    assert g.points.stats == c.points.stats and g.bundle.rms_px_after == c.bundle.rms_px_after
