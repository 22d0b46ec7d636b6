"""CPU tests of track completion: the host routine loftr_complete_tracks_host against the independent numpy statement of
the rule (tests/_completion_oracle.py) with bit equality, the split scene against its exact expected result, the hand-written cases, the
error bits, SfmResult.complete and SfmResult.reconstruct(complete=...).  The kernels are held to the host routine in
tests/test_hip_completion.py."""
import os

import numpy as np
import pytest
import torch

import _completion_cases as CC
import _completion_oracle as O
import _triangulation_cases as TC
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_CORR = MIN_INLIERS = 6


@pytest.fixture(scope="module", autouse=True)
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def same(got, want):
    """bit equality of the three outputs"""
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    assert np.array_equal(got["kp_row_new"], want["kp_row_new"]), np.nonzero(got["kp_row_new"] != want["kp_row_new"])[0][:8]
    assert np.array_equal(got["link_r2"].view(np.int32), want["link_r2"].view(np.int32))


def test_split_scene_is_completed_exactly():
    t, expected, detached = CC.split_scene()
    oracle = O.complete(*CC.args(t))
    CC.check_margins(t, oracle)
    # first the oracle alone against the generator's ground truth ...
    assert detached.sum() > 100 and np.array_equal(oracle["kp_row_new"], expected)
    assert oracle["counts"][0] == detached.sum() and oracle["counts"][6] == 0 and oracle["counts"][7] == 0
    assert np.array_equal(~np.isnan(oracle["link_r2"]), detached)
    # ... then the host routine
    host = ops.complete_tracks_host(*CC.args(t))
    assert np.array_equal(host["kp_row_new"], expected) and host["counts"][0] == detached.sum() and host["counts"][6] == host["counts"][7] == 0
    same(host, oracle)
    cell, status = ops.model_cells_host(t["kp_offsets"], t["keypoints"], t["kp_row"], len(t["status"]), *t["grid"])
    assert status == 0 and np.array_equal(cell, t["kp_cell"]) and np.array_equal(cell, O.cells(t["keypoints"], t["grid"][2], t["grid"][1], t["grid"][0]))


@pytest.mark.parametrize("reach", (0, 1, 2))
def test_hand_cases(reach):
    t, notes = CC.hand()
    oracle = O.complete(*CC.args(t, reach))
    CC.check_margins(t, oracle)
    CC.check_hand(t, notes, oracle, reach)
    host = ops.complete_tracks_host(*CC.args(t, reach))
    CC.check_hand(t, notes, host, reach)
    same(host, oracle)


def test_no_rows_no_keypoints_no_images():
    for name, t in CC.empties().items():
        host = ops.complete_tracks_host(*CC.args(t))
        same(host, O.complete(*CC.args(t)))
        assert host["counts"][0] == 0 and host["counts"][1] == 0, name
        assert np.array_equal(host["kp_row_new"], t["kp_row"]) and np.isnan(host["link_r2"]).all(), name


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_random_tables(seed):
    t = CC.random_table(seed)
    oracle = O.complete(*CC.args(t))
    assert oracle["counts"][0] > 10 and oracle["counts"][6] > 0 and oracle["counts"][7] > 0          # links, lost proposals and blocked pairs
    same(ops.complete_tracks_host(*CC.args(t)), oracle)


@pytest.mark.parametrize("reach", (0, 8))
def test_grid_corners(reach):
    t = CC.corners(reach)
    oracle = O.complete(*CC.args(t))
    assert oracle["counts"][4] == 4 and oracle["counts"][0] >= 3
    same(ops.complete_tracks_host(*CC.args(t)), oracle)


def _as_call(t, **over):
    """the arguments of loftr_amd.complete_tracks from a table"""
    kw = dict(offsets=t["offsets"], obs_image=t["obs_image"], kp_offsets=t["kp_offsets"], keypoints=t["keypoints"], kp_row=t["kp_row"], xyz=t["xyz"],
              status=t["status"], K=t["K"], T_cam_from_world=t["T_cam_from_world"], image_hw=CC.HW, cell_px=CC.CELL, posed=t["posed"],
              thresh_px=t["thresh_px"], reach=t["reach"])
    kw.update(over)
    return kw


@pytest.mark.parametrize("bit", (1, 2, 4, 8))
def test_every_error_bit_is_a_value_error(lib, bit):
    import ctypes
    t = CC.bad_tables()[bit]
    assert O.complete(*CC.args(t)) == dict(error=bit)
    text = {1: "obs_image outside", 2: "offsets must start at 0", 4: "must not descend within a row", 8: r"kp_row outside \[-1, T\)"}[bit]
    with pytest.raises(ValueError, match=text):
        loftr_amd.complete_tracks(**_as_call(t))
    with pytest.raises(ValueError, match=text):
        loftr_amd.complete_tracks(**{k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in _as_call(t).items()})
    a = CC.args(t)
    out = [np.full(len(t["kp_row"]), 7, np.int32), np.full(len(t["kp_row"]), 7, np.float32), np.full(8, 7, np.int64)]
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    st = lib.loftr_complete_tracks_host(p(a[0]), len(a[0]) - 1, p(a[1]), len(a[1]), p(a[2]), p(a[3]), p(a[4]), p(a[5]), p(a[6]), p(a[7]), len(a[7]),
                                        p(a[8]), p(a[9]), p(a[10]), len(a[10]), a[13], a[11], a[12], a[14], a[15], *[p(x) for x in out])
    assert st == -1 and out[2].tolist() == [0, bit, 0, 0, 0, 0, 0, 0] and (out[0] == 7).all() and (out[1] == 7).all()


def test_python_entry_point_on_the_hand_table():
    t, notes = CC.hand()
    done = loftr_amd.complete_tracks(**_as_call(t))
    host = ops.complete_tracks_host(*CC.args(t))
    assert isinstance(done, loftr_amd.Completion) and loftr_amd.Completion.FIELDS == ("kp_row_new", "link_r2", "linked")
    assert np.array_equal(done.kp_row_new.numpy(), host["kp_row_new"]) and np.array_equal(done.linked.numpy(), ~np.isnan(host["link_r2"]))
    s = done.stats
    assert [s[k] for k in ops.COMPLETE_NAMES if k != "error_bits"] == [int(host["counts"][i]) for i in (0, 2, 3, 4, 5, 6, 7)]
    assert s["n_links"] == 5 and s["n_links_from_loose"] == 4 and s["n_links_from_pointless_rows"] == 1 and s["reach"] == 2
    # reach=None is ceil(thresh_px / cell_px); a threshold too wide for the cells names cell_px
    assert loftr_amd.complete_tracks(**_as_call(t, reach=None)).stats["reach"] == 2
    assert loftr_amd.complete_tracks(**_as_call(t, reach=None, thresh_px=4.5)).stats["reach"] == 3
    with pytest.raises(ValueError, match="cell_px"):
        loftr_amd.complete_tracks(**_as_call(t, reach=None, thresh_px=16.5))
    for bad in (9, -1, 2.0, True):
        with pytest.raises(ValueError, match="cell_px"):
            loftr_amd.complete_tracks(**_as_call(t, reach=bad))
    with pytest.raises(ValueError, match="thresh_px"):
        loftr_amd.complete_tracks(**_as_call(t, thresh_px=float("nan")))
    # posed=None: every image; the unposed image's keypoint is then taken as well
    assert loftr_amd.complete_tracks(**_as_call(t, posed=None)).stats["n_links"] == 6
    # keypoints that do not ascend by cell within an image are refused by the cells' own check
    k = t["keypoints"].copy()
    b = int(t["kp_offsets"][CC.D])
    k[[b, b + 1]] = k[[b + 1, b]]
    with pytest.raises(ValueError, match="cells that do not ascend"):
        loftr_amd.complete_tracks(**_as_call(t, keypoints=k))


def _fields(x):
    return {k: getattr(x, k) for k in x.FIELDS}


def _valid_csr(sfm):
    offsets, image, local = sfm.tracks()
    assert offsets[0] == 0 and offsets[-1] == image.numel() and (offsets[1:] >= offsets[:-1]).all()
    row = torch.repeat_interleave(torch.arange(offsets.numel() - 1), offsets[1:] - offsets[:-1])
    assert torch.unique(row * 1000 + image).numel() == image.numel()                     # no row visits an image twice
    assert (local >= 0).all() and (sfm.kp_offsets[image] + local < sfm.kp_offsets[image + 1]).all()
    assert torch.equal(sfm.track_len.to(torch.int64), torch.bincount(sfm.track_id[sfm.track_id >= 0].to(torch.int64), minlength=sfm.track_len.numel()))
    return offsets, image, local


def test_sfm_complete_on_the_cpu_atlas():
    sfm, s, cut = CC.split_atlas("cpu")
    before = {k: v.clone() for k, v in _fields(sfm).items()}
    pts = sfm.triangulate(s["K"], s["T"])
    sfm2, done = sfm.complete(pts, s["K"], s["T"])
    assert done.stats["n_links"] == int(cut.sum()) and done.stats["n_links_from_pointless_rows"] == int(cut.sum())
    for k, v in _fields(sfm).items():                                                     # self is untouched ...
        assert torch.equal(v, before[k]), k
    for k in sfm.FIELDS:                                                                  # ... and shared, except for the two relabelled fields
        assert (getattr(sfm2, k) is getattr(sfm, k)) == (k not in ("track_id", "track_len")), k
    assert sfm2.image_hw == sfm.image_hw and sfm2.cell_px == sfm.cell_px and torch.equal(sfm2.track_ok, sfm.track_ok)
    _valid_csr(sfm2)
    changed = sfm2.track_id != sfm.track_id
    assert changed.sum() == cut.sum() and torch.equal(changed, done.linked)               # every changed keypoint is a link
    # a claimed keypoint is the true position of a cut point in image 3, and it went to the track of that point's views 0-2
    image = sfm.keypoint_image()
    assert (image[changed] == 3).all()
    first = sfm.kp_offsets[0] + torch.arange(len(cut))[torch.from_numpy(cut)]             # (image 0 holds the points in cell order, not point order)
    kp0 = {tuple(p): k for k, p in enumerate(sfm.keypoints[:sfm.kp_offsets[1]].tolist())}
    for pt in np.nonzero(cut)[0]:
        k3 = int(sfm.kp_offsets[3]) + [tuple(p) for p in sfm.keypoints[sfm.kp_offsets[3]:sfm.kp_offsets[4]].tolist()].index(tuple(s["px"][3][pt].tolist()))
        assert changed[k3] and sfm2.track_id[k3] == sfm.track_id[kp0[tuple(s["px"][0][pt].tolist())]], pt
    assert (sfm2.track_len.sort().values[:int(cut.sum())] == 1).all()                     # the pointless rows keep their other keypoint
    pts2 = sfm2.triangulate(s["K"], s["T"])
    assert pts2.stats["n_too_short"] == cut.sum() and pts2.stats["n_ok"] == pts.stats["n_ok"]
    assert pts2.stats["n_inlier_observations"] == pts.stats["n_inlier_observations"] + cut.sum()
    sfm3, again = sfm2.complete(pts2, s["K"], s["T"])                                     # a second completion runs, and finds nothing new
    assert again.stats["n_links"] == 0 and torch.equal(sfm3.track_id, sfm2.track_id)
    with pytest.raises(ValueError, match="carries no tracks"):
        sfm.complete(loftr_amd.Points3D(pts.stats, **{k: getattr(pts, k) for k in pts.FIELDS}), s["K"], s["T"])
    with pytest.raises(ValueError, match="rows"):
        sfm.complete(sfm.triangulate(s["K"], s["T"], consistent_only=False) if not sfm.track_ok.all() else _short(pts), s["K"], s["T"])


def test_sfm_complete_on_an_atlas_of_whole_tracks():
    """the atlas of _triangulation_cases.run_atlas: every point already is one track of five views, so nothing may change"""
    sfm, s = TC.run_atlas("cpu"), TC.sfm_scene()
    before = {k: v.clone() for k, v in _fields(sfm).items()}
    pts = sfm.triangulate(s["K"], s["T"])
    sfm2, done = sfm.complete(pts, s["K"], s["T"])
    assert done.stats["n_links"] == 0 and done.stats["n_sources"] == 60 and done.stats["n_pairs"] == 0 and not done.linked.any()
    for k, v in _fields(sfm).items():
        assert torch.equal(v, before[k]) and torch.equal(getattr(sfm2, k), v), k
    _valid_csr(sfm2)
    sfm3, again = sfm2.complete(sfm2.triangulate(s["K"], s["T"]), s["K"], s["T"], posed=np.array([1, 1, 0, 1, 1]))
    assert again.stats["n_links"] == 0 and torch.equal(sfm3.track_id, sfm.track_id)


def _short(pts):
    """pts with its last row cut off: no enumeration of the atlas's tracks has that many rows"""
    out = loftr_amd.Points3D(pts.stats, **{k: getattr(pts, k)[:-1] if k != "obs_inlier" else getattr(pts, k) for k in pts.FIELDS})
    out.offsets, out.image, out.keypoint = pts.offsets[:-1], pts.image, pts.keypoint
    return out


def _pose_errors(rec, s):
    """largest rotation error (degrees) and centre error of the reconstruction after aligning it to the truth through image a's pose and
    the scale of the baseline a-b"""
    a, b = rec.stats["init"]
    T = rec.T_cam_from_world.numpy()
    rel_true = [s["T"][i] @ np.linalg.inv(s["T"][a]) for i in range(len(T))]
    scale = np.linalg.norm(rel_true[b][:3, 3]) / np.linalg.norm((T[b] @ np.linalg.inv(T[a]))[:3, 3])
    rot = cen = 0.0
    for i in range(len(T)):
        rel = T[i] @ np.linalg.inv(T[a])
        dR = rel[:3, :3] @ rel_true[i][:3, :3].T
        rot = max(rot, float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))))
        cen = max(cen, float(np.linalg.norm(-rel[:3, :3].T @ rel[:3, 3] * scale + rel_true[i][:3, :3].T @ rel_true[i][:3, 3])))
    return rot, cen


def test_reconstruct_with_and_without_completion():
    sfm, s, cut = CC.split_atlas("cpu")
    plain = sfm.reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS)
    off = sfm.reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS, complete=False)
    # complete=False is today's call: every field
    eq = lambda x, y: torch.equal(x, y) or (x.is_floating_point() and torch.equal(x.contiguous().view(torch.int64 if x.element_size() == 8 else torch.int32),
                                                                                 y.contiguous().view(torch.int64 if y.element_size() == 8 else torch.int32)))
    for k in ("T_cam_from_world", "posed", "round_registered", "K"):
        assert eq(getattr(off, k), getattr(plain, k)), k
    for k in loftr_amd.Points3D.FIELDS + ("offsets", "image", "keypoint"):
        assert eq(getattr(off.points, k), getattr(plain.points, k)), k
    for k in ("T_cam_from_world", "xyz", "obs_active"):
        assert eq(getattr(off.bundle, k), getattr(plain.bundle, k)), k
    assert off.stats == plain.stats and off.sfm is None and "completion" not in off.stats
    full = sfm.reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS, complete=True)
    assert full.posed.all() and plain.posed.all()
    links = full.stats["completion"]["n_links"]
    assert links == int(cut.sum()) > 0
    assert full.points.stats["n_inlier_observations"] > plain.points.stats["n_inlier_observations"]
    assert full.sfm is not None and torch.equal(full.points.offsets, full.sfm.tracks()[0]) and (full.sfm.track_id != sfm.track_id).sum() == links
    assert full.stats["n_points"] == full.points.stats["n_ok"] and full.stats["rms_px_after"] == full.bundle.rms_px_after
    # the figures (recorded, not bounded: nobody has measured them before)
    lines = ["track completion on the CPU atlas of tests/_completion_cases.py split_atlas() (5 images, 60 points, every third point cut in two;",
             "SfmResult.reconstruct(min_corr=6, min_inliers=6), thresh 4 px), without and with complete=True",
             f"completion: {full.stats['completion']}"]
    for name, rec, atlas in (("without", plain, sfm), ("with", full, full.sfm)):
        length = (rec.points.offsets[1:] - rec.points.offsets[:-1])[rec.points.status == 0].float()      # of the tracks with a point
        rot, cen = _pose_errors(rec, s)
        lines.append(f"{name:8s} mean length of the tracks with a point {float(length.mean()):.4f}  ok points {rec.points.stats['n_ok']}  inlier observations "
                     f"{rec.points.stats['n_inlier_observations']}  rms_px_after {rec.bundle.rms_px_after:.6f}  worst rotation error "
                     f"{rot:.5f} deg  worst centre error {cen:.6f}")
    report = "\n".join(lines)
    print(report)
    if os.environ.get("LOFTR_WRITE_PROFILES"):
        with open(os.path.join(ROOT, "profiles", "complete_accuracy.txt"), "w") as fh:
            fh.write(report + "\n")
