"""CPU tests of track merging: the host routine loftr_merge_tracks_host against the independent numpy statement of the rule
(tests/_merge_oracle.py) with bit equality, the twin scene against its exact expected result, the hand-written cases, the error bits,
SfmResult.merge and SfmResult.reconstruct(merge=...).  The kernels are held to the host routine in tests/test_hip_merge.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _merge_cases as MC
import _merge_oracle as O
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_CORR = MIN_INLIERS = 6


@pytest.fixture(scope="module", autouse=True)
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def same(got, want):
    """bit equality of the four outputs"""
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    assert np.array_equal(got["row_into"], want["row_into"]), np.nonzero(got["row_into"] != want["row_into"])[0][:8]
    assert np.array_equal(got["kp_row_new"], want["kp_row_new"]), np.nonzero(got["kp_row_new"] != want["kp_row_new"])[0][:8]
    assert np.array_equal(got["merge_r2"].view(np.int32), want["merge_r2"].view(np.int32))


def cells_ascend(t):
    cell, status = ops.model_cells_host(t["kp_offsets"], t["keypoints"], t["kp_row"], len(t["status"]), *t["grid"])
    assert status == 0 and np.array_equal(cell, t["kp_cell"])


def test_twin_scene_is_merged_exactly():
    t, row_into, kp_row_new, twins = MC.twin_scene()
    cells_ascend(t)
    oracle = O.merge(*MC.args(t))
    MC.check_margins(t, oracle)
    # the generator's conditions, of the oracle alone: every twin meets (from both sides), every twin merges ...
    met = {(min(j, m), max(j, m)) for j, _, m, _ in oracle["meetings"]}
    sides = {(j, m) for j, _, m, _ in oracle["meetings"]}
    assert len(twins) >= 15 and met == set(twins) and all((lo, hi) in sides and (hi, lo) in sides for lo, hi in twins)
    assert set(oracle["scores"]) == set(twins)
    # ... first the oracle against the generator's ground truth, then the host routine against both
    MC.check_twins(t, oracle, row_into, kp_row_new, twins)
    host = ops.merge_tracks_host(*MC.args(t))
    MC.check_twins(t, host, row_into, kp_row_new, twins)
    same(host, oracle)


def test_hand_cases():
    t, notes = MC.hand()
    cells_ascend(t)
    oracle = O.merge(*MC.args(t))
    MC.check_margins(t, oracle)
    MC.check_hand(t, notes, oracle)
    host = ops.merge_tracks_host(*MC.args(t))
    MC.check_hand(t, notes, host)
    same(host, oracle)
    for reach in (0, 1, 8):                                                # (what a reach changes is only which keypoints are met)
        same(ops.merge_tracks_host(*MC.args(t, reach)), O.merge(*MC.args(t, reach)))
    # the one-sided meeting: found by the lower row only
    row = notes["row"]
    sides = {(j, m) for j, _, m, _ in oracle["meetings"]}
    assert (row["one_sided_in"], row["one_sided_out"]) in sides and (row["one_sided_out"], row["one_sided_in"]) not in sides


def test_no_rows_no_keypoints_no_images():
    for name, t in MC.empties().items():
        host = ops.merge_tracks_host(*MC.args(t))
        same(host, O.merge(*MC.args(t)))
        assert host["counts"][0] == 0 and host["counts"][1] == 0 and host["counts"][7] == 0, name
        assert np.array_equal(host["kp_row_new"], t["kp_row"]) and np.isnan(host["merge_r2"]).all(), name
        assert np.array_equal(host["row_into"], np.arange(len(t["status"]))), name


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_random_tables(seed):
    t = MC.random_table(seed)
    cells_ascend(t)
    oracle = O.merge(*MC.args(t))
    MC.check_margins(t, oracle)
    c = oracle["counts"]
    assert c[0] >= 3 and c[4] > c[5] > c[6] >= c[0]                        # merges; meetings that share an image; disjoint ones that disagree
    same(ops.merge_tracks_host(*MC.args(t)), oracle)


@pytest.mark.parametrize("shape", ((65, 7), (40, 2), (24, 65)))
def test_clustered_rows(shape):
    """many rows around one point: contention for the best partner, one merge per mutual pair and no chains"""
    t = MC.sized(*shape, seed=sum(shape))
    cells_ascend(t)
    oracle = O.merge(*MC.args(t))
    c = oracle["counts"]
    assert c[0] >= 1 and c[6] > 2 * c[0] and c[7] >= c[0]
    into = oracle["row_into"]
    assert (into[into] == into).all() and (np.bincount(into, minlength=len(into)) <= 2).all()      # no chains, no multi-way merges
    same(ops.merge_tracks_host(*MC.args(t)), oracle)


def test_star_long_row_and_corners():
    t = MC.star()
    host = ops.merge_tracks_host(*MC.args(t))
    assert host["counts"][0] == 1 and host["row_into"][1] == 0 and (np.delete(host["row_into"], 1) == np.delete(np.arange(512), 1)).all()
    assert host["counts"][6] == 128 + 511 and host["merge_r2"][0] == host["merge_r2"][1] == np.float32(9.0)
    t = MC.long_and_short()
    host = ops.merge_tracks_host(*MC.args(t))
    assert np.diff(t["offsets"]).tolist() == [70, 2] and host["row_into"].tolist() == [0, 0] and host["counts"][7] == 2
    same(host, O.merge(*MC.args(t)))
    for reach in (0, 8):
        t = MC.corners(reach)
        cells_ascend(t)
        host = ops.merge_tracks_host(*MC.args(t))
        assert host["counts"][0] == 4
        same(host, O.merge(*MC.args(t)))


def _as_call(t, **over):
    """the arguments of loftr_amd.merge_tracks from a table"""
    kw = dict(offsets=t["offsets"], obs_image=t["obs_image"], obs_xy=t["obs_xy"], obs_mask=t["obs_mask"], kp_offsets=t["kp_offsets"],
              keypoints=t["keypoints"], kp_row=t["kp_row"], xyz=t["xyz"], status=t["status"], K=t["K"], T_cam_from_world=t["T_cam_from_world"],
              image_hw=MC.CC.HW, cell_px=MC.CC.CELL, posed=t["posed"], thresh_px=t["thresh_px"], reach=t["reach"])
    kw.update(over)
    return kw


@pytest.mark.parametrize("bit", (1, 2, 4, 8))
def test_every_error_bit_is_a_value_error(lib, bit):
    t = MC.bad_tables()[bit]
    assert O.merge(*MC.args(t)) == dict(error=bit)
    text = {1: "obs_image outside", 2: "offsets must start at 0", 4: "must not descend within a row", 8: r"kp_row outside \[-1, T\)"}[bit]
    with pytest.raises(ValueError, match=text):
        loftr_amd.merge_tracks(**_as_call(t))
    with pytest.raises(ValueError, match=text):
        loftr_amd.merge_tracks(**{k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in _as_call(t).items()})
    a = MC.args(t)
    n_rows, n_kp = len(t["status"]), len(t["kp_row"])
    out = [np.full(n_rows, 7, np.int32), np.full(n_rows, 7, np.float32), np.full(n_kp, 7, np.int32), np.full(8, 7, np.int64)]
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    st = lib.loftr_merge_tracks_host(p(a[0]), n_rows, p(a[1]), p(a[2]), p(a[3]), len(a[1]), p(a[4]), p(a[5]), p(a[6]), p(a[7]), p(a[8]), p(a[9]), n_kp,
                                     p(a[10]), p(a[11]), p(a[12]), len(a[12]), a[15], a[13], a[14], a[16], a[17], *[p(x) for x in out])
    assert st == -1 and out[3].tolist() == [0, bit, 0, 0, 0, 0, 0, 0] and all((x == 7).all() for x in out[:3])


def test_python_entry_point_on_the_hand_table():
    t, notes = MC.hand()
    done = loftr_amd.merge_tracks(**_as_call(t))
    host = ops.merge_tracks_host(*MC.args(t))
    assert isinstance(done, loftr_amd.Merge) and loftr_amd.Merge.FIELDS == ("row_into", "merge_r2", "merged", "kp_row_new")
    assert np.array_equal(done.row_into.numpy(), host["row_into"]) and np.array_equal(done.kp_row_new.numpy(), host["kp_row_new"])
    assert np.array_equal(done.merged.numpy(), ~np.isnan(host["merge_r2"])) and done.merged.sum() == 8
    assert [done.stats[k] for k in ops.MERGE_NAMES if k != "error_bits"] == [int(host["counts"][i]) for i in (0, 2, 3, 4, 5, 6, 7)]
    assert done.stats["n_merges"] == 4 and done.stats["reach"] == 2 and done.stats["n_rows"] == len(t["status"])
    # bool masks and tensors are taken as they come; reach=None is ceil(thresh_px / cell_px)
    as_tensors = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in _as_call(t, reach=None).items()}
    again = loftr_amd.merge_tracks(**dict(as_tensors, obs_mask=as_tensors["obs_mask"].bool()))
    assert again.stats == done.stats and torch.equal(again.row_into, done.row_into)
    with pytest.raises(ValueError, match="cell_px"):
        loftr_amd.merge_tracks(**_as_call(t, reach=None, thresh_px=16.5))
    for bad in (9, -1, 2.0, True):
        with pytest.raises(ValueError, match="cell_px"):
            loftr_amd.merge_tracks(**_as_call(t, reach=bad))
    with pytest.raises(ValueError, match="thresh_px"):
        loftr_amd.merge_tracks(**_as_call(t, thresh_px=float("nan")))
    # posed=None: every image; the masked observation in image 8 then has a pose and that pair merges as well
    assert loftr_amd.merge_tracks(**_as_call(t, posed=None)).stats["n_merges"] == 5
    k = t["keypoints"].copy()
    b = int(t["kp_offsets"][1])
    k[[b, b + 1]] = k[[b + 1, b]]
    with pytest.raises(ValueError, match="cells that do not ascend"):
        loftr_amd.merge_tracks(**_as_call(t, keypoints=k))


def _fields(x):
    return {k: getattr(x, k) for k in x.FIELDS}


def _valid_csr(sfm):
    offsets, image, local = sfm.tracks()
    assert offsets[0] == 0 and offsets[-1] == image.numel() and (offsets[1:] >= offsets[:-1]).all()
    row = torch.repeat_interleave(torch.arange(offsets.numel() - 1), offsets[1:] - offsets[:-1])
    assert torch.unique(row * 1000 + image).numel() == image.numel()                     # no track visits an image twice
    assert (local >= 0).all() and (sfm.kp_offsets[image] + local < sfm.kp_offsets[image + 1]).all()
    assert torch.equal(sfm.track_len.to(torch.int64), torch.bincount(sfm.track_id[sfm.track_id >= 0].to(torch.int64), minlength=sfm.track_len.numel()))


def test_sfm_merge_on_the_cpu_atlas():
    sfm, s, cut = MC.twin_atlas("cpu")
    n_cut = int(cut.sum())
    before = {k: v.clone() for k, v in _fields(sfm).items()}
    pts = sfm.triangulate(s["K"], s["T"])
    assert pts.stats["n_ok"] == len(cut) + n_cut                                          # both halves of a cut point have a point
    sfm2, done = sfm.merge(pts, s["K"], s["T"])
    assert done.stats["n_merges"] == n_cut and done.stats["n_relabelled"] == 2 * n_cut
    for k, v in _fields(sfm).items():                                                     # self is untouched ...
        assert torch.equal(v, before[k]), k
    for k in sfm.FIELDS:                                                                  # ... and shared, except for the two relabelled fields
        assert (getattr(sfm2, k) is getattr(sfm, k)) == (k not in ("track_id", "track_len")), k
    assert sfm2.image_hw == sfm.image_hw and sfm2.cell_px == sfm.cell_px and sfm2.stats["n_merges"] == n_cut
    _valid_csr(sfm2)
    # every changed keypoint belonged to an absorbed row, lies in image 3 or 4, and went to the track of its point's views 0-2
    changed = sfm2.track_id != sfm.track_id
    absorbed = torch.nonzero(done.row_into != torch.arange(done.row_into.numel())).reshape(-1)
    assert changed.sum() == 2 * n_cut and absorbed.numel() == n_cut and torch.equal(changed, done.kp_row_new != _kp_row(sfm, pts))
    ids = torch.nonzero(sfm.track_ok).reshape(-1)
    assert set(sfm.track_id[changed].tolist()) == set(ids[absorbed].tolist()) and (sfm.keypoint_image()[changed] >= 3).all()
    assert (sfm2.track_len[ids[absorbed]] == 0).all() and (sfm2.track_len[ids[done.row_into[absorbed].long()]] == 5).all()
    pts2 = sfm2.triangulate(s["K"], s["T"])
    assert pts2.stats["n_ok"] == len(cut) and pts2.stats["n_too_short"] == n_cut
    assert pts2.stats["n_inlier_observations"] == pts.stats["n_inlier_observations"]
    sfm3, again = sfm2.merge(pts2, s["K"], s["T"])                                        # a second merge runs, and finds nothing new
    assert again.stats["n_merges"] == 0 and torch.equal(sfm3.track_id, sfm2.track_id)
    with pytest.raises(ValueError, match="carries no tracks"):
        sfm.merge(loftr_amd.Points3D(pts.stats, **{k: getattr(pts, k) for k in pts.FIELDS}), s["K"], s["T"])


def _kp_row(sfm, pts):
    kp_row = torch.full((sfm.keypoints.shape[0],), -1, dtype=torch.int32)
    row = torch.repeat_interleave(torch.arange(pts.offsets.numel() - 1), pts.offsets[1:] - pts.offsets[:-1])
    kp_row[sfm.kp_offsets[pts.image] + pts.keypoint] = row.to(torch.int32)
    return kp_row


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


def test_reconstruct_with_and_without_merging():
    sfm, s, cut = MC.twin_atlas("cpu")
    plain = sfm.reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS)
    off = sfm.reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS, merge=False)
    # merge=False is today's call: every field
    bits = lambda x: x.contiguous().view(torch.int64 if x.element_size() == 8 else torch.int32) if x.is_floating_point() else x
    eq = lambda x, y: torch.equal(bits(x), bits(y))
    for k in ("T_cam_from_world", "posed", "round_registered", "K"):
        assert eq(getattr(off, k), getattr(plain, k)), k
    for k in loftr_amd.Points3D.FIELDS + ("offsets", "image", "keypoint"):
        assert eq(getattr(off.points, k), getattr(plain.points, k)), k
    for k in ("T_cam_from_world", "xyz", "obs_active"):
        assert eq(getattr(off.bundle, k), getattr(plain.bundle, k)), k
    assert off.stats == plain.stats and off.sfm is None and "merge" not in off.stats
    full = sfm.reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS, merge=True)
    assert full.posed.all() and plain.posed.all()
    merges = full.stats["merge"]["n_merges"]
    assert merges >= 1 and "completion" not in full.stats
    # every half of a cut point is ok before and every merged pair is one ok point after: the ok points fall by exactly the merges
    assert plain.points.stats["n_ok"] == len(cut) + int(cut.sum()) and full.points.stats["n_ok"] == plain.points.stats["n_ok"] - merges
    assert full.sfm is not None and torch.equal(full.points.offsets, full.sfm.tracks()[0])
    assert full.stats["n_points"] == full.points.stats["n_ok"] and full.stats["rms_px_after"] == full.bundle.rms_px_after
    length = lambda rec: float((rec.points.offsets[1:] - rec.points.offsets[:-1])[rec.points.status == 0].float().mean())
    assert length(full) > length(plain)                                                   # of the tracks with a point
    both = sfm.reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS, complete=True, merge=True)
    assert both.stats["merge"]["n_merges"] == merges and "completion" in both.stats
    # the figures (recorded, not bounded: nobody has measured them before)
    lines = ["track merging on the CPU atlas of tests/_merge_cases.py twin_atlas() (5 images, 60 points, every third point two proper tracks:",
             "views 0-2 and views 3-4; SfmResult.reconstruct(min_corr=6, min_inliers=6), thresh 4 px), without and with merge=True",
             f"merge: {full.stats['merge']}"]
    for name, rec in (("without", plain), ("with", full)):
        rot, cen = _pose_errors(rec, s)
        lines.append(f"{name:8s} merges {rec.stats.get('merge', {}).get('n_merges', 0)}  mean length of the tracks with a point {length(rec):.4f}  ok points "
                     f"{rec.points.stats['n_ok']}  inlier observations {rec.points.stats['n_inlier_observations']}  rms_px_after "
                     f"{rec.bundle.rms_px_after:.6f}  worst rotation error {rot:.5f} deg  worst centre error {cen:.6f}")
    report = "\n".join(lines)
    print(report)
    if os.environ.get("LOFTR_WRITE_PROFILES"):
        with open(os.path.join(ROOT, "profiles", "merge_accuracy.txt"), "w") as fh:
            fh.write(report + "\n")
