"""CPU tests of the track triangulation (csrc/triangulate.hip through loftr_amd.triangulation): the pair enumeration and the
host routine against the independent numpy oracle, the result against ground truth, the hand-written tracks, and SfmResult.triangulate
with keypoint_xyz over a CPU atlas."""
import os

import numpy as np
import pytest
import torch

from loftr_amd import Points3D, _lib, build as build_mod, ops, triangulate_tracks
import _triangulation_cases as TC
import _triangulation_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def solved(lib):
    """(scene, host result as numpy dict, oracle results): computed once, left unchanged."""
    s = TC.scene()
    pts = triangulate_tracks(s["offsets"], s["obs_image"], s["obs_xy"], s["K"], s["T"], TC.THRESH_PX, TC.MIN_ANGLE_DEG)
    assert isinstance(pts, Points3D)
    ref = O.triangulate(s["offsets"], s["obs_image"], s["obs_xy"], s["K"], s["T"], TC.THRESH_PX, TC.COS_MIN)
    return s, pts.to_host(), ref


def test_pair_enumeration_equals_the_oracle(lib):
    for L in list(range(2, 14)) + [64, 70]:
        assert ops.triangulation_pairs(L) == O.pairs(L), L
    assert [len(ops.triangulation_pairs(L)) for L in (2, 3, 4, 5, 11, 12, 70)] == [1, 3, 6, 10, 55, 64, 64]
    assert ops.triangulation_pairs(0) == [] and ops.triangulation_pairs(1) == []
    for L in (12, 13, 64):                                              # every observation appears in the first L pairs of a long track
        assert {i for p in ops.triangulation_pairs(L)[:L] for i in p} == set(range(L))
    assert {i for p in ops.triangulation_pairs(70) for i in p} == set(range(65))          # (the 64 pairs of a track beyond 64 reach 65)


def test_host_routine_equals_the_oracle(solved):
    s, got, ref = solved
    off = s["offsets"]
    T = len(ref)
    assert T == 405 and got["stats"]["n_tracks"] == T and got["stats"]["n_observations"] == off[-1]
    # a track may be left out only when the oracle met a residual within 1e-6 px of the threshold or a cosine within 1e-9 of the limit
    borderline = [t for t, r in enumerate(ref) if r["px_margin"] < 1e-6 or r["cos_margin"] < 1e-9]
    assert len(borderline) <= T // 100, borderline
    worst = 0.0
    for t, r in enumerate(ref):
        if t in borderline:
            continue
        assert got["status"][t] == r["status"], (t, got["status"][t], r["status"])
        if r["status"] in (O.OK, O.SMALL_ANGLE):
            assert got["n_inliers"][t] == r["n_inliers"], t
            assert abs(got["rms_px"][t] - r["rms_px"]) <= 1e-5 * max(1.0, r["rms_px"]), t
            assert np.isnan(r["tri_cos"]) == np.isnan(got["tri_cos"][t]) and (np.isnan(r["tri_cos"]) or abs(got["tri_cos"][t] - r["tri_cos"]) <= 1e-6), t
        assert np.array_equal(got["obs_inlier"][off[t]:off[t + 1]], r["mask"]), t
        if r["status"] == O.OK:
            # the host's one fp32 rounding is 2^-24 relative; the two fp64 paths differ only in the order of their roundings
            err = np.abs(got["xyz"][t].astype(np.float64) - r["xyz"]).max() / max(1.0, np.abs(r["xyz"]).max())
            worst = max(worst, err)
            assert err <= 4 * 2.0 ** -24, (t, err)
        else:
            assert np.isnan(got["xyz"][t]).all(), t
    counts = np.bincount([r["status"] for r in ref], minlength=5)
    if not borderline:
        assert [got["stats"]["n_" + n] for n in ops.TRI_STATUS] == counts.tolist()
        assert got["stats"]["n_inlier_observations"] == sum(int(r["mask"].sum()) for r in ref)
    assert counts[O.OK] >= 350                                          # the scene is one that triangulates
    print(f"host vs oracle: {T} tracks, {len(borderline)} borderline, worst |dxyz| / max(1, |X|) = {worst:.3e} (limit {4 * 2.0 ** -24:.3e})")


def test_result_against_ground_truth(solved):
    """Figures: profiles/triangulation_accuracy.txt (tools/micro/triangulation_accuracy.py prints the same report)."""
    s, got, ref = solved
    fig = TC.ground_truth_figures(s, got)
    print(TC.accuracy_report(fig))
    assert fig["share"] >= 0.95, fig
    assert fig["n_ratio"] >= 0.95 * fig["n_long"] and fig["worst_ratio"] <= 1.01, fig


def test_hand_written_tracks(lib):
    inp, expect = TC.hand_cases()
    pts = triangulate_tracks(inp["offsets"], inp["obs_image"], inp["obs_xy"], inp["K"], inp["T"], TC.THRESH_PX, TC.MIN_ANGLE_DEG)
    res = pts.to_host()
    res["offsets"] = inp["offsets"]
    counts = TC.check_hand(res, expect)
    assert [pts.stats["n_" + n] for n in ops.TRI_STATUS] == counts
    assert pts.valid.tolist() == [e["status"] == 0 for e in expect]
    small = [t for t, e in enumerate(expect) if e["status"] == 3][0]
    assert np.degrees(np.arccos(res["tri_cos"][small])) == pytest.approx(1.432, abs=2e-3) and res["rms_px"][small] == pytest.approx(3.0, abs=0.01)
    # float32 cameras and torch tensors give the same result as float64 arrays when the values are float32 numbers
    K32, T32 = inp["K"].astype(np.float32), inp["T"].astype(np.float32)
    a = triangulate_tracks(inp["offsets"], inp["obs_image"], inp["obs_xy"], K32, T32).to_host()
    b = triangulate_tracks(torch.from_numpy(inp["offsets"]), torch.from_numpy(inp["obs_image"]).long(), torch.from_numpy(inp["obs_xy"]),
                           torch.from_numpy(K32.astype(np.float64)), torch.from_numpy(T32.astype(np.float64))).to_host()
    for k in Points3D.FIELDS:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


def test_no_tracks_and_bad_input(lib):
    K, T = TC.camera(500, (0, 0, 0))
    pts = triangulate_tracks(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, 2), np.float32), K[None], T[None])
    assert pts.xyz.shape == (0, 3) and pts.status.shape == (0,) and pts.obs_inlier.shape == (0,) and pts.stats["n_ok"] == 0
    pts = triangulate_tracks(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, 2), np.float32), np.zeros((0, 3, 3)), np.zeros((0, 4, 4)))
    assert pts.stats["n_tracks"] == 0
    xy = np.zeros((2, 2), np.float32)
    two = lambda off, im: triangulate_tracks(np.array(off), np.array(im), xy, K[None], T[None])
    assert two([0, 2], [0, 0]).status.tolist() == [2]
    for im in ([0, 1], [-1, 0]):
        with pytest.raises(ValueError, match="obs_image outside"):
            two([0, 2], im)
    for off in ([0, 1], [1, 2], [0, 2, 1, 2], [0, 3]):
        with pytest.raises(ValueError, match="offsets must start at 0"):
            two(off, [0, 0])
    with pytest.raises(ValueError, match="integers"):
        triangulate_tracks(np.array([0.0, 2.0]), np.array([0, 0]), xy, K[None], T[None])
    with pytest.raises(ValueError, match="min_angle_deg"):
        triangulate_tracks(np.array([0, 2]), np.array([0, 0]), xy, K[None], T[None], min_angle_deg=float("nan"))
    with pytest.raises(ValueError, match="group"):
        triangulate_tracks(np.array([0, 2]), np.array([0, 0]), xy, K[None], T[None], group=16)


def test_sfm_result_triangulate_and_keypoint_xyz(lib):
    s = TC.sfm_scene()
    sfm = TC.run_atlas("cpu")
    assert sfm.stats["n_tracks"] == len(s["X"]) and sfm.track_ok.all() and (sfm.track_len == 5).all()
    pts = sfm.triangulate(s["K"].astype(np.float32), torch.from_numpy(s["T"]), thresh_px=TC.THRESH_PX, min_angle_deg=TC.MIN_ANGLE_DEG)
    assert pts.valid.all() and (pts.n_inliers == 5).all() and pts.obs_inlier.all()
    # which point a track is: its keypoint in image 0 is the snapped projection of exactly one point
    first = pts.offsets[:-1]
    assert (pts.image[first] == 0).all()
    kp0 = sfm.keypoints[sfm.kp_offsets[pts.image[first]] + pts.keypoint[first]].numpy()
    which = [int(np.nonzero((s["px"][0] == k).all(1))[0][0]) for k in kp0]
    assert sorted(which) == list(range(len(s["X"])))
    X = s["X"][which]
    # Reach of the quantisation.  A keypoint is a cell centre: at most e = sqrt(2) cell_px / 2 pixels from the true projection, so the TRUE
    # point has an RMS error <= e over a track; the least-squares point has no greater RMS, hence at most sqrt(n) e in any one of the
    # n = 5 views, and it projects within (1 + sqrt(n)) e pixels of the true point in every view: an angle d = (1 + sqrt(n)) e / f_min
    # at each centre.  Two such cones around rays that meet under the angle theta intersect within 2 r d / sin(theta) of the point
    # (r: the greater distance to the two centres, small d); theta is taken from the widest pair of the track.
    e = np.sqrt(2) * TC.SFM_CELL / 2
    d = (1 + np.sqrt(5)) * e / s["K"][:, 0, 0].min()
    centres = np.stack([-t[:3, :3].T @ t[:3, 3] for t in s["T"]])
    err = np.linalg.norm(pts.xyz.numpy().astype(np.float64) - X, axis=1)
    for x, er in zip(X, err):
        rays = x - centres
        r = np.linalg.norm(rays, axis=1)
        cosines = (rays @ rays.T) / np.outer(r, r)
        theta = np.arccos(cosines.min())
        assert er <= 2 * r.max() * d / np.sin(theta), (er, 2 * r.max() * d / np.sin(theta))
    assert np.median(err) < 0.05                                        # and in practice a few hundredths of a unit at depth 4 to 7
    xyz, has = pts.keypoint_xyz(sfm)
    assert xyz.shape == (sfm.keypoints.shape[0], 3) and has.dtype == torch.bool and has.all()
    assert torch.equal(xyz[sfm.kp_offsets[pts.image] + pts.keypoint], pts.xyz.repeat_interleave(5, 0))
    # a tight threshold: a track keeps the keypoints that agree within 0.9 px and drops the rest, some tracks fail altogether; `has` is true
    # exactly at the inlier keypoints of the valid tracks
    tight = sfm.triangulate(s["K"], s["T"], thresh_px=0.9)
    xyz, has = tight.keypoint_xyz(sfm)
    want = np.zeros(sfm.keypoints.shape[0], bool)
    for t in range(tight.status.numel()):
        for o in range(int(tight.offsets[t]), int(tight.offsets[t + 1])):
            if tight.status[t] == 0 and tight.obs_inlier[o]:
                k = int(sfm.kp_offsets[tight.image[o]] + tight.keypoint[o])
                want[k] = True
                assert torch.equal(xyz[k], tight.xyz[t])
    assert np.array_equal(has.numpy(), want) and 0 < want.sum() < want.size and torch.isnan(xyz[~has]).all()
    with pytest.raises(ValueError, match="K \\[5,3,3\\]"):
        sfm.triangulate(s["K"][:4], s["T"][:4])
    with pytest.raises(ValueError, match="carries no tracks"):
        triangulate_tracks(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, 2), np.float32), s["K"], s["T"]).keypoint_xyz(sfm)
