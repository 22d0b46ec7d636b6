"""The radial coefficient through the chain on the CPU: SfmResult.undistorted, SfmResult.reconstruct(radial=...) and
QueryLocalizer.solve(radial=...)."""
import numpy as np
import pytest
import torch

import _completion_cases as CC
import _model_lookup_cases as MC
import _triangulation_cases as TC
import loftr_amd
from loftr_amd import LocalizationModel, QueryLocalizer, _lib, build as build_mod


@pytest.fixture(scope="module", autouse=True)
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def test_the_undistorted_view_shares_everything_but_the_keypoints():
    s = TC.sfm_scene()
    sfm = TC.run_atlas("cpu")
    k = np.array([-0.05, 0.03, 0.0, -0.02, 0.04])
    view = sfm.undistorted(s["K"], k)
    assert view.is_undistorted and not sfm.is_undistorted and view.image_hw == sfm.image_hw and view.cell_px == sfm.cell_px
    for f in sfm.FIELDS:
        assert (getattr(view, f) is getattr(sfm, f)) == (f != "keypoints"), f
    xy, ok = loftr_amd.undistort_points(sfm.keypoints, sfm.keypoint_image(), s["K"], k)
    assert ok.all() and torch.equal(view.keypoints, xy) and not torch.equal(view.keypoints, sfm.keypoints)
    at2 = sfm.keypoint_image() == 2                                     # k = 0: recomputed through K, equal to a rounding
    assert (view.keypoints[at2] - sfm.keypoints[at2]).abs().max() <= 2 * float(np.spacing(np.float32(1600.0)))
    pts = view.triangulate(s["K"], s["T"])
    assert pts.offsets is not None and pts.stats["n_tracks"] == sfm.triangulate(s["K"], s["T"]).stats["n_tracks"]
    for who in ("complete", "merge"):
        with pytest.raises(ValueError, match="undistorted view.*stored-pixel space"):
            getattr(view, who)(pts, s["K"], s["T"])
    model = LocalizationModel.from_atlas(sfm, pts)                      # the ORIGINAL result with the points of the view
    assert model.n_images == 5
    R, t, n = view.pairwise_poses(s["K"])
    assert tuple(R.shape) == (sfm.row_offsets.numel() - 1, 3, 3) and (n >= 0).all()
    with pytest.raises(ValueError, match=r"expected K \[5,3,3\] and radial \[5\]"):
        sfm.undistorted(s["K"], k[:4])
    zero = sfm.undistorted(s["K"], np.zeros(5))                         # no lens: the same points to a rounding of the pixels
    a, b = sfm.triangulate(s["K"], s["T"]), zero.triangulate(s["K"], s["T"])
    assert torch.equal(a.status, b.status) and (torch.nan_to_num(a.xyz) - torch.nan_to_num(b.xyz)).abs().max() < 1e-3


def test_sfm_reconstruct_carries_the_lens_and_refuses_completion_under_it():
    sfm, s, _ = CC.split_atlas("cpu")
    plain = sfm.reconstruct(s["K"], min_corr=6, min_inliers=6)
    known = sfm.reconstruct(s["K"], radial=np.zeros(5), min_corr=6, min_inliers=6)     # a known lens: here none
    assert known.posed.all() and torch.equal(known.radial, torch.zeros(5, dtype=torch.float64)) and plain.radial is None
    assert known.stats["n_points"] == plain.stats["n_points"] and abs(known.bundle.rms_px_after - plain.bundle.rms_px_after) < 1e-3
    ba = {"refine_focal": True, "refine_radial": True, "camera_ids": [3] * 5, "min_focal_obs": 5}
    rec = sfm.reconstruct(s["K"], ba=ba, min_corr=6, min_inliers=6)
    k = rec.radial.numpy()
    print(f"sfm.reconstruct(ba radial): posed {int(rec.posed.sum())}, k {k[0]:.5f}, rms {rec.bundle.rms_px_after:.4f} (pinhole {plain.bundle.rms_px_after:.4f})")
    assert rec.posed.all() and rec.bundle.cam_radial.all() and len(set(k.tolist())) == 1 and np.isfinite(k).all()
    assert rec.bundle.stats["n_radial_cameras"] == 5 and rec.bundle.status in ("converged", "max_iters")   # (no lens in this scene: k stays small)
    for kw in (dict(complete=True), dict(merge=True)):
        with pytest.raises(ValueError, match="complete / merge under distortion are not modelled"):
            sfm.reconstruct(s["K"], radial=np.zeros(5), **kw)
        with pytest.raises(ValueError, match="complete / merge under distortion are not modelled"):
            sfm.reconstruct(s["K"], ba=ba, **kw)


def _localizer(model, px_q):
    qs = MC.query_scene()
    loc = QueryLocalizer(model, MC.N_QUERIES)
    for q, d, kd, _, c in qs["rows"]:
        data = {"mkpts0_f": torch.from_numpy(px_q[q]), "mkpts1_f": torch.from_numpy(kd), "mconf": torch.from_numpy(c),
                "m_bids": torch.zeros(len(c), dtype=torch.int64)}
        loc.add([q], [d], data, db_side=1)
    return loc


def test_solve_undistorts_the_query_side():
    """The queries of the localisation scene seen through one lens each: solve(radial=k) finds the poses of the pinhole scene; without
    the keyword the distorted pixels lose inliers."""
    model, _, _ = MC.build_model("cpu")
    qs = MC.query_scene()
    k = np.linspace(-0.08, 0.08, MC.N_QUERIES)
    seen = []
    for q in range(MC.N_QUERIES):
        xy, ok = loftr_amd.distort_points(qs["px_q"][q], np.full(len(qs["px_q"][q]), q, np.int32), qs["K"], k)
        assert ok.all()
        seen.append(xy.numpy())
    kw = dict(thresh_px=3.0, conf=0.999, seed=0)
    plain = _localizer(model, qs["px_q"]).solve(qs["K"], **kw)
    wrong = _localizer(model, seen).solve(qs["K"], **kw)
    res = _localizer(model, seen).solve(qs["K"], radial=k, **kw)
    print("inliers: pinhole scene", plain.n_inliers.tolist(), "distorted, with radial", res.n_inliers.tolist(), "without", wrong.n_inliers.tolist())
    assert res.stats["n_not_undistorted"] == 0 and res.stats["n_correspondences"] == plain.stats["n_correspondences"]
    assert torch.equal(res.n_inliers, plain.n_inliers)                  # the undistorted pixels are the pinhole ones to 1e-4 px
    assert (res.R - plain.R).abs().max() < 1e-4 and (res.t - plain.t).abs().max() < 1e-3
    assert int(wrong.n_inliers.sum()) < int(plain.n_inliers.sum())
    far = [x.copy() for x in seen]
    far[0][:3] = (1e5, 1e5)                                              # beyond the fold of k = -0.08: three pixels of query 0 have no pinhole point
    out = _localizer(model, far).solve(qs["K"], radial=k, **kw)
    assert out.stats["n_not_undistorted"] == 3 and out.n_corr[0] == plain.n_corr[0] - 3 and torch.isfinite(out.kpts).all()     # (a query pixel is one correspondence)
    assert int(out.q_offsets[-1]) == out.stats["n_correspondences"] == plain.stats["n_correspondences"] - 3
    with pytest.raises(ValueError, match=r"expected radial \[8\]"):
        _localizer(model, seen).solve(qs["K"], radial=k[:3])
