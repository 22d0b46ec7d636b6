"""Track refinement on the CPU (loftr_amd/refinement.py, csrc/refine.hip): the host routine of the fine-window centres
against a numpy fp32 restatement, the planner against a Python-dict restatement on hand-built results, the apply rules on fabricated
network outputs, and the guards.  tests/test_hip_refine.py holds the kernels and the network path."""
import numpy as np
import pytest
import torch

import _refine_cases as cases
import _refine_oracle as oracle
from loftr_amd import _lib, ops
from loftr_amd.refinement import RefinePlan, apply_refinement, plan_track_refinement

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


# ---- 1. the centres ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales", [False, True])
def test_refine_centres_host_equals_the_oracle(scales):
    pts0, pts1, b_ids = cases.centre_points()
    sc0, sc1 = (cases.SCALE0, cases.SCALE1) if scales else (None, None)
    geo = (cases.N_PAIRS, cases.HW0_F, cases.HW1_F, cases.HW0_C, cases.HW1_C, cases.STRIDE, cases.S)
    got = ops.refine_centres(T(pts0), T(pts1), T(b_ids), *geo, None if sc0 is None else T(sc0), None if sc1 is None else T(sc1))
    want = oracle.centres(pts0, pts1, b_ids, *geo, sc0, sc1)
    assert set(got) == set(want)
    for k in want:
        assert got[k].numpy().dtype == want[k].dtype and np.array_equal(got[k].numpy(), want[k]), k
    ok = got["ok"].numpy()
    assert 0 < (ok == 0).sum() == 6 and not got["c0"].numpy()[ok == 0].any() and not got["j_ids"].numpy()[ok == 0].any()
    assert got["c0"][:, 0].max() == cases.HW0_F[1] - 1 and got["c1"][:, 1].max() == cases.HW1_F[0] - 1     # clamped on both maps
    assert got["i_ids"].max() < cases.HW0_C[0] * cases.HW0_C[1] and got["j_ids"].max() < cases.HW1_C[0] * cases.HW1_C[1]


def test_centres_on_cell_centres_give_back_the_cell_and_the_coarse_point():
    """c = stride * cell -> that cell, and pts_s has the bits of the forward's mkpts_c = cell * (stride * s * scale)."""
    hc, wc = cases.HW0_C
    cell = np.arange(hc * wc)
    scale = cases.SCALE0[:1]
    coarse = cases.STRIDE * np.float32(cases.S)
    mk = np.stack([(cell % wc).astype(np.float32) * (coarse * scale[0, 0]), (cell // wc).astype(np.float32) * (coarse * scale[0, 1])], 1)
    got = ops.refine_centres(T(mk), T(mk), torch.zeros(len(cell), dtype=torch.int64), 1, cases.HW0_F, cases.HW0_F, cases.HW0_C, cases.HW0_C,
                             cases.STRIDE, cases.S, T(scale), T(scale))
    assert got["i_ids"].tolist() == cell.tolist() and got["j_ids"].tolist() == cell.tolist()
    assert np.array_equal(got["pts0_s"].numpy().view(np.int32), mk.view(np.int32))
    assert got["c0"][:, 0].tolist() == (cases.STRIDE * (cell % wc)).tolist()


def test_a_pair_outside_the_batch_is_not_ok():
    pts = torch.tensor([[8.0, 8.0], [8.0, 8.0], [8.0, 8.0]])
    got = ops.refine_centres(pts, pts, torch.tensor([0, 3, -1]), 3, (32, 48), (32, 48), (8, 12), (8, 12), 4, 2.0, T(cases.SCALE0), None)
    assert got["ok"].tolist() == [1, 0, 0] and got["c0"].tolist() == [[2, 2], [0, 0], [0, 0]]


# ---- 2. the planner ------------------------------------------------------------------------------------------------------------
def _check_plan(sfm, obs_mask, min_jobs):
    plan = plan_track_refinement(sfm, obs_mask=None if obs_mask is None else T(obs_mask), min_jobs_per_pair=min_jobs)
    want = oracle.plan(sfm.to_host(), obs_mask, min_jobs)
    for k in RefinePlan.FIELDS:
        assert getattr(plan, k).dtype == torch.int64 and np.array_equal(getattr(plan, k).cpu().numpy(), want[k]), k
    for k, v in want["stats"].items():
        assert plan.stats[k] == v, k
    return plan


def test_plan_equals_the_oracle():
    sfm = cases.build_sfm(cases.SCENE5)
    plan = _check_plan(sfm, None, 1)
    assert plan.stats == dict(n_tracks=5, n_jobs=11, n_pairs=7, n_dropped_jobs=0, n_dropped_pairs=0, min_jobs_per_pair=1)
    kp_image = sfm.keypoint_image()
    assert plan.pairs.tolist() == [[0, 1], [0, 2], [0, 3], [2, 0], [2, 1], [2, 3], [2, 4]]
    tie = plan.job_track == 2                                            # the score tie: the keypoint of image 2, not of image 3
    assert kp_image[plan.job_ref_kp[tie]].tolist() == [2, 2] and sorted(kp_image[plan.job_query_kp[tie]].tolist()) == [1, 3]
    assert 4 not in plan.job_track.tolist()                              # the inconsistent track
    assert len(set(plan.job_query_kp.tolist())) == 11 and not set(plan.job_query_kp.tolist()) & set(plan.job_ref_kp.tolist())


def test_plan_with_an_observation_mask_and_a_pair_minimum():
    sfm = cases.build_sfm(cases.SCENE5)
    offsets, image, _ = sfm.tracks(consistent_only=True)
    mask = np.ones(image.numel(), bool)
    mask[int(offsets[3]) + 1] = False                                   # track 3 keeps one observation: skipped
    mask[int(offsets[0]) + 4] = False                                   # the chain loses its observation in image 4
    plan = _check_plan(sfm, mask, 1)
    assert 3 not in plan.job_track.tolist() and plan.stats["n_jobs"] == 9
    plan = _check_plan(sfm, None, 2)
    assert plan.pairs.tolist() == [[0, 1], [2, 1], [2, 3], [2, 4]] and plan.pair_offsets.tolist() == [0, 2, 4, 6, 8]
    assert plan.stats["n_dropped_jobs"] == 3 and plan.stats["n_dropped_pairs"] == 3
    plan = _check_plan(sfm, mask, 2)
    assert plan.pairs.tolist() == [[2, 1], [2, 3]]
    plan = _check_plan(sfm, np.zeros(image.numel(), bool), 1)            # nothing left
    assert plan.stats["n_jobs"] == 0 and plan.pairs.shape == (0, 2) and plan.pair_offsets.tolist() == [0]
    with pytest.raises(ValueError):
        plan_track_refinement(sfm, obs_mask=torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError):
        plan_track_refinement(sfm, min_jobs_per_pair=0)


# ---- 3. the apply rules ----------------------------------------------------------------------------------------------------------
def _fabricated(sfm, plan, seed=1):
    """refine_points outputs for the plan's jobs: every query moves by less than a pixel with a small std, every reference snaps."""
    rng = np.random.default_rng(seed)
    J = plan.job_query_kp.numel()
    kp = sfm.keypoints.numpy()
    return dict(pts0=np.round(kp[plan.job_ref_kp.numpy()] / 2) * 2, pts1=(kp[plan.job_query_kp.numpy()] + rng.uniform(-.7, .7, (J, 2))).astype(np.float32),
                expec_f=np.concatenate([rng.uniform(-1, 1, (J, 2)), rng.uniform(.05, .2, (J, 1))], 1).astype(np.float32), ok=np.ones(J, np.uint8))


def _apply(sfm, plan, res, **kw):
    view, ref = apply_refinement(sfm, plan, {k: T(v) for k, v in res.items()}, **kw)
    want_kp, want_state, accepted = oracle.apply(sfm.keypoints.numpy(), plan.job_ref_kp.numpy(), plan.job_query_kp.numpy(), res, sfm.image_hw,
                                                 kw.get("max_std"), kw.get("max_shift_px"))
    assert np.array_equal(view.keypoints.numpy().view(np.int32), want_kp.view(np.int32))
    assert ref.kp_state.dtype == torch.int8 and np.array_equal(ref.kp_state.numpy(), want_state)
    for s, name in enumerate(("n_untouched", "n_ref_moved", "n_query_accepted", "n_query_rejected", "n_ref_kept")):
        assert ref.stats[name] == int((want_state == s).sum()), name
    moved = np.linalg.norm(want_kp - sfm.keypoints.numpy(), axis=1)
    assert np.allclose(ref.kp_shift_px.numpy(), moved, atol=1e-5) and np.array_equal(ref.job_std.numpy(), res["expec_f"][:, 2])
    assert view.is_refined and not sfm.is_refined and ref.plan is plan
    for k in view.FIELDS:
        assert k == "keypoints" or getattr(view, k) is getattr(sfm, k)
    return view, ref, accepted


def test_apply_rules_and_the_five_states():
    sfm = cases.build_sfm(cases.SCENE5)
    plan = plan_track_refinement(sfm)
    res = _fabricated(sfm, plan)
    view, ref, accepted = _apply(sfm, plan, res)
    assert accepted.all() and set(ref.kp_state.tolist()) == {0, 1, 2}
    assert ref.stats["max_shift_px"] < 1.0 and 0 < ref.stats["mean_shift_px"] <= ref.stats["max_shift_px"]
    untouched = ref.kp_state == 0
    assert torch.equal(view.keypoints[untouched], sfm.keypoints[untouched]) and (ref.kp_shift_px[untouched] == 0).all()
    # every way a query is rejected; all the jobs of track 5 (one job) and of track 2 (two jobs) fail: their references are kept
    job_track = plan.job_track.numpy()
    chain = np.nonzero(job_track == 0)[0]
    res["ok"][chain[0]] = 0
    res["pts1"][chain[0]] = np.nan
    res["pts1"][chain[1]] = (-0.5, 10.0)                                # refined to outside the image
    res["pts1"][chain[2], 0] = 96.0
    res["pts1"][np.nonzero(job_track == 5)[0][0]] = (np.inf, 3.0)
    res["pts1"][job_track == 2] += 30.0                                 # inside the image or not: beyond max_shift_px
    res["expec_f"][np.nonzero(job_track == 1)[0][0], 2] = 0.9           # beyond max_std
    view, ref, accepted = _apply(sfm, plan, res, max_std=0.5, max_shift_px=3.0)
    assert set(ref.kp_state.tolist()) == {0, 1, 2, 3, 4}
    assert accepted.sum() == 11 - 7 and ref.stats["n_ref_kept"] == 2 and ref.stats["n_query_rejected"] == 7
    rejected = ref.kp_state >= 3
    assert torch.equal(view.keypoints[rejected], sfm.keypoints[rejected])
    # without the limits the std and the shift do not reject; the points outside the image still do
    view, ref, accepted = _apply(sfm, plan, res)
    assert accepted.sum() >= 11 - 6


def test_apply_refuses_results_of_another_length():
    sfm = cases.build_sfm(cases.SCENE5)
    plan = plan_track_refinement(sfm)
    res = {k: T(v[:-1]) for k, v in _fabricated(sfm, plan).items()}
    with pytest.raises(ValueError):
        apply_refinement(sfm, plan, res)


# ---- 4. guards -------------------------------------------------------------------------------------------------------------------
def test_topology_stages_refuse_a_refined_view():
    sfm = cases.build_sfm(cases.SCENE5)
    plan = plan_track_refinement(sfm)
    view, _ = apply_refinement(sfm, plan, {k: T(v) for k, v in _fabricated(sfm, plan).items()})
    n = 5
    K = torch.eye(3, dtype=torch.float64).repeat(n, 1, 1)
    pose = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    with pytest.raises(ValueError, match="refined view"):
        view.split()
    with pytest.raises(ValueError, match="refined view"):
        view.merge(None, K, pose)
    with pytest.raises(ValueError, match="refined view"):
        view.complete(None, K, pose)
    und = view.undistorted(K, torch.zeros(n, dtype=torch.float64))
    assert und.is_refined and und.is_undistorted
    with pytest.raises(ValueError, match="undistorted view"):
        und.refine_tracks(None, None)
    with pytest.raises(ValueError, match="undistorted view"):
        sfm.undistorted(K, torch.zeros(n, dtype=torch.float64)).refine_tracks(None, None)


def test_refine_points_guards():
    from loftr_amd import FeatureBank, LoFTR, get_cfg
    model = LoFTR(get_cfg()).eval()
    bank = FeatureBank(model, 4, (64, 96))
    pts = torch.zeros(3, 2)
    with pytest.raises(ValueError, match="ascend"):
        model.refine_points(bank, [0, 1], bank, [2, 3], [1, 0, 1], pts, pts)           # descending
    with pytest.raises(ValueError, match="ascend"):
        model.refine_points(bank, [0, 1], bank, [2, 3], torch.tensor([0, 1, 2]), pts, pts)   # a pair outside the batch
    with pytest.raises(ValueError):
        model.refine_points(bank, [0, 1], bank, [2, 3], [0, 0, 1], pts, pts[:2])
    with pytest.raises(ValueError):
        model.refine_points(bank, [0, 1], bank, [2, 3], [0.0, 0.0, 1.0], pts, pts)
    with pytest.raises(_lib.LoftrHipError):                               # the guards of match_pairs: the slots hold no image
        model.refine_points(bank, [0, 1], bank, [2, 3], [0, 0, 1], pts, pts)
    model.train()
    with pytest.raises(_lib.LoftrHipError, match="inference only"):
        model.refine_points(bank, [0, 1], bank, [2, 3], [0, 0, 1], pts, pts)
