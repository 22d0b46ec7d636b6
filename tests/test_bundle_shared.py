"""Bundle adjustment with one focal step per group of images on the CPU: the host routine
loftr_bundle_adjust_shared_host, which DEFINES the result, against the dense oracle with one focal column per group
(tests/_bundle_shared_oracle.py), against the per-image call on the same inputs, on the cases of the rule, through reconstruct_tracks --
and both per-image paths, and the grouped one, against digests taken on the commits before."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _bundle_cases as BC
import _bundle_focal_cases as FC
import _bundle_shared_cases as SC
import _bundle_shared_oracle as SO
import loftr_amd
from loftr_amd import _lib, build as build_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module", autouse=True)
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def shared(s, **kw):
    kw.setdefault("fixed", s["fixed"])
    kw.setdefault("refine_focal", True)
    kw.setdefault("camera_ids", s["camera_ids"])
    return loftr_amd.bundle_adjust(*BC.inputs(s), **kw)


@functools.lru_cache(maxsize=None)
def solved(name, huber=0.0, max_iters=30):
    """(scene, shared result, the per-image call of §18.1 on the same inputs, oracle), computed once."""
    s = SC.shared_case(name)
    res = shared(s, huber_px=huber, max_iters=max_iters)
    per = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True, huber_px=huber, max_iters=max_iters)
    got = res.to_host()
    focal = SO.carrying(s["obs_image"], got["obs_active"], s["K"], s["T_cam_from_world"], np.ones(len(s["K"]), bool), got["cam_group"], 20)
    orc = SO.adjust(s["offsets"], s["obs_image"], s["obs_xy"], got["obs_active"], s["xyz"], s["K"], s["T_cam_from_world"], s["fixed"], focal,
                    got["cam_group"], huber=huber)
    orc["focal"] = focal
    return s, res, per, orc


def _figures(name, huber=0.0, max_iters=30):
    s, res, per, orc = solved(name, huber, max_iters)
    got, free, focal, every = res.to_host(), res.cam_free.numpy(), res.cam_focal.numpy(), np.ones(len(s["K"]), bool)
    diff = np.abs(FC.projections(s, got["K"], got["T_cam_from_world"], got["xyz"], got["obs_active"]) -
                  FC.projections(s, orc["K"], orc["T"], orc["xyz"], got["obs_active"])).max()
    f0, f1, fo = (FC.focal_errors(K, s["K_true"], focal) for K in (s["K"], got["K"], orc["K"]))
    r1, c1 = BC.pose_errors(got["T_cam_from_world"], s["T_true"], free)
    ro, co = BC.pose_errors(orc["T"], s["T_true"], free)
    return dict(cost=res.cost_after, cost_oracle=orc["cost"], cost_ratio=res.cost_after / orc["cost"], projection_diff=diff, focal_before=f0,
                focal_after=f1, focal_oracle=fo, rot=r1, rot_oracle=ro, centre=c1, centre_oracle=co, rms=res.rms_px_after,
                rms_before=res.rms_px_before, trials=res.n_iters, pcg=res.n_pcg, status=res.status, rms_per=per.rms_px_after,
                focal_per=FC.focal_errors(per.K.numpy(), s["K_true"], every), n_per=per.stats["n_focal_cameras"], pcg_per=per.n_pcg,
                trials_per=per.n_iters, focal_all=FC.focal_errors(got["K"], s["K_true"], every))


def accuracy_lines():
    """The text of profiles/bundle_shared_accuracy.txt."""
    lines = ["bundle_adjust(refine_focal=True, camera_ids=...) on tests/_bundle_shared_cases.py (fx, skew, fy off by one factor of 4-10 % per "
             "camera,", "the fixed-pose images 0 and 1 included), host routine, defaults; oracle: tests/_bundle_shared_oracle.py (dense, ftol "
             "1e-14).  Required: cost ratio", "<= 1.0001, projection difference <= 0.01 px, focal error <= 0.5 x before and <= 1.01 x oracle, "
             "rotation and centre error <= 1.01 x oracle."]
    for name in ("one_a", "one_b", "bodies", "thin"):
        f = _figures(name)
        lines.append(f"{name}: cost {f['cost']:.12g} oracle {f['cost_oracle']:.12g} ratio {f['cost_ratio']:.15f}; projection difference "
                     f"{f['projection_diff']:.3g} px; {f['trials']} trials, {f['pcg']} pcg iterations, {f['status']}")
        lines.append(f"  focal error {f['focal_before']:.5f} -> {f['focal_after']:.7f} (oracle {f['focal_oracle']:.7f}, ratio "
                     f"{f['focal_after'] / f['focal_oracle']:.7f}); rotation {f['rot']:.6f} deg (oracle {f['rot_oracle']:.6f}, ratio "
                     f"{f['rot'] / f['rot_oracle']:.7f}); centre {f['centre']:.6f} (oracle {f['centre_oracle']:.6f}, ratio "
                     f"{f['centre'] / f['centre_oracle']:.7f})")
        lines.append(f"  per-image call (§18.1) on the same inputs: {f['n_per']} images refine, rms {f['rms_before']:.3f} -> {f['rms_per']:.4f} px, "
                     f"largest focal error over all images {f['focal_per']:.5f}, {f['trials_per']} trials, {f['pcg_per']} pcg iterations; shared: "
                     f"rms {f['rms']:.4f} px, largest focal error {f['focal_all']:.5f}")
    lines.append(f"thin: active observations per image {SC.thin_counts().tolist()} (min_focal_obs = 20)")
    return lines


@pytest.mark.parametrize("name", ["one_a", "one_b", "bodies"])
def test_optimum_equals_the_dense_oracle(name):
    """Measured (profiles/bundle_shared_accuracy.txt): cost ratios 1 +- 4e-14, projection differences below 1e-4 px, focal and pose error
    ratios 1 +- 1e-7, with the defaults and the scalar-per-group preconditioner of the issue."""
    s, res, _, orc = solved(name)
    f = _figures(name)
    print(f)
    n = len(s["K"])
    assert res.status == "converged" and res.obs_active.all() and res.point_active.all()
    assert res.cam_free.tolist() == (~s["fixed"]).tolist() and res.cam_focal.all() and orc["focal"].all()
    assert res.stats["n_focal_cameras"] == n and res.stats["n_focal_groups"] == len(set(s["camera_ids"].tolist())) == res.group_focal.numel()
    assert res.group_focal.all()
    assert f["cost"] <= 1.0001 * f["cost_oracle"]
    assert f["projection_diff"] <= 0.01
    assert f["focal_after"] <= 0.5 * f["focal_before"] and f["focal_after"] <= 1.01 * f["focal_oracle"]
    assert f["rot"] <= 1.01 * f["rot_oracle"] and f["centre"] <= 1.01 * f["centre_oracle"]
    K = res.K.numpy()
    assert np.array_equal(K[:, [0, 1, 1, 2, 2, 2], [2, 0, 2, 0, 1, 2]], s["K"][:, [0, 1, 1, 2, 2, 2], [2, 0, 2, 0, 1, 2]])     # cx, cy and the rest stay


@pytest.mark.parametrize("name", ["one_b", "bodies"])
def test_the_fixed_pose_images_take_their_groups_focal(name):
    """Images 0 and 1 keep their pose bit for bit and still refine: their focal ends within the oracle's bar and at the SAME relative
    factor as the other members of their group.  The members' K_out are their K_in times one double, each product rounded once, so
    the quotient K_out / K_in, itself rounded, is that double or a neighbour of it: every member agrees with the group's factor to 1 ulp
    (two quotients on opposite sides of it are 2 ulps apart; scene `bodies` has such a pair)."""
    s, res, _, orc = solved(name)
    K, fixed = res.K.numpy(), s["fixed"]
    assert fixed.tolist()[:2] == [True, True] and res.cam_focal[:2].all() and not res.cam_free[:2].any()
    assert np.array_equal(_bits(res.T_cam_from_world.numpy()[fixed]), _bits(s["T_cam_from_world"][fixed]))
    f0, f1, fo = (FC.focal_errors(k, s["K_true"], fixed) for k in (s["K"], K, orc["K"]))
    print(f"{name}: focal error of the fixed-pose images {f0:.5f} -> {f1:.7f} (oracle {fo:.7f})")
    assert f1 <= 0.5 * f0 and f1 <= 1.01 * fo
    group = res.cam_group.numpy()
    for g in range(res.group_focal.numel()):
        for r, c in ((0, 0), (1, 1)):
            ratio = K[group == g, r, c] / s["K"][group == g, r, c]
            near = ratio[0] + np.arange(-2, 3) * np.spacing(ratio[0])
            exact = [f for f in near if np.array_equal(s["K"][group == g, r, c] * f, K[group == g, r, c])]
            assert exact, (g, ratio)                                                      # ONE factor gives every member's bits ...
            assert np.abs(ratio - exact[0]).max() <= np.spacing(exact[0]), (g, ratio)     # ... and every quotient is within 1 ulp of it
    assert (K[:2, 0, 0] != s["K"][:2, 0, 0]).all()


def test_huber_loss_with_shared_focals():
    """§18.1's Huber bar: final Huber cost <= 1.001 x the oracle's under the same loss, max_iters = 100."""
    s, res, per, orc = solved("huber", huber=2.0, max_iters=100)
    focal = res.cam_focal.numpy()
    f0, f1 = FC.focal_errors(s["K"], s["K_true"], focal), FC.focal_errors(res.K.numpy(), s["K_true"], focal)
    print(f"huber + shared focal: cost {res.cost_after:.12g} oracle {orc['cost']:.12g} ratio {res.cost_after / orc['cost']:.9f}, {res.n_iters} "
          f"trials ({res.status}); focal error {f0:.4f} -> {f1:.5f}; rms {res.rms_px_after:.3f} (per image {per.rms_px_after:.3f})")
    assert res.obs_active.all() and res.stats["n_focal_groups"] == 3 and focal.all()
    assert res.cost_after <= 1.001 * orc["cost"]
    assert f1 <= 0.5 * f0


def test_thin_images_refine_through_their_group_where_the_per_image_call_cannot():
    """Every image of `thin` keeps 13-19 active observations, fewer than min_focal_obs = 20: the per-image call refines no image and its
    focal error stays at the detuning (0.088, rms 1.06 px); the groups hold 94 / 76 / 51 observations and reach the noise floor (largest
    focal error 0.0052, rms 0.39 px) -- the oracle's optimum."""
    s, res, per, orc = solved("thin")
    f = _figures("thin")
    print(f, SC.thin_counts())
    cnt = SC.thin_counts()
    assert cnt.max() <= SC.THIN_CAP < 20 and cnt.min() >= 1 and np.array_equal(cnt, np.bincount(s["obs_image"][res.obs_active.numpy()], minlength=12))
    assert per.stats["n_focal_cameras"] == 0 and np.array_equal(_bits(per.K.numpy()), _bits(s["K"]))
    assert res.cam_focal.all() and res.group_focal.all() and res.status == "converged"
    assert f["rms"] <= f["rms_per"] and f["focal_all"] <= f["focal_per"]
    assert f["focal_all"] <= 0.5 * f["focal_before"] and f["cost"] <= 1.0001 * f["cost_oracle"] and f["focal_after"] <= 1.01 * f["focal_oracle"]
    assert f["projection_diff"] <= 0.01 and f["rot"] <= 1.01 * f["rot_oracle"] and f["centre"] <= 1.01 * f["centre_oracle"]


def test_accuracy_profile_is_current():
    """profiles/bundle_shared_accuracy.txt holds the figures of this build (rewritten when LOFTR_WRITE_PROFILES=1)."""
    path, text = os.path.join(ROOT, "profiles", "bundle_shared_accuracy.txt"), "\n".join(accuracy_lines()) + "\n"
    if os.environ.get("LOFTR_WRITE_PROFILES") == "1":
        with open(path, "w") as fh:
            fh.write(text)
    assert os.path.exists(path) and open(path).read().splitlines()[:3] == text.splitlines()[:3]


# ---- singleton groups ------------------------------------------------------------------------------------------------------------------------
def test_singleton_groups_are_the_per_image_problem_plus_the_fixed_pose_images():
    """Every image its own group, on §18.1's scene B (the K of images 0 and 1 true): the active sets and cam_focal of the per-image call,
    except that the two fixed-pose images refine too.  The costs are compared with those two images held where the shared call left them,
    which makes the two problems the same one (other preconditioner, so no bit equality): measured 5.9e-13 relative.  Against the
    per-image call with their K TRUE the shared call has two more unknowns and fits the 0.5 px noise with them: measured 215.7548 against
    215.8913, 6.3e-4 relative, the size two more fitted parameters give (of the order of sigma^2 = 0.25 each, of 216); that pair can only be ordered,
    not equal to 1e-6, so it is asserted as <= and printed."""
    s = FC.focal_case("scene_b")
    per = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True)
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True, camera_ids=np.arange(12)[::-1].copy())
    assert res.cam_group.tolist() == list(range(12)) and res.stats["n_focal_groups"] == 12
    for k in ("obs_active", "point_active", "cam_free"):
        assert torch.equal(getattr(res, k), getattr(per, k)), k
    assert res.cam_focal.tolist() == [True] * 12 and per.cam_focal.tolist() == [False] * 2 + [True] * 10
    held = dict(s, K=s["K"].copy())
    held["K"][:2] = res.K.numpy()[:2]
    again = loftr_amd.bundle_adjust(*BC.inputs(held), fixed=s["fixed"], refine_focal=True)
    print(f"singletons: cost {res.cost_after:.12g}; per-image call with K[0], K[1] true {per.cost_after:.12g} (relative "
          f"{abs(res.cost_after / per.cost_after - 1):.3g}), with K[0], K[1] as the shared call left them {again.cost_after:.12g} (relative "
          f"{abs(res.cost_after / again.cost_after - 1):.3g})")
    assert abs(res.cost_after / again.cost_after - 1) <= 1e-6
    assert res.cost_after <= per.cost_after * (1 + 1e-6)


# ---- the cases of the rule ---------------------------------------------------------------------------------------------------------------------
def test_sparse_unsorted_ids_are_relabelled_by_first_member():
    s = SC.shared_case("bodies")
    res = shared(s, max_iters=0)
    assert res.cam_group.dtype == torch.int32 and res.cam_group.tolist() == SC.BODY_GROUP.tolist() and res.group_focal.tolist() == [True] * 3
    assert res.FIELDS == ("T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active", "K", "cam_focal", "cam_group", "group_focal")
    assert sorted(res.to_host()) == sorted(res.FIELDS + ("stats",)) and res.stats["n_focal_groups"] == 3
    same = shared(s, camera_ids=SC.BODY_GROUP.astype(np.int64) + 5)     # other labels, the same grouping: the same bits
    full, relabelled = shared(s), shared(s, camera_ids=torch.from_numpy(SC.BODY_GROUP.astype(np.int32)))
    assert torch.equal(full.K, relabelled.K) and torch.equal(full.T_cam_from_world, relabelled.T_cam_from_world) and full.stats == relabelled.stats
    assert torch.equal(same.K, shared(s, camera_ids=s["camera_ids"].tolist()).K)


def test_a_mixed_mask_inside_a_group_returns_the_bits_of_k_for_the_member_left_out():
    s = SC.shared_case("bodies")
    mask = np.ones(12, bool)
    mask[[3, 4]] = False                                                 # one member of body 0, one of body 1
    res = shared(s, refine_focal=mask)
    K = res.K.numpy()
    assert res.cam_focal.tolist() == mask.tolist() and res.group_focal.all() and res.stats["n_focal_cameras"] == 10
    assert np.array_equal(_bits(K[~mask]), _bits(s["K"][~mask])) and (K[mask, 0, 0] != s["K"][mask, 0, 0]).all()
    assert res.cam_free.tolist() == (~s["fixed"]).tolist()               # the members left out still move their pose
    # (the two members left out keep a K that is 7-9 % off, which the points and the refined focals partly absorb)
    assert FC.focal_errors(K, s["K_true"], mask) < 0.5 * FC.focal_errors(s["K"], s["K_true"], mask)


def test_a_group_at_min_focal_obs_and_at_one_more():
    s = SC.shared_case("thin")
    cnt = SC.thin_counts()
    total = [int(cnt[SC.BODY_GROUP == g].sum()) for g in range(3)]
    assert total == [94, 76, 51]
    for m, want in ((51, [True, True, True]), (52, [True, True, False]), (76, [True, True, False]), (77, [True, False, False]), (95, [False] * 3)):
        res = shared(s, min_focal_obs=m)
        member = np.array(want)[SC.BODY_GROUP]
        assert res.group_focal.tolist() == want and res.cam_focal.tolist() == member.tolist(), m
        assert res.stats["n_focal_groups"] == sum(want) and res.stats["n_focal_cameras"] == int(member.sum())
        assert np.array_equal(_bits(res.K.numpy()[~member]), _bits(s["K"][~member]))


def test_a_group_whose_members_all_keep_their_pose():
    s = SC.shared_case("bodies")
    fixed = SC.BODY_GROUP == 2                                           # images 2, 5, 8; nothing else is fixed, the damping holds the gauge
    fixed = fixed | s["fixed"]
    res = shared(s, fixed=fixed)
    K = res.K.numpy()
    assert res.cam_free.tolist() == (~fixed).tolist() and res.cam_focal.all() and res.group_focal.all()
    assert np.array_equal(_bits(res.T_cam_from_world.numpy()[fixed]), _bits(s["T_cam_from_world"][fixed]))
    assert (K[fixed, 0, 0] != s["K"][fixed, 0, 0]).all() and res.cost_after < res.cost_before


def test_a_group_without_an_active_observation():
    s = SC.shared_case("bodies")
    mask = s["obs_mask"] & ~np.isin(s["obs_image"], np.nonzero(SC.BODY_GROUP == 1)[0])
    res = shared(dict(s, obs_mask=mask))
    out = SC.BODY_GROUP == 1
    assert res.group_focal.tolist() == [True, False, True] and res.cam_focal.tolist() == (~out).tolist()
    assert not res.cam_free[out].any() and res.stats["n_focal_groups"] == 2
    assert np.array_equal(_bits(res.K.numpy()[out]), _bits(s["K"][out]))
    assert np.array_equal(_bits(res.T_cam_from_world.numpy()[out]), _bits(s["T_cam_from_world"][out]))


def test_a_first_trial_outside_the_bounds_is_rejected_and_nothing_leaves_them():
    s = SC.shared_case("bodies")
    kw = dict(focal_bounds=(0.97, 1.03))
    one = shared(s, max_iters=1, **kw)
    assert one.n_iters == 1 and one.n_accepted == 0 and one.status == "max_iters" and one.n_pcg > 0
    assert one.stats["lambda"] == 10.0 * 1e-4 and one.cost_after == one.cost_before
    assert np.array_equal(_bits(one.K.numpy()), _bits(s["K"])) and np.array_equal(one.xyz.numpy(), s["xyz"])
    assert shared(s, max_iters=1).n_accepted == 1                        # the same trial is accepted when the bounds admit it
    res = shared(s, max_iters=60, **kw)
    ratio = np.stack([res.K.numpy()[:, 0, 0] / s["K"][:, 0, 0], res.K.numpy()[:, 1, 1] / s["K"][:, 1, 1]])
    print(res.stats, ratio.min(), ratio.max())
    assert res.n_accepted < res.n_iters and (ratio > 0.97).all() and (ratio < 1.03).all() and res.cost_after <= res.cost_before


def test_a_start_at_the_optimum_runs_no_trial_and_returns_the_bits_of_k():
    s = BC.exact_problem()
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True, min_focal_obs=1, camera_ids=[4, 4, 9, 9])
    assert res.status == "converged" and res.n_iters == 0 and res.n_accepted == 0 and res.cost_before == res.cost_after == 0.0
    assert res.cam_focal.all() and res.group_focal.tolist() == [True, True] and res.cam_group.tolist() == [0, 0, 1, 1]
    assert np.array_equal(_bits(res.K.numpy()), _bits(s["K"])) and np.array_equal(res.T_cam_from_world.numpy(), s["T_cam_from_world"])


def test_known_poses_and_an_unknown_focal_move_the_focal():
    """Zero free cameras but a refining group is a problem of its own here: every pose is held at the truth, the focal is found."""
    s = SC.shared_case("one_b")
    s = dict(s, T_cam_from_world=s["T_true"].copy())
    res = shared(s, fixed=np.ones(12, bool))
    f0, f1 = FC.focal_errors(s["K"], s["K_true"], np.ones(12, bool)), FC.focal_errors(res.K.numpy(), s["K_true"], np.ones(12, bool))
    print(f"known poses: focal error {f0:.5f} -> {f1:.6f}, rms {res.rms_px_before:.3f} -> {res.rms_px_after:.4f}, {res.n_iters} trials, {res.n_pcg} pcg")
    assert not res.cam_free.any() and res.stats["n_free_cameras"] == 0 and res.cam_focal.all() and res.stats["n_focal_groups"] == 1
    assert np.array_equal(_bits(res.T_cam_from_world.numpy()), _bits(s["T_true"]))
    assert res.status == "converged" and res.n_pcg > 0 and f1 < 0.02 * f0 and res.rms_px_after < 0.6


def test_hand_written_cases_with_groups():
    s, n = BC.hand_problem()
    ids = [0, 0, 1, 1, 1, 2, 2, 3]                                       # body 2: the camera with fx = 0 and the one without observations
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True, min_focal_obs=1, camera_ids=ids)
    plain = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"])
    got = res.to_host()
    for k in ("obs_active", "point_active", "cam_free"):                 # the active set is §18's
        assert np.array_equal(got[k], getattr(plain, k).numpy()), k
    assert res.status == "converged" and res.cost_after < res.cost_before
    assert got["cam_focal"].tolist() == [True] * 5 + [False] * 3 and got["group_focal"].tolist() == [True, True, False, False]
    assert got["K"][n["bad_cam"], 0, 0] == 0.0 and np.array_equal(_bits(got["K"][5:]), _bits(s["K"][5:]))
    assert np.array_equal(_bits(got["T_cam_from_world"][~got["cam_free"]]), _bits(s["T_cam_from_world"][~got["cam_free"]]))
    assert res.stats["n_focal_cameras"] == 5 and res.stats["n_focal_groups"] == 2 and res.stats["n_free_cameras"] == 3


def test_value_errors():
    s = SC.shared_case("one_a")
    a = BC.inputs(s)
    with pytest.raises(ValueError, match="camera_ids shares the focal step of refine_focal"):
        loftr_amd.bundle_adjust(*a, camera_ids=np.zeros(5, np.int64))
    for ids in (np.zeros(4, np.int64), np.zeros(6, np.int64), np.zeros((5, 1), np.int64)):
        with pytest.raises(ValueError, match=r"camera_ids must have shape \(5,\)"):
            loftr_amd.bundle_adjust(*a, refine_focal=True, camera_ids=ids)
    with pytest.raises(ValueError, match="camera_ids must not be negative"):
        loftr_amd.bundle_adjust(*a, refine_focal=True, camera_ids=[0, 0, -1, 0, 0])
    for ids in (np.zeros(5), np.zeros(5, bool), torch.zeros(5)):
        with pytest.raises(ValueError, match="camera_ids must hold integers"):
            loftr_amd.bundle_adjust(*a, refine_focal=True, camera_ids=ids)

    class FakeGpu(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    with pytest.raises(ValueError, match="camera_ids is on the GPU.*no silent fallback"):
        loftr_amd.bundle_adjust(*a, refine_focal=True, camera_ids=torch.zeros(5, dtype=torch.int64).as_subclass(FakeGpu))
    with pytest.raises(ValueError, match="min_focal_obs must be an integer >= 1"):
        loftr_amd.bundle_adjust(*a, refine_focal=True, camera_ids=np.zeros(5, np.int64), min_focal_obs=0)


# ---- the per-image paths are the ones they were ----------------------------------------------------------------------------------------
def test_per_image_results_equal_the_digests_taken_on_the_parent_commit():
    spec = importlib.util.spec_from_file_location("make_bundle_focal_parent_digest", os.path.join(GOLDEN, "make_bundle_focal_parent_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = json.load(open(os.path.join(GOLDEN, "bundle_focal_parent_digest.json")))
    got = mod.digests()
    assert sorted(got) == sorted(want) == ["hand_problem", "scene_a", "scene_b", "scene_huber"]
    for case in want:
        assert got[case]["inputs"] == want[case]["inputs"], f"{case}: the scene itself is not the one the digests were taken on"
        assert got[case] == want[case], case
        assert sorted(want[case]["wide6"]) == ["T_cam_from_world", "cam_free", "counts", "obs_active", "point_active", "xyz"]
        assert sorted(want[case]["wide7"]) == ["K", "T_cam_from_world", "cam_focal", "cam_free", "counts", "obs_active", "point_active", "xyz"]


def test_shared_results_equal_the_digests_taken_on_the_parent_commit():
    """The grouped host routine returns the bits it returned before the three modes became instantiations of one sequence of phases."""
    spec = importlib.util.spec_from_file_location("make_bundle_shared_parent_digest", os.path.join(GOLDEN, "make_bundle_shared_parent_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = json.load(open(os.path.join(GOLDEN, "bundle_shared_parent_digest.json")))
    got = mod.digests()
    assert sorted(got) == sorted(want) == ["bodies", "hand_problem", "huber", "known_poses", "one_a", "one_b", "singletons_a", "thin",
                                           "thin_above_min", "thin_at_min"]
    for case in want:
        assert got[case]["inputs"] == want[case]["inputs"], f"{case}: the scene itself is not the one the digests were taken on"
        assert got[case] == want[case], case
        assert sorted(want[case]) == ["K", "T_cam_from_world", "cam_focal", "cam_free", "counts", "group_focal", "inputs", "obs_active",
                                      "point_active", "xyz"]
    assert want["thin_at_min"]["group_focal"] != want["thin_above_min"]["group_focal"]        # body 2 refines at 51, not at 52
    assert want["known_poses"]["cam_free"] != want["one_b"]["cam_free"]


def test_without_camera_ids_the_result_has_the_fields_it_had():
    s = SC.shared_case("one_a")
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True)
    assert res.FIELDS == ("T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active", "K", "cam_focal")
    assert not hasattr(res, "cam_group") and not hasattr(res, "group_focal") and "n_focal_groups" not in res.stats
    assert set(shared(s).stats) == set(res.stats) | {"n_focal_groups"}


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
def chain_run(device="cpu"):
    """reconstruct_tracks on the one-camera scene B from the true relative pose of images 0 and 1, all images one camera."""
    s = SC.shared_case("one_b")
    R = s["T_true"][1, :3, :3] @ s["T_true"][0, :3, :3].T
    t = s["T_true"][1, :3, 3] - R @ s["T_true"][0, :3, 3]
    a = [torch.from_numpy(np.ascontiguousarray(s[k])).to(device) for k in ("offsets", "obs_image", "obs_xy", "K")]
    ids = torch.zeros(12, dtype=torch.int64, device=device)
    return s, loftr_amd.reconstruct_tracks(*a, (0, 1, R, t), ba={"refine_focal": True, "camera_ids": ids}, min_corr=6, min_inliers=6)


def test_sfm_reconstruct_and_adjust_pass_the_camera_ids_through():
    """SfmResult.reconstruct(ba=...) with a completion pass, and SfmResult.adjust, on the split atlas of the completion tests (5 images
    of one camera whose focal is 6 % off): every image ends with the one factor of its camera."""
    import _completion_cases as CC
    sfm, s, _ = CC.split_atlas("cpu")
    K = s["K"].copy()
    for r, c in ((0, 0), (0, 1), (1, 1)):
        K[:, r, c] *= 1.06
    ba = {"refine_focal": True, "camera_ids": [3, 3, 3, 3, 3], "min_focal_obs": 5}
    for kw in (dict(), dict(complete=True)):
        rec = sfm.reconstruct(K, min_corr=6, min_inliers=6, ba=ba, **kw)
        ratio = rec.K.numpy()[:, 0, 0] / K[:, 0, 0]
        print(f"sfm.reconstruct({kw}): posed {int(rec.posed.sum())}, K_out / K_in {ratio.min():.6f} .. {ratio.max():.6f}, rms {rec.bundle.rms_px_after:.4f}")
        assert rec.posed.all() and rec.bundle.stats["n_focal_groups"] == 1 and rec.bundle.cam_group.tolist() == [0] * 5
        assert np.ptp(ratio) <= 1e-12 and abs(ratio[0] * 1.06 - 1) < 0.02
    pts = sfm.triangulate(rec.K, rec.T_cam_from_world)
    res = sfm.adjust(pts, rec.K, rec.T_cam_from_world, refine_focal=True, camera_ids=np.array([0, 0, 1, 1, 1]), min_focal_obs=5)
    assert res.stats["n_focal_groups"] == 2 and res.cam_focal.all() and res.cam_group.tolist() == [0, 0, 1, 1, 1]


def test_reconstruct_tracks_with_one_camera():
    s, rec = chain_run()
    every = np.ones(12, bool)
    K = rec.K.numpy()
    f0, f1 = FC.focal_errors(s["K"], s["K_true"], every), FC.focal_errors(K, s["K_true"], every)
    ratio = K[:, 0, 0] / s["K"][:, 0, 0]
    print(f"chain, one camera: posed {rec.stats['n_posed']}, rms {rec.bundle.rms_px_after:.4f} px, focal error {f0:.4f} -> {f1:.5f}, rounds "
          f"{rec.stats['n_rounds']}, spread of K_out / K_in {np.ptp(ratio) / ratio[0]:.3g}")
    assert rec.posed.all() and rec.stats["n_posed"] == 12
    assert rec.bundle.cam_focal.all() and rec.bundle.stats["n_focal_groups"] == 1
    assert f1 < 0.1 * f0
    assert np.ptp(ratio) <= 1e-12 * ratio[0] and np.ptp(K[:, 1, 1] / s["K"][:, 1, 1]) <= 1e-12 * ratio[0]     # one camera, one focal
