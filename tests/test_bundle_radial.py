"""Bundle adjustment with one radial coefficient per group of images on the CPU: the host routine
loftr_bundle_adjust_radial_host, which DEFINES the result, against the dense oracle with one more column per group
(tests/_bundle_radial_oracle.py), against the shared-focal call on the same distorted scenes (which cannot fit them), on the cases of the
rule, through reconstruct_tracks -- and every call without refine_radial against the digests taken on the commits before."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _bundle_cases as BC
import _bundle_focal_cases as FC
import _bundle_radial_cases as RC
import _bundle_radial_oracle as RO
import _bundle_shared_cases as SC
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


def radial(s, **kw):
    kw.setdefault("fixed", s["fixed"])
    kw.setdefault("refine_focal", True)
    kw.setdefault("refine_radial", True)
    kw.setdefault("camera_ids", s["camera_ids"])
    kw.setdefault("radial", s["radial"])
    return loftr_amd.bundle_adjust(*BC.inputs(s), **kw)


def shared(s, **kw):
    return loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True, camera_ids=s["camera_ids"], **kw)


@functools.lru_cache(maxsize=None)
def solved(name, huber=0.0, max_iters=30):
    """(scene, radial result, the shared-focal call of §18.2 on the same inputs, oracle), computed once."""
    s = RC.radial_case(name)
    res = radial(s, huber_px=huber, max_iters=max_iters)
    pin = shared(s, huber_px=huber, max_iters=max_iters)
    got, every = res.to_host(), np.ones(len(s["K"]), bool)
    focal, rad = RO.carrying(s["obs_image"], got["obs_active"], s["K"], s["T_cam_from_world"], every, every, got["cam_group"], 20)
    orc = RO.adjust(s["offsets"], s["obs_image"], s["obs_xy"], got["obs_active"], s["xyz"], s["K"], s["T_cam_from_world"], s["fixed"], focal, rad,
                    got["cam_group"], s["radial"], huber=huber)
    orc["focal"], orc["radial"] = focal, rad
    return s, res, pin, orc


def pixels(s, K, T, xyz, k, use):
    """The distorted projections [M,2] of the observations `use`."""
    track = np.repeat(np.arange(len(s["offsets"]) - 1), np.diff(s["offsets"]))
    return np.stack([RC.observe(K[s["obs_image"][o]], T[s["obs_image"][o]], np.asarray(xyz[track[o]], np.float64), k[s["obs_image"][o]])
                     for o in np.nonzero(use)[0]])


def _figures(name, huber=0.0, max_iters=30):
    s, res, pin, orc = solved(name, huber, max_iters)
    got, free, every = res.to_host(), res.cam_free.numpy(), np.ones(len(s["K"]), bool)
    diff = np.abs(pixels(s, got["K"], got["T_cam_from_world"], got["xyz"], got["radial"], got["obs_active"]) -
                  pixels(s, orc["K"], orc["T"], orc["xyz"], orc["k"], got["obs_active"])).max()
    f0, f1, fo, fp = (FC.focal_errors(K, s["K_true"], every) for K in (s["K"], got["K"], orc["K"], pin.K.numpy()))
    r1, c1 = BC.pose_errors(got["T_cam_from_world"], s["T_true"], free)
    ro, co = BC.pose_errors(orc["T"], s["T_true"], free)
    rp, cp = BC.pose_errors(pin.T_cam_from_world.numpy(), s["T_true"], free)
    return dict(cost=res.cost_after, cost_oracle=orc["cost"], cost_ratio=res.cost_after / orc["cost"], projection_diff=diff, focal_before=f0,
                focal_after=f1, focal_oracle=fo, focal_shared=fp, k_err=float(np.abs(got["radial"] - s["k_true"]).max()),
                k_err_oracle=float(np.abs(orc["k"] - s["k_true"]).max()), rot=r1, rot_oracle=ro, rot_shared=rp, centre=c1, centre_oracle=co,
                rms=res.rms_px_after, rms_before=res.rms_px_before, rms_shared=pin.rms_px_after, trials=res.n_iters, pcg=res.n_pcg,
                status=res.status, k=sorted(set(np.round(got["radial"], 7).tolist())), trials_shared=pin.n_iters, pcg_shared=pin.n_pcg)


def accuracy_lines():
    """The text of profiles/bundle_radial_accuracy.txt."""
    lines = ["bundle_adjust(refine_focal=True, refine_radial=True, camera_ids=...) on tests/_bundle_radial_cases.py (the scenes of §18.2 seen "
             "through one", "radial coefficient per camera, k = -0.12 / 0.08 / -0.05, 0.5 px noise; start k = 0), host routine, defaults; oracle: "
             "tests/_bundle_radial_oracle.py (dense,", "ftol 1e-14).  Required: cost ratio <= 1.0001, projection difference <= 0.01 px, focal, "
             "radial, rotation and centre error <= 1.01 x oracle."]
    for name in ("one_a", "one_b", "bodies"):
        f = _figures(name)
        lines.append(f"{name}: cost {f['cost']:.12g} oracle {f['cost_oracle']:.12g} ratio {f['cost_ratio']:.15f}; projection difference "
                     f"{f['projection_diff']:.3g} px; {f['trials']} trials, {f['pcg']} pcg iterations, {f['status']}; k found {f['k']}")
        lines.append(f"  focal error {f['focal_before']:.5f} -> {f['focal_after']:.7f} (oracle {f['focal_oracle']:.7f}, ratio "
                     f"{f['focal_after'] / f['focal_oracle']:.7f}); radial error {f['k_err']:.7f} (oracle {f['k_err_oracle']:.7f}, ratio "
                     f"{f['k_err'] / f['k_err_oracle']:.7f}); rotation {f['rot']:.6f} deg (oracle {f['rot_oracle']:.6f}, ratio "
                     f"{f['rot'] / f['rot_oracle']:.7f}); centre {f['centre']:.6f} (oracle {f['centre_oracle']:.6f}, ratio "
                     f"{f['centre'] / f['centre_oracle']:.7f})")
        lines.append(f"  shared-focal call (§18.2) on the same inputs: rms {f['rms_before']:.3f} -> {f['rms_shared']:.4f} px, focal error "
                     f"{f['focal_shared']:.5f}, rotation {f['rot_shared']:.4f} deg, {f['trials_shared']} trials, {f['pcg_shared']} pcg iterations; "
                     f"radial: rms {f['rms']:.4f} px ({f['rms_shared'] / f['rms']:.2f} x lower)")
    f = _figures("huber", 2.0, 100)
    lines.append(f"huber (radius 2 px, max_iters 100): cost {f['cost']:.12g} oracle {f['cost_oracle']:.12g} ratio {f['cost_ratio']:.9f}; {f['trials']} "
                 f"trials ({f['status']}); radial error {f['k_err']:.6f} (oracle {f['k_err_oracle']:.6f}); rms {f['rms']:.3f} px (shared {f['rms_shared']:.3f})")
    return lines


@pytest.mark.parametrize("name", ["one_a", "one_b", "bodies"])
def test_optimum_equals_the_dense_oracle(name):
    """§18.2's bars with the defaults.  Measured (profiles/bundle_radial_accuracy.txt): cost ratios 1 +- 6e-12, projection differences
    below 1e-4 px, focal, radial and pose error ratios 1 +- 1e-5."""
    s, res, _, orc = solved(name)
    f = _figures(name)
    print(f)
    n = len(s["K"])
    assert res.status == "converged" and res.obs_active.all() and res.point_active.all()
    assert res.cam_free.tolist() == (~s["fixed"]).tolist() and res.cam_focal.all() and res.cam_radial.all() and orc["radial"].all()
    assert res.stats["n_radial_cameras"] == n == res.stats["n_focal_cameras"] and res.group_radial.all() and res.group_focal.all()
    assert res.group_radial.numel() == len(set(s["camera_ids"].tolist()))
    assert f["cost"] <= 1.0001 * f["cost_oracle"]
    assert f["projection_diff"] <= 0.01
    assert f["focal_after"] <= 1.01 * f["focal_oracle"] and f["k_err"] <= 1.01 * f["k_err_oracle"]
    assert f["rot"] <= 1.01 * f["rot_oracle"] and f["centre"] <= 1.01 * f["centre_oracle"]
    K = res.K.numpy()
    assert np.array_equal(K[:, [0, 1, 1, 2, 2, 2], [2, 0, 2, 0, 1, 2]], s["K"][:, [0, 1, 1, 2, 2, 2], [2, 0, 2, 0, 1, 2]])     # cx, cy and the rest stay
    k, group = res.radial.numpy(), res.cam_group.numpy()
    for g in range(res.group_radial.numel()):                            # one step per group on equal starts: one value per group, bit for bit
        assert len(set(_bits(k[group == g]).tolist())) == 1


@pytest.mark.parametrize("name", ["one_b", "bodies"])
def test_the_pinhole_model_cannot_fit_a_distorted_scene_and_the_radial_model_does(name):
    """The test that fails without the feature.  The shared-focal call, today's best pinhole model, ends at 3.9 / 3.5 px rms on these
    scenes and pushes the distortion into the focal (30 % / 17 % off); the radial call ends at the 0.55 px noise floor.  The floor of 3 x
    is well under what the two dense oracles measure (7.1 x and 6.5 x)."""
    s, res, pin, _ = solved(name)
    f = _figures(name)
    print(f"{name}: shared-focal rms {pin.rms_px_after:.3f} px, focal error {f['focal_shared']:.4f}; radial rms {res.rms_px_after:.4f} px, focal "
          f"error {f['focal_after']:.5f}, k {f['k']}")
    assert pin.rms_px_after >= 3.0 * res.rms_px_after
    assert f["focal_after"] < 0.1 * f["focal_shared"]


def test_huber_loss_with_a_radial_coefficient():
    """§18.1's Huber bar: final Huber cost <= 1.001 x the oracle's under the same loss, max_iters = 100."""
    s, res, pin, orc = solved("huber", huber=2.0, max_iters=100)
    print(f"huber + radial: cost {res.cost_after:.12g} oracle {orc['cost']:.12g} ratio {res.cost_after / orc['cost']:.9f}, {res.n_iters} trials "
          f"({res.status}); k {sorted(set(np.round(res.radial.numpy(), 5).tolist()))}; rms {res.rms_px_after:.3f} (shared {pin.rms_px_after:.3f})")
    assert res.obs_active.all() and res.stats["n_focal_groups"] == 3 and res.cam_radial.all()
    assert res.cost_after <= 1.001 * orc["cost"]
    assert np.abs(res.radial.numpy() - s["k_true"]).max() < 0.01


def test_accuracy_profile_is_current():
    """profiles/bundle_radial_accuracy.txt holds the figures of this build (rewritten when LOFTR_WRITE_PROFILES=1)."""
    path, text = os.path.join(ROOT, "profiles", "bundle_radial_accuracy.txt"), "\n".join(accuracy_lines()) + "\n"
    if os.environ.get("LOFTR_WRITE_PROFILES") == "1":
        with open(path, "w") as fh:
            fh.write(text)
    assert os.path.exists(path) and open(path).read().splitlines()[:3] == text.splitlines()[:3]


# ---- the cases of the rule ---------------------------------------------------------------------------------------------------------------------
def test_a_mask_inside_a_group_returns_the_bits_of_k_for_the_member_left_out():
    s = RC.radial_case("bodies")
    s = dict(s, radial=np.linspace(-0.02, 0.02, 12))                     # distinct starts: the members of a group take ONE step on them
    mask = np.ones(12, bool)
    mask[[3, 4]] = False                                                 # one member of body 0, one of body 1
    res = radial(s, refine_radial=mask)
    k, group = res.radial.numpy(), res.cam_group.numpy()
    assert res.cam_radial.tolist() == mask.tolist() and res.cam_focal.all() and res.group_radial.all() and res.stats["n_radial_cameras"] == 10
    assert np.array_equal(_bits(k[~mask]), _bits(s["radial"][~mask])) and (k[mask] != s["radial"][mask]).all()
    assert res.FIELDS == ("T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active", "K", "cam_focal", "cam_group", "group_focal",
                          "radial", "cam_radial", "group_radial")
    assert sorted(res.to_host()) == sorted(res.FIELDS + ("stats",))
    for g in range(3):                                                   # k_out = k_in + a_g, one rounding: k_out - k_in is a_g to an ulp of k_out
        step = (k - s["radial"])[(group == g) & mask]
        assert np.ptp(step) <= 2 * np.spacing(np.abs(k).max())


def test_a_group_at_min_focal_obs_and_at_one_more():
    s = dict(RC.radial_case("bodies"))
    s["obs_mask"] = SC.thin_mask(s)
    cnt = np.bincount(s["obs_image"][s["obs_mask"]], minlength=12)
    assert [int(cnt[SC.BODY_GROUP == g].sum()) for g in range(3)] == [94, 76, 51]
    mask = np.ones(12, bool)
    mask[8] = False                                                      # body 2 = images 2, 5, 8: its radial count leaves image 8 out
    few = int(cnt[2] + cnt[5])
    assert few < 51
    for m, focal, rad in ((few, [True] * 3, [True] * 3), (few + 1, [True] * 3, [True, True, False]), (51, [True] * 3, [True, True, False]),
                          (52, [True, True, False], [True, True, False]), (95, [False] * 3, [False] * 3)):
        res = radial(s, refine_radial=mask, min_focal_obs=m)
        member = np.array(rad)[SC.BODY_GROUP] & mask
        assert res.group_focal.tolist() == focal and res.group_radial.tolist() == rad and res.cam_radial.tolist() == member.tolist(), m
        assert res.stats["n_radial_cameras"] == int(member.sum()) and res.stats["n_focal_groups"] == sum(focal)
        assert np.array_equal(_bits(res.radial.numpy()[~member]), _bits(s["radial"][~member]))


def test_a_group_whose_members_all_keep_their_pose_and_known_poses():
    s = RC.radial_case("bodies")
    fixed = (SC.BODY_GROUP == 2) | s["fixed"]                            # images 2, 5, 8 and 0, 1
    res = radial(s, fixed=fixed)
    assert res.cam_free.tolist() == (~fixed).tolist() and res.cam_radial.all() and res.group_radial.all()
    assert np.array_equal(_bits(res.T_cam_from_world.numpy()[fixed]), _bits(s["T_cam_from_world"][fixed]))
    assert (res.radial.numpy() != 0).all() and res.cost_after < res.cost_before      # (their poses are held where the scene perturbed them)
    one = RC.radial_case("one_b")
    known = radial(dict(one, T_cam_from_world=one["T_true"].copy()), fixed=np.ones(12, bool))      # zero free cameras, one refining group
    print(f"known poses: k {known.radial[0]:.5f}, rms {known.rms_px_before:.3f} -> {known.rms_px_after:.4f}, {known.n_iters} trials, {known.n_pcg} pcg")
    assert not known.cam_free.any() and known.stats["n_radial_cameras"] == 12 and known.status == "converged" and known.n_pcg > 0
    assert abs(float(known.radial[0]) - RC.K_ONE) < 0.01 and known.rms_px_after < 0.6


def test_a_first_trial_outside_the_bounds_is_rejected_and_nothing_moves():
    s = RC.radial_case("bodies")
    kw = dict(radial_bounds=(-0.01, 0.01))
    one = radial(s, max_iters=1, **kw)
    assert one.n_iters == 1 and one.n_accepted == 0 and one.status == "max_iters" and one.n_pcg > 0
    assert one.stats["lambda"] == 10.0 * 1e-4 and one.cost_after == one.cost_before
    assert np.array_equal(_bits(one.K.numpy()), _bits(s["K"])) and np.array_equal(_bits(one.radial.numpy()), _bits(s["radial"]))
    assert np.array_equal(one.xyz.numpy(), s["xyz"]) and np.abs(one.T_cam_from_world.numpy() - s["T_cam_from_world"]).max() < 1e-15
    assert radial(s, max_iters=1).n_accepted == 1                        # the same trial is accepted when the bounds admit it
    res = radial(s, max_iters=60, **kw)
    print(res.stats, res.radial.numpy().min(), res.radial.numpy().max())
    assert res.n_accepted < res.n_iters and (res.radial.numpy() >= -0.01).all() and (res.radial.numpy() <= 0.01).all()
    assert res.cost_after <= res.cost_before
    inside = radial(s, radial_bounds=(-0.5, 0.5))                        # bounds that never bind change nothing
    assert np.array_equal(_bits(inside.radial.numpy()), _bits(radial(s).radial.numpy()))


def test_a_start_at_a_cost_of_zero_runs_no_trial_and_returns_the_bits():
    """The issue's case re-observes the exact problem with k = 0.05.  No cost-0 start exists there in floats: 0.05 is no dyadic number, so
    x (1 + k r^2) is rounded in float64 and its pixel again in float32, and the residual of the routine's own arithmetic is not 0.  That
    case is dropped; what remains checkable is the exact problem itself with the start k = 0 (m = 1 exactly), where the cost is exactly 0."""
    s = BC.exact_problem()
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True, refine_radial=True, min_focal_obs=1, camera_ids=[4, 4, 9, 9])
    assert res.status == "converged" and res.n_iters == 0 and res.n_accepted == 0 and res.cost_before == res.cost_after == 0.0
    assert res.cam_radial.all() and res.group_radial.tolist() == [True, True] and res.cam_group.tolist() == [0, 0, 1, 1]
    assert np.array_equal(_bits(res.K.numpy()), _bits(s["K"])) and np.array_equal(_bits(res.radial.numpy()), _bits(np.zeros(4)))


def test_an_image_whose_start_value_is_not_finite_is_not_valid():
    s = RC.radial_case("bodies")
    for bad in (np.nan, np.inf):
        start = s["radial"].copy()
        start[6] = bad
        res = radial(s, radial=start)
        assert not res.cam_free[6] and not res.cam_focal[6] and not res.cam_radial[6] and not res.obs_active.numpy()[s["obs_image"] == 6].any()
        assert np.array_equal(_bits(res.radial.numpy()[6:7]), _bits(start[6:7])) and res.stats["n_radial_cameras"] == 11
        assert np.array_equal(_bits(res.T_cam_from_world.numpy()[6]), _bits(s["T_cam_from_world"][6])) and res.group_radial.all()


def test_singleton_groups_without_camera_ids():
    s = RC.radial_case("one_a")
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True, refine_radial=True)
    same = radial(s, camera_ids=np.arange(5))
    assert res.cam_group.tolist() == list(range(5)) and res.stats["n_focal_groups"] == 5 and res.stats == same.stats
    assert torch.equal(res.radial, same.radial) and torch.equal(res.K, same.K) and res.radial.dtype == torch.float64
    assert res.cost_after <= solved("one_a")[1].cost_after               # five lenses fit no worse than one


def test_value_errors():
    s = RC.radial_case("one_a")
    a = BC.inputs(s)
    with pytest.raises(ValueError, match="refine_radial refines a radial coefficient next to the focal step.*pass refine_focal"):
        loftr_amd.bundle_adjust(*a, refine_radial=True)
    with pytest.raises(ValueError, match="radial without refine_radial.*undistort the observations.*then make the pinhole call"):
        loftr_amd.bundle_adjust(*a, refine_focal=True, radial=np.zeros(5))
    with pytest.raises(ValueError, match="radial without refine_radial"):
        loftr_amd.bundle_adjust(*a, radial=np.zeros(5))
    with pytest.raises(ValueError, match="position_prior together with refine_radial is not modelled"):
        loftr_amd.bundle_adjust(*a, refine_focal=True, refine_radial=True, position_prior=np.zeros((5, 3)))
    with pytest.raises(ValueError, match="refine_radial must be None, True or an \\[n\\] mask"):
        loftr_amd.bundle_adjust(*a, refine_focal=True, refine_radial=False)
    for bad in (np.ones(4, bool), np.ones((5, 1), bool)):
        with pytest.raises(ValueError, match=r"refine_radial must have shape \(5,\)"):
            loftr_amd.bundle_adjust(*a, refine_focal=True, refine_radial=bad)
    with pytest.raises(ValueError, match=r"radial must have shape \(5,\)"):
        loftr_amd.bundle_adjust(*a, refine_focal=True, refine_radial=True, radial=np.zeros(6))
    for bad in (None, (0.0,), (0.5, -0.5), (float("nan"), 1.0), (-1.0, float("inf"))):
        with pytest.raises(ValueError, match="radial_bounds must be a pair|radial bounds must be finite"):
            loftr_amd.bundle_adjust(*a, refine_focal=True, refine_radial=True, radial_bounds=bad)


# ---- without refine_radial every call is the one it was ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["bundle", "bundle_focal", "bundle_shared"])
def test_calls_without_refine_radial_equal_the_digests_taken_on_the_commits_before(which):
    """The pose, per-image focal and grouped host routines through this build: the digests of tests/golden, recomputed."""
    spec = importlib.util.spec_from_file_location(f"make_{which}_parent_digest", os.path.join(GOLDEN, f"make_{which}_parent_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = json.load(open(os.path.join(GOLDEN, f"{which}_parent_digest.json")))
    got = mod.digests()
    assert sorted(got) == sorted(want) and len(want) >= 4
    for case in want:
        assert got[case] == want[case], case


def _digest_module(which):
    spec = importlib.util.spec_from_file_location(f"make_{which}_parent_digest", os.path.join(GOLDEN, f"make_{which}_parent_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("case", sorted(_digest_module("bundle_radial").CASES))
def test_the_radial_host_routine_equals_the_digest_taken_on_the_commit_before_the_modes_became_traits(case):
    """loftr_bundle_adjust_radial_host through this build: every output tensor and the 16 counts, bit for bit what the commit before
    the mode refactor returned (tests/golden/make_bundle_radial_parent_digest.py)."""
    want = json.load(open(os.path.join(GOLDEN, "bundle_radial_parent_digest.json")))
    got = _digest_module("bundle_radial").digests(only=[case])
    assert len(want) == 8 and sorted(got) == [case] and len(want[case]) == 13
    assert got[case] == want[case]


def test_without_refine_radial_the_result_has_the_fields_it_had():
    s = RC.radial_case("one_a")
    res = shared(s)
    assert res.FIELDS == ("T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active", "K", "cam_focal", "cam_group", "group_focal")
    assert not hasattr(res, "radial") and "n_radial_cameras" not in res.stats
    assert set(radial(s).stats) == set(res.stats) | {"n_radial_cameras"}


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_run():
    """reconstruct_tracks on the distorted one-camera scene B from the true relative pose of images 0 and 1."""
    s = RC.radial_case("one_b")
    R = s["T_true"][1, :3, :3] @ s["T_true"][0, :3, :3].T
    t = s["T_true"][1, :3, 3] - R @ s["T_true"][0, :3, 3]
    a = [torch.from_numpy(np.ascontiguousarray(s[k])) for k in ("offsets", "obs_image", "obs_xy", "K")]
    ids = torch.zeros(12, dtype=torch.int64)
    ba = {"refine_focal": True, "refine_radial": True, "camera_ids": ids}
    return s, a, ids, loftr_amd.reconstruct_tracks(*a, (0, 1, R, t), ba=ba, min_corr=6, min_inliers=6)


def test_reconstruct_tracks_with_one_lens():
    """All 12 images posed; Reconstruction.radial is the last adjustment's, bit for bit, and as near the truth as the oracle's.

    The issue asks that Reconstruction.radial equal, bit for bit, the radial of ONE bundle_adjust call made outside the loop on
    rec.T_cam_from_world, rec.K, rec.points and rec.radial as the start.  As stated that cannot hold: rec.points are triangulated AFTER
    the last adjustment, so they are not the adjustment's points, the outside call starts a little off its optimum (cost 240.96 against
    239.07), accepts trials and moves k in the tenth digit (measured 1.0e-10).  What does hold bit for bit, and is asserted: the loop's
    radial is its last adjustment's (rec.bundle.radial), and the outside call with max_iters = 0 returns its start.  The full outside call
    is made as well and must leave k where it is to 1 % of the oracle's own distance to the truth: re-adjusting the final state may not
    move the lens by more than a hundredth of its statistical error."""
    s, a, ids, rec = chain_run()
    every = np.ones(12, bool)
    k = rec.radial.numpy()
    orc = solved("one_b")[3]
    d, d_orc = float(np.abs(k - s["k_true"]).max()), float(np.abs(orc["k"] - s["k_true"]).max())
    f0, f1 = FC.focal_errors(s["K"], s["K_true"], every), FC.focal_errors(rec.K.numpy(), s["K_true"], every)
    print(f"chain, one lens: posed {rec.stats['n_posed']}, rounds {rec.stats['n_rounds']}, rms {rec.bundle.rms_px_after:.4f} px, k {k[0]:.7f} "
          f"(distance to the truth {d:.3g}, oracle {d_orc:.3g}), focal error {f0:.4f} -> {f1:.5f}")
    assert rec.posed.all() and rec.stats["n_posed"] == 12
    assert rec.bundle.cam_radial.all() and rec.bundle.stats["n_focal_groups"] == 1 and rec.radial.dtype == torch.float64
    assert np.array_equal(_bits(k), _bits(rec.bundle.radial.numpy())) and len(set(_bits(k).tolist())) == 1
    assert d <= 1.01 * d_orc
    assert f1 < 0.1 * f0
    kw = dict(fixed=torch.arange(12) == 0, refine_focal=True, refine_radial=True, camera_ids=ids, radial=rec.radial)
    args = (a[0], a[1], a[2], rec.points.obs_inlier, rec.points.xyz, rec.K, rec.T_cam_from_world)
    still = loftr_amd.bundle_adjust(*args, max_iters=0, **kw)
    assert np.array_equal(_bits(still.radial.numpy()), _bits(k)) and np.array_equal(_bits(still.K.numpy()), _bits(rec.K.numpy()))
    again = loftr_amd.bundle_adjust(*args, **kw)
    moved = float(np.abs(again.radial.numpy() - k).max())
    print(f"  one more adjustment from the final state: cost {again.cost_before:.6g} -> {again.cost_after:.6g}, k moves by {moved:.3g}")
    assert moved <= 0.01 * d_orc and again.status == "converged"


def test_the_chain_reads_undistorted_pixels_and_known_lenses_need_no_refinement():
    """undistort_points with the chain's final K and radial puts the observations within the noise of the pinhole projections of the
    final model; and with the lens KNOWN (radial=k_true, no refine_radial) the loop is the pinhole loop on undistorted pixels."""
    s, a, ids, rec = chain_run()
    xy, ok = loftr_amd.undistort_points(a[2], a[1], rec.K, rec.radial)
    assert ok.all()
    track = np.repeat(np.arange(len(s["offsets"]) - 1), np.diff(s["offsets"]))
    use = rec.points.obs_inlier.numpy()
    proj = FC.projections(s, rec.K.numpy(), rec.T_cam_from_world.numpy(), rec.points.xyz.numpy(), use)
    rms = float(np.sqrt(((proj - xy.numpy()[use]) ** 2).sum(1).mean()))
    print(f"undistorted observations against the pinhole projections of the final model: rms {rms:.3f} px over {int(use.sum())} observations")
    assert use.sum() >= 700 and rms < 1.5
    R = s["T_true"][1, :3, :3] @ s["T_true"][0, :3, :3].T
    t = s["T_true"][1, :3, 3] - R @ s["T_true"][0, :3, 3]
    known = loftr_amd.reconstruct_tracks(*a[:3], torch.from_numpy(s["K_true"]), (0, 1, R, t), radial=s["k_true"], min_corr=6, min_inliers=6)
    assert known.posed.all() and np.array_equal(_bits(known.radial.numpy()), _bits(s["k_true"])) and not hasattr(known.bundle, "radial")
    assert known.bundle.rms_px_after < 0.7
    with pytest.raises(ValueError, match="an argument of the loop"):
        loftr_amd.reconstruct_tracks(*a, (0, 1, R, t), ba={"refine_focal": True, "refine_radial": True, "radial": np.zeros(12)})
