"""Bundle adjustment with per-image focal refinement on the CPU: the host routine loftr_bundle_adjust_focal_host, which
DEFINES the result, against the dense oracle with a focal column (tests/_bundle_focal_oracle.py), against the fixed-intrinsics call on
the same inputs, on the cases of the rule, through reconstruct_tracks -- and the 6-wide path against digests taken before the camera
block became a template."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _bundle_cases as BC
import _bundle_focal_cases as FC
import _bundle_focal_oracle as FO
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module", autouse=True)
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


@functools.lru_cache(maxsize=None)
def solved(name, huber=0.0, max_iters=30):
    """(detuned scene, library result with focal refinement, the same call with fixed intrinsics, oracle), computed once."""
    s = FC.focal_case(name)
    kw = dict(fixed=s["fixed"], huber_px=huber, max_iters=max_iters)
    res = loftr_amd.bundle_adjust(*BC.inputs(s), refine_focal=True, **kw)
    plain = loftr_amd.bundle_adjust(*BC.inputs(s), **kw)
    orc = FO.adjust(s["offsets"], s["obs_image"], s["obs_xy"], s["obs_mask"], s["xyz"], s["K"], s["T_cam_from_world"], s["fixed"],
                    np.ones(len(s["K"]), bool), huber=huber)
    return s, res, plain, orc


def _figures(name, huber=0.0, max_iters=30):
    s, res, plain, orc = solved(name, huber, max_iters)
    got, free = res.to_host(), res.cam_free.numpy()
    diff = np.abs(FC.projections(s, got["K"], got["T_cam_from_world"], got["xyz"], got["obs_active"]) -
                  FC.projections(s, orc["K"], orc["T"], orc["xyz"], got["obs_active"])).max()
    f0, f1, fo = (FC.focal_errors(K, s["K_true"], free) for K in (s["K"], got["K"], orc["K"]))
    r1, c1 = BC.pose_errors(got["T_cam_from_world"], s["T_true"], free)
    ro, co = BC.pose_errors(orc["T"], s["T_true"], free)
    rp, cp = BC.pose_errors(plain.T_cam_from_world.numpy(), s["T_true"], free)
    return dict(cost=res.cost_after, cost_oracle=orc["cost"], cost_ratio=res.cost_after / orc["cost"], projection_diff=diff, focal_before=f0,
                focal_after=f1, focal_oracle=fo, rot=r1, rot_oracle=ro, centre=c1, centre_oracle=co, rot_plain=rp, centre_plain=cp,
                rms=res.rms_px_after, rms_plain=plain.rms_px_after, rms_before=res.rms_px_before, trials=res.n_iters, pcg=res.n_pcg,
                status=res.status)


def accuracy_lines():
    """The text of profiles/bundle_focal_accuracy.txt."""
    lines = ["bundle_adjust(refine_focal=True) on tests/_bundle_focal_cases.py (the focal of every free camera off by 4-10 %), host routine, "
             "defaults;", "oracle: tests/_bundle_focal_oracle.py (dense, ftol 1e-14).  Required: cost ratio <= 1.0001, projection difference "
             "<= 0.01 px,", "focal error <= 0.5 x before and <= 1.01 x oracle, rotation and centre error <= 1.01 x oracle."]
    for name in ("scene_a", "scene_b"):
        f = _figures(name)
        lines.append(f"{name}: cost {f['cost']:.12g} oracle {f['cost_oracle']:.12g} ratio {f['cost_ratio']:.15f}; projection difference "
                     f"{f['projection_diff']:.3g} px; {f['trials']} trials, {f['pcg']} pcg iterations, {f['status']}")
        lines.append(f"  focal error {f['focal_before']:.5f} -> {f['focal_after']:.7f} (oracle {f['focal_oracle']:.7f}, ratio "
                     f"{f['focal_after'] / f['focal_oracle']:.7f}); rotation {f['rot']:.6f} deg (oracle {f['rot_oracle']:.6f}, ratio "
                     f"{f['rot'] / f['rot_oracle']:.7f}); centre {f['centre']:.6f} (oracle {f['centre_oracle']:.6f}, ratio "
                     f"{f['centre'] / f['centre_oracle']:.7f})")
        lines.append(f"  fixed intrinsics on the same inputs: rms {f['rms_before']:.3f} -> {f['rms_plain']:.4f} px, rotation {f['rot_plain']:.4f} deg, "
                     f"centre {f['centre_plain']:.4f}; with the focal: rms {f['rms']:.4f} px")
    return lines


@pytest.mark.parametrize("name", ["scene_a", "scene_b"])
def test_optimum_equals_the_dense_oracle(name):
    """Measured (profiles/bundle_focal_accuracy.txt): cost ratios 1 + 4e-14, projection differences 2e-5 px, focal and pose error ratios
    1 +- 1e-7, with the defaults."""
    s, res, _, _ = solved(name)
    f = _figures(name)
    print(f)
    assert res.status == "converged" and res.obs_active.all() and res.point_active.all()
    assert res.cam_free.tolist() == (~s["fixed"]).tolist() == res.cam_focal.tolist() and res.stats["n_focal_cameras"] == int((~s["fixed"]).sum())
    assert f["cost"] <= 1.0001 * f["cost_oracle"]
    assert f["projection_diff"] <= 0.01
    assert f["focal_after"] <= 0.5 * f["focal_before"] and f["focal_after"] <= 1.01 * f["focal_oracle"]
    assert f["rot"] <= 1.01 * f["rot_oracle"] and f["centre"] <= 1.01 * f["centre_oracle"]
    fixed = s["fixed"]
    assert np.array_equal(res.K.numpy()[fixed].view(np.uint64), s["K"][fixed].view(np.uint64))
    K = res.K.numpy()
    assert np.array_equal(K[:, [0, 1, 1, 2, 2, 2], [2, 0, 2, 0, 1, 2]], s["K"][:, [0, 1, 1, 2, 2, 2], [2, 0, 2, 0, 1, 2]])     # cx, cy and the rest stay


@pytest.mark.parametrize("name", ["scene_a", "scene_b"])
def test_refinement_beats_fixed_intrinsics_on_the_same_inputs(name):
    f = _figures(name)
    assert f["rms"] < f["rms_plain"] and f["rot"] < f["rot_plain"] and f["centre"] < f["centre_plain"], f


def test_accuracy_profile_is_current():
    """profiles/bundle_focal_accuracy.txt holds the figures of this build (rewritten when LOFTR_WRITE_PROFILES=1)."""
    path, text = os.path.join(ROOT, "profiles", "bundle_focal_accuracy.txt"), "\n".join(accuracy_lines()) + "\n"
    if os.environ.get("LOFTR_WRITE_PROFILES") == "1":
        with open(path, "w") as fh:
            fh.write(text)
    assert os.path.exists(path) and open(path).read().splitlines()[:3] == text.splitlines()[:3]


# ---- the cases of the rule -----------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_a_mixed_mask_returns_the_bits_of_k_for_the_cameras_left_out():
    s = FC.focal_case("scene_b")
    mask = np.zeros(12, bool)
    mask[[0, 3, 4, 7, 10]] = True                                        # 0 is fixed: its flag changes nothing
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=mask)
    want = mask & ~s["fixed"]
    assert res.cam_focal.tolist() == want.tolist() and res.stats["n_focal_cameras"] == 4 and res.status == "converged"
    K = res.K.numpy()
    assert np.array_equal(_bits(K[~want]), _bits(s["K"][~want]))
    assert (K[want, 0, 0] != s["K"][want, 0, 0]).all() and (K[want, 1, 1] != s["K"][want, 1, 1]).all()
    assert FC.focal_errors(K, s["K_true"], want) < 0.5 * FC.focal_errors(s["K"], s["K_true"], want)
    # a list and a tensor are masks too
    again = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=torch.from_numpy(mask))
    assert torch.equal(again.K, res.K) and again.stats == res.stats
    assert torch.equal(loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=mask.tolist()).K, res.K)


def test_a_fixed_camera_with_its_flag_set_does_not_refine():
    s = FC.focal_case("scene_a")
    fixed = s["fixed"].copy()
    fixed[3] = True                                                      # a detuned camera that keeps its pose keeps its K
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=fixed, refine_focal=True)
    assert res.cam_focal.tolist() == [False, False, True, False, True] == res.cam_free.tolist()
    assert np.array_equal(_bits(res.K.numpy()[fixed]), _bits(s["K"][fixed]))
    assert np.array_equal(_bits(res.T_cam_from_world.numpy()[fixed]), _bits(s["T_cam_from_world"][fixed]))


def test_min_focal_obs_at_a_cameras_count_and_one_more():
    s = FC.focal_case("scene_a")
    base = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True, max_iters=0)
    cnt = np.bincount(s["obs_image"][base.obs_active.numpy()], minlength=5)
    assert base.obs_active.all() and cnt.tolist() == [45, 44, 40, 41, 40]
    for m in (40, 41, 42):
        res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True, min_focal_obs=m)
        want = ~s["fixed"] & (cnt >= m)
        assert res.cam_focal.tolist() == want.tolist() and res.stats["n_focal_cameras"] == int(want.sum()), m
        assert res.cam_free.tolist() == (~s["fixed"]).tolist()
        assert np.array_equal(_bits(res.K.numpy()[~want]), _bits(s["K"][~want]))


def test_a_first_trial_outside_the_bounds_is_rejected_and_lambda_grows():
    """Case B needs focal steps of up to 10 %; with bounds (0.97, 1.03) the first trials leave them and are rejected like a non-finite
    value: nothing accepted, lambda x 10 per trial, the state unchanged."""
    s = FC.focal_case("scene_b")
    kw = dict(fixed=s["fixed"], refine_focal=True, focal_bounds=(0.97, 1.03))
    one = loftr_amd.bundle_adjust(*BC.inputs(s), max_iters=1, **kw)
    assert one.n_iters == 1 and one.n_accepted == 0 and one.status == "max_iters" and one.n_pcg > 0
    assert one.stats["lambda"] == 10.0 * 1e-4 and one.cost_after == one.cost_before and one.rms_px_after == one.rms_px_before
    assert np.array_equal(_bits(one.K.numpy()), _bits(s["K"])) and np.array_equal(one.xyz.numpy(), s["xyz"])
    free = loftr_amd.bundle_adjust(*BC.inputs(s), max_iters=1, **dict(kw, focal_bounds=(0.5, 2.0)))
    assert free.n_accepted == 1                                          # the same trial is accepted when the bounds admit it
    res = loftr_amd.bundle_adjust(*BC.inputs(s), max_iters=60, **kw)
    ratio = np.stack([res.K.numpy()[:, 0, 0] / s["K"][:, 0, 0], res.K.numpy()[:, 1, 1] / s["K"][:, 1, 1]])
    print(res.stats, ratio.min(), ratio.max())
    assert res.n_accepted < res.n_iters and res.status in ("converged", "stalled", "max_iters")
    assert (ratio > 0.97).all() and (ratio < 1.03).all()
    assert res.cost_after <= res.cost_before and res.stats["n_focal_cameras"] == 10


def test_huber_loss_with_the_focal():
    """The bar of tests/test_bundle.py's Huber test: final Huber cost <= 1.001 x the oracle's under the same loss, max_iters = 100."""
    s, res, plain, orc = solved("scene_huber", huber=2.0, max_iters=100)
    free = res.cam_free.numpy()
    f0, f1 = FC.focal_errors(s["K"], s["K_true"], free), FC.focal_errors(res.K.numpy(), s["K_true"], free)
    print(f"huber + focal: cost {res.cost_after:.12g} oracle {orc['cost']:.12g} ratio {res.cost_after / orc['cost']:.9f}, {res.n_iters} trials "
          f"({res.status}); focal error {f0:.4f} -> {f1:.5f}; rms {res.rms_px_after:.3f} (fixed intrinsics {plain.rms_px_after:.3f})")
    assert res.obs_active.all() and res.stats["n_focal_cameras"] == 10
    assert res.cost_after <= 1.001 * orc["cost"]
    assert f1 <= 0.5 * f0 and res.cost_after < plain.cost_after


def test_hand_written_cases_with_every_flag_set():
    s, n = BC.hand_problem()
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True, min_focal_obs=1)
    plain = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"])
    got = res.to_host()
    act, pa, free = got["obs_active"], got["point_active"], got["cam_free"]
    assert res.status == "converged" and res.cost_after < res.cost_before
    for k in ("obs_active", "point_active", "cam_free"):                 # the active set is §18's
        assert np.array_equal(got[k], getattr(plain, k).numpy()), k
    assert free.tolist() == [False, False, True, True, True, False, False, False] == got["cam_focal"].tolist()
    assert not free[n["bad_cam"]] and not act[n["bad_cam_obs"]] and got["K"][n["bad_cam"], 0, 0] == 0.0     # fx = 0 stays invalid
    assert not pa[n["nan_point"]] and not act[slice(*n["nan_obs"])].any() and not act[n["masked"]] and not pa[n["single"]]
    assert np.array_equal(_bits(got["K"][~free]), _bits(s["K"][~free]))
    assert np.array_equal(_bits(got["T_cam_from_world"][~free]), _bits(s["T_cam_from_world"][~free]))
    for t in (n["single"], n["nan_point"]):
        assert np.array_equal(got["xyz"][t].view(np.uint32), s["xyz"][t].view(np.uint32))
    assert res.stats["n_focal_cameras"] == 3 and res.stats["n_free_cameras"] == 3 and res.stats["n_active_points"] == 24


def test_a_start_at_the_optimum_runs_no_trial_and_returns_the_bits_of_k():
    s = BC.exact_problem()
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True, min_focal_obs=1)
    assert res.status == "converged" and res.n_iters == 0 and res.n_accepted == 0 and res.cost_before == res.cost_after == 0.0
    assert res.cam_focal.tolist() == [False, False, True, True] and res.stats["n_focal_cameras"] == 2
    assert np.array_equal(_bits(res.K.numpy()), _bits(s["K"])) and np.array_equal(res.T_cam_from_world.numpy(), s["T_cam_from_world"])


def test_zero_free_cameras():
    s = FC.focal_case("scene_a")
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=np.ones(5, bool), refine_focal=True)
    assert not res.cam_free.any() and not res.cam_focal.any() and res.stats["n_focal_cameras"] == 0 and res.n_pcg == 0
    assert np.array_equal(_bits(res.K.numpy()), _bits(s["K"]))
    e = lambda *shape, dt=np.float32: np.zeros(shape, dt)
    res = loftr_amd.bundle_adjust(np.zeros(1, np.int64), e(0, dt=np.int32), e(0, 2), e(0, dt=bool), e(0, 3), s["K"], s["T_cam_from_world"],
                                  refine_focal=True)
    assert res.status == "nothing_to_adjust" and not res.cam_focal.any() and np.array_equal(_bits(res.K.numpy()), _bits(s["K"]))


def test_value_errors():
    s = FC.focal_case("scene_a")
    a = BC.inputs(s)
    for kw in (dict(focal_bounds=(float("nan"), 2.0)), dict(focal_bounds=(0.5, float("inf"))), dict(focal_bounds=(1.0, 2.0)),
               dict(focal_bounds=(0.5, 1.0)), dict(focal_bounds=(1.1, 2.0)), dict(focal_bounds=(0.5, 0.9)), dict(focal_bounds=(2.0, 0.5)),
               dict(min_focal_obs=0), dict(min_focal_obs=-3), dict(min_focal_obs=2.5)):
        with pytest.raises(ValueError, match="min_focal_obs must be an integer >= 1 and the focal bounds finite"):
            loftr_amd.bundle_adjust(*a, refine_focal=True, **kw)
    with pytest.raises(ValueError, match="focal_bounds must be a pair"):
        loftr_amd.bundle_adjust(*a, refine_focal=True, focal_bounds=0.5)
    for mask in (np.ones(4, bool), np.ones(6, bool), np.ones((5, 1), bool)):
        with pytest.raises(ValueError, match=r"mask of shape \(5,\)"):
            loftr_amd.bundle_adjust(*a, refine_focal=mask)
    with pytest.raises(ValueError, match="refine_focal must be None, True or"):
        loftr_amd.bundle_adjust(*a, refine_focal=False)

    class FakeGpu(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    with pytest.raises(ValueError, match="refine_focal is on the GPU.*no silent fallback"):
        loftr_amd.bundle_adjust(*a, refine_focal=torch.ones(5, dtype=torch.bool).as_subclass(FakeGpu))
    # without the keyword the other two are not looked at: the call is the one it was
    assert loftr_amd.bundle_adjust(*a, min_focal_obs=0, focal_bounds=None, max_iters=1).n_iters == 1


# ---- the 6-wide path is the one it was -------------------------------------------------------------------------------------------------
def test_fixed_intrinsics_results_equal_the_digests_taken_before_the_template():
    spec = importlib.util.spec_from_file_location("make_bundle_parent_digest", os.path.join(GOLDEN, "make_bundle_parent_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = json.load(open(os.path.join(GOLDEN, "bundle_parent_digest.json")))
    got = mod.digests()
    assert sorted(got) == sorted(want) == ["hand_problem", "scene_a", "scene_b", "scene_huber"]
    for case in want:
        assert got[case]["inputs"] == want[case]["inputs"], f"{case}: the scene itself is not the one the digests were taken on"
        assert got[case] == want[case], case
        assert sorted(want[case]) == ["T_cam_from_world", "cam_free", "counts", "inputs", "obs_active", "point_active", "xyz"]


def test_without_the_keyword_the_result_has_the_old_fields():
    s = BC.scene_a()
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"])
    old = ("T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active")
    assert res.FIELDS == loftr_amd.BundleResult.FIELDS == old and sorted(res.to_host()) == sorted(old + ("stats",))
    assert not hasattr(res, "K") and not hasattr(res, "cam_focal") and "n_focal_cameras" not in res.stats
    with_focal = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], refine_focal=True)
    assert with_focal.FIELDS == old + ("K", "cam_focal") and sorted(with_focal.to_host()) == sorted(old + ("K", "cam_focal", "stats"))
    assert with_focal.K.dtype == torch.float64 and tuple(with_focal.K.shape) == (5, 3, 3) and with_focal.cam_focal.dtype == torch.bool
    assert set(with_focal.stats) == set(res.stats) | {"n_focal_cameras"}


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------
def _relative(T, a, b):
    R = T[b, :3, :3] @ T[a, :3, :3].T
    return R, T[b, :3, 3] - R @ T[a, :3, 3]


def chain_runs(device="cpu"):
    """reconstruct_tracks on detuned scene B from the true relative pose of images 0 and 1, with and without the focal."""
    s = FC.focal_case("scene_b")
    R, t = _relative(s["T_true"], 0, 1)
    a = [torch.from_numpy(np.ascontiguousarray(s[k])).to(device) for k in ("offsets", "obs_image", "obs_xy", "K")]
    kw = dict(min_corr=6, min_inliers=6)
    return s, loftr_amd.reconstruct_tracks(*a, (0, 1, R, t), ba={"refine_focal": True}, **kw), loftr_amd.reconstruct_tracks(*a, (0, 1, R, t), **kw)


def test_reconstruct_tracks_with_refined_focals():
    s, rec, plain = chain_runs()
    every = np.ones(12, bool)
    f0, f1 = FC.focal_errors(s["K"], s["K_true"], every), FC.focal_errors(rec.K.numpy(), s["K_true"], every)
    print(f"chain: posed {rec.stats['n_posed']} (fixed intrinsics {plain.stats['n_posed']}), rms {rec.bundle.rms_px_after:.4f} px (fixed intrinsics "
          f"{plain.bundle.rms_px_after:.4f}), focal error {f0:.4f} -> {f1:.4f}, rounds {rec.stats['n_rounds']}")
    assert rec.posed.all() and rec.stats["n_posed"] == 12
    assert rec.bundle.rms_px_after < plain.bundle.rms_px_after
    assert f1 < f0
    assert torch.equal(rec.K, rec.bundle.K) and np.array_equal(_bits(rec.K.numpy()[0]), _bits(s["K"][0]))    # image 0 is the fixed one
    assert torch.equal(plain.K, torch.from_numpy(s["K"])) and not hasattr(plain.bundle, "K")              # without the keyword nothing changes
