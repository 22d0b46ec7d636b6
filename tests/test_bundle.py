"""Bundle adjustment on the CPU: the host routine loftr_bundle_adjust_host, which DEFINES the result, against an independent
numpy oracle (tests/_bundle_oracle.py: dense Jacobian, dense normal equations), against ground truth, under the Huber loss, on the
hand-written cases, through the atlas -> triangulate -> adjust -> triangulate chain, and its ordered sums restated in numpy."""
import functools

import numpy as np
import pytest
import torch

import _bundle_cases as BC
import _bundle_oracle as O
import _model_lookup_cases as MC
import _triangulation_cases as TC
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


@functools.lru_cache(maxsize=None)
def solved(name, huber=0.0, max_iters=30):
    """(scene, library result as a host dict, oracle result) of scene `name` under the same loss, computed once."""
    s = getattr(BC, name)()
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], huber_px=huber, max_iters=max_iters)
    got = dict(res.to_host(), res=res)
    orc = O.adjust(s["offsets"], s["obs_image"], s["obs_xy"], s["obs_mask"], s["xyz"], s["K"], s["T_cam_from_world"], s["fixed"], huber=huber)
    return s, got, orc


@pytest.mark.parametrize("name", ["scene_a", "scene_b"])
def test_optimum_equals_the_dense_oracle(lib, name):
    """Final cost <= 1.0001 x the oracle's and projections within 0.01 px of the oracle's over the active observations.  Measured
    (profiles/bundle_accuracy.txt): cost ratios 1 +- 1e-14, projection differences 2.2e-5 px (the float32 rounding of the points)."""
    s, got, orc = solved(name)
    st = got["stats"]
    assert st["status"] == "converged" and got["obs_active"].all() and got["point_active"].all()
    assert got["cam_free"].tolist() == (~s["fixed"]).tolist()
    diff = np.abs(BC.projections(s, got["T_cam_from_world"], got["xyz"], got["obs_active"]) -
                  BC.projections(s, orc["T"], orc["xyz"], got["obs_active"])).max()
    print(f"{name}: cost {st['cost_after']:.12g} oracle {orc['cost']:.12g} ratio {st['cost_after'] / orc['cost']:.15f} projection diff {diff:.3g} px, "
          f"{st['n_iters']} trials, {st['n_pcg']} pcg iterations")
    assert st["cost_after"] <= 1.0001 * orc["cost"]
    assert diff <= 0.01
    assert st["cost_after"] < st["cost_before"] and st["rms_px_after"] < st["rms_px_before"]
    assert abs(st["rms_px_after"] - np.sqrt(st["cost_after"] / st["n_active_observations"])) <= 1e-12        # squared loss: the same sum


@pytest.mark.parametrize("name", ["scene_a", "scene_b"])
def test_free_cameras_move_towards_the_truth(lib, name):
    s, got, orc = solved(name)
    free = got["cam_free"]
    r0, c0 = BC.pose_errors(s["T_cam_from_world"], s["T_true"], free)
    r1, c1 = BC.pose_errors(got["T_cam_from_world"], s["T_true"], free)
    ro, co = BC.pose_errors(orc["T"], s["T_true"], free)
    print(f"{name}: rotation {r0:.4f} -> {r1:.4f} deg (oracle {ro:.4f}), centre {c0:.4f} -> {c1:.4f} (oracle {co:.4f})")
    assert r1 <= 0.5 * r0 and c1 <= 0.5 * c0
    assert r1 <= 1.01 * ro and c1 <= 1.01 * co
    fixed = s["fixed"]
    assert np.array_equal(got["T_cam_from_world"][fixed].view(np.uint64), s["T_cam_from_world"][fixed].view(np.uint64))


HUBER_ITERS = 100


def test_huber_loss_against_the_oracle_and_the_squared_loss(lib):
    """Final Huber cost <= 1.001 x the oracle's under the same loss; pose errors below those of the squared loss on the same data.
    Measured (profiles/bundle_accuracy.txt) with max_iters = 100."""
    s, got, orc = solved("scene_huber", huber=2.0, max_iters=HUBER_ITERS)
    _, plain, _ = solved("scene_huber", huber=0.0)
    st = got["stats"]
    ratio = st["cost_after"] / orc["cost"]
    free = got["cam_free"]
    rh, ch = BC.pose_errors(got["T_cam_from_world"], s["T_true"], free)
    rp, cp = BC.pose_errors(plain["T_cam_from_world"], s["T_true"], free)
    print(f"huber: cost {st['cost_after']:.12g} oracle {orc['cost']:.12g} ratio {ratio:.9f}, {st['n_iters']} trials ({st['status']}); "
          f"rotation {rh:.4f} deg against {rp:.4f}, centre {ch:.4f} against {cp:.4f}")
    assert got["obs_active"].all()
    assert ratio <= 1.001
    assert rh < rp and ch < cp


def test_hand_written_cases_in_one_call(lib):
    s, n = BC.hand_problem()
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"])
    got = res.to_host()
    act, pa, free = got["obs_active"], got["point_active"], got["cam_free"]
    assert res.status == "converged" and res.cost_after < res.cost_before
    assert not act[n["masked"]] and pa[20] and act[s["offsets"][20]:s["offsets"][20] + 2].all()          # a masked-out observation
    assert not pa[n["single"]] and not act[slice(*n["single_obs"])].any()                                # one active observation left
    assert not pa[n["nan_point"]] and not act[slice(*n["nan_obs"])].any()                                # a NaN point
    assert not act[n["bad_cam_obs"]] and pa[23] and not free[n["bad_cam"]]                               # fx = 0
    assert not free[n["empty_cam"]]                                                                      # no observation
    assert not act[n["behind_obs"]] and pa[24] and not free[n["behind_cam"]]                             # behind its camera at the start
    assert free.tolist() == [False, False, True, True, True, False, False, False]
    for t in (n["single"], n["nan_point"]):                                                              # input bits back
        assert np.array_equal(got["xyz"][t].view(np.uint32), s["xyz"][t].view(np.uint32))
    assert np.array_equal(got["T_cam_from_world"][~free].view(np.uint64), s["T_cam_from_world"][~free].view(np.uint64))
    assert res.stats["n_active_observations"] == int(act.sum()) and res.stats["n_active_points"] == int(pa.sum()) == 24
    assert res.stats["n_free_cameras"] == 3
    r0, c0 = BC.pose_errors(s["T_cam_from_world"], s["T_true"], free)
    r1, c1 = BC.pose_errors(got["T_cam_from_world"], s["T_true"], free)
    assert r1 < 0.5 * r0 and c1 < 0.5 * c0
    R = got["T_cam_from_world"][free][:, :3, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14 and (got["T_cam_from_world"][free][:, 3] == [0, 0, 0, 1]).all()


def test_every_camera_fixed_moves_only_the_points(lib):
    s = BC.scene_a()
    args = BC.inputs(s)
    args[6] = s["T_true"]
    res = loftr_amd.bundle_adjust(*args, fixed=np.ones(5, bool))
    got = res.to_host()
    assert not got["cam_free"].any() and res.n_pcg == 0 and res.status == "converged" and res.stats["n_free_cameras"] == 0
    assert np.array_equal(got["T_cam_from_world"].view(np.uint64), s["T_true"].view(np.uint64))
    before, after = np.abs(s["xyz"] - s["X_true"]).max(), np.abs(got["xyz"] - s["X_true"]).max()
    assert after < 0.5 * before and res.cost_after < 0.01 * res.cost_before
    # fixed=None fixes image 0 only
    res0 = loftr_amd.bundle_adjust(*BC.inputs(s))
    assert res0.cam_free.tolist() == [False, True, True, True, True]


def test_a_start_at_the_optimum_converges_at_once(lib):
    s = BC.exact_problem()
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"])
    assert res.status == "converged" and res.n_accepted <= 1 and res.n_iters <= 1, res.stats
    assert res.cost_before == res.cost_after == 0.0 and res.rms_px_after == 0.0 and res.cam_free.tolist() == [False, False, True, True]
    assert np.array_equal(res.xyz.numpy(), s["xyz"]) and np.array_equal(res.T_cam_from_world.numpy(), s["T_cam_from_world"])


def test_no_track_no_observation_nothing_to_adjust(lib):
    s = BC.scene_a()
    e = lambda *shape, dt=np.float32: np.zeros(shape, dt)
    res = loftr_amd.bundle_adjust(np.zeros(1, np.int64), e(0, dt=np.int32), e(0, 2), e(0, dt=bool), e(0, 3), s["K"], s["T_cam_from_world"])
    assert res.status == "nothing_to_adjust" and res.n_iters == 0 and res.cost_after == 0.0 and res.rms_px_after == 0.0
    assert np.array_equal(res.T_cam_from_world.numpy(), s["T_cam_from_world"]) and res.xyz.shape == (0, 3) and not res.cam_free.any()
    res = loftr_amd.bundle_adjust(np.zeros(4, np.int64), e(0, dt=np.int32), e(0, 2), e(0, dt=bool), s["xyz"][:3], s["K"], s["T_cam_from_world"])
    assert res.status == "nothing_to_adjust" and not res.point_active.any() and np.array_equal(res.xyz.numpy(), s["xyz"][:3])
    masked = BC.inputs(s)
    masked[3] = np.zeros_like(s["obs_mask"])
    res = loftr_amd.bundle_adjust(*masked)
    assert res.status == "nothing_to_adjust" and not res.obs_active.any()
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], max_iters=0)
    assert res.status == "max_iters" and res.n_iters == 0 and res.cost_after == res.cost_before
    assert np.array_equal(res.xyz.numpy(), s["xyz"])


def _raw(s, **over):
    """The ops-level arguments of scene s (with the grouping by image), entries replaced by `over`."""
    a = [np.ascontiguousarray(s[k]) for k in BC.ARGS]
    a[3] = a[3].astype(np.uint8)
    n = len(s["K"])
    cam_obs = np.argsort(a[1], kind="stable").astype(np.int32)
    cam_offsets = np.zeros(n + 1, np.int64)
    cam_offsets[1:] = np.cumsum(np.bincount(a[1], minlength=n))
    d = dict(zip(BC.ARGS, a), fixed=s["fixed"].astype(np.uint8), cam_offsets=cam_offsets, cam_obs=cam_obs)
    d.update(over)
    return list(d.values())


def test_every_error_bit(lib):
    s = BC.scene_a()
    par = (0.0, 5, 10, 1e-2, 1e-9)
    assert ops.bundle_adjust_host(*_raw(s), *par)["counts"][0] in (0, 1)
    N = len(s["obs_image"])
    im = s["obs_image"].copy(); im[7] = 5
    off = s["offsets"].copy(); off[3] = off[2] - 1
    for k, bad in (("obs_image", im), ("offsets", off), ("offsets", np.r_[1, s["offsets"][1:]]), ("offsets", np.r_[s["offsets"][:-1], N - 1])):
        with pytest.raises(ValueError, match="obs_image outside|offsets must"):
            loftr_amd.bundle_adjust(*[bad if n == k else s[n] for n in BC.ARGS])
        with pytest.raises(_lib.LoftrHipError, match="status -1"):
            ops.bundle_adjust_host(*_raw(s, **{k: bad}), *par)
    good = _raw(s)
    swapped = good[9].copy(); swapped[[0, 1]] = swapped[[1, 0]]                       # descending within an image
    foreign = good[9].copy(); foreign[0] = good[9][-1]                                # an observation of another image
    outside = good[9].copy(); outside[3] = N
    short = good[8].copy(); short[1] -= 1                                             # a boundary one too early
    late = good[8].copy(); late[-1] = N + 1
    for k, bad in (("cam_obs", swapped), ("cam_obs", foreign), ("cam_obs", outside), ("cam_offsets", short), ("cam_offsets", late)):
        with pytest.raises(_lib.LoftrHipError, match="status -1"):
            ops.bundle_adjust_host(*_raw(s, **{k: bad}), *par)


def test_guards_of_the_parameters(lib):
    s = BC.scene_a()
    for kw in (dict(huber_px=-1.0), dict(huber_px=float("nan")), dict(huber_px=float("inf")), dict(max_iters=-1), dict(max_iters=1001),
               dict(max_iters=2.5), dict(pcg_iters=0), dict(pcg_iters=201), dict(pcg_tol=-0.1), dict(pcg_tol=1.0), dict(pcg_tol=float("nan")),
               dict(ftol=-1e-9), dict(ftol=float("inf"))):
        with pytest.raises(ValueError, match="huber_px and ftol must be"):
            loftr_amd.bundle_adjust(*BC.inputs(s), **kw)
    with pytest.raises(ValueError, match="must hold integers"):
        loftr_amd.bundle_adjust(s["offsets"].astype(np.float64), *BC.inputs(s)[1:])
    res = loftr_amd.bundle_adjust(*[torch.from_numpy(np.ascontiguousarray(a)) for a in BC.inputs(s)], fixed=torch.from_numpy(s["fixed"]), max_iters=2)
    assert res.n_iters == 2 and res.status == "max_iters" and isinstance(res.xyz, torch.Tensor)


# ---- the ordered sums, restated ----------------------------------------------------------------------------------------------------------
def osum64(v):
    a = np.zeros(64)
    for i, x in enumerate(v):
        a[i % 64] = a[i % 64] + x
    s = 32
    while s >= 1:
        a[:s] = a[:s] + a[s:2 * s]
        s //= 2
    return a[0]


def osum(v):
    while True:
        sums = [osum64(v[i:i + 4096]) for i in range(0, max(len(v), 1), 4096)]
        if len(sums) == 1:
            return sums[0]
        v = sums


@pytest.mark.parametrize("length", [0, 1, 63, 64, 65, 4096, 4097])
def test_osum_restated_in_numpy_equals_the_librarys(lib, length):
    """One fixed camera with the identity pose and `length` tracks of two observations each: cost_before is osum over the tracks of
    (rho_1 + rho_2), and every rho can be restated in numpy with the rule's operation order (R = I: P = X exactly)."""
    rng = np.random.default_rng(length)
    fx, fy, sk, cx, cy = 500.0, 510.0, 0.5, 320.0, 240.0
    K = np.array([[[fx, sk, cx], [0, fy, cy], [0, 0, 1]]])
    X = rng.uniform([-1, -1, 3], [1, 1, 6], (length, 3)).astype(np.float32)
    xy = rng.uniform(0, 600, (2 * length, 2)).astype(np.float32)
    res = loftr_amd.bundle_adjust(2 * np.arange(length + 1, dtype=np.int64), np.zeros(2 * length, np.int32), xy, np.ones(2 * length, bool), X, K,
                                  np.eye(4)[None], max_iters=0)
    Xd, o = np.repeat(X.astype(np.float64), 2, axis=0), xy.astype(np.float64)
    a, b = Xd[:, 0] / Xd[:, 2], Xd[:, 1] / Xd[:, 2]
    ru, rv = ((fx * a + sk * b) + cx) - o[:, 0], (fy * b + cy) - o[:, 1]
    rho = ru * ru + rv * rv
    per_track = rho[0::2] + rho[1::2]                                     # 0.0 + rho_1 + rho_2, sequentially
    want = osum(list(per_track))
    assert res.stats["n_active_observations"] == 2 * length
    assert np.float64(res.cost_before).tobytes() == np.float64(want).tobytes(), (res.cost_before, want)


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------
def chain(device):
    """sfm_scene() through the atlas, triangulated with scene_a's perturbed poses, adjusted, triangulated again."""
    s, a = TC.sfm_scene(), BC.scene_a()
    sfm = TC.run_atlas(device)
    pts1 = sfm.triangulate(s["K"], a["T_cam_from_world"])
    res = sfm.adjust(pts1, s["K"], a["T_cam_from_world"], fixed=a["fixed"])
    pts2 = sfm.triangulate(s["K"], res.T_cam_from_world)
    return sfm, pts1, res, pts2


def median_centre_error(sfm, pts):
    from loftr_amd import LocalizationModel
    from loftr_amd.evaluation import absolute_pose_error
    qs = MC.query_scene()
    out = MC.localize_scene(LocalizationModel.from_atlas(sfm, pts)).solve(qs["K"], thresh_px=3.0, conf=0.999, seed=0)
    return float(np.median([absolute_pose_error(qs["T"][q], out.R[q].cpu().numpy(), out.t[q].cpu().numpy())[1] for q in range(MC.N_QUERIES)]))


def test_chain_atlas_triangulate_adjust_triangulate_localize(lib):
    sfm, pts1, res, pts2 = chain("cpu")
    n1, n2 = pts1.stats["n_inlier_observations"], pts2.stats["n_inlier_observations"]
    e1, e2 = median_centre_error(sfm, pts1), median_centre_error(sfm, pts2)
    print(f"chain: inlier observations {n1} -> {n2}, ok tracks {pts1.stats['n_ok']} -> {pts2.stats['n_ok']}, rms {res.rms_px_before:.3f} -> "
          f"{res.rms_px_after:.3f} px, median query centre error {e1:.5f} -> {e2:.5f}")
    assert res.status in ("converged", "max_iters") and res.cost_after < res.cost_before
    assert torch.equal(res.obs_active, pts1.obs_inlier)                  # what the triangulation kept is what is adjusted
    assert n2 >= n1
    assert e2 <= e1
    K, T = TC.sfm_scene()["K"], TC.sfm_scene()["T"]
    loose = loftr_amd.triangulate_tracks(pts1.offsets, pts1.image.to(torch.int32), torch.zeros(pts1.image.numel(), 2), K, T)
    with pytest.raises(ValueError, match="carries no tracks"):
        sfm.adjust(loose, K, T)
