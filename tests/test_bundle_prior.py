"""Bundle adjustment with position priors on the camera centres, on the CPU: the host routine
loftr_bundle_adjust_prior_host, which DEFINES the result, against the dense oracle with prior rows (tests/_bundle_prior_oracle.py) in the
three modes, on the scaled scene the feature exists for, against the calls without priors (an all-zero mask is those calls bit for
bit), on a hand-written problem, on the ways a prior is switched off, its ordered sum restated in numpy, the Python errors and the
align -> adjust -> triangulate chain of Reconstruction.align(refine=...)."""
import functools
import os

import numpy as np
import pytest
import torch

import _bundle_cases as BC
import _bundle_oracle as O
import _bundle_prior_cases as PC
import _bundle_prior_oracle as PO
import _bundle_shared_oracle as SO
import _triangulation_cases as TC
import loftr_amd
from loftr_amd import _lib, build as build_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def oracle_kwargs(name, s):
    """What selects the oracle's problem for case `name`: every image is flagged, so the focal case refines every free camera and the
    shared case every carrying member (default min_focal_obs = 20)."""
    every = np.ones(len(s["K"]), bool)
    if name == "focal":
        return dict(refine=every)
    if name == "shared":
        group = np.unique(s["camera_ids"], return_inverse=True)[1]
        return dict(focal=SO.carrying(s["obs_image"], s["obs_mask"], s["K"], s["T_cam_from_world"], every, group, 20), group=group)
    return {}


@functools.lru_cache(maxsize=None)
def solved(name):
    """(scene, library result as a host dict, oracle result) of prior case `name`, computed once."""
    s = PC.prior_case(name)
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], **PC.mode_kwargs(name, s), **PC.prior_kwargs(s))
    orc = PO.adjust(s["offsets"], s["obs_image"], s["obs_xy"], s["obs_mask"], s["xyz"], s["K"], s["T_cam_from_world"], s["fixed"], s["prior_xyz"],
                    s["prior_sigma"], s["prior_mask"], **oracle_kwargs(name, s))
    return s, dict(res.to_host(), res=res), orc


@pytest.mark.parametrize("name", ["scene_a", "scene_b", "focal", "shared"])
def test_optimum_equals_the_dense_oracle_with_prior_rows(lib, name):
    """No camera fixed, priors at truth + N(0, 0.02) on every camera.  Final cost <= 1.0001 x the oracle's, projections within 0.01 px of
    the oracle's, largest and rms centre error against the truth <= 1.01 x the oracle's: the bars of tests/test_bundle.py.  Measured
    (profiles/bundle_prior_accuracy.txt): cost ratios 1 + 1e-9 at most, projection differences 4e-5 px, centre-error ratios 1 +- 1e-4."""
    s, got, orc = solved(name)
    st = got["stats"]
    n = len(s["K"])
    assert st["status"] == "converged" and got["obs_active"].all() and got["cam_free"].all() and got["cam_prior"].all()
    assert st["n_prior_cameras"] == n and got["res"].FIELDS[-1] == "cam_prior"
    Kg = got["K"] if "K" in got else s["K"]
    diff = np.abs(BC.projections(dict(s, K=Kg), got["T_cam_from_world"], got["xyz"], got["obs_active"]) -
                  BC.projections(dict(s, K=orc["K"]), orc["T"], orc["xyz"], got["obs_active"])).max()
    c1, co = PC.centre_max(got["T_cam_from_world"], s["T_true"]), PC.centre_max(orc["T"], s["T_true"])
    r1, ro = PC.centre_rms(got["T_cam_from_world"], s["T_true"]), PC.centre_rms(orc["T"], s["T_true"])
    print(f"{name}: cost {st['cost_after']:.12g} oracle {orc['cost']:.12g} ratio {st['cost_after'] / orc['cost']:.15f} projection diff {diff:.3g} px, "
          f"centre max {c1:.6g} (oracle {co:.6g}) rms {r1:.6g} (oracle {ro:.6g}), prior cost {st['prior_cost_before']:.6g} -> "
          f"{st['prior_cost_after']:.6g} (oracle {orc['prior_cost']:.6g}), prior rms {st['prior_rms_before']:.6g} -> {st['prior_rms_after']:.6g}, "
          f"{st['n_iters']} trials, {st['n_pcg']} pcg iterations")
    assert st["cost_after"] <= 1.0001 * orc["cost"]
    assert diff <= 0.01
    assert c1 <= 1.01 * co and r1 <= 1.01 * ro
    assert st["cost_after"] < st["cost_before"] and st["prior_cost_after"] < st["prior_cost_before"] and st["prior_rms_after"] < st["prior_rms_before"]
    # the report's figures, restated: the prior cost in sigma^2 and the rms distance from the priors in world units
    d = PC.centres(got["T_cam_from_world"]) - s["prior_xyz"]
    assert abs(st["prior_rms_after"] - np.sqrt((d * d).sum() / n)) <= 1e-12
    assert abs(st["prior_cost_after"] - (d * d).sum() / s["prior_sigma"] ** 2) <= 1e-9 * st["prior_cost_after"]
    # rms_px stays over the observations only
    assert abs(st["rms_px_after"] - np.sqrt((st["cost_after"] - st["prior_cost_after"]) / st["n_active_observations"])) <= 1e-9


def test_priors_remove_a_scale_error_that_reprojection_cannot_see(lib):
    """The case the feature exists for: scene B (generator seed 13) with poses and points shrunk by 0.95 about their joint centroid --
    a gauge freedom of the reprojection error -- plus the usual perturbation, no camera fixed.  Without priors the rms centre error
    against the truth stays >= 0.9 x its start; with priors at sigma = the position noise (0.02) it falls to <= 0.5 x its start and to
    <= 1.01 x the oracle's.  The oracle alone meets both bars on this seed (checked first).  Measured
    (profiles/bundle_prior_accuracy.txt): start 0.2741, without priors 0.2719 (oracle without priors 0.2588), with priors 0.0110845
    (oracle 0.0110846).  Without priors what is left of the gauge wanders with the damping: over the generator seeds 12..19 the ratio
    to the start was 0.894, 0.992, 1.058, 0.921, 0.949, 1.099, 0.974, 0.960 for the library and 0.935..1.025 for the oracle, so the
    0.9 bar has little room on any seed and seed 12 (scene B's default) misses it by 0.006; 13 is the next."""
    s, got, orc = solved("scaled")
    start = PC.centre_rms(s["T_cam_from_world"], s["T_true"])
    plain_orc = O.adjust(s["offsets"], s["obs_image"], s["obs_xy"], s["obs_mask"], s["xyz"], s["K"], s["T_cam_from_world"], s["fixed"])
    eo, eo_plain = PC.centre_rms(orc["T"], s["T_true"]), PC.centre_rms(plain_orc["T"], s["T_true"])
    assert eo_plain >= 0.9 * start and eo <= 0.5 * start                 # the oracle alone meets both bars
    plain = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"])
    e_plain, e = PC.centre_rms(plain.T_cam_from_world.numpy(), s["T_true"]), PC.centre_rms(got["T_cam_from_world"], s["T_true"])
    st = got["stats"]
    lines = ["Bundle adjustment with position priors (DESIGN 18.3) on tests/_bundle_prior_cases.py prior_case('scaled'): scene B (generator seed 13,",
             "12 cameras, 200 points) shrunk by 0.95 about the joint centroid of centres and points, the usual perturbation, no camera fixed;",
             f"priors = true centres + N(0, {PC.SIGMA}) per axis at sigma = {PC.SIGMA}.  rms centre error against the truth over the 12 cameras:",
             f"start {start:.6g}",
             f"without priors: library {e_plain:.6g} ({e_plain / start:.4f} x start; {plain.status}, {plain.n_iters} trials), oracle {eo_plain:.6g} "
             f"({eo_plain / start:.4f} x start)",
             f"with priors: library {e:.6g} ({e / start:.4f} x start; {st['status']}, {st['n_iters']} trials, {st['n_pcg']} pcg iterations), oracle "
             f"{eo:.6g} (ratio {e / eo:.6f})",
             f"cost {st['cost_before']:.8g} -> {st['cost_after']:.8g} (oracle {orc['cost']:.8g}); prior cost {st['prior_cost_before']:.6g} -> "
             f"{st['prior_cost_after']:.6g} sigma^2; rms |c - g| {st['prior_rms_before']:.6g} -> {st['prior_rms_after']:.6g}; rms_px "
             f"{st['rms_px_before']:.6g} -> {st['rms_px_after']:.6g}"]
    report = "\n".join(lines)
    print(report)
    if os.environ.get("LOFTR_WRITE_PROFILES"):
        with open(os.path.join(ROOT, "profiles", "bundle_prior_accuracy.txt"), "w") as fh:
            fh.write(report + "\n")
    assert e_plain >= 0.9 * start, report
    assert e <= 0.5 * start and e <= 1.01 * eo, report
    assert st["cost_after"] <= 1.0001 * orc["cost"], report


def _bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype.is_floating_point:
        view = torch.int64 if a.element_size() == 8 else torch.int32
        a, b = a.view(view), b.view(view)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("name", ["scene_b", "focal", "shared"])
def test_an_all_zero_mask_is_the_call_without_priors_bit_for_bit(lib, name):
    """Every shared tensor and counts[0:16] (through the ops layer, which returns the counts as they are)."""
    s = PC.prior_case(name)
    s = dict(s, fixed=BC.scene_b()["fixed"]) if name != "focal" else dict(s, fixed=BC.scene_a()["fixed"])
    kw = PC.mode_kwargs(name, s)
    zero = np.zeros(len(s["K"]), bool)
    for huber in (0.0, 2.0):
        want = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], huber_px=huber, **kw)
        got = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], huber_px=huber, position_prior=s["prior_xyz"], prior_sigma=0.02, prior_mask=zero, **kw)
        assert got.FIELDS == want.FIELDS + ("cam_prior",) and not got.cam_prior.any()
        for k in want.FIELDS:
            assert _bits_equal(getattr(got, k), getattr(want, k)), (name, huber, k)
        for k, v in want.stats.items():
            assert np.array_equal(np.float64(got.stats[k]).view(np.uint64), np.float64(v).view(np.uint64)) if isinstance(v, float) else got.stats[k] == v, k
        assert got.stats["n_prior_cameras"] == 0 and got.stats["prior_cost_before"] == 0.0 and got.stats["prior_rms_after"] == 0.0


def test_counts_of_an_all_zero_mask_through_the_ops_layer(lib):
    from loftr_amd import _tracks, ops
    s = PC.prior_case("shared")
    n = len(s["K"])
    base = [np.ascontiguousarray(s["offsets"], np.int64), s["obs_image"], s["obs_xy"], s["obs_mask"].astype(np.uint8), s["xyz"], s["K"],
            s["T_cam_from_world"], BC.scene_b()["fixed"].astype(np.uint8), *_tracks.group_by_image(s["obs_image"], n)]
    ones, groups = np.ones(n, np.uint8), _tracks.group_by_camera(s["camera_ids"])
    prior = (s["prior_xyz"], np.full((n, 3), 0.02), np.zeros(n, np.uint8))
    params, focal = (0.0, 30, 30, 1e-2, 1e-9), (20, 0.5, 2.0)
    for mode, want in ((0, ops.bundle_adjust_host(*base, *params)), (1, ops.bundle_adjust_focal_host(*base, ones, *params, *focal)),
                       (2, ops.bundle_adjust_shared_host(*base, ones, *groups, *params, *focal))):
        got = ops.bundle_adjust_prior_host(mode, *base, ones if mode else None, *(groups if mode == 2 else (None,) * 3), *prior, *params, *focal)
        assert got["counts"].shape == (24,) and want["counts"].shape == (16,)
        assert np.array_equal(got["counts"][:16], want["counts"]) and not got["counts"][16:].any(), mode
        assert sorted(got) == sorted(list(want) + ["cam_prior"])
        for k in set(want) - {"counts"}:
            assert got[k].tobytes() == want[k].tobytes(), (mode, k)


def _digest_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_bundle_prior_parent_digest", os.path.join(ROOT, "tests", "golden", "make_bundle_prior_parent_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("case", sorted(_digest_module().CASES))
def test_the_prior_host_routine_equals_the_digest_taken_on_the_commit_before_the_modes_became_traits(lib, case):
    """loftr_bundle_adjust_prior_host in modes 0, 1 and 2 through this build: every output tensor and the 24 counts, bit for bit what
    the commit before the mode refactor returned (tests/golden/make_bundle_prior_parent_digest.py)."""
    import json
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "bundle_prior_parent_digest.json")))
    got = _digest_module().digests(only=[case])
    assert len(want) == 18 and sorted(got) == [case] and len(want[case]) == 8 + (2 if "K" in want[case] else 0) + ("group_focal" in want[case])
    assert got[case] == want[case]


def test_one_prior_moves_a_camera_along_the_free_scale(lib):
    """Two cameras with exact observations of 24 grid points: camera 0 fixed at the origin, camera 1 free at (1, 0, 0).  The start is an
    optimum of the reprojection error with a cost of exactly 0, and the only direction the observations leave free is the scale about
    camera 0.  One prior puts camera 1 at (1.25, 0.3, 0) with sigma (0.01, 1e6, 1e6): only its x holds, so the optimum is the start
    scaled by 1.25 -- centre (1.25, 0, 0), every point times 1.25, reprojection error 0."""
    cams = [TC.camera(500, (0, 0, 0)), TC.camera(500, (1, 0, 0))]
    K, T = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    X = np.array([(x, y, z) for z in (4.0, 8.0) for x in (-0.5, 0.0, 0.5, 1.0) for y in (-0.25, 0.0, 0.25)])
    s = BC.perturbed(np.random.default_rng(0), K, T, X, [[0, 1]] * len(X), noise_px=0.0, rot_deg=0.0, centre_sigma=0.0, point_sigma=0.0, n_fixed=1)
    prior = np.array([[0.0, 0, 0], [1.25, 0.3, 0.0]])
    sigma = np.array([[1.0, 1, 1], [0.01, 1e6, 1e6]])
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=s["fixed"], position_prior=prior, prior_sigma=sigma, max_iters=100)
    c = PC.centres(res.T_cam_from_world.numpy())
    print(f"hand: {res.status} after {res.n_iters} trials, centre {c[1]}, cost {res.cost_before:.6g} -> {res.cost_after:.3g}, rms_px {res.rms_px_after:.3g}")
    assert res.cam_prior.tolist() == [False, True] and res.stats["n_prior_cameras"] == 1                 # camera 0 is fixed: no prior
    assert res.stats["prior_cost_before"] == res.cost_before and abs(res.cost_before - (25.0 ** 2 + 0.3e-6 ** 2)) <= 1e-9 * 625
    assert res.cost_after <= 1e-6 * res.cost_before
    # at a total cost of 1e-6 x 625 the prior alone bounds |c_x - 1.25| by 0.01 sqrt(6.25e-4) = 2.5e-4; y and z are held by the observations
    assert abs(c[1, 0] - 1.25) <= 2.5e-4 and np.abs(c[1, 1:]).max() <= 1e-3 * 0.25
    assert np.abs(res.xyz.numpy()[:, 2] / X[:, 2] - 1.25).max() <= 1e-3 and res.rms_px_after <= 0.05
    assert np.array_equal(res.T_cam_from_world.numpy()[0].view(np.uint64), T[0].view(np.uint64))


def test_what_switches_a_prior_off(lib):
    s = PC.prior_case("scene_b")
    n = len(s["K"])
    prior, sigma, mask, fixed = s["prior_xyz"].copy(), np.full((n, 3), 0.02), np.ones(n, bool), np.zeros(n, bool)
    prior[0, 1] = np.nan
    sigma[1, 2], sigma[2, 0], sigma[3, 1], sigma[4, 0] = 0.0, -0.02, np.inf, np.nan
    fixed[5] = True
    mask[6] = False
    prior[7, 0] = np.inf
    want = np.array([False] * 8 + [True] * (n - 8))
    res = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=fixed, position_prior=prior, prior_sigma=sigma, prior_mask=mask)
    assert res.cam_prior.tolist() == want.tolist() and res.stats["n_prior_cameras"] == n - 8
    assert res.cam_free.tolist() == (~fixed).tolist() and res.status == "converged"
    # the default mask is the finite rows; a per-camera sigma [n]
    res2 = loftr_amd.bundle_adjust(*BC.inputs(s), fixed=fixed, position_prior=prior, prior_sigma=np.full(n, 0.02))
    assert res2.cam_prior.tolist() == [False] + [True] * 4 + [False, True, False] + [True] * (n - 8)
    # a camera without an active observation is not free: no prior either
    m = s["obs_mask"] & (s["obs_image"] != 9)
    res3 = loftr_amd.bundle_adjust(s["offsets"], s["obs_image"], s["obs_xy"], m, *BC.inputs(s)[4:], fixed=fixed, position_prior=s["prior_xyz"], prior_sigma=0.02)
    assert not res3.cam_free[9] and not res3.cam_prior[9] and res3.stats["n_prior_cameras"] == n - 2


# ---- the ordered sum over the cameras, restated ------------------------------------------------------------------------------------------
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


def sum_problem(count, seed):
    """Camera 0 fixed, then `count` free cameras with a prior, all with the identity rotation (R(q) = I exactly, so c = -t exactly), two
    tracks seen by every camera.  -> (arguments, prior, sigma, per-camera shares (e0^2 + e1^2) + e2^2 and (d0^2 + d1^2) + d2^2)."""
    rng = np.random.default_rng(seed)
    n = count + 1
    K = np.tile(np.array([[500.0, 0.5, 320.0], [0, 510.0, 240.0], [0, 0, 1]]), (n, 1, 1))
    T = np.tile(np.eye(4), (n, 1, 1))
    T[1:, :3, 3] = rng.uniform(-0.5, 0.5, (count, 3))
    X = np.array([[0.3, -0.2, 5.0], [-0.4, 0.1, 6.0]], np.float32)
    image = np.tile(np.arange(n, dtype=np.int32), 2)
    xy = rng.uniform(0, 600, (2 * n, 2)).astype(np.float32)
    prior, sigma = rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(0.01, 0.1, (n, 3))
    d = -T[:, :3, 3] - prior
    e = d / sigma
    share, sq = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2], (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    share[0] = sq[0] = 0.0                                               # camera 0 is fixed: +0
    return (np.array([0, n, 2 * n], np.int64), image, xy, np.ones(2 * n, bool), X, K, T), prior, sigma, share, sq


@pytest.mark.parametrize("count", [1, 63, 64, 65, 4096, 4097])
def test_camera_osum_restated_in_numpy_equals_the_librarys(lib, count):
    """prior_cost_before is osum over the cameras of their shares, cost_before the tracks' osum plus it (one addition, tracks first),
    prior_rms_before the root of the second camera osum over the count: each bit for bit."""
    args, prior, sigma, share, sq = sum_problem(count, count)
    res = loftr_amd.bundle_adjust(*args, position_prior=prior, prior_sigma=sigma, max_iters=0)
    plain = loftr_amd.bundle_adjust(*args, max_iters=0)
    same = lambda a, b: np.float64(a).tobytes() == np.float64(b).tobytes()
    assert res.stats["n_prior_cameras"] == count and res.cam_prior.tolist() == [False] + [True] * count
    assert same(res.stats["prior_cost_before"], osum(list(share))), (res.stats["prior_cost_before"], osum(list(share)))
    assert same(res.cost_before, plain.cost_before + osum(list(share)))
    assert same(res.stats["prior_rms_before"], np.sqrt(osum(list(sq)) / np.float64(count)))
    assert same(res.stats["prior_cost_after"], res.stats["prior_cost_before"]) and same(res.rms_px_before, plain.rms_px_before)


# ---- Python errors ------------------------------------------------------------------------------------------------------------------------
def test_python_errors(lib):
    s = PC.prior_case("scene_a")
    a, n = BC.inputs(s), len(s["K"])
    call = lambda **kw: loftr_amd.bundle_adjust(*a, **dict(dict(position_prior=s["prior_xyz"], prior_sigma=0.02), **kw))
    for bad in (dict(position_prior=s["prior_xyz"][:4]), dict(position_prior=s["prior_xyz"][:, :2]), dict(prior_sigma=np.ones(n - 1)),
                dict(prior_sigma=np.ones((n, 2))), dict(prior_mask=np.ones(n + 1, bool)), dict(prior_sigma=0.0), dict(prior_sigma=-1.0),
                dict(prior_sigma=float("nan")), dict(prior_sigma=float("inf")), dict(prior_sigma=None), dict(prior_sigma=True)):
        with pytest.raises(ValueError, match="position_prior|prior_sigma|prior_mask"):
            call(**bad)
    if torch.cuda.is_available():                                        # a GPU prior next to CPU arguments, and the reverse
        with pytest.raises(ValueError, match="position_prior is on the GPU"):
            call(position_prior=torch.from_numpy(s["prior_xyz"]).cuda())
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]
        with pytest.raises(ValueError, match="position_prior is on the CPU"):
            loftr_amd.bundle_adjust(*dev, position_prior=s["prior_xyz"])
        with pytest.raises(ValueError, match="prior_mask is on the CPU"):
            loftr_amd.bundle_adjust(*dev, position_prior=torch.from_numpy(s["prior_xyz"]).cuda(), prior_mask=np.ones(n, bool))
    # torch tensors on the CPU are taken as numpy arrays are
    res = call(position_prior=torch.from_numpy(s["prior_xyz"]), prior_sigma=torch.full((n,), 0.02, dtype=torch.float64), prior_mask=torch.ones(n, dtype=torch.bool))
    assert res.stats["n_prior_cameras"] == n - 1 and not res.cam_prior[0]       # fixed=None still fixes image 0


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------
def test_align_refine_chain_on_the_cpu(lib):
    s, rec, ref, aligned, refined, al = PC.refine_chain("cpu")
    posed = rec.posed.numpy()
    assert posed.tolist() == [True] * 4 + [False] and al.inliers.tolist() == posed.tolist()
    Ta, Tr = aligned.T_cam_from_world.numpy(), refined.T_cam_from_world.numpy()
    assert np.isnan(Tr[4]).all() and np.isnan(Ta[4]).all()               # the unposed image comes back as it went in
    b = refined.bundle
    assert b.cam_prior.tolist() == posed.tolist() and b.cam_free.tolist() == posed.tolist() and b.stats["n_prior_cameras"] == 4
    assert b.status in ("converged", "max_iters") and b.cost_after < b.cost_before
    ea, er = PC.centre_rms(Ta, s["T"], posed), PC.centre_rms(Tr, s["T"], posed)
    ma, mr = PC.centre_max(Ta[posed], s["T"][posed]), PC.centre_max(Tr[posed], s["T"][posed])
    print(f"align(refine): rms centre error {ea:.6g} -> {er:.6g}, largest {ma:.6g} -> {mr:.6g}; prior rms {b.stats['prior_rms_before']:.6g} -> "
          f"{b.stats['prior_rms_after']:.6g}; points {aligned.points.stats['n_ok']} -> {refined.points.stats['n_ok']}")
    assert er <= ea and mr <= ma
    assert refined.points is not aligned.points and refined.points.stats["n_ok"] > 0 and refined.K is not None
    assert refined.points.offsets is not None and refined.T_cam_from_world is b.T_cam_from_world
    with pytest.raises(ValueError, match="refine needs sfm"):
        rec.align(ref, thresh=0.05, refine=dict(sigma=0.005))
