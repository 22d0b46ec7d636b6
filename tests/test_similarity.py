"""3D similarity between two point sets, host side (csrc/similarity.hip: loftr_similarity_minimal, loftr_estimate_similarity,
loftr_transform_model_host; evaluation.estimate_similarity_native, ops.transform_model on CPU tensors, loftr_amd.alignment) against the
float64 numpy oracle of tests/_similarity_oracle.py.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _registration_oracle as RO
import _similarity_cases as SC
import _similarity_oracle as O
import loftr_amd
from loftr_amd import _lib, alignment, build as build_mod, evaluation as EV, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR, CONF = SC.THR, SC.CONF
TOL = 1e-6               # the bar of tests/test_absolute_pose.py for loftr_p3p on exact problems


@pytest.fixture(scope="module", autouse=True)
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def _minimal(lib, src, dst, with_scale):
    src, dst = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(dst, np.float64)
    s, R, t, n = np.full(1, 7.0), np.full(9, 7.0), np.full(3, 7.0), C.c_int(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.loftr_similarity_minimal(ptr(src), ptr(dst), int(with_scale), ptr(s), ptr(R), ptr(t), C.byref(n)) == 0
    return n.value, float(s[0]), R.reshape(3, 3), t


def _triple(rng, with_scale):
    """A well-conditioned exact triple: the triangle's smallest sine-scaled area is 0.1 of its longest squared side."""
    while True:
        sc = O.make_scene(rng, 3, with_scale=with_scale)
        a, b = sc["src"][1] - sc["src"][0], sc["src"][2] - sc["src"][0]
        longest = max(a @ a, b @ b, (b - a) @ (b - a))
        if np.linalg.norm(np.cross(a, b)) >= 0.1 * longest:
            return sc


@pytest.mark.parametrize("with_scale", [True, False])
def test_minimal_solver_recovers_the_transform_on_exact_triples(lib, with_scale):
    """40 exact triples per mode: (s, R, t) equal the truth and the numpy oracle to 1e-6, R is a proper rotation.  Measured on
    these triples: worst distance to truth or oracle 1.7e-13 with scale, 3.4e-14 rigid."""
    rng = np.random.default_rng(40 + with_scale)
    worst = 0.0
    for _ in range(40):
        sc = _triple(rng, with_scale)
        n, s, R, t = _minimal(lib, sc["src"], sc["dst"], with_scale)
        so, Ro, to = O.umeyama(sc["src"], sc["dst"], with_scale)
        assert n == 1
        for want in ((sc["s"], sc["R"], sc["t"]), (so, Ro, to)):
            err = max(abs(s - want[0]), np.abs(R - want[1]).max(), np.abs(t - want[2]).max())
            worst = max(worst, err)
            assert err <= TOL, err
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0
        if not with_scale:
            assert s == 1.0
    print(f"with_scale {with_scale}: worst distance to truth / oracle {worst:.3e}")


def test_minimal_solver_returns_a_rotation_where_numpy_needs_the_reflection_fix(lib):
    rng = np.random.default_rng(42)
    seen = 0
    for _ in range(200):
        sc = _triple(rng, True)
        if not O.needs_reflection_fix(sc["src"], sc["dst"]):
            continue
        seen += 1
        n, s, R, t = _minimal(lib, sc["src"], sc["dst"], True)
        assert n == 1 and abs(np.linalg.det(R) - 1) <= 1e-12 and np.abs(R - sc["R"]).max() <= TOL and abs(s - sc["s"]) <= TOL
    assert seen >= 20, seen


def test_minimal_solver_degenerate_triples_give_no_solution(lib):
    sc = _triple(np.random.default_rng(43), True)
    src, dst = sc["src"], sc["dst"]
    line = lambda p: np.stack([p[0], p[0] + 0.4 * (p[1] - p[0]), p[1]])
    for a, b in ((line(src), dst), (src, line(dst)), (np.stack([src[0], src[0], src[1]]), dst), (src, np.stack([dst[0], dst[1], dst[1]])),
                 (np.stack([src[0]] * 3), dst), (1e6 * line(src), dst)):
        n, s, R, t = _minimal(lib, a, b, True)
        assert n == 0 and s == 0 and not R.any() and not t.any()
    assert _minimal(lib, 1e6 * src, 1e-6 * dst, True)[0] == 1                          # the rule is relative
    nan = src.copy()
    nan[1, 1] = np.nan
    assert _minimal(lib, nan, dst, True)[0] == 0
    assert lib.loftr_similarity_minimal(None, None, 1, None, None, None, None) == -1


@pytest.mark.parametrize("with_scale", [True, False])
@pytest.mark.parametrize("seed", [0, 11])
def test_noise_free_scene_with_outliers_gives_exactly_the_true_inliers(seed, with_scale):
    sc = O.make_scene(np.random.default_rng(50), 400, 0.0, 0.4, with_scale=with_scale, thresh=THR)
    s, R, t, mask = EV.estimate_similarity_native(sc["src"], sc["dst"], with_scale, THR, CONF, seed)
    assert np.array_equal(mask, ~sc["is_outlier"])
    assert np.array_equal(O.residual(sc["s"], sc["R"], sc["t"], sc["src"], sc["dst"]) <= THR, ~sc["is_outlier"])   # the oracle agrees
    assert np.array_equal(O.residual(s, R, t, sc["src"], sc["dst"]) <= THR, mask)
    assert abs(s - sc["s"]) <= TOL and np.abs(R - sc["R"]).max() <= TOL and np.abs(t - sc["t"]).max() <= TOL
    if not with_scale:
        assert s == 1.0


def _rms_to_clean(sc, s, R, t):
    inl = ~sc["is_outlier"]
    return float(np.sqrt(np.mean(O.residual(s, R, t, sc["src"][inl], sc["clean"][inl]) ** 2)))


@pytest.mark.parametrize("with_scale", [True, False])
@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("outliers", [0.0, 0.4])
@pytest.mark.parametrize("n", [300, 2000])
def test_noisy_scenes_equal_the_oracle_on_the_returned_inliers_and_fit_the_true_ones(n, outliers, planar, with_scale):
    """Noise 0.008 per coordinate, thresh 0.05 (6 sigma).  The returned model is the numpy Umeyama over the RETURNED inlier set (the
    same estimator algebraically: 1e-6, the exact-problem bar), and, over the true inliers, its RMS distance to the noise-free
    destinations is at most 2 x that of the oracle's fit on the true inliers (the margin of tests/test_absolute_pose.py)."""
    rng = np.random.default_rng(60 + n + int(10 * outliers) + planar + 2 * with_scale)
    for seed in (0, 1, 2):
        sc = O.make_scene(rng, n, 0.008, outliers, with_scale, planar, THR)
        s, R, t, mask = EV.estimate_similarity_native(sc["src"], sc["dst"], with_scale, THR, CONF, seed)
        so, Ro, to = O.umeyama(sc["src"][mask], sc["dst"][mask], with_scale)
        err = max(abs(s - so), np.abs(R - Ro).max(), np.abs(t - to).max())
        inl = ~sc["is_outlier"]
        ratio = _rms_to_clean(sc, s, R, t) / _rms_to_clean(sc, *O.umeyama(sc["src"][inl], sc["dst"][inl], with_scale))
        print(f"n {n} outliers {outliers} planar {planar} scale {with_scale} seed {seed}: to oracle {err:.2e}, ratio {ratio:.4f}, "
              f"{mask.sum()} inliers of {inl.sum()} true")
        assert err <= TOL, err
        assert ratio <= 2.0, ratio
        assert not mask[sc["is_outlier"]].any() and np.array_equal(O.residual(s, R, t, sc["src"], sc["dst"]) <= THR, mask)
        assert (s == 1.0) if not with_scale else (s > 0)


def test_too_few_correspondences_and_the_minimal_case():
    sc = O.make_scene(np.random.default_rng(70), 3)
    for m in (0, 2):
        assert EV.estimate_similarity_native(sc["src"][:m], sc["dst"][:m]) is None
        assert EV.estimate_similarity_native_gpu(sc["src"][:m], sc["dst"][:m]) is None      # (returns before it touches a GPU)
    s, R, t, mask = EV.estimate_similarity_native(sc["src"], sc["dst"])
    assert mask.tolist() == [True, True, True] and abs(s - sc["s"]) <= TOL
    col = O.make_collinear_scene()
    assert EV.estimate_similarity_native(col["src"], col["dst"]) is None               # every sample is degenerate
    with pytest.raises(ValueError):
        EV.estimate_similarity_native(sc["src"], sc["dst"][:2])


def test_adoption_scene_keeps_the_exact_model():
    sc = O.make_adoption_scene(np.random.default_rng(71), THR)
    s, R, t, mask = EV.estimate_similarity_native(sc["src"], sc["dst"], True, THR, CONF, 0)
    assert mask.all() and (O.residual(*O.umeyama(sc["src"], sc["dst"]), sc["src"], sc["dst"]) <= THR).sum() < len(mask)


# ---- moving a model ---------------------------------------------------------------------------------------------------------------
def _tensors(case):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in case]


@pytest.mark.parametrize("N,n", [(1, 1), (257, 65), (0, 4), (9, 0)])
def test_transform_model_on_the_cpu_against_numpy(N, n):
    xyz, T, posed, s, R, t = case = SC.model_case(N, n)
    want_xyz, want_T = O.transform_model(xyz, T, posed, s[0], R, t)
    got_xyz, got_T = ops.transform_model(*_tensors(case))
    assert got_xyz.dtype == torch.float32 and got_T.dtype == torch.float64 and got_xyz.shape == (N, 3) and got_T.shape == (n, 4, 4)
    g, w = got_xyz.numpy(), want_xyz.astype(np.float32)
    assert np.array_equal(np.isnan(g), np.isnan(w))
    ok = ~np.isnan(w)
    ulps = np.abs(g[ok].view(np.int32).astype(np.int64) - w[ok].view(np.int32).astype(np.int64))
    assert ulps.max(initial=0) <= 1, ulps.max()                                         # the f32 rounding of the f64 value, or its neighbour
    gT = got_T.numpy()
    assert gT[~posed].tobytes() == T[~posed].tobytes()                                  # unposed rows: the input's bits, NaN included
    assert np.abs(gT[posed] - want_T[posed]).max(initial=0) <= 1e-13 * max(1.0, np.abs(want_T[posed]).max(initial=0))
    assert (gT[posed, 3] == [0, 0, 0, 1]).all()
    # camera coordinates of a moved point through the moved pose: s times the original ones (directions kept, depths scaled)
    X = np.random.default_rng(9).uniform(-3, 3, (5, 3))
    X2 = s[0] * X @ R.T + t
    for i in np.flatnonzero(posed):
        before, after = X @ T[i, :3, :3].T + T[i, :3, 3], X2 @ gT[i, :3, :3].T + gT[i, :3, 3]
        assert np.abs(after - s[0] * before).max() <= 1e-12 * max(1.0, np.abs(before).max())
    # in place
    tens = _tensors(case)
    a, b = ops.transform_model(*tens, out_xyz=tens[0], out_T=tens[1])
    assert a is tens[0] and b is tens[1] and a.numpy().tobytes() == g.tobytes() and b.numpy().tobytes() == gT.tobytes()


def test_transform_model_refusals():
    xyz, T, posed, s, R, t = _tensors(SC.model_case(4, 3))
    for bad in ((xyz.double(), T, posed, s, R, t), (xyz, T.float(), posed, s, R, t), (xyz, T, posed.float(), s, R, t), (xyz, T, posed, s, R.float(), t),
                (xyz[:, :2], T, posed, s, R, t), (xyz, T[:, :3], posed, s, R, t), (xyz, T, posed[:2], s, R, t), (xyz, T, posed, s, R[:2], t),
                (xyz, T, posed, torch.zeros(2, dtype=torch.float64), R, t), (xyz.numpy(), T, posed, s, R, t)):
        with pytest.raises(_lib.LoftrHipError):
            ops.transform_model(*bad)
    with pytest.raises(_lib.LoftrHipError):
        ops.transform_model(xyz, T, posed, s, R, t, out_xyz=torch.zeros(4, 3, dtype=torch.float64))


# ---- alignment --------------------------------------------------------------------------------------------------------------------
def _errors(T, T_ref, which):
    """(largest rotation error in degrees, largest centre error) of poses already in the reference frame."""
    rot = cen = 0.0
    for i in np.flatnonzero(which):
        rot = max(rot, O.rotation_error_deg(T[i, :3, :3], T_ref[i, :3, :3]))
        cen = max(cen, float(np.linalg.norm(O.centres(T[i:i + 1])[0] - O.centres(T_ref[i:i + 1])[0])))
    return rot, cen


def test_align_recovers_the_frame_despite_grossly_wrong_positions():
    """scene_b reconstructed on the CPU; reference positions = the true centres in another frame (random similarity), one image
    without a position, three of the twelve displaced by 10-30 x thresh.  The inliers are exactly the known, uncorrupted images; after
    align the largest rotation and centre errors against the truth (in the reference frame) are at most 2 x those the private Umeyama
    of tests/_registration_oracle.py reaches when it is given the uncorrupted set (the ratio rule of tests/test_registration.py); the
    least-squares fit over all known positions is worse than both."""
    s, rec, al_sc = SC.alignment_case()
    good = al_sc["known"] & ~al_sc["bad"]
    assert rec.posed.all() and al_sc["bad"].sum() == 3 and (~al_sc["known"]).sum() == 1 and good.sum() == 8
    rec2, al = rec.align(al_sc["ref"], al_sc["known"], thresh=SC.ALIGN_THR)
    assert isinstance(al, loftr_amd.Alignment) and al.ok and int(al.n_inliers) == 8
    assert np.array_equal(al.inliers.numpy(), good)
    every = np.ones(12, bool)
    T0 = rec.T_cam_from_world.numpy()
    got = _errors(rec2.T_cam_from_world.numpy(), al_sc["T_ref"], every)
    # the oracle: its own Umeyama on the uncorrupted centres, its poses moved by the numpy formulae
    so, Ro, to = RO.umeyama(O.centres(T0)[good], al_sc["ref"][good])
    want = _errors(O.transform_model(np.zeros((0, 3)), T0, every, so, Ro, to)[1], al_sc["T_ref"], every)
    sn, Rn, tn = RO.umeyama(O.centres(T0)[al_sc["known"]], al_sc["ref"][al_sc["known"]])
    naive = _errors(O.transform_model(np.zeros((0, 3)), T0, every, sn, Rn, tn)[1], al_sc["T_ref"], every)
    plain = alignment.fit_centres(rec.T_cam_from_world, rec.posed, torch.from_numpy(al_sc["ref"]), torch.from_numpy(al_sc["known"]))
    before = RO.aligned_errors(T0, s["T_true"], every)
    lines = ["Reconstruction.align on tests/_bundle_cases.py scene_b (12 cameras, reconstructed on the CPU): reference positions = true centres moved by a",
             f"random similarity (scale {al_sc['s']:.4f}), 1 image without a position, 3 displaced by 10-30 x thresh, thresh = {SC.ALIGN_THR}.",
             "Errors over all 12 images against the true poses in the reference frame: largest rotation error [deg], largest centre error.",
             f"reconstruction in its own frame, aligned by the test oracle over all 12 true centres (units of the truth): {before[0]:.6g}, {before[1]:.6g}",
             f"after align (RANSAC, {int(al.n_inliers)} inliers, rms {float(al.rms):.6g}, s {float(al.s):.6f}): {got[0]:.6g}, {got[1]:.6g}",
             f"oracle Umeyama over the 8 uncorrupted known images: {want[0]:.6g}, {want[1]:.6g}",
             f"least squares over all 11 known images (non-robust): {naive[0]:.6g}, {naive[1]:.6g}"]
    report = "\n".join(lines)
    print(report)
    if os.environ.get("LOFTR_WRITE_PROFILES"):
        with open(os.path.join(ROOT, "profiles", "alignment_accuracy.txt"), "w") as fh:
            fh.write(report + "\n")
    for g, w, nv in zip(got, want, naive):
        assert g <= 2 * w, report
        assert nv > g and nv > w, report
    # the library's own non-robust fit is the oracle's
    assert abs(float(plain.s) - sn) <= TOL and np.abs(plain.R.numpy() - Rn).max() <= TOL and np.abs(plain.t.numpy() - tn).max() <= TOL
    assert int(plain.n_inliers) == 11
    # what is shared and what is new
    assert rec2 is not rec and rec2.bundle is rec.bundle and rec2.posed is rec.posed and rec2.points.status is rec.points.status
    assert rec2.points is not rec.points and not torch.equal(rec2.points.xyz, rec.points.xyz)
    t2 = rec.transformed(al.s, al.R, al.t)
    assert torch.equal(t2.T_cam_from_world, rec2.T_cam_from_world) and t2.points.xyz.numpy().tobytes() == rec2.points.xyz.numpy().tobytes()
    same, al0 = rec.align(al_sc["ref"], al_sc["known"], thresh=SC.ALIGN_THR, apply=False)
    assert same is rec and torch.equal(al0.R, al.R)
    # known=None: the finite rows
    _, al1 = rec.align(al_sc["ref"], thresh=SC.ALIGN_THR)
    assert torch.equal(al1.inliers, al.inliers) and torch.equal(al1.t, al.t)


def test_align_without_a_model_returns_the_reconstruction_unchanged():
    s, rec, al_sc = SC.alignment_case()
    known = np.zeros(12, bool)
    known[[1, 4]] = True                                                               # two positions: no similarity
    same, al = rec.align(al_sc["ref"], known, thresh=SC.ALIGN_THR)
    assert same is rec and not al.ok and int(al.n_inliers) == -1 and not al.inliers.any() and not al.R.any() and np.isnan(float(al.rms))
    with pytest.raises(ValueError):
        alignment.align_centres(rec.T_cam_from_world, rec.posed, torch.zeros(11, 3), torch.ones(12, dtype=torch.bool), 0.1)


def test_trajectory_errors_against_the_registration_oracle():
    s, rec, _ = SC.alignment_case()
    T0 = rec.T_cam_from_world.numpy()
    every = np.ones(12, bool)
    rot, cen = EV.trajectory_errors(rec.T_cam_from_world, rec.posed, s["T_true"])
    want = RO.aligned_errors(T0, s["T_true"], every)
    assert abs(rot.max() - want[0]) <= 1e-6 and abs(cen.max() - want[1]) <= 1e-9 and rot.shape == cen.shape == (12,)
    # one grossly wrong pose: the robust form keeps the others' errors, the plain one spreads the damage
    T_bad = T0.copy()
    T_bad[5, :3, 3] += 3.0
    r_rot, r_cen = EV.trajectory_errors(T_bad, every, s["T_true"], thresh=0.05)
    p_rot, p_cen = EV.trajectory_errors(T_bad, every, s["T_true"])
    keep = np.arange(12) != 5
    assert r_cen[keep].max() <= 2 * want[1] and p_cen[keep].max() > 10 * r_cen[keep].max() and r_cen[5] > 1.0
    posed = every.copy()
    posed[[2, 7]] = False
    rot2, cen2 = EV.trajectory_errors(T0, posed, s["T_true"])
    assert np.isnan(rot2[[2, 7]]).all() and np.isfinite(cen2[posed]).all()
