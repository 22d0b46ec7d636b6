"""CPU checks of image registration and incremental reconstruction (loftr_amd/registration.py, csrc/register.hip): the host
routine of the correspondence table against the numpy oracle, register_images against the host estimator on the table's slices,
triangulate(posed=...) against a CSR filtered by hand, and the reconstruction loop against ground truth, measured against a reference
run that uses existing code only (triangulation from the true poses, then bundle adjustment)."""
import os

import numpy as np
import pytest
import torch

import _bundle_cases as BC
import _registration_cases as RC
import _registration_oracle as O
import _triangulation_cases as TC
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops
from loftr_amd.evaluation import estimate_absolute_pose_native, estimate_pose_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_CORR = MIN_INLIERS = 6            # scene_b: an unposed image sees 8-30 of the points of the first rounds; 6 leaves P3P two spare points
TABLE_CASES = {**RC.scene_cases(), **RC.edge_cases(), "list_65": RC.list_case(65), "images_65": RC.images_case(65), "long_track": RC.long_track(),
               "random": RC.random_case(7, 9, 300, 9)}


@pytest.fixture(scope="module", autouse=True)
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_host_routine_equals_the_oracle(name):
    c = TABLE_CASES[name]
    got, want = ops.register_corr_host(*RC.args(c)), O.table(*RC.args(c))
    assert sorted(got) == sorted(want) == sorted(RC.OUT)
    for k in RC.OUT:
        assert got[k].dtype == want[k].dtype and RC.same(got[k], want[k]), (name, k)


def test_hand_case_counts_and_threshold():
    h = RC.hand()
    out = ops.register_corr_host(*RC.args(h))
    assert out["n_corr"].tolist() == h["expect_n_corr"] and out["counts"].tolist() == [9, 2, 0, 4, 3, 12, 5, 0]
    assert out["cand_rank"].tolist() == [-1, 0, -1, 1, -1, -1] and out["cand_image"][:2].tolist() == [1, 3]     # n_corr = min_corr is in,
    assert out["cand_offsets"][:3].tolist() == [0, 4, 9]                                                        # min_corr - 1 is out
    obs3 = out["corr_obs"][4:9].tolist()
    assert obs3 == sorted(obs3) and h["obs_image"][obs3].tolist() == [3] * 5
    assert obs3[1] + 1 == obs3[2]                                       # the two observations of image 3 in track 1, in observation order
    five = ops.register_corr_host(*RC.args(h)[:-1], 5)
    assert five["counts"][:2].tolist() == [5, 1] and five["cand_image"][0] == 3


@pytest.mark.parametrize("name,case,bit", RC.bad_inputs(), ids=[b[0] for b in RC.bad_inputs()])
def test_every_error_bit(lib, name, case, bit):
    with pytest.raises(O.BadInput) as e:
        O.table(*RC.args(case))
    assert e.value.bits & bit
    with pytest.raises(_lib.LoftrHipError, match="status -1"):
        ops.register_corr_host(*RC.args(case))
    import ctypes
    a = [np.ascontiguousarray(case[k]) for k in RC.NAMES]
    T, N, n = len(a[0]) - 1, len(a[1]), len(a[5])
    out = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros((N, 3), np.float32),
           np.zeros((N, 2), np.float32), np.zeros(N, np.int64), np.zeros(N, np.int32), np.full(8, 7, np.int64)]
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    st = lib.loftr_register_corr_host(p(a[0]), T, p(a[1]), p(a[2]), N, p(a[3]), p(a[4]), p(a[5]), n, p(a[6]), p(a[7]), 4, *[p(x) for x in out])
    assert st == -1 and out[8].tolist() == [0, 0, bit, 0, 0, 0, 0, 0]


# ---- register_images ---------------------------------------------------------------------------------------------------------------------
def _true_model(s):
    """scene -> Points3D-like inputs from the true poses (existing code)."""
    return loftr_amd.triangulate_tracks(s["offsets"], s["obs_image"], s["obs_xy"], s["K"], s["T_true"])


def test_register_images_equals_the_estimator_on_the_slices():
    s = BC.scene_b()
    pts = _true_model(s)
    n = len(s["K"])
    posed = np.zeros(n, bool)
    posed[[0, 1, 4, 7]] = True
    T_in = s["T_true"].copy()
    T_in[~posed] = np.nan
    T_in[2] = np.arange(16).reshape(4, 4) * np.pi                       # an unposed image's matrix is handed back untouched, whatever it holds
    reg = loftr_amd.register_images(s["offsets"], s["obs_image"], s["obs_xy"], pts.xyz, pts.status, s["K"], T_in, posed, min_corr=60,
                                    min_inliers=55, thresh_px=4.0, conf=0.999, seed=3)
    P, C = reg.stats["n_candidates"], reg.stats["n_correspondences"]
    assert 0 < P < 8 and reg.cand_offsets[-1] == C == reg.corr_xyz.shape[0] and (reg.n_corr.numpy()[posed] == 0).all()
    assert reg.n_corr.dtype == torch.int32 and reg.n_inliers.dtype == torch.int64 and reg.T_cam_from_world.dtype == torch.float64
    registered = reg.registered.numpy()
    seen = 0
    for p, im in enumerate(reg.cand_image.tolist()):
        sl = slice(int(reg.cand_offsets[p]), int(reg.cand_offsets[p + 1]))
        assert sl.stop - sl.start == reg.n_corr[im] >= 60
        R, t, inl = estimate_absolute_pose_native(reg.corr_xyz[sl].numpy(), reg.corr_xy[sl].numpy(), s["K"][im].astype(np.float32), 4.0, 0.999, 3)
        assert reg.n_inliers[im] == inl.sum() and torch.equal(reg.corr_inlier[sl], torch.from_numpy(inl))
        assert registered[im] == (inl.sum() >= 55)
        if registered[im]:
            want = torch.eye(4, dtype=torch.float64)
            want[:3, :3], want[:3, 3] = torch.from_numpy(R), torch.from_numpy(t)
            assert torch.equal(reg.T_cam_from_world[im], want)
            seen += 1
            err = BC.pose_errors(reg.T_cam_from_world.numpy(), s["T_true"], np.arange(n) == im)
            assert err[0] < 0.5 and err[1] < 0.05, err                  # a sane pose (0.5 px noise, > 55 points)
    assert seen >= 1 and seen == registered.sum()
    untouched = ~registered
    assert reg.T_cam_from_world.numpy()[untouched].tobytes() == T_in[untouched].tobytes()      # NaN poses included: the bytes
    assert torch.equal(reg.posed, torch.from_numpy(posed) | reg.registered)
    assert (reg.n_inliers.numpy()[np.setdiff1d(np.arange(n), reg.cand_image.numpy())] == -1).all()
    # nothing to do: every image posed
    none = loftr_amd.register_images(s["offsets"], s["obs_image"], s["obs_xy"], pts.xyz, pts.status, s["K"], s["T_true"], np.ones(n, bool),
                                     min_corr=4, min_inliers=4)
    assert none.stats["n_candidates"] == 0 and not none.registered.any() and none.T_cam_from_world.numpy().tobytes() == s["T_true"].tobytes()


def test_register_images_refuses_bad_input():
    s = BC.scene_a()
    pts = _true_model(s)
    a = [s["offsets"], s["obs_image"], s["obs_xy"], pts.xyz, pts.status, s["K"], s["T_true"], np.zeros(5, bool)]
    with pytest.raises(ValueError, match="min_corr must be an integer >= 4"):
        loftr_amd.register_images(*a, min_corr=3, min_inliers=3)
    with pytest.raises(ValueError, match="obs_image outside"):
        loftr_amd.register_images(a[0], np.where(np.arange(len(a[1])) == 3, 5, a[1]), *a[2:], min_corr=4, min_inliers=4)
    bad = a[0].copy()
    bad[3] = bad[2] - 1
    with pytest.raises(ValueError, match="offsets must start at 0"):
        loftr_amd.register_images(bad, *a[1:], min_corr=4, min_inliers=4)
    with pytest.raises(ValueError, match="must hold integers"):
        loftr_amd.register_images(a[0], a[1].astype(np.float32), *a[2:], min_corr=4, min_inliers=4)
    with pytest.raises(_lib.LoftrHipError, match=r"expected K \[n,3,3\]"):
        loftr_amd.register_images(*a[:5], s["K"][:4], *a[6:], min_corr=4, min_inliers=4)
    with pytest.raises(_lib.LoftrHipError, match="must be|expected offsets"):
        loftr_amd.register_images(*a[:3], pts.xyz[:-1], *a[4:], min_corr=4, min_inliers=4)


# ---- triangulate(posed=...) ---------------------------------------------------------------------------------------------------------------
def test_triangulate_posed_none_is_todays_call():
    sfm, s = TC.run_atlas("cpu"), TC.sfm_scene()
    a, b = sfm.triangulate(s["K"], s["T"]), sfm.triangulate(s["K"], s["T"], posed=None)
    for k in loftr_amd.Points3D.FIELDS + ("offsets", "image", "keypoint"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and RC.same(x.numpy(), y.numpy()), k
    assert a.stats == b.stats
    assert loftr_amd.Points3D.FIELDS == ("xyz", "n_inliers", "rms_px", "tri_cos", "status", "obs_inlier")
    assert loftr_amd.SfmResult.FIELDS == ("kp_offsets", "keypoints", "score", "n_obs", "row_offsets", "matches", "match_conf", "track_id",
                                          "track_len", "track_ok", "row_images")


def test_triangulate_posed_mask_equals_a_csr_filtered_by_hand():
    sfm, s = TC.run_atlas("cpu"), TC.sfm_scene()
    posed = np.array([1, 0, 1, 1, 0], bool)
    T = s["T"].copy()
    T[~posed] = np.nan                                                  # never read
    got = sfm.triangulate(s["K"], T, posed=torch.from_numpy(posed))
    offsets, image, local = (x.numpy() for x in sfm.tracks())
    xy = sfm.keypoints.numpy()[sfm.kp_offsets.numpy()[image] + local]
    off2, keep = [0], []
    for t in range(len(offsets) - 1):
        keep += [o for o in range(offsets[t], offsets[t + 1]) if posed[image[o]]]
        off2.append(len(keep))
    T_any = s["T"].copy()
    T_any[~posed] = np.eye(4)
    want = loftr_amd.triangulate_tracks(np.array(off2), image[keep].astype(np.int32), xy[keep], s["K"], T_any)
    for k in ("xyz", "n_inliers", "rms_px", "tri_cos", "status"):
        assert RC.same(getattr(got, k).numpy(), getattr(want, k).numpy()), k
    full = np.zeros(len(image), bool)
    full[keep] = want.obs_inlier.numpy()
    assert np.array_equal(got.obs_inlier.numpy(), full) and not got.obs_inlier.numpy()[~posed[image]].any()
    assert np.array_equal(got.offsets.numpy(), offsets) and np.array_equal(got.image.numpy(), image) and got.status.numel() == len(offsets) - 1
    assert (got.status.numpy()[np.diff(off2) < 2] == 1).all() and (got.status == 0).sum() > 30
    one = sfm.triangulate(s["K"], T, posed=np.array([1, 0, 0, 0, 0], bool))          # fewer than 2 posed observations: too_short
    assert (one.status == 1).all() and not one.obs_inlier.any() and one.stats["n_too_short"] == one.status.numel()
    u8 = sfm.triangulate(s["K"], T, posed=posed.astype(np.uint8))
    assert RC.same(u8.xyz.numpy(), got.xyz.numpy())
    with pytest.raises(ValueError, match=r"expected posed \[5\]"):
        sfm.triangulate(s["K"], T, posed=np.ones(4, bool))
    # SfmResult.register is register_images over the atlas's keypoints
    reg = sfm.register(got, s["K"], T, posed, min_corr=MIN_CORR, min_inliers=MIN_INLIERS, seed=1)
    want = loftr_amd.register_images(offsets, image.astype(np.int32), xy, got.xyz, got.status, s["K"], T, posed, min_corr=MIN_CORR,
                                     min_inliers=MIN_INLIERS, seed=1)
    assert reg.registered.tolist() == [False, True, False, False, True]
    for k in loftr_amd.Registration.FIELDS:
        assert RC.same(getattr(reg, k).numpy(), getattr(want, k).numpy()), k


# ---- the loop ------------------------------------------------------------------------------------------------------------------------------
def _relative(T, a, b):
    Ra, Rb = T[a, :3, :3], T[b, :3, :3]
    R = Rb @ Ra.T
    return R, T[b, :3, 3] - R @ T[a, :3, 3]


def _filtered_triangulation(s, T, posed):
    """triangulate over the posed images with existing code: the CSR filtered by hand."""
    off, image = s["offsets"], s["obs_image"]
    off2, keep = [0], []
    for t in range(len(off) - 1):
        keep += [o for o in range(off[t], off[t + 1]) if posed[image[o]]]
        off2.append(len(keep))
    T2 = np.where(posed[:, None, None], T, np.eye(4))
    pts = loftr_amd.triangulate_tracks(np.array(off2), image[keep], s["obs_xy"][keep], s["K"], T2)
    mask = np.zeros(len(image), bool)
    mask[keep] = pts.obs_inlier.numpy()
    return pts, mask


def _test_side_loop(s, a, b, R, t):
    """The loop written out from the oracle's table plus the existing host routines -> (T, posed, final BundleResult)."""
    n = len(s["K"])
    T = np.full((n, 4, 4), np.nan)
    T[a] = np.eye(4)
    T[b] = np.eye(4)
    T[b, :3, :3], T[b, :3, 3] = R, t / np.linalg.norm(t)
    posed, fixed = np.zeros(n, bool), np.zeros(n, bool)
    posed[[a, b]], fixed[a] = True, True

    def refine(T):
        pts, mask = _filtered_triangulation(s, T, posed)
        res = loftr_amd.bundle_adjust(s["offsets"], s["obs_image"], s["obs_xy"], mask, pts.xyz, s["K"], T, fixed=fixed)
        return _filtered_triangulation(s, res.T_cam_from_world.numpy(), posed)[0], res

    for _ in range(50):
        pts, res = refine(T)
        T = res.T_cam_from_world.numpy().copy()
        tab = RC.trimmed(O.table(s["offsets"], s["obs_image"], s["obs_xy"], pts.xyz.numpy(), pts.status.numpy(), posed.astype(np.uint8),
                                 *O.groups(s["obs_image"], n), MIN_CORR))
        new = []
        for p, im in enumerate(tab["cand_image"]):
            sl = slice(tab["cand_offsets"][p], tab["cand_offsets"][p + 1])
            est = estimate_absolute_pose_native(tab["corr_xyz"][sl], tab["corr_xy"][sl], s["K"][im].astype(np.float32), 4.0, 0.999, 0)
            if est is not None and est[2].sum() >= MIN_INLIERS:
                T[im] = np.eye(4)
                T[im, :3, :3], T[im, :3, 3] = est[0], est[1]
                new.append(im)
        posed[new] = True
        if not new or posed.all():
            break
    return T, posed, refine(T)


@pytest.fixture(scope="module")
def scene_b_runs():
    s = BC.scene_b()
    R, t = _relative(s["T_true"], 0, 1)
    rec = loftr_amd.reconstruct_tracks(s["offsets"], s["obs_image"], s["obs_xy"], s["K"], (0, 1, R, t), min_corr=MIN_CORR, min_inliers=MIN_INLIERS)
    fixed = np.zeros(12, bool)
    fixed[0] = True
    ref_pts = loftr_amd.triangulate_tracks(s["offsets"], s["obs_image"], s["obs_xy"], s["K"], s["T_true"])
    ref = loftr_amd.bundle_adjust(s["offsets"], s["obs_image"], s["obs_xy"], ref_pts.obs_inlier, ref_pts.xyz, s["K"], s["T_true"], fixed=fixed)
    return s, (R, t), rec, ref


def test_the_test_side_loop_poses_every_image_and_agrees():
    """The condition of the accuracy test, checked with code that is not under test: a loop made of the oracle's table and the existing
    host routines poses all 12 images of scene_b (seed 12, the generator's default) -- and, every step being order-defined, it ends
    with the library's poses bit for bit."""
    s = BC.scene_b()
    R, t = _relative(s["T_true"], 0, 1)
    T, posed, (pts, res) = _test_side_loop(s, 0, 1, R, t)
    assert posed.all()
    rec = loftr_amd.reconstruct_tracks(s["offsets"], s["obs_image"], s["obs_xy"], s["K"], (0, 1, R, t), min_corr=MIN_CORR, min_inliers=MIN_INLIERS)
    assert RC.same(rec.T_cam_from_world.numpy(), res.T_cam_from_world.numpy()) and RC.same(rec.points.xyz.numpy(), pts.xyz.numpy())


def test_reconstruct_tracks_against_the_reference_run(scene_b_runs):
    """All 12 images end posed; after a similarity alignment of the camera centres, rotation and centre errors and the final rms are at
    most 2 x those of the reference run (triangulation from the TRUE poses, then bundle adjustment with the same fixed camera, aligned
    the same way): the two runs keep different observation sets and sit on the same 0.5 px noise floor."""
    s, _, rec, ref = scene_b_runs
    assert rec.posed.all() and rec.stats["n_posed"] == 12 and (rec.round_registered >= 0).all()
    assert rec.round_registered[:2].tolist() == [0, 0] and (rec.round_registered[2:] >= 1).all() and rec.round_registered.dtype == torch.int32
    assert rec.stats["n_rounds"] == int(rec.round_registered.max()) == len(rec.stats["rounds"])
    assert rec.points.status.numel() == 200 and rec.bundle.status in ops.BUNDLE_STATUS and np.isfinite(rec.T_cam_from_world.numpy()).all()
    every = np.ones(12, bool)
    got = O.aligned_errors(rec.T_cam_from_world.numpy(), s["T_true"], every) + (rec.bundle.rms_px_after,)
    want = O.aligned_errors(ref.T_cam_from_world.numpy(), s["T_true"], every) + (ref.rms_px_after,)
    lines = ["reconstruct_tracks on tests/_bundle_cases.py scene_b (12 cameras, 200 points, 0.5 px noise), initialised with the true relative pose of",
             f"images 0 and 1, min_corr = min_inliers = {MIN_CORR}; reference: triangulate_tracks from the true poses, then bundle_adjust (image 0 fixed).",
             "Both aligned to the true camera centres by a similarity (Umeyama).  Required: every ratio <= 2.",
             f"rounds: {rec.stats['n_rounds']}, round of registration per image: {rec.round_registered.tolist()}",
             f"points: {int((rec.points.status == 0).sum())} (reference {int(ref.point_active.sum())} active)"]
    for name, g, w in zip(("largest rotation error [deg]", "largest centre error", "rms_px_after"), got, want):
        lines.append(f"{name}: {g:.6g} (reference {w:.6g}, ratio {g / w:.3f})")
    report = "\n".join(lines)
    print(report)
    if os.environ.get("LOFTR_WRITE_PROFILES"):
        with open(os.path.join(ROOT, "profiles", "registration_accuracy.txt"), "w") as fh:
            fh.write(report + "\n")
    for g, w in zip(got, want):
        assert g <= 2 * w, report


def test_sfm_reconstruct_on_the_cpu_atlas():
    sfm, s = TC.run_atlas("cpu"), TC.sfm_scene()
    rec = sfm.reconstruct(s["K"], min_corr=MIN_CORR, min_inliers=MIN_INLIERS)
    # the automatic initial row, recomputed here from estimate_pose_native
    rows, off, kp_off, kp, m = sfm.row_images.tolist(), sfm.row_offsets.tolist(), sfm.kp_offsets.tolist(), sfm.keypoints.numpy(), sfm.matches.numpy()
    est = []
    for r, (a, b) in enumerate(rows):
        sl = slice(off[r], off[r + 1])
        est.append(estimate_pose_native(kp[kp_off[a] + m[sl, 0]], kp[kp_off[b] + m[sl, 1]], s["K"][a], s["K"][b], 4.0, 0.99999, 0))
    ninl = [-1 if e is None else int(e[2].sum()) for e in est]
    assert rec.stats["pair_inliers"] == ninl
    cand = sorted(sorted((r for r in range(len(rows)) if ninl[r] >= 0), key=lambda r: (-ninl[r], r))[:8])
    n_ok = []
    for r in cand:
        a, b = rows[r]
        T = np.tile(np.eye(4), (5, 1, 1))
        T[b, :3, :3], T[b, :3, 3] = est[r][0], est[r][1] / np.linalg.norm(est[r][1])
        n_ok.append(int((sfm.triangulate(s["K"], T, posed=np.isin(np.arange(5), (a, b))).status == 0).sum()))
    want_row = cand[int(np.argmax(n_ok))]                               # argmax: the first of equals, i.e. the earliest row
    assert rec.stats["init_row"] == want_row and rec.stats["init"] == tuple(rows[want_row])
    assert rec.posed.all() and sorted(rec.round_registered.tolist())[:2] == [0, 0]
    assert rec.points.offsets is not None and torch.equal(rec.points.offsets, sfm.tracks()[0])
    # the same 2 x rule on rms_px_after; the reference run: the true poses, then bundle adjustment (existing code)
    ref_pts = sfm.triangulate(s["K"], s["T"])
    ref = sfm.adjust(ref_pts, s["K"], s["T"])
    print(f"SfmResult.reconstruct: init row {want_row} {rows[want_row]}, rms_px_after {rec.bundle.rms_px_after:.6g} (reference {ref.rms_px_after:.6g})")
    assert rec.bundle.rms_px_after <= 2 * ref.rms_px_after
    explicit = sfm.reconstruct(s["K"], init_row=want_row, min_corr=MIN_CORR, min_inliers=MIN_INLIERS)
    assert RC.same(explicit.T_cam_from_world.numpy(), rec.T_cam_from_world.numpy())


def test_value_errors():
    s = BC.scene_a()
    R, t = _relative(s["T_true"], 0, 1)
    a = [s["offsets"], s["obs_image"], s["obs_xy"], s["K"]]
    with pytest.raises(ValueError, match="two different images.*a = 2, b = 2"):
        loftr_amd.reconstruct_tracks(*a, (2, 2, R, t), min_corr=4, min_inliers=4)
    with pytest.raises(ValueError, match=r"two different images in \[0, 5\)"):
        loftr_amd.reconstruct_tracks(*a, (0, 5, R, t), min_corr=4, min_inliers=4)
    with pytest.raises(ValueError, match=r"no relative pose.*\|t\| = 0"):                   # what a refused five-point / P3P model leaves
        loftr_amd.reconstruct_tracks(*a, (0, 1, np.zeros((3, 3)), np.zeros(3)), min_corr=4, min_inliers=4)
    with pytest.raises(ValueError, match="no relative pose"):
        loftr_amd.reconstruct_tracks(*a, (0, 1, R, t * np.nan), min_corr=4, min_inliers=4)
    with pytest.raises(ValueError, match=r"initial pair \(0, 1\) triangulates nothing: \d+ observations in 60 tracks"):
        loftr_amd.reconstruct_tracks(*a, (0, 1, np.eye(3), np.array([0.0, 0, 1])), min_corr=4, min_inliers=4, thresh_px=0.01)
    with pytest.raises(ValueError, match="fixed_extra"):
        loftr_amd.reconstruct_tracks(*a, (0, 1, R, t), ba=dict(fixed=np.ones(5, bool)), min_corr=4, min_inliers=4)
    sfm, sc = TC.run_atlas("cpu"), TC.sfm_scene()
    with pytest.raises(ValueError, match=r"row 10 has no five-point model \(rows: 10"):
        sfm.reconstruct(sc["K"], init_row=10, min_corr=4, min_inliers=4)
    with pytest.raises(ValueError, match=r"expected K \[5,3,3\]"):
        sfm.reconstruct(sc["K"][:4], min_corr=4, min_inliers=4)
