"""Inputs shared by the triangulation tests (tests/test_triangulation.py on the CPU, tests/test_hip_triangulation.py on the GPU):
the seeded scenes with ground truth, the hand-written tracks with the status each must get, and a synthetic pair list for the atlas."""
import functools

import numpy as np

THRESH_PX, MIN_ANGLE_DEG = 4.0, 1.5
COS_MIN = float(np.cos(np.radians(MIN_ANGLE_DEG)))
LENGTHS = (2, 3, 4, 5, 8, 12, 20, 40, 70)
RATES = (0.0, 0.2, 0.4)


def rotation(axis, deg):
    """Rodrigues."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * A + (1 - np.cos(t)) * (A @ A)


def camera(f, centre, R=None, pp=(320.0, 240.0)):
    """-> (K [3,3], T_cam_from_world [4,4]) of a camera at `centre` with rotation R (camera from world)."""
    R = np.eye(3) if R is None else R
    K = np.array([[f, 0, pp[0]], [0, f, pp[1]], [0, 0, 1.0]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ np.asarray(centre, np.float64)
    return K, T


def project(K, T, X):
    p = K @ (T[:3, :3] @ np.asarray(X, np.float64) + T[:3, 3])
    return p[:2] / p[2]


# ---- seeded scenes with ground truth ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(seed=3, n_tracks=405):
    """12 cameras (f in [450, 650], principal point (320, 240), rotations up to 20 degrees about random axes, centres in
    [-2,2] x [-1,1] x [-0.5,0.5]), points in [-2,2] x [-1.5,1.5] x [3,8], 0.5 px Gaussian noise, outliers displaced 15-80 px at positions
    >= 2 of a track at rate 0, 0.2 or 0.4, lengths cycling through LENGTHS (n_tracks = 405: 45 tracks of every length, 15 per rate).
    -> dict(offsets, obs_image, obs_xy, K, T, X_true [T,3], true_inlier [N] bool)."""
    rng = np.random.default_rng(seed)
    cams = []
    for _ in range(12):
        c = rng.uniform([-2, -1, -0.5], [2, 1, 0.5])
        cams.append(camera(rng.uniform(450, 650), c, rotation(rng.standard_normal(3), rng.uniform(0, 20))))
    K, T = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    offsets, image, xy, truth, X_true = [0], [], [], [], []
    for t in range(n_tracks):
        L, rate = LENGTHS[t % len(LENGTHS)], RATES[(t // len(LENGTHS)) % len(RATES)]
        X = rng.uniform([-2, -1.5, 3], [2, 1.5, 8])
        ims = rng.permutation(12)[:L] if L <= 12 else rng.integers(0, 12, L)
        for pos, im in enumerate(ims):
            p = project(K[im], T[im], X) + 0.5 * rng.standard_normal(2)
            out = pos >= 2 and rng.random() < rate
            if out:
                ang = rng.uniform(0, 2 * np.pi)
                p = p + rng.uniform(15, 80) * np.array([np.cos(ang), np.sin(ang)])
            image.append(im); xy.append(p); truth.append(not out)
        offsets.append(len(image))
        X_true.append(X)
    return dict(offsets=np.array(offsets, np.int64), obs_image=np.array(image, np.int32), obs_xy=np.array(xy, np.float32), K=K, T=T,
                X_true=np.array(X_true), true_inlier=np.array(truth, bool))


def ground_truth_figures(s, got):
    """scene() and the library's result on it (to_host() dict) -> the figures of the ground-truth check, for tracks with L >= 4:
    share of tracks whose final mask equals the true inlier set, and, where there is a point, the worst RMS reprojection error over the
    TRUE inliers relative to the Gauss-Newton optimum over the true inliers (the oracle's, 50 steps from the true point) -- measured
    against that optimum, never against the library."""
    import _triangulation_oracle as O
    off = s["offsets"]
    cams = [O.Camera(k, t) for k, t in zip(s["K"], s["T"])]
    long_tracks = [t for t in range(len(off) - 1) if off[t + 1] - off[t] >= 4]
    same = [t for t in long_tracks if np.array_equal(got["obs_inlier"][off[t]:off[t + 1]], s["true_inlier"][off[t]:off[t + 1]])]
    worst, n_ratio = 0.0, 0
    for t in long_tracks:
        if got["status"][t] != 0:
            continue
        sl = slice(off[t], off[t + 1])
        tc, xy, truth = [cams[i] for i in s["obs_image"][sl]], s["obs_xy"][sl].astype(np.float64), s["true_inlier"][sl]
        opt = O.gauss_newton(tc, xy, truth, s["X_true"][t].copy(), 50)
        assert opt is not None, t
        ratio = O.reprojection_rms(tc, xy, truth, got["xyz"][t].astype(np.float64)) / O.reprojection_rms(tc, xy, truth, opt)
        worst, n_ratio = max(worst, ratio), n_ratio + 1
    return dict(n_tracks=len(off) - 1, n_long=len(long_tracks), n_same=len(same), share=len(same) / len(long_tracks), worst_ratio=worst,
                n_ratio=n_ratio)


def accuracy_report(f):
    return (f"triangulation against ground truth ({f['n_tracks']} tracks of tests/_triangulation_cases.py scene(), thresh 4 px, 1.5 degrees)\n"
            f"tracks with L >= 4: {f['n_long']}\n"
            f"final mask equals the true inlier set: {f['n_same']} of {f['n_long']} ({100 * f['share']:.2f} %; required >= 95 %)\n"
            f"worst RMS(result) / RMS(50-step Gauss-Newton optimum) over the true inliers, {f['n_ratio']} tracks with a point: "
            f"{f['worst_ratio']:.9f} (required <= 1.01; the result is rounded to float32)")


# ---- hand-written tracks ----------------------------------------------------------------------------------------------------------------
X0 = np.array([0.5, 0.25, 4.0])              # pixels (382.5, 271.25) in camera 0 and (257.5, 271.25) in camera 1: exact in float32
X1 = np.array([0.05, 0.0, 4.0])              # seen from cameras 0 and 6 under 2 atan(0.05 / 4) = 1.432 degrees, below the limit


def hand_cases():
    """-> (inputs dict, expect): expect[t] = dict(name, status, and optionally xyz, n_inliers, mask).  One call holds all the tracks, so that
    the bad cameras sit next to healthy tracks."""
    cams = [camera(500, (0, 0, 0)),                                              # 0  A
            camera(500, (1, 0, 0)),                                              # 1  B
            camera(500, (0.001, 0, 0)),                                          # 2  C: 0.014 degrees from A at depth 4
            camera(500, (0, 0, 10)),                                             # 3  D: looks along +z from behind the points
            camera(520, (-1, 0.5, 0), rotation((0, 1, 0), 10)),                  # 4  E
            camera(480, (0.5, -1, 0.2), rotation((1, 0.2, 0), -12)),             # 5  F
            camera(500, (0.1, 0, 0)),                                            # 6  H: 1.432 degrees from A at X1
            camera(500, (2, 0, 0)),                                              # 7  G
            camera(500, (1, 1, 0)),                                              # 8  fx = 0 below
            camera(500, (1, -1, 0))]                                             # 9  NaN in t below
    K, T = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    K[8, 0, 0] = 0.0
    T[9, 1, 3] = np.nan
    P = lambda im, X, d=(0, 0): project(cams[im][0], cams[im][1], X) + np.asarray(d, np.float64)
    OK, TOO_SHORT, NO_HYP, SMALL, BAD = range(5)
    tracks = [
        ("two exact rays", [(0, P(0, X0)), (1, P(1, X0))], dict(status=OK, xyz=X0, n_inliers=2, mask=[1, 1])),
        ("parallel rays", [(0, (320, 240)), (1, (320, 240))], dict(status=NO_HYP)),
        ("point behind one camera", [(0, P(0, X0)), (3, P(3, X0))], dict(status=NO_HYP)),
        ("both observations in one image", [(0, P(0, X0)), (0, P(0, X0, (30, 0)))], dict(status=NO_HYP)),
        ("angle below the limit at the hypothesis", [(0, P(0, X0)), (2, P(2, X0))], dict(status=NO_HYP)),
        # the rays of A and H differ by 1.432 degrees across and, through the 6 px gap, 0.69 degrees along v: 1.589 degrees between the
        # RAYS, so the hypothesis passes (the midpoint of the skew rays sits at depth 3.25 with residuals of 3.33 px; the refit brings the
        # point back to depth 4 with 3 px each); the third observation is an outlier; the final angle at X is 1.432 degrees
        ("only surviving inlier pair is narrow", [(0, P(0, X1, (0, -3.0))), (6, P(6, X1, (0, 3.0))), (1, P(1, X1, (0, 60)))],
         dict(status=SMALL, n_inliers=2)),
        ("one outlier among five", [(0, P(0, X0)), (1, P(1, X0)), (4, P(4, X0)), (5, P(5, X0, (25, -30))), (7, P(7, X0))],
         dict(status=OK, xyz=X0, n_inliers=4, mask=[1, 1, 1, 0, 1])),
        ("one observation", [(0, P(0, X0))], dict(status=TOO_SHORT)),
        ("no observation", [], dict(status=TOO_SHORT)),
        ("camera with fx = 0", [(0, P(0, X0)), (8, (300, 200)), (1, P(1, X0))], dict(status=BAD)),
        ("camera with a NaN in t", [(9, (300, 200)), (1, P(1, X0))], dict(status=BAD)),
        ("two exact rays again", [(1, P(1, X0)), (0, P(0, X0))], dict(status=OK, xyz=X0, n_inliers=2, mask=[1, 1])),
    ]
    offsets, image, xy, expect = [0], [], [], []
    for name, obs, exp in tracks:
        for im, p in obs:
            image.append(im); xy.append(p)
        offsets.append(len(image))
        expect.append(dict(name=name, **exp))
    inputs = dict(offsets=np.array(offsets, np.int64), obs_image=np.array(image, np.int32),
                  obs_xy=np.array(xy, np.float32).reshape(-1, 2), K=K, T=T)
    return inputs, expect


def check_hand(res, expect):
    """res: dict of numpy arrays (xyz, n_inliers, status, obs_inlier) + offsets; asserts what hand_cases() promises."""
    off = res["offsets"]
    counts = [0] * 5
    for t, e in enumerate(expect):
        mask = res["obs_inlier"][off[t]:off[t + 1]]
        assert res["status"][t] == e["status"], (e["name"], int(res["status"][t]))
        counts[e["status"]] += 1
        if e["status"] != 0:
            assert np.isnan(res["xyz"][t]).all() and not mask.any(), e["name"]
        if "n_inliers" in e:
            assert res["n_inliers"][t] == e["n_inliers"], (e["name"], int(res["n_inliers"][t]))
        if "mask" in e:
            assert mask.astype(int).tolist() == e["mask"], (e["name"], mask)
        if "xyz" in e and len(e.get("mask", ())) == 2:                           # exact pixels: the point itself after the fp32 rounding
            assert np.array_equal(res["xyz"][t], e["xyz"].astype(np.float32)), (e["name"], res["xyz"][t])
        elif "xyz" in e:                                                          # pixels rounded to fp32 (3e-5 px): 1e-5 of the depth is ample
            assert np.abs(res["xyz"][t] - e["xyz"]).max() <= 4e-5, (e["name"], res["xyz"][t])
    return counts


# ---- a synthetic pair list of known 3D points for the atlas -----------------------------------------------------------------------------
SFM_HW, SFM_CELL = (1200.0, 1600.0), 2.0


@functools.lru_cache(maxsize=None)
def sfm_scene(seed=5, n_points=60):
    """5 cameras on a 4-unit baseline, 60 points in [-1.5,1.5] x [-1,1] x [4,7], every pair of images a row whose matches are the
    projections of the points snapped to the centres of the atlas's 2 px cells.
    -> dict(K, T, X, rows = [(a, b, k0 [M,2] f32, k1 [M,2] f32, conf [M] f32)])."""
    rng = np.random.default_rng(seed)
    cams = [camera(rng.uniform(450, 650), (x, rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)), rotation(rng.standard_normal(3), rng.uniform(0, 8)),
                   pp=(800.0, 600.0)) for x in (-2.0, -1.0, 0.0, 1.0, 2.0)]
    K, T = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    X = rng.uniform([-1.5, -1, 4], [1.5, 1, 7], (n_points, 3))
    snap = lambda p: (np.floor(p / SFM_CELL) * SFM_CELL + SFM_CELL / 2).astype(np.float32)
    px = [snap(np.stack([project(K[i], T[i], x) for x in X])) for i in range(5)]
    for p in px:
        assert (p > 0).all() and (p[:, 0] < SFM_HW[1]).all() and (p[:, 1] < SFM_HW[0]).all()
        assert len({tuple(q) for q in p.tolist()}) == n_points                    # no two points share a cell
    rows = [(a, b, px[a], px[b], rng.uniform(0.5, 1.0, n_points).astype(np.float32)) for a in range(5) for b in range(a + 1, 5)]
    return dict(K=K, T=T, X=X, rows=rows, px=px)


def run_atlas(device):
    """KeypointAtlas over sfm_scene() on `device` -> SfmResult."""
    import torch
    from loftr_amd import KeypointAtlas
    s = sfm_scene()
    atlas = KeypointAtlas(5, SFM_HW, SFM_CELL, device=device)
    dev = torch.device(device)
    for a, b, k0, k1, c in s["rows"]:
        data = {"mkpts0_f": torch.from_numpy(k0).to(dev), "mkpts1_f": torch.from_numpy(k1).to(dev), "mconf": torch.from_numpy(c).to(dev),
                "m_bids": torch.zeros(len(c), dtype=torch.int64, device=dev)}
        atlas.add(np.array([[a, b]]), data)
    return atlas.finalize()
