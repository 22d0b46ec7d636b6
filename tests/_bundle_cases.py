"""Inputs shared by the bundle-adjustment tests (tests/test_bundle.py on the CPU, tests/test_hip_bundle.py on the GPU): the seeded
scenes with ground truth and perturbed poses, the Huber case, the hand-written problem and the synthetic edge problems."""
import functools

import numpy as np

from _triangulation_cases import camera, project, rotation, scene, sfm_scene

ARGS = ("offsets", "obs_image", "obs_xy", "obs_mask", "xyz", "K", "T_cam_from_world")


def perturbed(rng, K, T, X, tracks, noise_px=0.5, rot_deg=1.0, centre_sigma=0.05, point_sigma=0.05, n_fixed=2):
    """Observations of the points X [P,3] in the cameras listed per track (with Gaussian pixel noise), poses perturbed except for the
    first n_fixed (rotated by rot_deg about a random axis, centres moved by N(0, centre_sigma) per axis), points moved by
    N(0, point_sigma).  -> dict(inputs of bundle_adjust ..., fixed, T_true, X_true)."""
    offsets, image, xy = [0], [], []
    for X_t, cams in zip(X, tracks):
        for im in cams:
            image.append(im)
            xy.append(project(K[im], T[im], X_t) + noise_px * rng.standard_normal(2))
        offsets.append(len(image))
    T0 = T.copy()
    for i in range(n_fixed, len(K)):
        R = rotation(rng.standard_normal(3), rot_deg) @ T[i, :3, :3]
        centre = -T[i, :3, :3].T @ T[i, :3, 3] + centre_sigma * rng.standard_normal(3)
        T0[i, :3, :3], T0[i, :3, 3] = R, -R @ centre
    fixed = np.zeros(len(K), bool)
    fixed[:n_fixed] = True
    N = len(image)
    return dict(offsets=np.array(offsets, np.int64), obs_image=np.array(image, np.int32), obs_xy=np.array(xy, np.float32).reshape(N, 2),
                obs_mask=np.ones(N, bool), xyz=(X + point_sigma * rng.standard_normal(X.shape)).astype(np.float32), K=K.copy(),
                T_cam_from_world=T0, fixed=fixed, T_true=T.copy(), X_true=X.copy())


@functools.lru_cache(maxsize=None)
def scene_a(seed=11):
    """5 cameras on a 4-unit baseline (sfm_scene's), its 60 points at depth 4-7, track lengths 2-5, 0.5 px noise."""
    s, rng = sfm_scene(), np.random.default_rng(seed)
    tracks = [np.sort(rng.permutation(5)[:2 + t % 4]) for t in range(len(s["X"]))]
    return perturbed(rng, s["K"], s["T"], s["X"], tracks)


@functools.lru_cache(maxsize=None)
def scene_b(seed=12, n_points=200):
    """The 12 cameras of the triangulation scene, 200 points in [-2,2] x [-1.5,1.5] x [3,8], track lengths 2-6."""
    s, rng = scene(), np.random.default_rng(seed)
    X = rng.uniform([-2, -1.5, 3], [2, 1.5, 8], (n_points, 3))
    tracks = [np.sort(rng.permutation(12)[:2 + t % 5]) for t in range(n_points)]
    return perturbed(rng, s["K"], s["T"], X, tracks)


@functools.lru_cache(maxsize=None)
def scene_huber(seed=13):
    """scene_b with 5 % of the observations displaced by 15-40 px, all left in the mask."""
    s, rng = {k: v.copy() for k, v in scene_b().items()}, np.random.default_rng(seed)
    N = len(s["obs_image"])
    out = rng.permutation(N)[:N // 20]
    ang = rng.uniform(0, 2 * np.pi, len(out))
    s["obs_xy"][out] += (rng.uniform(15, 40, len(out))[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
    s["outlier"] = np.zeros(N, bool)
    s["outlier"][out] = True
    return s


def inputs(s):
    return [s[k] for k in ARGS]


def pose_errors(T, T_true, which):
    """-> (largest rotation error in degrees, largest centre error) over the cameras `which`."""
    rot, cen = 0.0, 0.0
    for i in np.nonzero(which)[0]:
        dR = T[i, :3, :3] @ T_true[i, :3, :3].T
        rot = max(rot, float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))))
        cen = max(cen, float(np.linalg.norm(T[i, :3, :3].T @ T[i, :3, 3] - T_true[i, :3, :3].T @ T_true[i, :3, 3])))
    return rot, cen


def projections(s, T, xyz, use):
    """pixels [M,2] of the observations `use` under the poses T and the points xyz."""
    track = np.repeat(np.arange(len(s["offsets"]) - 1), np.diff(s["offsets"]))
    return np.stack([project(s["K"][s["obs_image"][o]], T[s["obs_image"][o]], np.asarray(xyz[track[o]], np.float64)) for o in np.nonzero(use)[0]])


# ---- the hand-written problem: one call that holds the cases which can share one --------------------------------------------------------
def hand_problem(seed=21):
    """8 cameras: 0 and 1 fixed, 2-4 free, 5 with fx = 0, 6 without an observation, 7 behind the points looking along +z.  20 healthy
    points seen by cameras 0-4, then the special tracks.  -> (inputs dict, notes dict of the indices the test looks at)."""
    rng = np.random.default_rng(seed)
    cams = [camera(500, (-1.5, 0, 0)), camera(520, (1.5, 0.1, 0)), camera(480, (-0.5, 0.4, 0.1), rotation((0, 1, 0), 4)),
            camera(510, (0.5, -0.3, 0), rotation((1, 0, 0), -3)), camera(530, (0, 0.5, -0.1), rotation((0, 1, 1), 5)),
            camera(500, (1, 1, 0)), camera(500, (2, 2, 0)), camera(500, (0, 0, 10))]
    K, T = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    X = rng.uniform([-1, -0.8, 4], [1, 0.8, 7], (26, 3))
    tracks = [[0, 1, 2, 3, 4]] * 20 + [[0, 1, 2],            # 20: its observation in camera 2 is masked out
                                       [0, 3],               # 21: the observation in camera 0 is masked: one active observation left
                                       [0, 1, 4],            # 22: a NaN point
                                       [0, 1, 5],            # 23: camera 5 has fx = 0
                                       [0, 1, 7],            # 24: behind camera 7 at the start
                                       [2, 3, 4]]            # 25: free cameras only
    s = perturbed(rng, K, T, X, tracks)
    s["K"][5, 0, 0] = 0.0
    off = s["offsets"]
    s["obs_mask"][off[20] + 2] = False
    s["obs_mask"][off[21]] = False
    s["xyz"][22, 1] = np.nan
    s["obs_xy"][off[23] + 2] = (300, 200)
    s["obs_xy"][off[24] + 2] = (320, 240)
    notes = dict(masked=off[20] + 2, single=21, single_obs=(off[21], off[21] + 1), nan_point=22, nan_obs=(off[22], off[22] + 3),
                 bad_cam=5, bad_cam_obs=off[23] + 2, empty_cam=6, behind_cam=7, behind_obs=off[24] + 2)
    return s, notes


def exact_problem():
    """A start at the optimum with a cost of exactly 0: identity rotations, integer centres, f = 500 and points on a grid at depths 4
    and 8, so that every projection is exact in float64 and representable in float32."""
    cams = [camera(500, c) for c in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 1, 0))]
    K, T = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    X = np.array([(x, y, z) for z in (4.0, 8.0) for x in (-0.5, 0.0, 0.5, 1.0) for y in (-0.25, 0.0, 0.25)])
    s = perturbed(np.random.default_rng(0), K, T, X, [[0, 1, 2, 3]] * len(X), noise_px=0.0, rot_deg=0.0, centre_sigma=0.0, point_sigma=0.0)
    assert np.array_equal(s["obs_xy"].astype(np.float64), np.stack([project(K[i], T[i], x) for x in X for i in range(4)]))
    return s


# ---- synthetic problems for the edges of the kernels -----------------------------------------------------------------------------------
def ring(n_cams, seed):
    """n_cams cameras on a circle of radius 2 in the plane z = 0, looking along +z with small random rotations."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n_cams) / max(n_cams, 1)
    cams = [camera(rng.uniform(450, 650), (2 * np.cos(a), 1.2 * np.sin(a), rng.uniform(-0.2, 0.2)), rotation(rng.standard_normal(3), rng.uniform(0, 5)))
            for a in ang]
    return np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])


def synthetic(n_cams, tracks, seed=31, **kw):
    """Cameras of ring(), one point per entry of `tracks` (the list of cameras that see it) -> perturbed(...)."""
    rng = np.random.default_rng(seed)
    K, T = ring(n_cams, seed + 1)
    X = rng.uniform([-1, -0.8, 4], [1, 0.8, 7], (len(tracks), 3))
    return perturbed(rng, K, T, X, tracks, **kw)


def all_see_all(n_cams, n_tracks, **kw):
    return synthetic(n_cams, [list(range(n_cams))] * n_tracks, **kw)


def spread(n_free, n_tracks, seed=32):
    """Cameras 0 and 1 fixed and seen by every track; track j also sees free cameras 2 + j mod n_free and 2 + (7 j + 3) mod n_free."""
    tracks = [sorted({0, 1, 2 + j % n_free, 2 + (7 * j + 3) % n_free}) for j in range(n_tracks)]
    return synthetic(2 + n_free, tracks, seed=seed)
