"""Inputs shared by the view-overlap tests (tests/test_overlap.py on the CPU, tests/test_hip_overlap.py on the GPU): the seeded scenes, the
spoiled scenes, the hand-placed points on every boundary of the predicate, the empty tables, the size edges of the kernels and the ring
of the behavioural case.  A case is a dict of numpy arrays in the argument order of ops.view_overlap (ARGS) plus the three scalars."""
import functools
import math

import numpy as np
import torch

import _bundle_cases as BC
from _triangulation_cases import camera, rotation

ARGS = ("vis_offsets", "vis_point", "xyz", "point_ok", "K_src", "T_src", "src_ok", "K_tgt", "T_tgt", "tgt_ok", "tgt_hw")
SCALARS = ("border", "cos_min", "max_scale2")
COS45 = math.cos(math.radians(45.0))


def case(vis, xyz, src, tgt, tgt_hw, border=0.0, cos_min=COS45, max_scale2=4.0, point_ok=None, src_ok=None, tgt_ok=None):
    """vis: one list of point ids per source; src / tgt: lists of (K, T)."""
    n, m, T = len(src), len(tgt), len(xyz)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([len(v) for v in vis])
    stack = lambda cams, k, shape: np.stack([c[k] for c in cams]).astype(np.float64) if cams else np.zeros((0,) + shape)
    return dict(vis_offsets=offsets, vis_point=np.array([p for v in vis for p in v], np.int32), xyz=np.asarray(xyz, np.float32).reshape(T, 3),
                point_ok=np.ones(T, np.uint8) if point_ok is None else np.asarray(point_ok, np.uint8),
                K_src=stack(src, 0, (3, 3)), T_src=stack(src, 1, (4, 4)), src_ok=np.ones(n, np.uint8) if src_ok is None else np.asarray(src_ok, np.uint8),
                K_tgt=stack(tgt, 0, (3, 3)), T_tgt=stack(tgt, 1, (4, 4)), tgt_ok=np.ones(m, np.uint8) if tgt_ok is None else np.asarray(tgt_ok, np.uint8),
                tgt_hw=np.asarray(tgt_hw, np.float64).reshape(m, 2), border=float(border), cos_min=float(cos_min), max_scale2=float(max_scale2))


def oracle_args(c):
    return [c[k] for k in ARGS] + [c[k] for k in SCALARS]


def tensors(c, device="cpu"):
    """The arguments of ops.view_overlap: K as [n,9], T as [n,16]."""
    flat = {"K_src": 9, "T_src": 16, "K_tgt": 9, "T_tgt": 16}
    t = [torch.from_numpy(np.ascontiguousarray(c[k].reshape(len(c[k]), flat[k]) if k in flat else c[k])).to(device) for k in ARGS]
    return t + [c[k] for k in SCALARS]


# ---- seeded scenes ------------------------------------------------------------------------------------------------------------------
def _from_bundle(s, hw, **kw):
    n = len(s["K"])
    track = np.repeat(np.arange(len(s["offsets"]) - 1), np.diff(s["offsets"]))
    vis = [track[s["obs_image"] == i].tolist() for i in range(n)]
    cams = [(s["K"][i], s["T_true"][i]) for i in range(n)]
    return case(vis, s["X_true"], cams, cams, [hw] * n, **kw)


@functools.lru_cache(maxsize=None)
def scene_a():
    """Scene A of the bundle tests: 5 cameras (principal point (800, 600)), 60 points, each camera its own target."""
    return _from_bundle(BC.scene_a(), (1200.0, 1600.0), border=16.0)


@functools.lru_cache(maxsize=None)
def scene_b():
    """Scene B: 12 cameras (principal point (320, 240)), 200 points; a tight angle and scale so that every test of the predicate rejects."""
    return _from_bundle(BC.scene_b(), (480.0, 640.0), border=4.0, cos_min=math.cos(math.radians(20.0)), max_scale2=1.3 ** 2)


def spoiled():
    """Scene B with points that are not ok, NaN / inf coordinates, invalid and switched-off sources and targets, and bad extents."""
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in scene_b().items()}
    c["point_ok"][[3, 50, 51]] = 0
    c["xyz"][7, 0], c["xyz"][8, 1], c["xyz"][9, 2], c["xyz"][10] = np.nan, np.inf, -np.inf, np.nan
    c["K_src"], c["T_src"] = c["K_src"].copy(), c["T_src"].copy()
    c["K_src"][1, 0, 0] = 0.0                       # source 1: fx = 0
    c["T_src"][2, 1, 3] = np.nan                    # source 2: a NaN pose
    c["src_ok"][3] = 0
    c["K_tgt"][4, 1, 1] = np.inf                    # target 4: fy = inf
    c["T_tgt"][5, 0, 0] = np.nan
    c["tgt_ok"][6] = 0
    c["tgt_hw"][7] = (np.nan, 640.0)
    c["tgt_hw"][8] = (480.0, np.inf)
    c["tgt_hw"][9] = (0.0, 640.0)
    c["tgt_hw"][10] = (480.0, -640.0)
    return c


# ---- hand-placed points on the boundaries of the predicate --------------------------------------------------------------------------
# The source sits at the origin with identity rotation and f = 512; with z = 4 a point (x, y, 4) projects to (128 x + 320, 128 y + 240)
# in a target of the same pose: every product below is exact in float64 and every coordinate representable in float32.
SRC = camera(512.0, (0, 0, 0))
LOOK_MINUS_X = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])          # a camera whose axis is the world's -x


def hand_cases():
    """-> list of (name, case, expected overlap [n,m] or None)."""
    out = []
    xs = [-2.5, -2.5 - 2.0 ** -20, 2.5, 2.5 - 2.0 ** -20, -2.0, -2.0 - 2.0 ** -20, 2.0, 2.0 - 2.0 ** -20]
    pts = [(x, 0.0, 4.0) for x in xs] + [(0.0, y, 4.0) for y in (-1.875, -1.875 - 2.0 ** -20, 1.875, 1.875 - 2.0 ** -20, -1.375, 1.375)]
    vis = [list(range(len(pts)))]
    # u = 0, just below 0, u = W, just below W, u = 64, ..., u = 576; v = 0, just below, v = H, just below, v = 64, v = H - 64
    out.append(("image_edges", case(vis, pts, [SRC], [SRC], [(480.0, 640.0)], max_scale2=math.inf), [[1 + 1 + 4 + 1 + 1 + 2]]))
    out.append(("border_edges", case(vis, pts, [SRC], [SRC], [(480.0, 640.0)], border=64.0, max_scale2=math.inf), [[1 + 1 + 1]]))
    # z = 0 and z < 0: targets beside and beyond the point, looking along +z
    out.append(("z_zero", case([[0]], [(0.0, 0.0, 4.0)], [SRC], [camera(512.0, (1, 0, 4)), camera(512.0, (0, 0, 4)), camera(512.0, (0, 0, 5)),
                                                                  camera(512.0, (0, 0, 3))], [(480.0, 640.0)] * 4, cos_min=-1.0, max_scale2=math.inf),
                [[0, 0, 0, 1]]))
    # the angle at equality: a = (0,0,-4), b = (4,0,0), d = 0 = cos_min * sqrt(aa bb) with cos_min = 0; then just above 0
    side = camera(512.0, (4, 0, 4), LOOK_MINUS_X)
    for name, cm, want in (("angle_equal_0", 0.0, 1), ("angle_above_0", 2.0 ** -60, 0)):
        out.append((name, case([[0]], [(0.0, 0.0, 4.0)], [SRC], [side], [(480.0, 640.0)], cos_min=cm, max_scale2=math.inf), [[want]]))
    # a = (0,0,-4), b = (3,0,-4): d = 16, sqrt(aa bb) = 20, cos = 0.8; 0.8 * 20 rounds to 16 (equality), the next double above 0.8 does not
    wide = camera(512.0, (3, 0, 0), pp=(512.0, 240.0))
    for name, cm, want in (("angle_equal_08", 0.8, 1), ("angle_above_08", float(np.nextafter(0.8, 1.0)), 0), ("angle_below_08", 0.75, 1)):
        out.append((name, case([[0]], [(0.0, 0.0, 4.0)], [SRC], [wide], [(480.0, 1024.0)], cos_min=cm, max_scale2=math.inf), [[want]]))
    # the scale at equality: distances 4 and 8 at equal focals (ratio 2), focals 512 and 256 at equal distance (ratio 2), both ways round
    far, half = camera(512.0, (0, 0, -4)), camera(256.0, (0, 0, 0))
    # (the second source, `far`, sees both targets at ratio 1)
    for name, ms2, want in (("scale_equal", 4.0, [[1, 1], [1, 1]]), ("scale_below", float(np.nextafter(4.0, 0.0)), [[0, 0], [1, 1]]),
                            ("scale_inf", math.inf, [[1, 1], [1, 1]]), ("scale_one", 1.0, [[0, 0], [1, 1]])):
        out.append((name, case([[0], [0]], [(0.0, 0.0, 4.0)], [SRC, far], [far, half], [(480.0, 640.0)] * 2, cos_min=-1.0, max_scale2=ms2), want))
    return out


# ---- empty tables ---------------------------------------------------------------------------------------------------------------------
def empty_cases():
    b = scene_a()
    cams = [(b["K_src"][i], b["T_src"][i]) for i in range(5)]
    hw = [(1200.0, 1600.0)] * 5
    return [("empty_list", case([[0, 1, 2], [], [3, 4], [], []], b["xyz"], cams, cams, hw)),
            ("no_entries", case([[], [], [], [], []], b["xyz"], cams, cams, hw)),
            ("no_points", case([[], [], [], [], []], np.zeros((0, 3)), cams, cams, hw)),
            ("no_sources", case([], b["xyz"], [], cams, hw)),
            ("no_targets", case([[0, 1, 2], [], [3, 4], [], []], b["xyz"], cams, [], [])),
            ("nothing", case([], np.zeros((0, 3)), [], [], []))]


def bad_lists():
    """-> list of (name, case, expected error bits)."""
    out = []
    for name, edit, bits in (("point_high", lambda c: c["vis_point"].__setitem__(5, len(c["xyz"])), 1),
                             ("point_negative", lambda c: c["vis_point"].__setitem__(0, -1), 1),
                             ("offsets_start", lambda c: c["vis_offsets"].__setitem__(0, 1), 2),
                             ("offsets_end", lambda c: c["vis_offsets"].__setitem__(-1, len(c["vis_point"]) - 1), 2),
                             ("offsets_descend", lambda c: c["vis_offsets"].__setitem__(2, int(c["vis_offsets"][1]) - 1), 2),
                             ("offsets_beyond", lambda c: c["vis_offsets"].__setitem__(3, len(c["vis_point"]) + 7), 2),
                             ("both", lambda c: (c["vis_point"].__setitem__(9, -3), c["vis_offsets"].__setitem__(1, -2)), 3)):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in scene_a().items()}
        edit(c)
        out.append((name, c, bits))
    return out


# ---- seeded cases of a given size (the lane, wave, tile and chunk edges of the kernels) ---------------------------------------------
def _look_at(centre, f, rng, jitter_deg=6.0):
    z = -np.asarray(centre, np.float64) / np.linalg.norm(centre)
    x = np.cross(z, (0.0, 0.0, 1.0))
    x /= np.linalg.norm(x)
    R = rotation(rng.standard_normal(3), rng.uniform(0, jitter_deg)) @ np.stack([x, np.cross(z, x), z])
    return camera(f, centre, R)


def _ring(rng, count, radius=(3.0, 6.0)):
    ang = rng.uniform(0, 2 * np.pi, count)
    r = rng.uniform(*radius, count)
    return [_look_at((r[i] * np.cos(ang[i]), r[i] * np.sin(ang[i]), rng.uniform(-0.5, 0.5)), rng.uniform(400, 700), rng) for i in range(count)]


def sized(n, m, T, per_source, seed=0, unusable=0.0):
    """n sources and m targets around a ball of T points; every source lists `per_source` random points (an int, or one int per source);
    a share `unusable` of the points is not ok or not finite."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, 3))
    X *= (rng.uniform(0.2, 1.0, T) ** (1 / 3) / np.maximum(np.linalg.norm(X, axis=1), 1e-9))[:, None]
    ok = np.ones(T, np.uint8)
    bad = rng.random(T) < unusable
    ok[bad & (np.arange(T) % 2 == 0)] = 0
    X[bad & (np.arange(T) % 2 == 1), rng.integers(0, 3)] = np.nan
    per = [per_source] * n if isinstance(per_source, int) else list(per_source)
    vis = [rng.integers(0, max(T, 1), k).tolist() for k in per]
    return case(vis, X, _ring(rng, n), _ring(rng, m), [(480.0, 640.0)] * m, border=2.0, cos_min=math.cos(math.radians(60.0)), max_scale2=4.0,
                point_ok=ok)


def exactly_usable(count, seed=0, m=70):
    """One source whose list has exactly `count` usable entries, with unusable ones strewn between them."""
    rng = np.random.default_rng(seed + count)
    c = sized(1, m, max(2 * count, 8), 0, seed=seed)
    T = len(c["xyz"])
    c["point_ok"][T // 2:] = 0
    c["xyz"][T // 2:][::3] = np.nan
    good, badp = rng.integers(0, T // 2, count), rng.integers(T // 2, T, count // 3 + 1)
    lst = np.concatenate([good, badp]).astype(np.int32)
    rng.shuffle(lst)
    c["vis_point"], c["vis_offsets"] = lst, np.array([0, len(lst)], np.int64)
    return c


# ---- the behavioural case: a ring of cameras matched as an open chain -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ring_scene(n=24, radius=4.0, n_points=600, seed=1):
    """24 cameras on a ring of radius 4 looking at the origin (f = 500, 480 x 640), 600 points on the unit sphere; a camera sees a point
    inside its image whose normal faces it (normal . view direction > 0.3), at a keep rate of 0.7.  -> (case, existing [n-1,2])."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n_points, 3))
    X /= np.linalg.norm(X, axis=1)[:, None]
    cams, vis = [], []
    still = np.random.default_rng(0)
    for i in range(n):
        a = 2 * np.pi * i / n
        cams.append(_look_at((radius * np.cos(a), radius * np.sin(a), 0.0), 500.0, still, jitter_deg=0.0))
    for K, T in cams:
        c = -T[:3, :3].T @ T[:3, 3]
        pc = (T[:3, :3] @ X.T).T + T[:3, 3]
        uv = (K @ pc.T).T
        uv = uv[:, :2] / uv[:, 2:]
        view = c - X
        view /= np.linalg.norm(view, axis=1)[:, None]
        seen = (pc[:, 2] > 0) & (uv[:, 0] >= 0) & (uv[:, 0] < 640) & (uv[:, 1] >= 0) & (uv[:, 1] < 480) & ((X * view).sum(1) > 0.3)
        seen &= rng.random(n_points) < 0.7
        vis.append(np.nonzero(seen)[0].tolist())
    existing = np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.int64)
    return case(vis, X, cams, cams, [(480.0, 640.0)] * n), existing


def ring_reconstruction(device="cpu"):
    """The ring as a Reconstruction and the atlas it came from, as far as propose_pairs reads them: a track per point over the cameras
    that see it; camera 5 never got a pose, a few tracks have no point, a few observations are outliers.
    -> (rec, sfm, case with exactly the lists propose_pairs must build)."""
    import types
    from loftr_amd.registration import Reconstruction
    from loftr_amd.triangulation import Points3D
    c, existing = ring_scene()
    n, T = len(c["src_ok"]), len(c["xyz"])
    sees = np.zeros((T, n), bool)
    for i in range(n):
        sees[c["vis_point"][c["vis_offsets"][i]:c["vis_offsets"][i + 1]], i] = True
    track, image = np.nonzero(sees)                                                      # grouped by track, images ascending
    offsets = np.zeros(T + 1, np.int64)
    offsets[1:] = np.cumsum(sees.sum(1))
    N = len(image)
    status, inlier = np.zeros(T, np.uint8), np.ones(N, bool)
    status[::37], inlier[::11] = 2, False
    xyz = c["xyz"].copy()
    xyz[status != 0] = np.nan
    posed = np.ones(n, bool)
    posed[5] = False
    T_cam = c["T_src"].copy()
    T_cam[5] = np.nan
    dev = lambda a: torch.from_numpy(a).to(device)
    pts = Points3D({}, xyz=dev(xyz), n_inliers=dev(np.zeros(T, np.int32)), rms_px=dev(np.zeros(T, np.float32)), tri_cos=dev(np.zeros(T, np.float32)),
                   status=dev(status), obs_inlier=dev(inlier))
    pts.offsets, pts.image, pts.keypoint = dev(offsets), dev(image.astype(np.int32)), dev(np.zeros(N, np.int32))
    rec = Reconstruction(dev(T_cam), dev(posed), dev(np.zeros(n, np.int32)), pts, None, {}, K=dev(c["K_src"]))
    sfm = types.SimpleNamespace(row_images=dev(existing.astype(np.int32)), image_hw=(480.0, 640.0))
    use = inlier & (status[track] == 0)
    vis = [track[use & (image == i)].tolist() for i in range(n)]
    cams = [(c["K_src"][i], T_cam[i]) for i in range(n)]
    want = case(vis, xyz, cams, cams, [(480.0, 640.0)] * n, point_ok=status == 0, src_ok=posed, tgt_ok=posed)
    return rec, sfm, want


def ring_model(device="cpu"):
    """The ring as a LocalizationModel (the keypoints are the projections of the points a camera sees, one per 2 px cell, ordered by
    cell; every seventh has no 3D point) and 9 query views between and beside the database cameras.
    -> (model, K_db, T_db, K_query, T_query, query_hw, case with exactly the lists propose_for_poses must build)."""
    from loftr_amd.localization import LocalizationModel
    c, _ = ring_scene()
    n = len(c["src_ok"])
    kp_offsets, keypoints, kp_point, vis = [0], [], [], []
    for i in range(n):
        ids = c["vis_point"][c["vis_offsets"][i]:c["vis_offsets"][i + 1]]
        pc = (c["T_src"][i, :3, :3] @ c["xyz"][ids].astype(np.float64).T).T + c["T_src"][i, :3, 3]
        uv = ((c["K_src"][i] @ pc.T).T[:, :2] / pc[:, 2:]).astype(np.float32)
        cell = np.floor(uv[:, 1] * 0.5).astype(np.int64) * 320 + np.floor(uv[:, 0] * 0.5).astype(np.int64)
        cell, first = np.unique(cell, return_index=True)
        point = ids[first].astype(np.int32)
        point[::7] = -1
        keypoints.append(uv[first]), kp_point.append(point), kp_offsets.append(kp_offsets[-1] + len(first)), vis.append(point[point >= 0].tolist())
    rng = np.random.default_rng(3)
    queries = [_look_at((r * np.cos(a), r * np.sin(a), h), f, rng, jitter_deg=10.0)
               for a, r, h, f in zip(rng.uniform(0, 2 * np.pi, 9), rng.uniform(3.0, 5.0, 9), rng.uniform(-0.5, 0.5, 9), rng.uniform(400, 600, 9))]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    model = LocalizationModel(dev(np.array(kp_offsets, np.int64)), dev(np.concatenate(keypoints)), dev(np.concatenate(kp_point)), dev(c["xyz"]),
                              (480.0, 640.0), 2.0)
    Kq, Tq = np.stack([q[0] for q in queries]), np.stack([q[1] for q in queries])
    cams = [(c["K_src"][i], c["T_src"][i]) for i in range(n)]
    want = case(vis, c["xyz"], cams, queries, [(480.0, 640.0)] * 9)
    return model, dev(c["K_src"]), dev(c["T_src"]), dev(Kq), dev(Tq), (480.0, 640.0), want
