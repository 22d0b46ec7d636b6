"""Seeded synthetic view graphs for the calibration tests.

Cameras stand on a perturbed ring and each looks at its OWN random target near the origin, so the optical axes do not meet (axes
through one point are the known degenerate case of focal lengths from F; ``ring(..., degenerate=True)`` builds exactly that case).
The focals are distinct (or shared per camera id).  The F of an edge is a normalised eight-point fit over noisy projections of the
common points, rank 2 enforced, unit norm, rounded through float32 as the estimator's output is.  Edges go from every image to the
next ``k`` images; planted false edges are random rank-2 matrices."""
from types import SimpleNamespace

import numpy as np

W, H = 1000.0, 750.0


def look_at(c, target):
    z = target - c
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])                            # camera-from-world rotation


def eight_point(xa, xb):
    """x_b^T F x_a = 0 from pixel points [P,2]: Hartley normalisation, least squares, rank 2, unit norm, through float32."""
    def norm(x):
        c = x.mean(0)
        s = np.sqrt(2.0) / np.sqrt(((x - c) ** 2).sum(1)).mean()
        T = np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
        return np.c_[x, np.ones(len(x))] @ T.T, T
    a, Ta = norm(xa)
    b, Tb = norm(xb)
    A = (b[:, :, None] * a[:, None, :]).reshape(len(a), 9)
    Fn = np.linalg.svd(A)[2][-1].reshape(3, 3)
    U, S, Vt = np.linalg.svd(Fn)
    F = Tb.T @ (U @ np.diag([S[0], S[1], 0.0]) @ Vt) @ Ta
    return (F / np.linalg.norm(F)).astype(np.float32).astype(np.float64)


def random_rank2(rng):
    """A false edge: a random rank-2 matrix in pixel units (the epipoles anywhere), unit norm, through float32."""
    U, _, Vt = np.linalg.svd(rng.standard_normal((3, 3)))
    F = U @ np.diag([1.0, rng.uniform(0.2, 1.0), 0.0]) @ Vt
    S = np.diag([1.0 / W, 1.0 / W, 1.0])
    F = S @ F @ S
    return (F / np.linalg.norm(F)).astype(np.float32).astype(np.float64)


def ring(seed, n=12, k=3, noise=0.5, n_points=80, false_frac=0.0, camera_ids=None, degenerate=False, start=None, closed=True,
         f_range=(600.0, 1100.0), half=1.5):
    """-> SimpleNamespace(edge_image [E,2] i32, edge_F [E,3,3] f64, edge_weight [E] i32, pp [n,2] f64, f0 [n] f64, f_true [n] f64,
    camera_ids, planted [E] bool, n, R, c, X, xy)."""
    rng = np.random.default_rng(seed)
    ids = np.arange(n) if camera_ids is None else np.asarray(camera_ids)
    f_id = {i: rng.uniform(*f_range) for i in np.unique(ids)}
    f_true = np.array([f_id[i] for i in ids])
    ang = 2 * np.pi * (np.arange(n) + rng.uniform(-0.2, 0.2, n)) / n
    c = np.stack([6.0 * np.cos(ang) * rng.uniform(0.9, 1.1, n), rng.uniform(-1.0, 1.0, n), 6.0 * np.sin(ang) * rng.uniform(0.9, 1.1, n)], 1)
    target = np.zeros((n, 3)) if degenerate else rng.uniform(-1.0, 1.0, (n, 3))
    R = np.stack([look_at(c[i], target[i]) for i in range(n)])
    X = rng.uniform(-half, half, (n_points, 3))
    pp = np.tile([W / 2, H / 2], (n, 1))
    xy = np.zeros((n, n_points, 2))
    for i in range(n):
        pc = (X - c[i]) @ R[i].T
        xy[i] = f_true[i] * pc[:, :2] / pc[:, 2:3] + pp[i] + noise * rng.standard_normal((n_points, 2))
    pairs = []
    for i in range(n):
        for j in range(1, k + 1):
            if closed or i + j < n:
                pairs.append((i, (i + j) % n))
    pairs = [p for p in dict.fromkeys(pairs) if p[0] != p[1]]
    E = len(pairs)
    planted = np.zeros(E, bool)
    if false_frac > 0:
        planted[rng.choice(E, int(round(false_frac * E)), replace=False)] = True
    F = np.stack([random_rank2(rng) if planted[e] else eight_point(xy[a], xy[b]) for e, (a, b) in enumerate(pairs)]) if E else np.zeros((0, 3, 3))
    f0 = np.full(n, 1.2 * W) if start is None else f_true * (1.0 + start * np.where(np.arange(n) % 2 == 0, 1.0, -1.0))
    if camera_ids is not None and start is not None:
        f0 = f_true * (1.0 + start)
    return SimpleNamespace(edge_image=np.asarray(pairs, np.int32).reshape(-1, 2), edge_F=F, edge_weight=np.full(E, n_points, np.int32), pp=pp,
                           f0=f0, f_true=f_true, camera_ids=None if camera_ids is None else ids, planted=planted, n=n, R=R, c=c, X=X, xy=xy)


def small():
    """The smallest scene the status-code tests and the host check mirror: 5 images, every pair next to it."""
    return ring(1, n=5, k=2, noise=0.3, n_points=40)


# the general scenes: (name, keyword arguments of ring)
GENERAL = (("ring12", dict(seed=2, n=12, k=3, noise=0.5)),
           ("ring20_noise1", dict(seed=3, n=20, k=4, noise=1.0)),
           ("ring30", dict(seed=4, n=30, k=3, noise=0.5)),
           ("open16", dict(seed=5, n=16, k=3, noise=1.0, closed=False)))
# scenes with planted false edges (a quarter of the edges)
PLANTED = (("ring12_false", dict(seed=6, n=12, k=4, noise=0.5, false_frac=0.25)),
           ("ring30_false", dict(seed=7, n=30, k=4, noise=1.0, false_frac=0.25)))
SHARED = (("two_cameras", dict(seed=8, n=12, k=3, noise=0.5, camera_ids=[7, 7, 7, 7, 7, 7, 3, 3, 3, 3, 3, 3])),
          ("hub", dict(seed=9, n=16, k=3, noise=0.5, camera_ids=[5] * 13 + [40, 41, 42])))


DEGENERATE_SEEDS = (20, 21, 22)                 # ring(seed, n=12, k=3, noise=0.5, degenerate=True, start=0.1)


def lists(edge_image, group, G):
    """The incidence lists of the groups: (grp_offsets [G+1] i64, grp_inc [2E] i32), the stable ascending grouping."""
    key = np.asarray(group)[np.asarray(edge_image).reshape(-1)]
    inc = np.argsort(key, kind="stable").astype(np.int32)
    off = np.zeros(G + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(key, minlength=G))
    return off, inc


def compact(camera_ids, n):
    """camera ids -> (group [n] i32, G): dense groups ordered by their smallest member image; the identity without ids."""
    if camera_ids is None:
        return np.arange(n, dtype=np.int32), n
    ids = np.asarray(camera_ids)
    order = {}
    for v in ids.tolist():
        order.setdefault(v, len(order))
    return np.array([order[v] for v in ids.tolist()], np.int32), len(order)


def raw_args(sc):
    """The eight arrays of ops_calib.calibrate_view_graph_host for a scene."""
    group, G = compact(sc.camera_ids, sc.n)
    off, inc = lists(sc.edge_image, group, G)
    return [np.ascontiguousarray(sc.edge_image, np.int32), np.ascontiguousarray(sc.edge_F, np.float64), np.ascontiguousarray(sc.edge_weight, np.int32),
            np.ascontiguousarray(sc.pp, np.float64), np.ascontiguousarray(sc.f0, np.float64), group, off, inc]


def synthetic(E, n, seed=0, topology="path", one_camera=False):
    """A large seeded graph for the kernels' size edges: random rank-2 edges need no geometry.  topology 'path': edge e joins
    images e % (n - 1) and e % (n - 1) + 1; 'star': image 0 and 1 + e % (n - 1).  -> the eight raw arrays."""
    rng = np.random.default_rng(seed)
    e = np.arange(E)
    a = e % (n - 1) if topology == "path" else np.zeros(E, np.int64)
    b = a + 1 if topology == "path" else 1 + e % (n - 1)
    ei = np.stack([a, b], 1).astype(np.int32)
    flip = rng.random(E) < 0.5
    ei[flip] = ei[flip][:, ::-1]
    U, _, Vt = np.linalg.svd(rng.standard_normal((E, 3, 3)))
    S = np.zeros((E, 3, 3))
    S[:, 0, 0], S[:, 1, 1] = 1.0, rng.uniform(0.6, 1.0, E)
    F = U @ S @ Vt
    D = np.diag([1.0 / 800, 1.0 / 800, 1.0])
    F = D @ F @ D
    F = (F / np.linalg.norm(F, axis=(1, 2), keepdims=True)).astype(np.float32).astype(np.float64)
    group = np.zeros(n, np.int32) if one_camera else np.arange(n, dtype=np.int32)
    G = 1 if one_camera else n
    off, inc = lists(ei, group, G)
    return [np.ascontiguousarray(ei), F, rng.integers(1, 200, E).astype(np.int32), np.tile([W / 2, H / 2], (n, 1)),
            rng.uniform(700.0, 1300.0, n), group, off, inc]


# ---- an atlas for the end-to-end tests ---------------------------------------------------------------------------------------------------
ATLAS_HW, ATLAS_CELL = (int(H), int(W)), 2.0


def atlas_scene(device, seed=11, n=8, k=3, n_points=220):
    """A KeypointAtlas built from a ring scene: 8 images, every image paired with the next `k`, the matches of a row are the points
    that both images see, snapped to the centres of 2 px cells (so about 0.6 px of noise).  The principal points are the image centre
    and the pixels are square: what the calibration assumes holds.  -> (SfmResult on `device`, the scene with K_true and T_true)."""
    import torch
    from loftr_amd import KeypointAtlas
    sc = ring(seed, n=n, k=k, noise=0.0, n_points=n_points, f_range=(650.0, 950.0), half=1.3)
    snap = np.floor(sc.xy / ATLAS_CELL) * ATLAS_CELL + ATLAS_CELL / 2
    seen = (sc.xy[..., 0] > 1) & (sc.xy[..., 0] < W - 1) & (sc.xy[..., 1] > 1) & (sc.xy[..., 1] < H - 1)
    atlas = KeypointAtlas(n, ATLAS_HW, ATLAS_CELL, device=device)
    dev = torch.device(device)
    for a, b in sc.edge_image.tolist():
        both = np.nonzero(seen[a] & seen[b])[0]
        data = {"mkpts0_f": torch.from_numpy(snap[a][both].astype(np.float32)).to(dev), "mkpts1_f": torch.from_numpy(snap[b][both].astype(np.float32)).to(dev),
                "mconf": torch.full((len(both),), 0.9, dtype=torch.float32, device=dev), "m_bids": torch.zeros(len(both), dtype=torch.int64, device=dev)}
        atlas.add(np.array([[a, b]]), data)
    sc.K_true = np.zeros((n, 3, 3))
    sc.K_true[:, 0, 0] = sc.K_true[:, 1, 1] = sc.f_true
    sc.K_true[:, :2, 2], sc.K_true[:, 2, 2] = sc.pp, 1.0
    sc.T_true = np.tile(np.eye(4), (n, 1, 1))
    sc.T_true[:, :3, :3] = sc.R
    sc.T_true[:, :3, 3] = -np.einsum("nij,nj->ni", sc.R, sc.c)
    sc.n_seen = int(seen.all(0).sum())
    return atlas.finalize(), sc


def align_error(c, c_gt):
    """The largest distance between the centres c and the truth after the least-squares similarity (Umeyama) c -> c_gt."""
    a, g = c - c.mean(0), c_gt - c_gt.mean(0)
    U, sv, Vt = np.linalg.svd(g.T @ a)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    s = (sv * np.diag(D)).sum() / (a * a).sum()
    return float(np.linalg.norm(s * (U @ D @ Vt @ a.T).T - g, axis=1).max())


def reconstruction_errors(rec, sc):
    """(largest relative focal error of the final K, largest centre error after a similarity; the ring has radius 6) of a
    Reconstruction of atlas_scene's scene; every image must be posed."""
    T = rec.T_cam_from_world.cpu().numpy()
    K = rec.K.cpu().numpy()
    assert bool(rec.posed.all())
    c = -np.einsum("nji,nj->ni", T[:, :3, :3], T[:, :3, 3])
    f = 0.5 * (K[:, 0, 0] + K[:, 1, 1])
    return float(np.abs(f / sc.f_true - 1).max()), align_error(c, sc.c)


def spoiled(a, weight_every=7, nan_every=11):
    """The raw arrays `a` with invalid edges spread over the list: weight 0 on every 7th edge, a NaN in F on every 11th."""
    b = [x.copy() for x in a]
    b[2][::weight_every] = 0
    b[1][::nan_every, 1, 2] = np.nan
    return b


def error_cases(make):
    """Every error bit on the raw arrays that make() returns -> [(name, arrays, bit)]."""
    out = []

    def case(name, bit, i, idx, v):
        a = [x.copy() for x in make()]
        a[i][idx] = v(a) if callable(v) else v
        out.append((name, a, bit))

    n = len(make()[4])
    E = len(make()[0])
    case("image_outside", 1, 0, (E // 2, 1), n)
    case("image_negative", 1, 0, (E - 1, 0), -1)
    case("self_edge", 1, 0, (E // 2, slice(None)), 0)
    case("group_outside", 2, 5, n - 1, lambda a: len(a[6]) - 1)
    case("group_negative", 2, 5, 0, -1)
    case("slot_outside", 4, 7, 2 * E - 1, 2 * E)
    case("slot_negative", 4, 7, 0, -1)
    case("offsets_shifted", 4, 6, 1, lambda a: a[6][1] + 1)
    case("offsets_end", 4, 6, -1, lambda a: a[6][-1] - 1)
    case("focal_zero", 8, 4, n // 2, 0.0)
    case("focal_nan", 8, 4, n - 1, np.nan)
    case("pp_infinite", 8, 3, (0, 1), np.inf)
    if E >= 2:
        a = [x.copy() for x in make()]
        k = int(a[6][np.argmax(np.diff(a[6]) >= 2)])                  # the first list with two slots: swap them
        a[7][[k, k + 1]] = a[7][[k + 1, k]]
        out.append(("slots_swapped", a, 4))
    return out
