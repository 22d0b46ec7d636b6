"""Seeded synthetic scenes for the global-positioning tests (tests/test_position.py, tests/test_hip_position.py): cameras on a ring or on
a straight line looking at a cloud of points, tracks in CSR form, pixel noise, rotation noise, gross outliers, and a spanning tree (a
path, or a star) with the true translation direction of each of its pairs."""
import numpy as np

from _scenes import random_rotation

F, CX, CY = 500.0, 320.0, 240.0


def look_at(centre, target):
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x = x / np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])                    # camera-from-world


class Scene:
    """The arguments of loftr_amd.global_positions in order (``args``), the truth (c_gt [n,3], X_gt [T,3]) and the planted outliers
    (outlier [N] bool)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def args(self):
        return [self.offsets, self.obs_image, self.obs_xy, self.K, self.R, self.in_graph, self.root, self.tree_image, self.tree_t]


def make_scene(name, n, T, seed, shape="ring", noise_px=0.5, rot_noise_deg=0.0, outliers=0.0, per_point=None, tree="path", obs_per_cam=None):
    """n cameras (ring of radius 6 around the cloud, or a line along x at distance 6 from it), T points in a unit-ish cloud; every point
    is seen by `per_point` cameras (all when None); `outliers`: the share of observations whose pixels are replaced by random ones."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.5, 1.5, size=(T, 3))
    if shape == "ring":
        ang = 2 * np.pi * np.arange(n) / max(n, 1)
        c = np.stack([6 * np.cos(ang), 0.3 * np.sin(3 * ang), 6 * np.sin(ang)], 1)
        R = np.stack([look_at(ci, np.zeros(3)) for ci in c]) if n else np.zeros((0, 3, 3))
    else:
        c = np.stack([np.linspace(-3, 3, n) if n > 1 else np.zeros(1), np.zeros(n), np.full(n, -6.0)], 1)
        R = np.stack([look_at(ci, np.array([0.3 * ci[0], 0.0, 0.0])) for ci in c])
    K = np.tile(np.array([[F, 0, CX], [0, F, CY], [0, 0, 1.0]]), (n, 1, 1))
    offsets, image, xy, outl = [0], [], [], []
    for t in range(T):
        cams = np.arange(n) if per_point is None else np.sort(rng.choice(n, size=min(per_point, n), replace=False))
        # at most ONE outlier per track (with probability outliers * length, so the share of observations is `outliers`): a loss on the
        # residual can single out an observation only against a majority of its track; a track with half of its pixels random is lost to
        # any method and says nothing about this one
        planted = rng.integers(len(cams)) if rng.uniform() < outliers * len(cams) else -1
        for k, i in enumerate(cams):
            p = K[i] @ (R[i] @ (X[t] - c[i]))
            px = p[:2] / p[2] + rng.normal(size=2) * noise_px
            bad = k == planted
            if bad:                                             # gross: at least 200 px away, a chord of 0.24 = 200 * 500 / (500^2 + 400^2)
                far = px                                        # even in a corner of the image, more than twice the default huber
                while np.linalg.norm(far - px) < 200.0:
                    far = rng.uniform([0, 0], [2 * CX, 2 * CY])
                px = far
            image.append(i); xy.append(px); outl.append(bad)
        offsets.append(len(image))
    R_in = R.copy()
    if rot_noise_deg > 0:
        for i in range(1, n):
            R_in[i] = random_rotation(rng, rot_noise_deg) @ R[i]
    pairs = [(i, i + 1) for i in range(n - 1)] if tree == "path" else [(0, i) if i % 2 else (i, 0) for i in range(1, n)]
    tree_t = np.array([(R[b] @ (c[a] - c[b])) * rng.uniform(0.5, 2.0) for a, b in pairs]).reshape(-1, 3)
    return Scene(name=name, offsets=np.array(offsets, np.int64), obs_image=np.array(image, np.int32).reshape(-1),
                 obs_xy=np.array(xy, np.float32).reshape(-1, 2), K=K, R=R_in, in_graph=np.ones(n, np.uint8), root=0,
                 tree_image=np.array(pairs, np.int32).reshape(-1, 2), tree_t=tree_t, c_gt=c, X_gt=X, outlier=np.array(outl, bool), n=n)


# the scenes of the accuracy tests: the prototype's sizes
def ring(seed=1, **kw):
    return make_scene("ring", 12, 150, seed, "ring", rot_noise_deg=0.5, outliers=0.07, per_point=6, **kw)


def line(seed=2, **kw):
    return make_scene("line", 10, 150, seed, "line", rot_noise_deg=0.5, outliers=0.07, per_point=6, **kw)


def exact(shape, seed=3):
    return make_scene("exact_" + shape, 10, 120, seed, shape, noise_px=0.0, per_point=5)


def small(seed=4, **kw):
    """The smallest scene the tests share: 5 cameras, 40 points."""
    return make_scene("small", 5, 40, seed, "ring", per_point=4, **kw)


def sized(N, n=3, seed=5, tree="path", seen_by=None):
    """A scene with exactly N observations: tracks of 2 over n cameras (over the cameras `seen_by` when given, so that the others have
    no observation at all), the last one of 3 when N is odd (N >= 2)."""
    rng = np.random.default_rng(seed)
    sc = make_scene(f"sized_{N}_{n}", n, 1, seed, "ring", tree=tree)
    T = N // 2
    X = rng.uniform(-1.5, 1.5, size=(T, 3))
    offsets, image, xy = [0], [], []
    pool = np.arange(n) if seen_by is None else np.asarray(seen_by)
    for t in range(T):
        k = 3 if (t == T - 1 and N % 2 and len(pool) >= 3) else 2
        cams = np.sort(rng.choice(pool, size=k, replace=False))
        for i in cams:
            p = sc.K[i] @ (sc.R[i] @ (X[t] - sc.c_gt[i]))
            image.append(i); xy.append(p[:2] / p[2] + rng.normal(size=2) * 0.5)
        offsets.append(len(image))
    sc.offsets, sc.obs_image, sc.obs_xy = np.array(offsets, np.int64), np.array(image, np.int32), np.array(xy, np.float32).reshape(-1, 2)
    sc.X_gt, sc.outlier = X, np.zeros(len(image), bool)
    return sc


def one_camera_list(count, seed=6, n=3):
    """n cameras; camera 1 has exactly `count` observations, every point is also seen by camera 0 and by one of the cameras 2 .. n - 1
    in turn."""
    rng = np.random.default_rng(seed)
    sc = make_scene(f"list_{count}_{n}", n, 1, seed, "ring")
    T = max(count, 4)
    X = rng.uniform(-1.5, 1.5, size=(T, 3))
    offsets, image, xy = [0], [], []
    for t in range(T):
        for i in ((0, 1, 2 + t % (n - 2)) if t < count else (0, 2 + t % (n - 2))):
            p = sc.K[i] @ (sc.R[i] @ (X[t] - sc.c_gt[i]))
            image.append(i); xy.append(p[:2] / p[2] + rng.normal(size=2) * 0.5)
        offsets.append(len(image))
    sc.offsets, sc.obs_image, sc.obs_xy = np.array(offsets, np.int64), np.array(image, np.int32), np.array(xy, np.float32).reshape(-1, 2)
    sc.X_gt, sc.outlier = X, np.zeros(len(image), bool)
    return sc


def many_cameras(n, tree, seed=7):
    """n cameras on a ring (a path or a star as the tree), 2 n points seen by 3 neighbouring cameras each."""
    rng = np.random.default_rng(seed)
    sc = make_scene(f"cams_{n}_{tree}", n, 1, seed, "ring", tree=tree)
    T = 2 * n
    X = rng.uniform(-1.5, 1.5, size=(T, 3))
    offsets, image, xy = [0], [], []
    for t in range(T):
        for i in sorted({(t // 2 + k) % n for k in range(3)}):
            p = sc.K[i] @ (sc.R[i] @ (X[t] - sc.c_gt[i]))
            image.append(i); xy.append(p[:2] / p[2] + rng.normal(size=2) * 0.5)
        offsets.append(len(image))
    sc.offsets, sc.obs_image, sc.obs_xy = np.array(offsets, np.int64), np.array(image, np.int32), np.array(xy, np.float32).reshape(-1, 2)
    sc.X_gt, sc.outlier = X, np.zeros(len(image), bool)
    return sc


def strip_camera(sc, cam):
    """The scene without the observations of camera `cam` (which stays in the graph and in the tree)."""
    keep = sc.obs_image != cam
    cnt = np.add.reduceat(keep.astype(np.int64), sc.offsets[:-1])
    cnt[np.diff(sc.offsets) == 0] = 0
    sc.offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    sc.obs_image, sc.obs_xy, sc.outlier = sc.obs_image[keep], sc.obs_xy[keep], sc.outlier[keep]
    return sc


def with_further_cases(sc, outside, empty=None, nan_step=7, nodir=(1, 3)):
    """The further cases applied to a scene of any size, all at once: every `nan_step`-th observation loses its x (so points with one
    usable observation and inactive observations sit anywhere in a wave or a chunk), camera `outside` (a leaf of the tree) leaves the
    graph with its edge, camera `empty` loses its observations (chained only), tree edge nodir[0] gets t = 0 and nodir[1] a t that is
    not finite."""
    if empty is not None:
        strip_camera(sc, empty)
    sc.obs_xy = sc.obs_xy.copy()
    sc.obs_xy[::nan_step, 0] = np.nan
    sc.tree_t = sc.tree_t.copy()
    sc.tree_t[nodir[0]] = 0.0
    sc.tree_t[nodir[1], 1] = np.inf
    touches = (sc.tree_image == outside).any(1)
    assert touches.sum() == 1 and outside != sc.root
    sc.in_graph = sc.in_graph.copy()
    sc.in_graph[outside] = 0
    sc.tree_image, sc.tree_t = sc.tree_image[~touches], sc.tree_t[~touches]
    sc.name += "_further"
    return sc


def large_further_cases():
    """The further cases at the sizes where the kernels take another path: 4097 observations (a chunk and a wave edge; camera 4 has no
    observation at all, so N is exact), a camera list of 4097, 1025 cameras as a path and as a star."""
    return [with_further_cases(sized(4097, n=6, seen_by=(0, 1, 2, 3, 5)), outside=5),
            with_further_cases(one_camera_list(4097, n=6), outside=5, empty=4),
            with_further_cases(many_cameras(1025, "path"), outside=1024, empty=512, nodir=(1, 700)),
            with_further_cases(many_cameras(1025, "star"), outside=1024, empty=512, nodir=(1, 700))]


# ---- the further cases: one change to the small scene each ----------------------------------------------------------------------------
def further_cases():
    out = []
    sc = strip_camera(small(), 4)                               # camera 4 loses its observations: chained only
    sc.name = "no_observations"
    out.append(sc)
    sc = small()                                                # a point with one usable observation: the others are not finite
    sc.obs_xy = sc.obs_xy.copy(); sc.obs_xy[sc.offsets[3] + 1:sc.offsets[4], 0] = np.nan; sc.name = "one_usable"
    out.append(sc)
    sc = small()                                                # images outside the graph: the last one, a leaf of the path
    sc.in_graph = sc.in_graph.copy(); sc.in_graph[4] = 0
    sc.tree_image, sc.tree_t, sc.name = sc.tree_image[:-1], sc.tree_t[:-1], "outside_graph"
    out.append(sc)
    sc = small()                                                # a tree edge with t = 0, another that is not finite
    sc.tree_t = sc.tree_t.copy(); sc.tree_t[1] = 0.0; sc.tree_t[3, 1] = np.inf; sc.name = "no_direction"
    out.append(sc)
    return out


def error_cases(base=small):
    """-> [(name, scene, the bit of counts[1] that must be set)]: every bit, on the scene base() (at least 5 cameras on a path)."""
    out = []

    def case(name, bit, edit):
        sc = base()
        for k in ("offsets", "obs_image", "in_graph", "tree_image", "tree_t"):
            setattr(sc, k, getattr(sc, k).copy())
        edit(sc)
        out.append((name, sc, bit))
    case("image_outside", 1, lambda s: s.obs_image.__setitem__(5, s.n))
    case("image_negative", 1, lambda s: s.obs_image.__setitem__(2, -1))
    case("offsets_descend", 2, lambda s: s.offsets.__setitem__(3, s.offsets[2] - 1))
    case("offsets_end", 2, lambda s: s.offsets.__setitem__(-1, s.offsets[-1] - 1))
    case("root_outside", 8, lambda s: setattr(s, "root", s.n))
    case("root_not_in_graph", 8, lambda s: s.in_graph.__setitem__(0, 0))
    case("edge_outside", 16, lambda s: s.tree_image.__setitem__((2, 1), s.n))
    case("edge_not_in_graph", 16, lambda s: s.in_graph.__setitem__(3, 0))
    case("end_reached_twice", 16, lambda s: s.tree_image.__setitem__(3, (1, 3)))         # (1, 3) next to (1, 2), (2, 3)
    case("cycle", 16, lambda s: setattr(s, "tree_image", np.concatenate([s.tree_image, [[0, 2]]]).astype(np.int32)) or
         setattr(s, "tree_t", np.concatenate([s.tree_t, [[1.0, 0, 0]]])))
    case("edge_never_reached", 16, lambda s: s.tree_image.__setitem__(0, (1, 2)))         # nothing leaves the root
    return out
