"""Float64 numpy oracle for the 3D similarity estimators (csrc/similarity.hip, csrc/similarity_gpu.hip), the routine that moves a model
and the alignment of a reconstruction, written for the tests: Umeyama's closed form through numpy.linalg.svd, the residual, the scene
generators the tests and tools/micro/similarity_bench.py share, and the numpy formulae of a moved model.  Nothing here calls the library."""
import numpy as np


def rot(axis, ang):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def needs_reflection_fix(src, dst):
    """numpy's SVD of the cross-covariance returns det(U) det(V^T) < 0: without the diag(1, 1, -1) the product is a reflection."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    U, _, Vt = np.linalg.svd((dst - dst.mean(0)).T @ (src - src.mean(0)))
    return np.linalg.det(U) * np.linalg.det(Vt) < 0


def umeyama(src, dst, with_scale=True):
    """Least-squares (s, R, t) with dst ~ s R src + t (Umeyama 1991); s = 1 and the Kabsch rotation when with_scale is false."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    ms, md = src.mean(0), dst.mean(0)
    xs, xd = src - ms, dst - md
    U, D, Vt = np.linalg.svd(xd.T @ xs)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1
    R = U @ np.diag(S) @ Vt
    s = float((D * S).sum() / (xs ** 2).sum()) if with_scale else 1.0
    return s, R, md - s * R @ ms


def residual(s, R, t, src, dst):
    """|s R src + t - dst| per correspondence."""
    return np.linalg.norm(s * np.asarray(src, np.float64) @ np.asarray(R).T + t - np.asarray(dst, np.float64), axis=1)


def rotation_error_deg(R, R_gt):
    return float(np.degrees(np.arccos(np.clip((np.trace(np.asarray(R).T @ np.asarray(R_gt)) - 1) / 2, -1, 1))))


def random_similarity(rng, with_scale=True):
    return (float(rng.uniform(0.5, 2.0)) if with_scale else 1.0), rot(rng.standard_normal(3), np.pi * rng.random()), rng.uniform(-2, 2, 3)


def make_scene(rng, n, noise=0.0, outliers=0.0, with_scale=True, planar=False, thresh=0.05):
    """n correspondences: source points in a 6 x 4 x 4 box (coplanar: on a tilted plane through it), a random similarity (any rotation,
    scale 0.5-2 or 1, a shift of up to 2), Gaussian noise on every destination coordinate, and a fraction `outliers` of the destinations
    drawn over the destination's bounding box until they lie at least 10 x thresh from the true one.
    -> dict: src, dst [n,3] f64, s, R, t (truth), clean [n,3], is_outlier [n] bool."""
    src = np.c_[rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n)]
    if planar:
        src[:, 2] = 0.3 * src[:, 0] - 0.2 * src[:, 1] + 0.5
    s, R, t = random_similarity(rng, with_scale)
    clean = s * src @ R.T + t
    dst = clean + noise * rng.standard_normal((n, 3))
    is_out = np.zeros(n, bool)
    k = int(round(outliers * n))
    if k:
        lo, hi = clean.min(0) - 1, clean.max(0) + 1
        for i in rng.choice(n, k, replace=False):
            while True:
                cand = rng.uniform(lo, hi)
                if np.linalg.norm(cand - clean[i]) >= 10 * thresh:
                    dst[i], is_out[i] = cand, True
                    break
    return dict(src=src, dst=dst, s=s, R=R, t=t, clean=clean, is_outlier=is_out)


def make_adoption_scene(rng, thresh=0.05, n=260, big=45, small=15, with_scale=True):
    """A noise-free scene whose refit is rejected by the adoption rule (built like _absolute_pose_oracle.make_adoption_scene): the
    correspondences nearest to a corner of the source box form two clusters whose destinations are displaced to opposite sides by
    0.96 x thresh (`big` and `small` of them).  The exact model holds every correspondence as an inlier; the least-squares fit over all
    of them moves towards the big cluster and loses the small one."""
    sc = make_scene(rng, n, with_scale=with_scale)
    near = np.argsort(sc["src"].sum(1))[:big + small]
    sign = rng.permutation(np.r_[np.ones(big), -np.ones(small)])
    sc["dst"] = sc["clean"].copy()
    sc["dst"][near] += np.outer(sign * 0.96 * thresh, sc["R"][:, 0])         # along the image of the source's x axis
    return sc


def make_collinear_scene(n=60):
    """Source points on one line (every coordinate a multiple of 1 / 128), moved exactly: every sample is degenerate."""
    k = np.arange(n, dtype=np.float64) / 16.0
    src = np.c_[-2.0 + k, -1.0 + 0.5 * k, 4.0 + 0.25 * k]
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return dict(src=src, dst=2.0 * src @ R.T + np.array([1.0, 2.0, 3.0]))


# ---- a moved model, in numpy ------------------------------------------------------------------------------------------------------------
def transform_model(xyz, T, posed, s, R, t):
    """The float64 formulae of loftr_transform_model: X' = s R X + t; R_c' = R_c R^T, t_c' = s t_c - R_c' t for posed images, the
    input for the others -> (xyz' [N,3] f64, T' [n,4,4] f64)."""
    xyz, T = np.asarray(xyz, np.float64), np.asarray(T, np.float64)
    out = T.copy()
    for i in np.flatnonzero(posed):
        Rc = T[i, :3, :3] @ R.T
        out[i] = np.eye(4)
        out[i, :3, :3], out[i, :3, 3] = Rc, s * T[i, :3, 3] - Rc @ t
    return s * xyz @ R.T + t, out


def centres(T):
    return np.stack([-M[:3, :3].T @ M[:3, 3] for M in np.asarray(T, np.float64)])


def make_alignment_scene(T_true, rng, thresh, bad_fraction=0.25, unknown=1):
    """Reference positions for the cameras of a scene with true poses T_true [n,4,4]: the true centres moved by a random similarity
    (scale 0.5-2), `unknown` images without a position (NaN rows), and a share `bad_fraction` of ALL images, among the known ones, whose
    position is grossly wrong: displaced by 10-30 x thresh in a random direction.
    -> dict: ref [n,3], known [n] bool, bad [n] bool, s, R, t, T_ref [n,4,4] (the true poses in the reference frame)."""
    n = len(T_true)
    s, R, t = random_similarity(rng)
    ref = s * centres(T_true) @ R.T + t
    order = rng.permutation(n)
    known, bad = np.ones(n, bool), np.zeros(n, bool)
    known[order[:unknown]] = False
    bad[order[unknown:unknown + int(round(bad_fraction * n))]] = True
    for i in np.flatnonzero(bad):
        d = rng.standard_normal(3)
        ref[i] += d / np.linalg.norm(d) * thresh * rng.uniform(10, 30)
    ref[~known] = np.nan
    return dict(ref=ref, known=known, bad=bad, s=s, R=R, t=t, T_ref=transform_model(np.zeros((0, 3)), T_true, np.ones(n, bool), s, R, t)[1])
