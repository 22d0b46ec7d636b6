"""Float64 numpy oracle for the absolute-pose estimators (csrc/absolute_pose.hip, csrc/absolute_pose_gpu.hip) and the lifting kernel,
written for the tests: the scene generators the tests and tools/micro/absolute_pose_accuracy.py share, the reprojection residual, a
Levenberg-Marquardt fit on a given inlier set (numerical rotation by Rodrigues' formula, solve by np.linalg), and the lifting arithmetic
of the reference's warp_kpts restated per operation.  Nothing here calls the library."""
import numpy as np

FRAME_W, FRAME_H = 640, 480
K_DEFAULT = np.array([[525.0, 0, 320], [0, 525.0, 240], [0, 0, 1]])


def rot(axis, ang):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def project(K, R, t, X):
    """Pixels [n,2] and depths [n] of the world points X [n,3] in the camera x_cam = R X + t."""
    Y = np.asarray(X, np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    p = Y @ np.asarray(K, np.float64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return p[:, :2] / p[:, 2:], Y[:, 2]


def residual(K, R, t, X, kpts):
    """Reprojection distance in pixels per match; inf where the point is not in front of the camera."""
    p, z = project(K, R, t, X)
    d = np.linalg.norm(p - np.asarray(kpts, np.float64), axis=1)
    return np.where(z > 0, d, np.inf)


def rotation_error_deg(R, R_gt):
    return float(np.degrees(np.arccos(np.clip((np.trace(np.asarray(R).T @ np.asarray(R_gt)) - 1) / 2, -1, 1))))


def fit_pose(K, X, kpts, R0, t0, iters=30):
    """Levenberg-Marquardt on the reprojection error over all the given matches, from (R0, t0) -> (R, t)."""
    K, X, kpts = np.asarray(K, np.float64), np.asarray(X, np.float64), np.asarray(kpts, np.float64)
    R, t, lam = np.array(R0, np.float64), np.array(t0, np.float64), 1e-6

    def cost_jac(R, t):
        Y = X @ R.T
        Xc = Y + t
        z = Xc[:, 2]
        pu = (K[0, 0] * Xc[:, 0] + K[0, 1] * Xc[:, 1]) / z + K[0, 2]
        pv = K[1, 1] * Xc[:, 1] / z + K[1, 2]
        r = np.r_[pu - kpts[:, 0], pv - kpts[:, 1]]
        o = np.zeros(len(X))
        gu = np.c_[K[0, 0] / z, K[0, 1] / z, -(K[0, 0] * Xc[:, 0] + K[0, 1] * Xc[:, 1]) / z ** 2]
        gv = np.c_[o, K[1, 1] / z, -K[1, 1] * Xc[:, 1] / z ** 2]
        J = np.r_[np.c_[np.cross(Y, gu), gu], np.c_[np.cross(Y, gv), gv]]
        return r, J

    r, J = cost_jac(R, t)
    for _ in range(iters):
        A, g = J.T @ J, J.T @ r
        d = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
        ang = np.linalg.norm(d[:3])
        Rn = (rot(d[:3], ang) if ang > 0 else np.eye(3)) @ R
        tn = t + d[3:]
        rn, Jn = cost_jac(Rn, tn)
        if rn @ rn <= r @ r:
            R, t, r, J, lam = Rn, tn, rn, Jn, max(lam / 10, 1e-12)
            if np.linalg.norm(d) < 1e-13:
                break
        else:
            lam *= 10
    return R, t


def make_scene(rng, n, noise_px=0.0, outliers=0.0, planar=False, thresh_px=3.0, K=K_DEFAULT):
    """n 2D-3D matches of one camera: intrinsics 525 / 320 / 240 on a 640 x 480 frame, depths 2-8 (near-planar: a tilted plane at depth
    about 5 with 1e-3 of relief), a rotation of at most 40 degrees, Gaussian pixel noise, and a fraction `outliers` of the matches with
    pixels drawn over the frame until they lie at least 10 x thresh_px from the true projection.  The 3D points are given in a frame
    rotated and shifted against the camera.  -> dict: X [n,3] f32, kpts [n,2] f32, K [3,3], R, t (float64 truth, x_cam = R X + t),
    clean [n,2] (noise-free projections of the float32 points), is_outlier [n] bool."""
    px = np.c_[rng.uniform(20, FRAME_W - 20, n), rng.uniform(20, FRAME_H - 20, n)]
    if planar:
        nrm = np.array([0.25 * rng.standard_normal(), 0.25 * rng.standard_normal(), 1.0])
        rays = np.c_[(px - K[:2, 2]) / np.array([K[0, 0], K[1, 1]]), np.ones(n)]
        z = 5.0 * nrm[2] / (rays @ nrm) + 1e-3 * rng.standard_normal(n)
    else:
        z = rng.uniform(2, 8, n)
    Xc = np.c_[(px - K[:2, 2]) / np.array([K[0, 0], K[1, 1]]) * z[:, None], z]
    R = rot(rng.standard_normal(3), np.radians(40) * rng.random())
    t = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.5, 0.5)])
    X = ((Xc - t) @ R).astype(np.float32)                      # x_cam = R X + t
    clean = project(K, R, t, X)[0]
    kpts = clean + noise_px * rng.standard_normal((n, 2))
    is_out = np.zeros(n, bool)
    k = int(round(outliers * n))
    if k:
        for i in rng.choice(n, k, replace=False):
            while True:
                cand = np.array([rng.uniform(0, FRAME_W), rng.uniform(0, FRAME_H)])
                if np.linalg.norm(cand - clean[i]) >= 10 * thresh_px:
                    kpts[i], is_out[i] = cand, True
                    break
    return dict(X=X, kpts=kpts.astype(np.float32), K=np.array(K, np.float64), R=R, t=t, clean=clean, is_outlier=is_out)


def make_adoption_scene(rng, thresh_px=3.0, n=260, big=45, small=15):
    """A noise-free scene whose refit is rejected by the adoption rule: the matches nearest to a corner of the frame form two clusters
    displaced to opposite sides of their true projections by 0.96 x thresh_px (`big` and `small` of them).  The exact pose holds
    every match as an inlier; the least-squares fit over all of them moves towards the big cluster and loses the small one."""
    sc = make_scene(rng, n)
    kpts = sc["clean"].copy()
    near = np.argsort(kpts[:, 0] + kpts[:, 1])[:big + small]
    sign = rng.permutation(np.r_[np.ones(big), -np.ones(small)])
    kpts[near, 0] += sign * 0.96 * thresh_px
    sc["kpts"] = kpts.astype(np.float32)
    return sc


def make_collinear_scene(n=60):
    """World points on one line, every coordinate exactly representable in float32 (multiples of 1 / 128), with consistent pixels."""
    s = np.arange(n, dtype=np.float64) / 16.0
    X = np.c_[-2.0 + s, -1.0 + 0.5 * s, 4.0 + 0.25 * s]
    return dict(X=X.astype(np.float32), kpts=project(K_DEFAULT, np.eye(3), np.zeros(3), X)[0].astype(np.float32), K=K_DEFAULT.copy())


# ---- lifting (the first half of the reference's warp_kpts, per operation in float32 / float64) -----------------------------------------
def lift(kpts, m_bids, depth, K, T=None, dtype=np.float32):
    """-> (pts3d [M,3], valid [M]).  Every product and sum is rounded on its own in `dtype`, in the order the header documents."""
    f = dtype
    kpts, depth, K = np.asarray(kpts, f), np.asarray(depth, f), np.asarray(K, f)
    M = len(kpts)
    P, dh, dw = depth.shape
    x, y = kpts[:, 0], kpts[:, 1]
    xr, yr = np.rint(x), np.rint(y)
    ok = (m_bids >= 0) & (m_bids < P) & (xr >= 0) & (xr < dw) & (yr >= 0) & (yr < dh)
    b = np.where(ok, m_bids, 0)
    d = np.where(ok, depth[b, np.where(ok, yr, 0).astype(np.int64), np.where(ok, xr, 0).astype(np.int64)], f(0))
    valid = d != 0
    k = K[b]
    with np.errstate(divide="ignore", invalid="ignore"):
        hx, hy = x * d, y * d
        Y = (hy - k[:, 1, 2] * d) / k[:, 1, 1]
        X = (hx - k[:, 0, 1] * Y - k[:, 0, 2] * d) / k[:, 0, 0]
        Z = d
        if T is not None:
            t = np.asarray(T, f)[b]
            X, Y, Z = (t[:, 0, 0] * X + t[:, 0, 1] * Y + t[:, 0, 2] * Z + t[:, 0, 3], t[:, 1, 0] * X + t[:, 1, 1] * Y + t[:, 1, 2] * Z + t[:, 1, 3],
                       t[:, 2, 0] * X + t[:, 2, 1] * Y + t[:, 2, 2] * Z + t[:, 2, 3])
    out = np.where(valid[:, None], np.c_[X, Y, Z], f(0)).astype(f)
    return out, valid
