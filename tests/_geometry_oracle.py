"""Float64 numpy oracle for the homography / fundamental-matrix estimators (csrc/geometry.hip, csrc/geometry_gpu.hip), written for the
tests: Hartley normalisation, null spaces by np.linalg.svd, the library's residual definitions restated from their formulas, and the
scene generators the tests and tools/micro/geometry_accuracy.py share.  Nothing here calls the library."""
import numpy as np

FRAME_W, FRAME_H = 640, 480


# ---- normalisation, fits ------------------------------------------------------------------------------------------------------
def hartley(p):
    """T with T [x, y, 1] = normalised point: centroid 0, mean distance sqrt 2."""
    c = p.mean(0)
    s = np.sqrt(2.0) / np.linalg.norm(p - c, axis=1).mean()
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def _h(p):
    return np.c_[p, np.ones(len(p))]


def unit(m):
    """Unit Frobenius norm, the entry of largest magnitude positive (removes scale and sign before a comparison)."""
    m = np.asarray(m, np.float64) / np.linalg.norm(m)
    return m * np.sign(m.ravel()[np.abs(m).argmax()])


def fit_homography(p0, p1):
    """Normalised DLT over all correspondences (>= 4): x1 ~ H x0."""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    T0, T1 = hartley(p0), hartley(p1)
    a, b = (_h(p0) @ T0.T)[:, :2], (_h(p1) @ T1.T)[:, :2]
    z, o = np.zeros(len(a)), np.ones(len(a))
    A = np.r_[np.c_[-a[:, 0], -a[:, 1], -o, z, z, z, b[:, 0] * a[:, 0], b[:, 0] * a[:, 1], b[:, 0]],
              np.c_[z, z, z, -a[:, 0], -a[:, 1], -o, b[:, 1] * a[:, 0], b[:, 1] * a[:, 1], b[:, 1]]]
    Hn = np.linalg.svd(A)[2][-1].reshape(3, 3)
    return unit(np.linalg.inv(T1) @ Hn @ T0)


def fit_fundamental(p0, p1):
    """Normalised eight-point algorithm over all correspondences (>= 8) with the rank-2 projection: x1^T F x0 = 0."""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    T0, T1 = hartley(p0), hartley(p1)
    a, b = (_h(p0) @ T0.T)[:, :2], (_h(p1) @ T1.T)[:, :2]
    A = np.c_[b[:, 0] * a[:, 0], b[:, 0] * a[:, 1], b[:, 0], b[:, 1] * a[:, 0], b[:, 1] * a[:, 1], b[:, 1], a[:, 0], a[:, 1], np.ones(len(a))]
    Fn = np.linalg.svd(A)[2][-1].reshape(3, 3)
    U, s, Vt = np.linalg.svd(Fn)
    Fn = U @ np.diag([s[0], s[1], 0.0]) @ Vt
    return unit(T1.T @ Fn @ T0)


# ---- residuals (pixels) -------------------------------------------------------------------------------------------------------
def transfer_distance(H, p0, p1):
    """|x1 - pi(H x0)| per correspondence; inf where H x0 has a non-positive third coordinate for the sign of H that makes the
    majority positive."""
    q = _h(np.asarray(p0, np.float64)) @ np.asarray(H, np.float64).T
    if (q[:, 2] > 0).sum() < (q[:, 2] < 0).sum():
        q = -q
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.linalg.norm(q[:, :2] / q[:, 2:] - np.asarray(p1, np.float64), axis=1)
    return np.where(q[:, 2] > 0, d, np.inf)


def sampson_distance(F, p0, p1):
    """sqrt of (x1^T F x0)^2 / ((F x0)_0^2 + (F x0)_1^2 + (F^T x1)_0^2 + (F^T x1)_1^2) per correspondence."""
    F = np.asarray(F, np.float64)
    h0, h1 = _h(np.asarray(p0, np.float64)), _h(np.asarray(p1, np.float64))
    l, m = h0 @ F.T, h1 @ F
    r = np.sum(h1 * l, 1)
    return np.abs(r) / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2)


def residual(model, mat, p0, p1):
    return transfer_distance(mat, p0, p1) if model == "homography" else sampson_distance(mat, p0, p1)


def corner_error(H, H_gt, hw=(FRAME_H, FRAME_W)):
    h, w = hw
    c = np.array([[0, 0, 1], [w - 1, 0, 1], [w - 1, h - 1, 1], [0, h - 1, 1]], np.float64)
    a, b = c @ np.asarray(H, np.float64).T, c @ np.asarray(H_gt, np.float64).T
    return float(np.linalg.norm(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:], axis=1).mean())


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def _rot(axis, ang):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def random_homography(rng, jitter=80.0):
    """The homography that moves the four corners of the frame by up to `jitter` pixels each (orientation preserving, positive third
    coordinate over the frame)."""
    c = np.array([[0, 0], [FRAME_W, 0], [FRAME_W, FRAME_H], [0, FRAME_H]], np.float64)
    return fit_homography(c, c + rng.uniform(-jitter, jitter, (4, 2)))


def random_two_view(rng, n):
    """n 3-D points in front of two cameras -> (p0, p1 pixels [n,2], F with x1^T F x0 = 0)."""
    K0 = np.array([[580.0, 0, 320], [0, 585.0, 240], [0, 0, 1]])
    K1 = np.array([[575.0, 0, 318], [0, 578.0, 243], [0, 0, 1]])
    R = _rot(rng.standard_normal(3), 0.1 + 0.4 * rng.random())
    t = rng.standard_normal(3)
    t /= np.linalg.norm(t)
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)]
    Y = X @ R.T + t
    p0, p1 = (X / X[:, 2:]) @ K0.T, (Y / Y[:, 2:]) @ K1.T
    F = np.linalg.inv(K1).T @ np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R @ np.linalg.inv(K0)
    return p0[:, :2], p1[:, :2], unit(F)


def make_pair(rng, model, n, noise_px=0.0, outliers=0.0, thresh_px=1.0):
    """One pair with n matches (float32 pixels): the true model, Gaussian noise of noise_px per coordinate on both images, and a
    fraction `outliers` of the matches with image-1 points drawn over the frame until they lie at least 10 x thresh_px from the true
    model's prediction (the oracle's residual).  -> p0, p1 [n,2] f32, true matrix [3,3], is_outlier [n] bool."""
    if model == "homography":
        mat = random_homography(rng)
        p0 = np.c_[rng.uniform(0, FRAME_W, n), rng.uniform(0, FRAME_H, n)]
        q = _h(p0) @ mat.T
        p1 = q[:, :2] / q[:, 2:]
    else:
        p0, p1, mat = random_two_view(rng, n)
    p0 = p0 + noise_px * rng.standard_normal((n, 2))
    p1 = p1 + noise_px * rng.standard_normal((n, 2))
    is_out = np.zeros(n, bool)
    k = int(round(outliers * n))
    if k:
        sel = rng.choice(n, k, replace=False)
        for i in sel:
            # (a match whose image-0 point lies at the epipole agrees with every image-1 point: after 200 draws it stays an inlier)
            is_out[i] = False
            for _ in range(200):
                cand = np.array([rng.uniform(0, FRAME_W), rng.uniform(0, FRAME_H)]).astype(np.float32)
                if residual(model, mat, p0[i:i + 1].astype(np.float32), cand[None])[0] >= 10 * thresh_px:
                    p1[i], is_out[i] = cand, True
                    break
    return p0.astype(np.float32), p1.astype(np.float32), mat, is_out


def make_adoption_pair(rng, model, thresh_px, n=260, big=45, small=15):
    """A noise-free pair whose refit is rejected by the adoption rule: the matches nearest to a corner of image 0 form two clusters
    displaced to opposite sides of the true model by 0.96 x thresh_px (`big` and `small` of them).  The exact model holds every match
    as an inlier; the least-squares fit over all of them moves towards the big cluster and loses the small one.
    -> p0, p1 [n,2] f32, true matrix."""
    if model == "homography":
        mat = random_homography(rng)
        p0 = np.c_[rng.uniform(0, FRAME_W, n), rng.uniform(0, FRAME_H, n)]
        q = _h(p0) @ mat.T
        p1 = q[:, :2] / q[:, 2:]
        normal = np.tile([[1.0, 0.0]], (n, 1))
    else:
        p0, p1, mat = random_two_view(rng, n)
        l = _h(p0) @ mat.T                                        # epipolar lines in image 1
        normal = l[:, :2] / np.linalg.norm(l[:, :2], axis=1, keepdims=True)
    near = np.argsort(p0[:, 0] + p0[:, 1])[:big + small]
    sign = rng.permutation(np.r_[np.ones(big), -np.ones(small)])            # the two clusters share one region
    for i, sg in zip(near, sign):
        step = normal[i] * sg
        unit_res = residual(model, mat, p0[i:i + 1], p1[i:i + 1] + step)[0]         # residual of a one-pixel displacement
        p1[i] = p1[i] + step * (0.96 * thresh_px / unit_res)
    return p0.astype(np.float32), p1.astype(np.float32), mat
