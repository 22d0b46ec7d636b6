"""An independent statement of bundle adjustment for the tests (numpy float64): rotation matrices updated by Rodrigues' formula, one dense
Jacobian of all residuals with respect to all free parameters, dense damped normal equations solved by np.linalg.solve, the same loss
(squared or Huber, the latter by iteratively reweighted least squares).  It shares no formula text with csrc/bundle_core.h: no quaternions,
no Schur complement, no conjugate gradients, no ordered sums.  Run to ftol = 1e-14 or 100 iterations it stands for "the optimum"."""
import numpy as np


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rodrigues(w):
    """exp of the rotation vector w."""
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3) + hat(w)
    A = hat(w / th)
    return np.eye(3) + np.sin(th) * A + (1.0 - np.cos(th)) * (A @ A)


def pixels(K, R, t, X):
    y = K @ (R @ X + t)
    return y[:2] / y[2]


def huber_cost(r, delta):
    """r [M,2] -> sum of the loss."""
    n = np.linalg.norm(r, axis=1)
    if delta <= 0:
        return float((n ** 2).sum())
    return float(np.where(n <= delta, n ** 2, 2 * delta * n - delta ** 2).sum())


class Problem:
    def __init__(self, offsets, image, xy, use, K, fixed):
        self.track = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
        self.obs = np.nonzero(use)[0]
        self.image, self.xy, self.K = image, xy.astype(np.float64), K
        self.free = [i for i in range(len(K)) if not fixed[i] and (image[self.obs] == i).any()]
        self.pts = sorted(set(self.track[self.obs].tolist()))
        self.col_c = {c: 6 * k for k, c in enumerate(self.free)}
        self.col_p = {p: 6 * len(self.free) + 3 * k for k, p in enumerate(self.pts)}
        self.n_par = 6 * len(self.free) + 3 * len(self.pts)

    def residuals(self, R, t, X):
        return np.stack([pixels(self.K[self.image[o]], R[self.image[o]], t[self.image[o]], X[self.track[o]]) - self.xy[o] for o in self.obs])

    def jacobian(self, R, t, X):
        J = np.zeros((2 * len(self.obs), self.n_par))
        for row, o in enumerate(self.obs):
            c, p = self.image[o], self.track[o]
            Y = R[c] @ X[p] + t[c]
            h = self.K[c] @ Y
            dpi = np.array([[1.0 / h[2], 0.0, -h[0] / h[2] ** 2], [0.0, 1.0 / h[2], -h[1] / h[2] ** 2]]) @ self.K[c]     # d pixel / d Y
            if c in self.col_c:
                J[2 * row:2 * row + 2, self.col_c[c]:self.col_c[c] + 3] = dpi @ (-hat(R[c] @ X[p]))
                J[2 * row:2 * row + 2, self.col_c[c] + 3:self.col_c[c] + 6] = dpi
            J[2 * row:2 * row + 2, self.col_p[p]:self.col_p[p] + 3] = dpi @ R[c]
        return J

    def moved(self, R, t, X, d):
        R, t, X = R.copy(), t.copy(), X.copy()
        for c, k in self.col_c.items():
            R[c] = rodrigues(d[k:k + 3]) @ R[c]
            t[c] = t[c] + d[k + 3:k + 6]
        for p, k in self.col_p.items():
            X[p] = X[p] + d[k:k + 3]
        return R, t, X


def adjust(offsets, image, xy, use, xyz, K, T, fixed, huber=0.0, iters=100, ftol=1e-14):
    """-> dict(T [n,4,4], xyz [T,3] float64, cost, n_iters): the optimum over the observations `use` (bool [N]) from the given start."""
    pr = Problem(np.asarray(offsets), np.asarray(image), np.asarray(xy), np.asarray(use, bool), np.asarray(K, np.float64), fixed)
    R, t, X = np.array(T[:, :3, :3], np.float64), np.array(T[:, :3, 3], np.float64), np.array(xyz, np.float64)
    cost, lam, n = huber_cost(pr.residuals(R, t, X), huber), 1e-4, 0
    for n in range(1, iters + 1):
        r = pr.residuals(R, t, X)
        nr = np.linalg.norm(r, axis=1)
        w = np.ones_like(nr) if huber <= 0 else np.where(nr <= huber, 1.0, huber / np.maximum(nr, 1e-300))
        sw = np.repeat(np.sqrt(w), 2)
        J = pr.jacobian(R, t, X) * sw[:, None]
        H, g = J.T @ J, J.T @ (r.reshape(-1) * sw)
        stop = False
        while True:
            d = np.linalg.solve(H + lam * np.diag(np.maximum(np.diag(H), 1e-12)), -g)
            R2, t2, X2 = pr.moved(R, t, X, d)
            c2 = huber_cost(pr.residuals(R2, t2, X2), huber)
            if c2 < cost:
                stop = cost - c2 <= ftol * c2
                R, t, X, cost, lam = R2, t2, X2, c2, max(lam / 10, 1e-12)
                break
            lam *= 10
            if lam > 1e12:
                stop = True
                break
        if stop:
            break
    Tn = np.array(T, np.float64)
    Tn[:, :3, :3], Tn[:, :3, 3] = R, t
    return dict(T=Tn, xyz=X, cost=cost, n_iters=n)
