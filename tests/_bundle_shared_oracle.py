"""The dense oracle of tests/_bundle_focal_oracle.py with one focal column per GROUP of cameras instead of one per camera:
the column of a group is the sum, over the observations of its members that carry the focal, of the per-camera column; a relative step d
scales K[0,0], K[0,1] and K[1,1] of every such member by (1 + d).  A member may have a fixed pose: it then has no pose columns but still
feeds its group's.  Same dense Jacobian, same damped normal equations solved by np.linalg.solve, same damping loop; run to ftol = 1e-14 or
100 iterations it stands for "the optimum".  It imports the existing oracles and shares no text with csrc/bundle_core.h."""
import numpy as np

import _bundle_focal_oracle as FO
import _bundle_oracle as O


def carrying(image, use, K, T, refine, group, min_focal_obs):
    """-> bool [n]: the images whose focal moves: flagged, with at least one observation in `use`, in a group whose such members
    together have at least min_focal_obs of them.  (The scenes of the tests have only valid cameras.)"""
    n = len(K)
    cnt = np.bincount(np.asarray(image)[np.asarray(use, bool)], minlength=n)
    carries = np.asarray(refine, bool) & (cnt >= 1) & np.isfinite(np.asarray(T).reshape(n, -1)).all(1)
    total = np.bincount(np.asarray(group), weights=np.where(carries, cnt, 0), minlength=int(np.max(group)) + 1 if n else 0)
    return carries & (total[np.asarray(group)] >= min_focal_obs)


class SharedProblem(O.Problem):
    def __init__(self, offsets, image, xy, use, K, fixed, focal, group):
        super().__init__(offsets, image, xy, use, K, fixed)
        self.n_dense = self.n_par
        self.focal, self.group = np.asarray(focal, bool), np.asarray(group)
        groups = sorted(set(self.group[self.focal].tolist()))
        self.col_g = {g: self.n_dense + k for k, g in enumerate(groups)}
        self.n_cols = self.n_dense + len(groups)

    with_K = FO.FocalProblem.with_K

    def jacobian(self, R, t, X):
        J = np.concatenate([super().jacobian(R, t, X), np.zeros((2 * len(self.obs), len(self.col_g)))], axis=1)
        for row, o in enumerate(self.obs):
            c = self.image[o]
            if self.focal[c]:
                Y = R[c] @ X[self.track[o]] + t[c]
                scaled = np.array([[self.K[c][0, 0], self.K[c][0, 1]], [0.0, self.K[c][1, 1]]])      # d pixel / d (1 + d) at d = 0
                J[2 * row:2 * row + 2, self.col_g[self.group[c]]] = scaled @ (Y[:2] / Y[2])
        return J

    def moved_K(self, K, d):
        K = K.copy()
        for c in np.nonzero(self.focal)[0]:
            f = 1 + d[self.col_g[self.group[c]]]
            K[c, 0, 0], K[c, 0, 1], K[c, 1, 1] = K[c, 0, 0] * f, K[c, 0, 1] * f, K[c, 1, 1] * f
        return K


def adjust(offsets, image, xy, use, xyz, K, T, fixed, focal, group, huber=0.0, iters=100, ftol=1e-14):
    """-> dict(T [n,4,4], xyz [T,3] float64, K [n,3,3], cost, n_iters): the optimum over the observations `use` from the given start;
    the images of the bool mask `focal` (see carrying()) move their focal, one relative step per entry of `group` [n]."""
    K = np.array(K, np.float64)
    pr = SharedProblem(np.asarray(offsets), np.asarray(image), np.asarray(xy), np.asarray(use, bool), K, fixed, focal, group)
    R, t, X = np.array(T[:, :3, :3], np.float64), np.array(T[:, :3, 3], np.float64), np.array(xyz, np.float64)
    cost, lam, n = O.huber_cost(pr.with_K(K).residuals(R, t, X), huber), 1e-4, 0
    for n in range(1, iters + 1):
        r = pr.with_K(K).residuals(R, t, X)
        nr = np.linalg.norm(r, axis=1)
        w = np.ones_like(nr) if huber <= 0 else np.where(nr <= huber, 1.0, huber / np.maximum(nr, 1e-300))
        sw = np.repeat(np.sqrt(w), 2)
        J = pr.jacobian(R, t, X) * sw[:, None]
        H, g = J.T @ J, J.T @ (r.reshape(-1) * sw)
        stop = False
        while True:
            d = np.linalg.solve(H + lam * np.diag(np.maximum(np.diag(H), 1e-12)), -g)
            R2, t2, X2 = pr.moved(R, t, X, d)
            K2 = pr.moved_K(K, d)
            c2 = O.huber_cost(pr.with_K(K2).residuals(R2, t2, X2), huber)
            if c2 < cost:
                stop = cost - c2 <= ftol * c2
                R, t, X, K, cost, lam = R2, t2, X2, K2, c2, max(lam / 10, 1e-12)
                break
            lam *= 10
            if lam > 1e12:
                stop = True
                break
        if stop:
            break
    Tn = np.array(T, np.float64)
    Tn[:, :3, :3], Tn[:, :3, 3] = R, t
    return dict(T=Tn, xyz=X, K=K, cost=cost, n_iters=n)
