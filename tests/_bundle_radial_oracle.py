"""The dense oracle of tests/_bundle_shared_oracle.py with one more column per GROUP of cameras: an additive step of the
radial coefficient k of the model x_d = x (1 + k r^2) on normalised coordinates.  Analytic Jacobians by the chain rule in matrix form
(d pixel / d x_d = the 2 x 2 of K, d x_d / d x = m I + 2 k x x^T, d x / d Y the pinhole's), the same damped normal equations solved by
np.linalg.solve and the same damping loop as the other oracles; run to ftol = 1e-14 or 100 iterations it stands for "the optimum".  It
imports the existing oracles (indexing, Rodrigues, the loss, who carries) and shares no text with csrc/bundle_core.h."""
import numpy as np

import _bundle_oracle as O
import _bundle_shared_oracle as SO


def carrying(image, use, K, T, refine_focal, refine_radial, group, min_focal_obs):
    """-> (focal [n], radial [n]) bool: the images whose focal / radial coefficient moves.  Focal: §18.2's.  Radial: those of them that
    are flagged, in a group whose such members together have at least min_focal_obs observations in `use`."""
    focal = SO.carrying(image, use, K, T, refine_focal, group, min_focal_obs)
    cnt = np.bincount(np.asarray(image)[np.asarray(use, bool)], minlength=len(K))
    cand = focal & np.asarray(refine_radial, bool)
    total = np.bincount(np.asarray(group), weights=np.where(cand, cnt, 0), minlength=int(np.max(group)) + 1 if len(K) else 0)
    return focal, cand & (total[np.asarray(group)] >= min_focal_obs)


class RadialProblem(O.Problem):
    def __init__(self, offsets, image, xy, use, K, fixed, focal, radial, group):
        super().__init__(offsets, image, xy, use, K, fixed)
        self.focal, self.radial, self.group = np.asarray(focal, bool), np.asarray(radial, bool), np.asarray(group)
        gf, gr = sorted(set(self.group[self.focal].tolist())), sorted(set(self.group[self.radial].tolist()))
        self.col_f = {g: self.n_par + i for i, g in enumerate(gf)}
        self.col_k = {g: self.n_par + len(gf) + i for i, g in enumerate(gr)}
        self.n_cols = self.n_par + len(gf) + len(gr)

    def residuals(self, R, t, X, K, k):
        out = np.zeros((len(self.obs), 2))
        for row, o in enumerate(self.obs):
            c = self.image[o]
            Y = R[c] @ X[self.track[o]] + t[c]
            x = Y[:2] / Y[2]
            out[row] = K[c][:2, :2] @ (x * (1.0 + k[c] * (x @ x))) + K[c][:2, 2] - self.xy[o]
        return out

    def jacobian(self, R, t, X, K, k):
        J = np.zeros((2 * len(self.obs), self.n_cols))
        for row, o in enumerate(self.obs):
            c, p = self.image[o], self.track[o]
            P = R[c] @ X[p]
            Y = P + t[c]
            x = Y[:2] / Y[2]
            r2 = x @ x
            lens = (1.0 + k[c] * r2) * np.eye(2) + 2.0 * k[c] * np.outer(x, x)                       # d x_d / d x
            dpi = K[c][:2, :2] @ lens @ np.array([[1.0 / Y[2], 0.0, -x[0] / Y[2]], [0.0, 1.0 / Y[2], -x[1] / Y[2]]])     # d pixel / d Y
            rows = slice(2 * row, 2 * row + 2)
            if c in self.col_c:
                J[rows, self.col_c[c]:self.col_c[c] + 3] = dpi @ (-O.hat(P))
                J[rows, self.col_c[c] + 3:self.col_c[c] + 6] = dpi
            J[rows, self.col_p[p]:self.col_p[p] + 3] = dpi @ R[c]
            if self.focal[c]:
                J[rows, self.col_f[self.group[c]]] = K[c][:2, :2] @ (x * (1.0 + k[c] * r2))          # d pixel / d (1 + d) at d = 0
            if self.radial[c]:
                J[rows, self.col_k[self.group[c]]] = K[c][:2, :2] @ (x * r2)
        return J

    def moved_lens(self, K, k, d):
        K, k = K.copy(), k.copy()
        for c in np.nonzero(self.focal)[0]:
            K[c][:2, :2] = K[c][:2, :2] * (1 + d[self.col_f[self.group[c]]])
        for c in np.nonzero(self.radial)[0]:
            k[c] = k[c] + d[self.col_k[self.group[c]]]
        return K, k


def adjust(offsets, image, xy, use, xyz, K, T, fixed, focal, radial, group, k0, huber=0.0, iters=100, ftol=1e-14):
    """-> dict(T [n,4,4], xyz [T,3] float64, K [n,3,3], k [n], cost, n_iters): the optimum over the observations `use` from the given
    start; the images of the bool masks `focal` / `radial` (see carrying()) move their focal by one relative step and their k by one
    additive step per entry of `group` [n]."""
    K, k = np.array(K, np.float64), np.array(k0, np.float64)
    pr = RadialProblem(np.asarray(offsets), np.asarray(image), np.asarray(xy), np.asarray(use, bool), K, fixed, focal, radial, group)
    R, t, X = np.array(T[:, :3, :3], np.float64), np.array(T[:, :3, 3], np.float64), np.array(xyz, np.float64)
    cost, lam, n = O.huber_cost(pr.residuals(R, t, X, K, k), huber), 1e-4, 0
    for n in range(1, iters + 1):
        r = pr.residuals(R, t, X, K, k)
        nr = np.linalg.norm(r, axis=1)
        w = np.ones_like(nr) if huber <= 0 else np.where(nr <= huber, 1.0, huber / np.maximum(nr, 1e-300))
        sw = np.repeat(np.sqrt(w), 2)
        J = pr.jacobian(R, t, X, K, k) * sw[:, None]
        H, g = J.T @ J, J.T @ (r.reshape(-1) * sw)
        stop = False
        while True:
            d = np.linalg.solve(H + lam * np.diag(np.maximum(np.diag(H), 1e-12)), -g)
            R2, t2, X2 = pr.moved(R, t, X, d)
            K2, k2 = pr.moved_lens(K, k, d)
            c2 = O.huber_cost(pr.residuals(R2, t2, X2, K2, k2), huber)
            if c2 < cost:
                stop = cost - c2 <= ftol * c2
                R, t, X, K, k, cost, lam = R2, t2, X2, K2, k2, c2, max(lam / 10, 1e-12)
                break
            lam *= 10
            if lam > 1e12:
                stop = True
                break
        if stop:
            break
    Tn = np.array(T, np.float64)
    Tn[:, :3, :3], Tn[:, :3, 3] = R, t
    return dict(T=Tn, xyz=X, K=K, k=k, cost=cost, n_iters=n)
