"""The dense oracle of tests/_bundle_oracle.py with one more column per camera that refines its focal: a relative step d
that scales K[0,0], K[0,1] and K[1,1] by (1 + d).  Same dense Jacobian, same damped normal equations solved by np.linalg.solve, same
damping loop; run to ftol = 1e-14 or 100 iterations it stands for "the optimum".  It shares no text with csrc/bundle_core.h."""
import numpy as np

import _bundle_oracle as O


class FocalProblem(O.Problem):
    def __init__(self, offsets, image, xy, use, K, fixed, refine):
        super().__init__(offsets, image, xy, use, K, fixed)
        self.focal = [c for c in self.free if refine[c]]
        self.col_f = {c: self.n_par + k for k, c in enumerate(self.focal)}
        self.n_par += len(self.focal)

    def with_K(self, K):
        self.K = K
        return self

    def jacobian(self, R, t, X):
        n_dense = self.n_par
        self.n_par -= len(self.focal)
        J = np.concatenate([super().jacobian(R, t, X), np.zeros((2 * len(self.obs), len(self.focal)))], axis=1)
        self.n_par = n_dense
        for row, o in enumerate(self.obs):
            c = self.image[o]
            if c in self.col_f:
                Y = R[c] @ X[self.track[o]] + t[c]
                n = Y[:2] / Y[2]
                scaled = np.array([[self.K[c][0, 0], self.K[c][0, 1]], [0.0, self.K[c][1, 1]]])      # d pixel / d (1 + d) at d = 0
                J[2 * row:2 * row + 2, self.col_f[c]] = scaled @ n
        return J

    def moved_K(self, K, d):
        K = K.copy()
        for c, k in self.col_f.items():
            K[c, 0, 0], K[c, 0, 1], K[c, 1, 1] = K[c, 0, 0] * (1 + d[k]), K[c, 0, 1] * (1 + d[k]), K[c, 1, 1] * (1 + d[k])
        return K


def adjust(offsets, image, xy, use, xyz, K, T, fixed, refine, huber=0.0, iters=100, ftol=1e-14):
    """-> dict(T [n,4,4], xyz [T,3] float64, K [n,3,3], cost, n_iters): the optimum over the observations `use` from the given start,
    the cameras of the bool mask `refine` that are free also moving their focal."""
    K = np.array(K, np.float64)
    pr = FocalProblem(np.asarray(offsets), np.asarray(image), np.asarray(xy), np.asarray(use, bool), K, fixed, np.asarray(refine, bool))
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
