"""The dense oracles of tests/_bundle_oracle.py, _bundle_focal_oracle.py and _bundle_shared_oracle.py with position priors on the camera
centres: three more residual rows per camera that has a prior, (centre - measured) / sigma with centre = -R^T t, and
their rows of the dense Jacobian under the oracles' own update (R <- exp(w) R by Rodrigues' formula, t <- t + dt).  The prior's loss is
the square whatever the loss of the observations is.  Same damped dense normal equations solved by np.linalg.solve, same damping loop;
run to ftol = 1e-14 or 100 iterations it stands for "the optimum".  It shares no text with csrc/bundle_core.h."""
import numpy as np

import _bundle_focal_oracle as FO
import _bundle_oracle as O
import _bundle_shared_oracle as SO


class PriorRows:
    """Mixed into a Problem: which free cameras have a prior, their residual rows and Jacobian rows."""

    def set_prior(self, xyz, sigma, has):
        self.g, self.sigma = np.asarray(xyz, np.float64), np.broadcast_to(np.asarray(sigma, np.float64), np.shape(xyz))
        ok = np.asarray(has, bool) & np.isfinite(self.g).all(1) & np.isfinite(self.sigma).all(1) & (self.sigma > 0).all(1)
        self.prior_cams = [c for c in self.free if ok[c]]
        return self

    def centre(self, R, t, c):
        return -(R[c].T @ t[c])

    def prior_residuals(self, R, t):
        return np.concatenate([(self.centre(R, t, c) - self.g[c]) / self.sigma[c] for c in self.prior_cams] or [np.zeros(0)])

    def prior_jacobian(self, R, t, n_cols):
        J = np.zeros((3 * len(self.prior_cams), n_cols))
        for row, c in enumerate(self.prior_cams):
            k = self.col_c[c]
            # exp(w) R: the centre becomes -R^T exp(-w) t = c + R^T (w x t) to first order, so d centre / d w = -R^T hat(t)
            J[3 * row:3 * row + 3, k:k + 3] = -(R[c].T @ O.hat(t[c])) / self.sigma[c][:, None]
            J[3 * row:3 * row + 3, k + 3:k + 6] = -R[c].T / self.sigma[c][:, None]
        return J


class PosePrior(PriorRows, O.Problem):
    pass


class FocalPrior(PriorRows, FO.FocalProblem):
    pass


class SharedPrior(PriorRows, SO.SharedProblem):
    pass


def solve(pr, xyz, K, T, huber=0.0, iters=100, ftol=1e-14):
    """The damping loop of the three oracles over the stacked residuals of `pr` (a PosePrior, FocalPrior or SharedPrior after set_prior)
    -> dict(T, xyz, K, cost, prior_cost, n_iters)."""
    K = np.array(K, np.float64)
    with_K = getattr(pr, "with_K", lambda K: pr)
    moved_K = getattr(pr, "moved_K", lambda K, d: K)
    R, t, X = np.array(T[:, :3, :3], np.float64), np.array(T[:, :3, 3], np.float64), np.array(xyz, np.float64)

    def cost_of(R, t, X, K):
        e = pr.prior_residuals(R, t)
        return O.huber_cost(with_K(K).residuals(R, t, X), huber) + float(e @ e)

    cost, lam, n = cost_of(R, t, X, K), 1e-4, 0
    for n in range(1, iters + 1):
        r = with_K(K).residuals(R, t, X)
        nr = np.linalg.norm(r, axis=1)
        w = np.ones_like(nr) if huber <= 0 else np.where(nr <= huber, 1.0, huber / np.maximum(nr, 1e-300))
        sw = np.repeat(np.sqrt(w), 2)
        Jo = pr.jacobian(R, t, X) * sw[:, None]
        J = np.concatenate([Jo, pr.prior_jacobian(R, t, Jo.shape[1])])
        res = np.concatenate([r.reshape(-1) * sw, pr.prior_residuals(R, t)])
        H, g = J.T @ J, J.T @ res
        stop = False
        while True:
            d = np.linalg.solve(H + lam * np.diag(np.maximum(np.diag(H), 1e-12)), -g)
            R2, t2, X2 = pr.moved(R, t, X, d)
            K2 = moved_K(K, d)
            c2 = cost_of(R2, t2, X2, K2)
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
    e = pr.prior_residuals(R, t)
    return dict(T=Tn, xyz=X, K=K, cost=cost, prior_cost=float(e @ e), n_iters=n)


def adjust(offsets, image, xy, use, xyz, K, T, fixed, prior_xyz, prior_sigma, prior_mask, refine=None, focal=None, group=None, **kw):
    """-> solve(...) of the problem of the pose oracle; with `refine` (bool [n]) of the focal oracle; with `focal` (bool [n], see
    _bundle_shared_oracle.carrying) and `group` [n] of the shared oracle; each with the priors prior_xyz [n,3], prior_sigma (anything
    that broadcasts to [n,3]) of the cameras in prior_mask [n]."""
    args = (np.asarray(offsets), np.asarray(image), np.asarray(xy), np.asarray(use, bool), np.array(K, np.float64), fixed)
    if group is not None:
        pr = SharedPrior(*args, focal, group)
    elif refine is not None:
        pr = FocalPrior(*args, np.asarray(refine, bool))
    else:
        pr = PosePrior(*args)
    return solve(pr.set_prior(prior_xyz, prior_sigma, prior_mask), xyz, K, T, **kw)
