"""Independent numpy float64 statement of the triangulation rule (include/loftr_hip.h): plain loops, numpy's linear algebra,
no code shared with the library.  Slow on purpose; the tests run it on a few hundred short tracks."""
import numpy as np

OK, TOO_SHORT, NO_HYPOTHESIS, SMALL_ANGLE, BAD_CAMERA = range(5)
MAX_HYP = 64


def pairs(L):
    out = []
    for s in range(1, L // 2 + 1):
        for i in range(L // 2 if 2 * s == L else L):
            if len(out) == MAX_HYP:
                return out
            out.append((i, (i + s) % L))
    return out


class Camera:
    def __init__(self, K, T):
        K, T = np.asarray(K, np.float64), np.asarray(T, np.float64)
        Ku = np.array([[K[0, 0], K[0, 1], K[0, 2]], [0.0, K[1, 1], K[1, 2]], [0.0, 0.0, 1.0]])      # only fx, skew, cx, fy, cy are read
        R, t = T[:3, :3], T[:3, 3]
        self.valid = bool(np.isfinite(Ku).all() and np.isfinite(T[:3]).all() and Ku[0, 0] != 0 and Ku[1, 1] != 0)
        if self.valid:
            self.P = Ku @ T[:3]
            self.c = -R.T @ t
            self.M = R.T @ np.linalg.inv(Ku)
            self.valid = bool(np.isfinite(self.P).all() and np.isfinite(self.c).all() and np.isfinite(self.M).all())

    def ray(self, uv):
        d = self.M @ np.array([uv[0], uv[1], 1.0])
        return d / np.linalg.norm(d)

    def residual(self, X, uv):
        """(in front, squared pixel distance)"""
        p = self.P @ np.append(X, 1.0)
        if not p[2] > 0:
            return False, np.inf
        return True, float((p[0] / p[2] - uv[0]) ** 2 + (p[1] / p[2] - uv[1]) ** 2)


def midpoint(ci, di, cj, dj, cos_min, info=None):
    w = ci - cj
    a, b, c, d, e = di @ di, di @ dj, dj @ dj, di @ w, dj @ w
    den = a * c - b * b
    if not den > 1e-12 * a * c:
        return None
    cs = b / np.sqrt(a * c)
    if info is not None:
        info["cos_margin"] = min(info["cos_margin"], abs(cs - cos_min))
    if not cs <= cos_min:
        return None
    s, t = (b * e - c * d) / den, (a * e - b * d) / den
    if not s > 0 or not t > 0:
        return None
    return 0.5 * ((ci + s * di) + (cj + t * dj))


def inliers(cams, xy, X, thr2, info=None):
    m = np.zeros(len(cams), bool)
    r2s = np.full(len(cams), np.inf)
    for k, (cam, uv) in enumerate(zip(cams, xy)):
        front, r2 = cam.residual(X, uv)
        m[k] = front and r2 <= thr2
        r2s[k] = r2
        if info is not None and front and np.isfinite(r2):
            info["px_margin"] = min(info["px_margin"], abs(np.sqrt(r2) - np.sqrt(thr2)))
    return m, r2s


def gauss_newton(cams, xy, mask, X, steps):
    """`steps` Gauss-Newton steps over the observations of `mask` (fixed); None when a step fails."""
    Y = X.copy()
    for _ in range(steps):
        H, g = np.zeros((3, 3)), np.zeros(3)
        for k in np.nonzero(mask)[0]:
            P = cams[k].P
            p = P @ np.append(Y, 1.0)
            if not p[2] > 0:
                continue
            u, v = p[0] / p[2], p[1] / p[2]
            J = np.stack([(P[0, :3] - u * P[2, :3]) / p[2], (P[1, :3] - v * P[2, :3]) / p[2]])
            r = np.array([u - xy[k][0], v - xy[k][1]])
            H += J.T @ J
            g += J.T @ r
        # elimination without pivoting meets a non-positive pivot exactly when a leading principal minor is not positive
        if not (H[0, 0] > 0 and np.linalg.det(H[:2, :2]) > 0 and np.linalg.det(H) > 0):
            return None
        step = np.linalg.solve(H, -g)
        if not np.isfinite(step).all():
            return None
        Y = Y + step
    return Y


def triangulate_track(cams, xy, thresh_px, cos_min):
    """cams: the Camera of every observation, xy [L,2].  -> dict(status, xyz, n_inliers, rms_px, tri_cos, mask, px_margin, cos_margin):
    the margins are the smallest distances of a residual (px) / a cosine from its limit met on the way, for the borderline rule."""
    L = len(cams)
    thr2 = float(thresh_px) ** 2
    info = {"px_margin": np.inf, "cos_margin": np.inf}
    out = dict(status=None, xyz=np.full(3, np.nan), n_inliers=0, rms_px=np.nan, tri_cos=np.nan, mask=np.zeros(L, bool))
    xy = np.asarray(xy, np.float64)
    if L < 2:
        out["status"] = TOO_SHORT
    elif not all(c.valid for c in cams):
        out["status"] = BAD_CAMERA
    else:
        rays = [c.ray(uv) for c, uv in zip(cams, xy)]
        best, bestX = (0, 0), None
        for h, (i, j) in enumerate(pairs(L)):
            X = midpoint(cams[i].c, rays[i], cams[j].c, rays[j], cos_min, info)
            if X is None:
                continue
            m, _ = inliers(cams, xy, X, thr2, info)
            if not (m[i] and m[j]):
                continue
            if m.sum() > best[0]:                                     # strict: the smallest h wins a tie
                best, bestX = (int(m.sum()), h), X
        if bestX is None:
            out["status"] = NO_HYPOTHESIS
        else:
            X = bestX
            mask, _ = inliers(cams, xy, X, thr2)
            for _ in range(4):
                F = gauss_newton(cams, xy, mask, X, 5) if mask.sum() >= 2 else None
                if F is None:
                    break
                m2, _ = inliers(cams, xy, F, thr2, info)
                if m2.sum() < mask.sum():
                    break
                grew = m2.sum() > mask.sum()
                X, mask = F, m2
                if not grew:
                    break
            _, r2 = inliers(cams, xy, X, thr2)
            tri_cos = None
            for i, j in pairs(L):
                if mask[i] and mask[j]:
                    a, b = X - cams[i].c, X - cams[j].c
                    if a @ a > 0 and b @ b > 0:
                        cs = (a @ b) / np.sqrt((a @ a) * (b @ b))
                        tri_cos = cs if tri_cos is None else min(tri_cos, cs)
            if tri_cos is not None:
                info["cos_margin"] = min(info["cos_margin"], abs(tri_cos - cos_min))
            ok = tri_cos is not None and not tri_cos > cos_min
            out.update(status=OK if ok else SMALL_ANGLE, n_inliers=int(mask.sum()), rms_px=float(np.sqrt(r2[mask].mean())) if mask.any() else 0.0,
                       tri_cos=np.nan if tri_cos is None else float(tri_cos))
            if ok:
                out.update(xyz=X, mask=mask)
    out.update(info)
    return out


def triangulate(offsets, obs_image, obs_xy, K, T, thresh_px, cos_min):
    """The whole rule on CSR tracks -> list of triangulate_track results."""
    cams = [Camera(k, t) for k, t in zip(K, T)]
    res = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        res.append(triangulate_track([cams[i] for i in obs_image[a:b]], obs_xy[a:b], thresh_px, cos_min))
    return res


def reprojection_rms(cams, xy, mask, X):
    """RMS pixel error of X over the observations of mask."""
    r2 = [cams[k].residual(X, xy[k])[1] for k in np.nonzero(mask)[0]]
    return float(np.sqrt(np.mean(r2)))
