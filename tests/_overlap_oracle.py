"""The view-overlap rule (include/loftr_hip.h) in numpy: a loop over sources and entries, float64 arrays over the targets.
It shares no code with csrc/overlap_core.h; every expression is written in the operation order the header states (numpy's element-wise
+ - * / and sqrt are IEEE operations without contraction), so the integers must come out equal, not close."""
import numpy as np

NAN = float("nan")


def camera_table(K, T):
    """K [3,3], T [4,4] float64 -> (P [3,4], centre [3]) or None for an invalid camera (the triangulation's table)."""
    K, T = np.asarray(K, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(4, 4)
    fx, sk, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    if not (np.isfinite([fx, sk, cx, fy, cy]).all() and fx != 0.0 and fy != 0.0 and np.isfinite(T[:3]).all()):
        return None
    with np.errstate(all="ignore"):
        P = np.empty((3, 4))
        for c in range(4):
            P[0, c] = (fx * T[0, c] + sk * T[1, c]) + cx * T[2, c]
            P[1, c] = fy * T[1, c] + cy * T[2, c]
            P[2, c] = T[2, c]
        centre = np.array([-((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3]) for r in range(3)])
        k00, k11 = 1.0 / fx, 1.0 / fy
        k01, k12 = -(sk / fy) / fx, -cy / fy
        k02 = -(cx + sk * k12) / fx
        M = np.array([[T[0, r] * k00, T[0, r] * k01 + T[1, r] * k11, (T[0, r] * k02 + T[1, r] * k12) + T[2, r]] for r in range(3)])
    if not (np.isfinite(P).all() and np.isfinite(centre).all() and np.isfinite(M).all()):
        return None
    return P, centre


def _dot(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def view_overlap(vis_offsets, vis_point, xyz, point_ok, K_src, T_src, src_ok, K_tgt, T_tgt, tgt_ok, tgt_hw, border, cos_min, max_scale2):
    """-> (overlap [n,m] i32, n_vis [n] i32, counts [8] i64); on a bad list only counts[1] is set."""
    n, m, T, V = len(src_ok), len(tgt_ok), len(point_ok), len(vis_point)
    overlap, n_vis, counts = np.zeros((n, m), np.int32), np.zeros(n, np.int32), np.zeros(8, np.int64)
    vis_offsets, vis_point = np.asarray(vis_offsets, np.int64), np.asarray(vis_point, np.int64)
    err = 0
    if V and ((vis_point < 0) | (vis_point >= T)).any():
        err |= 1
    if n and (vis_offsets[0] != 0 or vis_offsets[-1] != V or (np.diff(vis_offsets) < 0).any() or (vis_offsets < 0).any() or (vis_offsets > V).any()):
        err |= 2
    if err:
        counts[1] = err
        return overlap, n_vis, counts
    border, cos_min, max_scale2 = np.float64(border), np.float64(cos_min), np.float64(max_scale2)
    hw = np.asarray(tgt_hw, np.float64).reshape(m, 2)
    P, C, f2, ok = np.full((m, 3, 4), NAN), np.full((m, 3), NAN), np.full(m, NAN), np.zeros(m, bool)
    for j in range(m):
        tab = camera_table(K_tgt[j], T_tgt[j]) if tgt_ok[j] else None
        if tab is None or not (np.isfinite(hw[j]).all() and hw[j, 0] > 0 and hw[j, 1] > 0):
            continue
        P[j], C[j], ok[j] = tab[0], tab[1], True
        fj = np.float64(np.asarray(K_tgt[j], np.float64).reshape(9)[0])
        with np.errstate(all="ignore"):
            f2[j] = fj * fj
    with np.errstate(all="ignore"):
        hi_u, hi_v = hw[:, 1] - border, hw[:, 0] - border
    counts[3] = ok.sum()
    with np.errstate(all="ignore"):
        for i in range(n):
            tab = camera_table(K_src[i], T_src[i]) if src_ok[i] else None
            if tab is None:
                continue
            counts[2] += 1
            ci = tab[1]
            fi = np.float64(np.asarray(K_src[i], np.float64).reshape(9)[0])
            f2i = fi * fi
            for k in range(vis_offsets[i], vis_offsets[i + 1]):
                p = vis_point[k]
                if not point_ok[p] or not np.isfinite(np.asarray(xyz[p], np.float32)).all():
                    continue
                n_vis[i] += 1
                X0, X1, X2 = (np.float64(v) for v in xyz[p])
                a0, a1, a2 = ci[0] - X0, ci[1] - X1, ci[2] - X2
                aa = _dot(a0, a1, a2, a0, a1, a2)
                x = _dot(P[:, 0, 0], P[:, 0, 1], P[:, 0, 2], X0, X1, X2) + P[:, 0, 3]
                y = _dot(P[:, 1, 0], P[:, 1, 1], P[:, 1, 2], X0, X1, X2) + P[:, 1, 3]
                z = _dot(P[:, 2, 0], P[:, 2, 1], P[:, 2, 2], X0, X1, X2) + P[:, 2, 3]
                u, v = x / z, y / z
                good = ok & (z > 0.0) & (u >= border) & (u < hi_u) & (v >= border) & (v < hi_v)
                b0, b1, b2 = C[:, 0] - X0, C[:, 1] - X1, C[:, 2] - X2
                bb, d = _dot(b0, b1, b2, b0, b1, b2), _dot(a0, a1, a2, b0, b1, b2)
                good &= d >= cos_min * np.sqrt(aa * bb)
                sj, si = f2 * aa, f2i * bb
                good &= (sj <= max_scale2 * si) & (si <= max_scale2 * sj)
                overlap[i] += good
    counts[0], counts[4] = n_vis.sum(), np.count_nonzero(overlap)
    return overlap, n_vis, counts
