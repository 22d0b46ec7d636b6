"""Independent statement of the track-merging rule (include/loftr_hip.h, rules 1-8): numpy scalars, plain loops and dicts (a
dict per image from cell to keypoint), no code shared with the library's core headers, its own camera table written in the documented
operation order.  Python floats are IEEE doubles and nothing here is fused, so bit equality with the host routine is required of every
output and count, not a tolerance.  Slow on purpose; the tests run it on a few hundred rows."""
import math

import numpy as np

NAN_BITS = 0x7FC00000


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def finite32(x):
    return (f32_bits(x) & 0x7F800000) != 0x7F800000


def camera(K, T):
    """K [3,3], T [4,4] -> P as 3 rows of 4 floats, or None for an invalid camera: fx, skew, cx, fy, cy and the top 3 x 4 of T finite,
    fx, fy not 0, and every entry of P, of the centre -R^T t and of M = R^T K^-1 finite."""
    fx, sk, cx, fy, cy = float(K[0][0]), float(K[0][1]), float(K[0][2]), float(K[1][1]), float(K[1][2])
    t = [[float(T[r][c]) for c in range(4)] for r in range(3)]
    if not all(math.isfinite(v) for v in [fx, sk, cx, fy, cy] + [v for row in t for v in row]) or fx == 0.0 or fy == 0.0:
        return None
    P = [[(fx * t[0][c] + sk * t[1][c]) + cx * t[2][c] for c in range(4)], [fy * t[1][c] + cy * t[2][c] for c in range(4)], list(t[2])]
    centre = [-((t[0][r] * t[0][3] + t[1][r] * t[1][3]) + t[2][r] * t[2][3]) for r in range(3)]
    k00, k11 = 1.0 / fx, 1.0 / fy
    k01, k12 = -(sk / fy) / fx, -cy / fy
    k02 = -(cx + sk * k12) / fx
    M = [v for r in range(3) for v in (t[0][r] * k00, t[0][r] * k01 + t[1][r] * k11, (t[0][r] * k02 + t[1][r] * k12) + t[2][r])]
    if not all(math.isfinite(v) for v in [v for row in P for v in row] + centre + M):
        return None
    return P


def cell_coord(x, inv, g):
    with np.errstate(all="ignore"):
        f = np.floor(np.float32(x) * np.float32(inv))
    return int(f) if f >= 0 and f < np.float32(g) else -1


def project(P, X):
    """(u, v) of X in P, None unless in front"""
    dot = lambda p: (p[0] * X[0] + p[1] * X[1]) + p[2] * X[2]
    x, y, z = dot(P[0]) + P[0][3], dot(P[1]) + P[1][3], dot(P[2]) + P[2][3]
    return (x / z, y / z) if z > 0.0 else None


def dist2(uv, xy):
    du, dv = uv[0] - float(xy[0]), uv[1] - float(xy[1])
    return du * du + dv * dv


def error_bits(offsets, obs_image, kp_offsets, kp_row, n, n_kp):
    T, N = len(offsets) - 1, len(obs_image)
    err = 0
    for t in range(T):
        b, e = int(offsets[t]), int(offsets[t + 1])
        if b < 0 or e < b or e > N or (t == 0 and b != 0) or (t == T - 1 and e != N):
            err |= 2
            continue
        for o in range(b, e):
            err |= 1 if obs_image[o] < 0 or obs_image[o] >= n else 0
            err |= 4 if o > b and obs_image[o] < obs_image[o - 1] else 0
    for i in range(n):
        b, e = int(kp_offsets[i]), int(kp_offsets[i + 1])
        if b < 0 or e < b or e > n_kp or (i == 0 and b != 0) or (i == n - 1 and e != n_kp):
            err |= 2
    for k in range(n_kp):
        err |= 8 if kp_row[k] < -1 or kp_row[k] >= T else 0
    return err


def merge(offsets, obs_image, obs_xy, obs_mask, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, T_cam_from_world, posed, gh, gw, inv,
          thresh_px, reach):
    """-> dict(row_into [T] i32, merge_r2 [T] f32, kp_row_new [K] i32, counts [8] i64, meetings [(j, i, m, candidate bits)],
    scores {(a, b): bits of the accepted pairs}); with a bad table only dict(error=bits)."""
    T, n, n_kp = len(offsets) - 1, len(posed), len(keypoints)
    err = error_bits(offsets, obs_image, kp_offsets, kp_row, n, n_kp)
    if err:
        return dict(error=err)
    thr2 = float(thresh_px) * float(thresh_px)
    cams = [camera(K[i], T_cam_from_world[i]) for i in range(n)]
    usable = [bool(posed[i]) and cams[i] is not None for i in range(n)]
    by_cell = [{int(kp_cell[k]): k for k in range(int(kp_offsets[i]), int(kp_offsets[i + 1]))} for i in range(n)]
    obs = [list(range(int(offsets[j]), int(offsets[j + 1]))) for j in range(T)]
    source = [status[j] == 0 and all(finite32(v) for v in xyz[j]) for j in range(T)]                 # 1. source
    w = [sum(1 for o in obs[j] if obs_mask[o] != 0) for j in range(T)]
    counts = [0] * 8
    best, meetings, scores = {}, [], {}

    def score(a, b):                                                                                 # 4. agreement of a < b
        if w[a] == 0 or w[b] == 0:
            return None
        X = [(float(w[a]) * float(xyz[a][c]) + float(w[b]) * float(xyz[b][c])) / float(w[a] + w[b]) for c in range(3)]
        worst = 0.0
        for o in obs[a] + obs[b]:
            if obs_mask[o] == 0:
                continue
            i = int(obs_image[o])
            uv = project(cams[i], X) if usable[i] else None
            if uv is None or not dist2(uv, obs_xy[o]) <= thr2:
                return None
            worst = max(worst, dist2(uv, obs_xy[o]))
        return f32_bits(worst)

    for j in range(T):
        if not source[j]:
            continue
        counts[2] += 1
        X = [float(v) for v in xyz[j]]
        visited = {int(obs_image[o]) for o in obs[j]}
        for i in range(n):
            if not usable[i] or i in visited:                                                        # 2. target
                continue
            counts[3] += 1
            uv = project(cams[i], X)
            if uv is None:
                continue
            cx, cy = cell_coord(uv[0], inv, gw), cell_coord(uv[1], inv, gh)
            if cx < 0 or cy < 0:
                continue
            cand = None
            for yy in range(max(cy - reach, 0), min(cy + reach, gh - 1) + 1):
                for xx in range(max(cx - reach, 0), min(cx + reach, gw - 1) + 1):
                    k = by_cell[i].get(yy * gw + xx)
                    if k is None:
                        continue
                    m = int(kp_row[k])
                    if m < 0 or m == j or not source[m] or not dist2(uv, keypoints[k]) <= thr2:
                        continue
                    c = (f32_bits(dist2(uv, keypoints[k])), k)
                    if cand is None or c < cand:
                        cand = c
            if cand is None:
                continue
            m = int(kp_row[cand[1]])
            counts[4] += 1                                                                           # a meeting
            meetings.append((j, i, m, cand[0]))
            if visited & {int(obs_image[o]) for o in obs[m]}:                                        # 3. disjoint
                continue
            counts[5] += 1
            a, b = min(j, m), max(j, m)
            bits = score(a, b)
            if bits is None:
                continue
            counts[6] += 1
            scores[(a, b)] = bits
            for row, partner in ((j, m), (m, j)):                                                    # 5. choice
                word = (bits << 32) | partner
                if row not in best or word < best[row]:
                    best[row] = word
    row_into = np.arange(T, dtype=np.int32)
    r2 = np.full(T, NAN_BITS, np.uint32)
    for j, word in best.items():                                                                     # 6. merge
        m = word & 0xFFFFFFFF
        if m in best and (best[m] & 0xFFFFFFFF) == j:
            row_into[j] = min(j, m)
            r2[j] = word >> 32
            counts[0] += j < m
    kp_row_new = np.array([r if r < 0 else row_into[r] for r in kp_row], np.int32).reshape(n_kp)     # 7. output
    counts[7] = int((kp_row_new != np.asarray(kp_row, np.int32)).sum())
    return dict(row_into=row_into, merge_r2=r2.view(np.float32), kp_row_new=kp_row_new, counts=np.array(counts, np.int64),
                meetings=meetings, scores=scores)
