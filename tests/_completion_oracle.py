"""Independent statement of the track-completion rule (include/loftr_hip.h, rules 1-8): numpy scalars, plain loops and
dicts, no code shared with the library, its own camera table written in the documented operation order.  Python floats are IEEE
doubles and nothing here is fused, so bit equality with the host routine is required of every output and count, not a tolerance.
Slow on purpose; the tests run it on a few hundred rows."""
import math

import numpy as np

F32_EXP = 0x7F800000


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def finite32(x):
    return (f32_bits(x) & F32_EXP) != F32_EXP


def camera_table(K, T):
    """K [3,3], T [4,4] -> P as 3 rows of 4 floats, or None for an invalid camera: fx, skew, cx, fy, cy and the top 3 x 4 of T finite,
    fx, fy not 0, and every entry of P, of the centre -R^T t and of M = R^T K^-1 finite."""
    fx, sk, cx, fy, cy = (float(K[0][0]), float(K[0][1]), float(K[0][2]), float(K[1][1]), float(K[1][2]))
    t = [[float(T[r][c]) for c in range(4)] for r in range(3)]
    vals = [fx, sk, cx, fy, cy] + [v for row in t for v in row]
    if not all(math.isfinite(v) for v in vals) or fx == 0.0 or fy == 0.0:
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
    """floorf((float) x * inv) on a side of g cells, -1 outside; one fp32 multiply"""
    with np.errstate(all="ignore"):
        f = np.floor(np.float32(x) * np.float32(inv))
    return int(f) if f >= 0 and f < np.float32(g) else -1


def cells(keypoints, inv, gw, gh):
    """kp_cell [K] i32 of keypoints [K,2]: cy * gw + cx, -1 outside the grid or not finite"""
    out = np.full(len(keypoints), -1, np.int32)
    for k, (x, y) in enumerate(keypoints):
        if finite32(x) and finite32(y):
            cx, cy = cell_coord(x, inv, gw), cell_coord(y, inv, gh)
            if cx >= 0 and cy >= 0:
                out[k] = cy * gw + cx
    return out


def dot(p, X):
    return (p[0] * X[0] + p[1] * X[1]) + p[2] * X[2]


def error_bits(offsets, obs_image, kp_offsets, kp_row, n, n_kp):
    T, N = len(offsets) - 1, len(obs_image)
    err = 0
    for t in range(T):
        b, e = int(offsets[t]), int(offsets[t + 1])
        if b < 0 or e < b or e > N or (t == 0 and b != 0) or (t == T - 1 and e != N):
            err |= 2
            continue
        for o in range(b, e):
            if obs_image[o] < 0 or obs_image[o] >= n:
                err |= 1
            if o > b and obs_image[o] < obs_image[o - 1]:
                err |= 4
    for i in range(n):
        b, e = int(kp_offsets[i]), int(kp_offsets[i + 1])
        if b < 0 or e < b or e > n_kp or (i == 0 and b != 0) or (i == n - 1 and e != n_kp):
            err |= 2
    for k in range(n_kp):
        if kp_row[k] < -1 or kp_row[k] >= T:
            err |= 8
    return err


def complete(offsets, obs_image, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, T_cam_from_world, posed, gh, gw, inv, thresh_px, reach):
    """-> dict(kp_row_new [K] i32, link_r2 [K] f32, counts [8] i64, proposals {(row, image): (keypoint, bits)}); with a bad table only
    dict(error=bits)."""
    T, n, n_kp = len(offsets) - 1, len(posed), len(keypoints)
    err = error_bits(offsets, obs_image, kp_offsets, kp_row, n, n_kp)
    if err:
        return dict(error=err)
    thr2 = float(thresh_px) * float(thresh_px)
    cams = [camera_table(K[i], T_cam_from_world[i]) for i in range(n)]
    by_cell = [{int(kp_cell[k]): k for k in range(int(kp_offsets[i]), int(kp_offsets[i + 1]))} for i in range(n)]
    counts = [0] * 8
    claim, proposals = {}, {}
    for j in range(T):
        if status[j] != 0 or not all(finite32(v) for v in xyz[j]):                      # 1. source
            continue
        counts[2] += 1
        X = [float(v) for v in xyz[j]]
        visited = {int(i) for i in obs_image[int(offsets[j]):int(offsets[j + 1])]}
        for i in range(n):
            if not posed[i] or cams[i] is None or i in visited:                         # 2. target
                continue
            counts[3] += 1
            P = cams[i]
            x, y, z = dot(P[0], X) + P[0][3], dot(P[1], X) + P[1][3], dot(P[2], X) + P[2][3]      # 3. projection
            if not z > 0.0:
                continue
            u, v = x / z, y / z
            cx, cy = cell_coord(u, inv, gw), cell_coord(v, inv, gh)
            if cx < 0 or cy < 0:
                continue
            counts[4] += 1
            best, blocked = None, False
            for yy in range(max(cy - reach, 0), min(cy + reach, gh - 1) + 1):           # 4. candidates
                for xx in range(max(cx - reach, 0), min(cx + reach, gw - 1) + 1):
                    k = by_cell[i].get(yy * gw + xx)
                    if k is None:
                        continue
                    du, dv = x / z - float(keypoints[k][0]), y / z - float(keypoints[k][1])
                    r2 = du * du + dv * dv
                    if not r2 <= thr2:
                        continue
                    if kp_row[k] != -1 and status[kp_row[k]] == 0:
                        blocked = True
                        continue
                    cand = (f32_bits(r2), k)
                    if best is None or cand < best:                                     # 5. proposal
                        best = cand
            if best is None:
                counts[7] += blocked
                continue
            counts[5] += 1
            proposals[(j, i)] = (best[1], best[0])
            word = (best[0] << 32) | j                                                  # 6. winner
            if best[1] not in claim or word < claim[best[1]]:
                claim[best[1]] = word
    kp_row_new = np.array(kp_row, np.int32).copy()
    bits = np.full(n_kp, 0x7FC00000, np.uint32)
    for k, word in claim.items():
        kp_row_new[k] = word & 0xFFFFFFFF
        bits[k] = word >> 32
    counts[0] = len(claim)
    counts[6] = counts[5] - counts[0]
    return dict(kp_row_new=kp_row_new, link_r2=bits.view(np.float32), counts=np.array(counts, np.int64), proposals=proposals)
