"""An independent float64 numpy restatement of rotation averaging over the view graph, the yardstick of
tests/test_rotation.py.  Written from the rule, not from csrc/rotation_core.h: dictionaries and sets for the graph, rotation matrices
for the cycle test, the quaternion of a matrix as the dominant eigenvector of Bar-Itzhack's symmetric 4 x 4 matrix, Kruskal over sorted
tuples, a queue for the start values, numpy sums in numpy's order, and for the step either a dense ``numpy.linalg.solve`` of the
reduced Laplacian (solver='dense') or the same Jacobi-preconditioned conjugate gradients (solver='pcg')."""
import math
from collections import deque

import numpy as np


def quat_of(R):
    """Unit quaternion (w, x, y, z) of a rotation matrix, w >= 0: the eigenvector of the largest eigenvalue of Bar-Itzhack's K."""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    vals, vecs = np.linalg.eigh(K)
    x, y, z, w = vecs[:, -1]
    q = np.array([w, x, y, z])
    return q if w >= 0 else -q


def rot_of(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def left(q):
    """The matrix of p -> q (x) p."""
    w, x, y, z = q
    return np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])


def conj(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def average(edge_image, edge_R, edge_weight, n, root=-1, cycle_deg=5.0, loss_deg=5.0, max_err_deg=10.0, max_iters=20, pcg_iters=30,
            pcg_tol=1e-4, step_tol_deg=1e-3, solver="dense"):
    E = len(edge_image)
    cos_half, d2 = math.cos(math.radians(cycle_deg) / 2), (2 * math.sin(math.radians(loss_deg) / 2)) ** 2
    max_chord, step_tol = 2 * math.sin(math.radians(max_err_deg) / 2), math.radians(step_tol_deg)
    valid = np.zeros(E, bool)
    for e in range(E):
        R = edge_R[e]
        valid[e] = edge_weight[e] > 0 and np.isfinite(R).all() and np.linalg.det(R) > 0 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-3
    best = {}
    for e in range(E):
        if valid[e]:
            key = tuple(sorted(edge_image[e].tolist()))
            if key not in best or edge_weight[e] > edge_weight[best[key]]:
                best[key] = e
    use = np.zeros(E, bool)
    use[list(best.values())] = True
    # relative rotation from i to j over the used edge of the pair
    rel = {i: {} for i in range(n)}
    for e in np.nonzero(use)[0]:
        a, b = edge_image[e]
        rel[a][b] = (e, edge_R[e])
        rel[b][a] = (e, edge_R[e].T)
    support = np.zeros(E, np.int32)
    for e in np.nonzero(use)[0]:
        a, b = edge_image[e]
        for c in set(rel[a]) & set(rel[b]):
            cyc = rel[c][a][1] @ rel[b][c][1] @ edge_R[e]
            support[e] += math.sqrt(max(0.0, (1.0 + np.trace(cyc)) / 4.0)) >= cos_half
    support = np.minimum(support, 65535)
    wsum = np.zeros(n, np.int64)
    for e in np.nonzero(use)[0]:
        wsum[edge_image[e]] += int(edge_weight[e])
    if root < 0:
        root = int(np.argmax(wsum)) if n else -1
    # Kruskal, greatest (support, weight, lowest edge) first
    order = sorted(np.nonzero(use)[0], key=lambda e: (-min(int(support[e]), 65535), -min(int(edge_weight[e]), 65535), e))
    comp = list(range(n))

    def find(i):
        while comp[i] != i:
            i = comp[i]
        return i
    tree = np.zeros(E, bool)
    for e in order:
        x, y = find(edge_image[e][0]), find(edge_image[e][1])
        if x != y:
            comp[x] = y
            tree[e] = True
    q = np.full((n, 4), np.nan)
    depth = np.full(n, -1)
    qe = {e: quat_of(edge_R[e]) for e in np.nonzero(valid)[0]}
    if root >= 0:
        q[root], depth[root] = (1.0, 0.0, 0.0, 0.0), 0
        queue = deque([root])
        while queue:
            i = queue.popleft()
            for j, (e, _) in rel[i].items():
                if tree[e] and depth[j] < 0:
                    qq = left(qe[e] if edge_image[e][0] == i else conj(qe[e])) @ q[i]
                    q[j], depth[j] = qq / np.linalg.norm(qq), depth[i] + 1
                    queue.append(j)
    inside = depth >= 0
    active = np.array([e for e in np.nonzero(use)[0] if inside[edge_image[e][0]]], np.int64)
    a_idx, b_idx = (edge_image[active, 0], edge_image[active, 1]) if active.size else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    wt = edge_weight[active].astype(np.float64)

    def residuals(edges):
        r = np.zeros((len(edges), 3))
        for k, e in enumerate(edges):
            a, b = edge_image[e]
            err = left(conj(q[b])) @ left(qe[e]) @ q[a]
            r[k] = 2.0 * err[1:] * (1.0 if err[0] >= 0 else -1.0)
        return r

    def cost_of(r):
        r2 = (r * r).sum(1)
        return float((wt * d2 * r2 / (d2 + r2)).sum())

    status, iters, n_pcg, last_step = (1, 0, 0, 0.0) if active.size else (3, 0, 0, 0.0)
    q0 = q.copy()
    cost0 = cost_of(residuals(active))
    free = np.array([i for i in range(n) if inside[i] and i != root], np.int64)
    slot = -np.ones(n, np.int64)
    slot[free] = np.arange(free.size)
    for _ in range(max_iters if active.size else 0):
        r = residuals(active)
        w = wt * (d2 / (d2 + (r * r).sum(1))) ** 2
        L = np.zeros((n, n))
        g = np.zeros((n, 3))
        for k in range(active.size):
            a, b = a_idx[k], b_idx[k]
            L[a, a] += w[k]; L[b, b] += w[k]; L[a, b] -= w[k]; L[b, a] -= w[k]
            g[b] += w[k] * r[k]; g[a] -= w[k] * r[k]
        Lf, gf = L[np.ix_(free, free)], g[free]
        if solver == "dense":
            om = np.linalg.solve(Lf, gf)
        else:
            diag = np.diag(Lf)[:, None]
            om = np.zeros_like(gf)
            res = gf.copy()
            z = res / diag
            p = z.copy()
            rz = rz0 = float((res * z).sum())
            for _k in range(pcg_iters):
                if rz <= pcg_tol ** 2 * rz0:
                    break
                Lp = Lf @ p
                alpha = rz / float((p * Lp).sum())
                n_pcg += 1
                om += alpha * p
                res -= alpha * Lp
                z = res / diag
                rz_new = float((res * z).sum())
                if rz_new <= pcg_tol ** 2 * rz0:
                    rz = rz_new
                    break
                p = z + (rz_new / rz) * p
                rz = rz_new
        if not np.isfinite(om).all():
            status = 2
            break
        for i in free:
            qq = left(q[i]) @ np.concatenate([[1.0], 0.5 * om[slot[i]]])
            q[i] = qq / np.linalg.norm(qq)
        iters += 1
        last_step = float(np.sqrt((om * om).sum(1)).max()) if free.size else 0.0
        if last_step < step_tol:
            status = 0
            break
    cost = cost_of(residuals(active))
    judged = [e for e in range(E) if valid[e] and inside[edge_image[e][0]] and inside[edge_image[e][1]]]
    chord = np.full(E, np.nan)
    if judged:
        chord[judged] = np.linalg.norm(residuals(judged), axis=1)
    state = np.zeros(E, np.uint8)
    state[valid] = 1
    state[judged] = np.where(chord[judged] <= max_chord, 2, 3)
    R = np.full((n, 3, 3), np.nan)
    for i in np.nonzero(inside)[0]:
        R[i] = rot_of(q[i])
    R0 = np.full((n, 3, 3), np.nan)
    for i in np.nonzero(inside)[0]:
        R0[i] = rot_of(q0[i])
    ok = state == 2
    counts = [int(inside.sum()), 0, int((~valid).sum()), int((valid & ~use).sum()), int(use.sum()), int(support.sum()), int(tree.sum()),
              int((tree & (support == 0)).sum()), int(depth.max()) if n else 0, n - int(tree.sum()), iters, n_pcg, int(ok.sum()),
              int((state == 3).sum()), status, root]
    return dict(R=R, R_start=R0, in_graph=inside, edge_state=state, edge_chord=chord, support=support, tree=tree, edge_use=use,
                counts=counts, info=[cost0, cost, last_step, float(chord[ok].max()) if ok.any() else 0.0], root=root)
