"""An independent numpy statement of global positioning (include/loftr_global.h) for tests/test_position.py: dictionaries
for the tree, a dense Jacobian of the active residuals, numpy sums.  Two legs: ``solver="dense"`` solves the damped normal equations of
a trial over all unknowns at once (no elimination); ``solver="pcg"`` eliminates scales and points with dense blocks and repeats the
routine's conjugate gradients on the reduced system, so that every count, the iterations included, can be compared."""
import numpy as np

LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-4, 1e-10, 1e10


def bearings(xy, image, K, R):
    out = np.zeros((len(image), 3))
    for o, i in enumerate(image):
        ray = np.linalg.solve(K[i], np.array([xy[o, 0], xy[o, 1], 1.0], np.float64))
        w = R[i].T @ ray
        out[o] = w / np.linalg.norm(w)
    return out


def tree_levels(n, in_graph, root, tree_image, tree_t, R):
    """-> (depth by image, start centres by image, edges without a direction, error) by a breadth-first walk over dictionaries."""
    nb = {}
    for e, (a, b) in enumerate(tree_image):
        if not (0 <= a < n and 0 <= b < n) or a == b or not in_graph[a] or not in_graph[b]:
            return None, None, 0, True
        nb.setdefault(int(a), []).append((int(b), e, +1.0))
        nb.setdefault(int(b), []).append((int(a), e, -1.0))
    gamma, nodir = {}, 0
    for e, (a, b) in enumerate(tree_image):
        t = np.asarray(tree_t[e], np.float64)
        nt = np.linalg.norm(t) if np.isfinite(t).all() else 0.0
        if not (nt > 0 and np.isfinite(nt)):
            gamma[e] = np.zeros(3)
            nodir += 1
        else:
            gamma[e] = -(R[b].T @ t) / nt
    depth, centre, used = {root: 0}, {root: np.zeros(3)}, set()
    frontier = [root]
    while frontier:
        nxt = []
        for a in frontier:
            for b, e, sign in nb.get(a, []):
                if e in used:
                    continue
                if b in depth:                       # an end reached twice
                    return None, None, 0, True
                used.add(e)
                depth[b] = depth[a] + 1
                centre[b] = centre[a] + sign * gamma[e]
                nxt.append(b)
        frontier = nxt
    if len(used) != len(tree_image):                 # an edge never reached
        return None, None, 0, True
    return depth, centre, nodir, False


def positions(offsets, obs_image, obs_xy, K, R, in_graph, root, tree_image, tree_t, huber=0.1, max_iters=50, pcg_iters=30, pcg_tol=1e-2,
              ftol=1e-7, min_cam_obs=8, solver="pcg"):
    offsets, image = np.asarray(offsets, np.int64), np.asarray(obs_image, np.int64)
    xy = np.asarray(obs_xy, np.float32).astype(np.float64)
    K, R = np.asarray(K, np.float64), np.asarray(R, np.float64)
    n, T, N = len(in_graph), len(offsets) - 1, len(image)
    track = np.repeat(np.arange(T), np.diff(offsets))
    depth, centre, nodir, bad = tree_levels(n, in_graph, root, np.asarray(tree_image), np.asarray(tree_t), R)
    assert not bad
    graph = np.array([bool(in_graph[i]) and i in depth for i in range(n)])
    v = np.zeros((N, 3))
    usable = np.zeros(N, bool)
    for o in range(N):
        if graph[image[o]] and np.isfinite(xy[o]).all():
            v[o] = bearings(xy[o:o + 1], image[o:o + 1], K, R)[0]
            usable[o] = np.isfinite(v[o]).all()
    point_active = np.bincount(track[usable], minlength=T) >= 2 if N else np.zeros(T, bool)
    active = usable & point_active[track] if N else usable
    n_cam = np.bincount(image[active], minlength=n) if N else np.zeros(n, int)
    cam_state = np.zeros(n, np.uint8)
    for i in range(n):
        if graph[i]:
            cam_state[i] = 3 if i == root else (2 if n_cam[i] >= min_cam_obs else 1)
    c = np.full((n, 3), np.nan)
    for i in range(n):
        if graph[i]:
            c[i] = centre[i]
    X = np.zeros((T, 3))
    d = np.zeros(N)
    for t in range(T):
        idx = [o for o in range(offsets[t], offsets[t + 1]) if active[o]]
        if idx:
            X[t] = np.mean([c[image[o]] + v[o] for o in idx], axis=0)
            for o in idx:
                e = X[t] - c[image[o]]
                d[o] = v[o] @ e / (e @ e) if e @ e > 0 else 0.0
    start = dict(centres=c.copy(), X=X.copy(), d=d.copy())

    obs = np.nonzero(active)[0]
    free = np.nonzero(cam_state == 2)[0]
    pts = np.nonzero(point_active)[0]
    col_c = {int(i): 3 * k for k, i in enumerate(free)}
    col_X = {int(t): 3 * len(free) + 3 * k for k, t in enumerate(pts)}
    col_d = {int(o): 3 * len(free) + 3 * len(pts) + k for k, o in enumerate(obs)}
    nc, nX, nd = 3 * len(free), 3 * len(pts), len(obs)

    def residuals(c, X, d):
        return np.stack([v[o] - d[o] * (X[track[o]] - c[image[o]]) for o in obs]) if len(obs) else np.zeros((0, 3))

    def loss(r):
        nr = np.linalg.norm(r, axis=1)
        out = (huber > 0) & ~(nr <= huber)
        w = np.where(out, huber / np.where(out, nr, 1.0), 1.0)
        rho = np.where(out, 2 * huber * nr - huber * huber, nr * nr)
        return w, float(rho.sum())

    w, cost = loss(residuals(c, X, d))
    cost0, lam, status = cost, LAMBDA0, 1
    trials = accepted = n_pcg = 0
    last_step = 0.0
    done = False
    if len(obs) == 0 or len(free) == 0:
        done, status = True, 3
    elif cost == 0.0:
        done, status = True, 0
    weights_last = w
    while not done and trials < max_iters:
        r = residuals(c, X, d)
        w, _ = loss(r)
        J = np.zeros((3 * len(obs), nc + nX + nd))
        for k, o in enumerate(obs):
            e = X[track[o]] - c[image[o]]
            rows = slice(3 * k, 3 * k + 3)
            if int(image[o]) in col_c:
                J[rows, col_c[int(image[o])]:col_c[int(image[o])] + 3] = d[o] * np.eye(3)
            J[rows, col_X[int(track[o])]:col_X[int(track[o])] + 3] = -d[o] * np.eye(3)
            J[rows, col_d[int(o)]] = -e
        W = np.repeat(w, 3)
        H = J.T @ (W[:, None] * J)
        b = -J.T @ (W * r.reshape(-1))
        dg = np.diag(H).copy()
        H[np.diag_indices_from(H)] = np.where(dg == 0.0, lam, dg * (1.0 + lam))
        bad = False
        try:
            if solver == "dense":
                delta = np.linalg.solve(H, b)
            else:
                Hcc, HcX, Hcd = H[:nc, :nc], H[:nc, nc:nc + nX], H[:nc, nc + nX:]
                HXX, HXd, Hdd = H[nc:nc + nX, nc:nc + nX], H[nc:nc + nX, nc + nX:], np.diag(H)[nc + nX:]
                bc, bX, bd = b[:nc], b[nc:nc + nX], b[nc + nX:]
                # eliminate d
                Acc = Hcc - (Hcd / Hdd) @ Hcd.T
                AcX = HcX - (Hcd / Hdd) @ HXd.T
                AXX = HXX - (HXd / Hdd) @ HXd.T
                gc, gX = bc - Hcd @ (bd / Hdd), bX - HXd @ (bd / Hdd)
                # eliminate X
                AXXi = np.linalg.inv(AXX)
                S = Acc - AcX @ AXXi @ AcX.T
                rhs = gc - AcX @ AXXi @ gX
                Minv = np.zeros_like(Acc)
                for k in range(len(free)):
                    Minv[3 * k:3 * k + 3, 3 * k:3 * k + 3] = np.linalg.inv(Acc[3 * k:3 * k + 3, 3 * k:3 * k + 3])
                x = np.zeros(nc)
                rr = rhs.copy()
                z = Minv @ rr
                p = z.copy()
                rz = rz0 = rr @ z
                stop = not rz > 0
                for _ in range(pcg_iters):
                    if stop:
                        break
                    Sp = S @ p
                    psp = p @ Sp
                    if not psp > 0:
                        break
                    n_pcg += 1
                    alpha = rz / psp
                    x += alpha * p
                    rr -= alpha * Sp
                    z = Minv @ rr
                    rz_new = rr @ z
                    beta, rz = rz_new / rz, rz_new
                    if rz <= pcg_tol ** 2 * rz0:
                        break
                    p = z + beta * p
                dX = AXXi @ (gX - AcX.T @ x)
                dd = (bd - Hcd.T @ x - HXd.T @ dX) / Hdd
                delta = np.concatenate([x, dX, dd])
        except np.linalg.LinAlgError:
            bad = True
        trials += 1
        if not bad and np.isfinite(delta).all():
            ct, Xt, dt = c.copy(), X.copy(), d.copy()
            for i, k in col_c.items():
                ct[i] += delta[k:k + 3]
            for t, k in col_X.items():
                Xt[t] += delta[k:k + 3]
            for o, k in col_d.items():
                dt[o] += delta[k]
            wt, cost_t = loss(residuals(ct, Xt, dt))
        else:
            cost_t = np.inf
        if cost_t < cost:
            gain = cost - cost_t
            c, X, d, cost = ct, Xt, dt, cost_t
            accepted += 1
            weights_last = wt
            last_step = float(np.sqrt(max((delta[k:k + 3] @ delta[k:k + 3] for k in col_c.values()), default=0.0)))
            lam = max(lam / 10.0, LAMBDA_MIN)
            if gain <= ftol * cost:
                done, status = True, 0
        else:
            lam *= 10.0
            if lam > LAMBDA_MAX:
                done, status = True, 2
    obs_state = np.zeros(N, np.uint8)
    obs_state[active] = np.where(d[active] > 0, 1, 2)
    xyz = np.where(point_active[:, None], X, np.nan).astype(np.float32)
    weights = np.zeros(N)
    weights[obs] = loss(residuals(c, X, d))[0] if len(obs) else []
    counts = [trials, 0, accepted, n_pcg, int(active.sum()), int(point_active.sum()), len(free), int((obs_state == 2).sum()), nodir, status,
              max(depth.values()), int(graph.sum()), int((cam_state == 1).sum()), 0, 0, 0]
    return dict(centres=c, xyz=xyz, depth_scale=np.where(active, d, 0.0), obs_state=obs_state, cam_state=cam_state,
                point_active=point_active, counts=counts, info=[cost0, cost, lam, last_step], start=start, weights=weights, X=X)


def align_error(c, c_gt):
    """The largest distance between the centres c and the truth after the least-squares similarity (Umeyama) c -> c_gt."""
    mu, mg = c.mean(0), c_gt.mean(0)
    a, g = c - mu, c_gt - mg
    U, sv, Vt = np.linalg.svd(g.T @ a)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    Rm = U @ D @ Vt
    s = (sv * np.diag(D)).sum() / (a * a).sum()
    return float(np.linalg.norm(s * (Rm @ a.T).T - g, axis=1).max())
