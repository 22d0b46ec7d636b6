"""An independent numpy statement of view-graph calibration for the tests: matrices, ``numpy.linalg.svd`` and
``einsum`` instead of the written-out products of csrc/calib_core.h, plain numpy sums instead of the ordered ones.

The residual norm is taken from the singular values, ``(s1^2 - s2^2) / (s1^2 + s2^2)``, not from the nine-component formula under
test (for the rank-2 matrices of the scenes the two agree to rounding).  The Jacobian is the analytic form written with einsum.
``solver='dense'`` solves the damped normal equations with ``numpy.linalg.solve``; ``solver='pcg'`` repeats the Jacobi-preconditioned
conjugate gradients, so its integer outputs can be compared one for one."""
import numpy as np

DEFAULTS = dict(loss=0.05, max_resid=0.05, prior_weight=1e-3, weight_cap=100, bound_lo=0.2, bound_hi=5.0, min_edges=1, max_iters=50,
                pcg_iters=30, pcg_tol=1e-2, ftol=1e-9)
P2 = np.diag([1.0, 1.0, 0.0])


def centred(F, pp_a, pp_b):
    Ta, Tb = np.eye(3), np.eye(3)
    Ta[:2, 2], Tb[:2, 2] = pp_a, pp_b
    Fp = Tb.T @ F @ Ta
    return Fp / np.linalg.norm(Fp)


def essential(Fp, fa, fb):
    """diag(f_b, f_b, 1) F' diag(f_a, f_a, 1) for every edge"""
    return np.einsum("ei,eij,ej->eij", np.stack([fb, fb, np.ones_like(fb)], 1), Fp, np.stack([fa, fa, np.ones_like(fa)], 1))


def resid_svd(Em):
    s = np.linalg.svd(Em, compute_uv=False)
    return (s[:, 0] ** 2 - s[:, 1] ** 2) / (s[:, 0] ** 2 + s[:, 1] ** 2)


def rho_and_jacobian(Em, ma, mb):
    """rho [E,9] and d rho / d m on side a and b [E,9] (analytic)."""
    EEt = np.einsum("eik,ejk->eij", Em, Em)
    t = np.einsum("eii->e", EEt)
    N = 2 * np.einsum("eij,ejk->eik", EEt, Em) - t[:, None, None] * Em
    rho = N / t[:, None, None] ** 1.5
    out = [rho.reshape(-1, 9)]
    for dE in (np.einsum("eij,jk->eik", Em, P2) / ma[:, None, None], np.einsum("ij,ejk->eik", P2, Em) / mb[:, None, None]):
        A = np.einsum("eik,ejk->eij", dE, Em)
        dN = (2 * (np.einsum("eij,ejk->eik", A + A.transpose(0, 2, 1), Em) + np.einsum("eij,ejk->eik", EEt, dE))
              - 2 * np.einsum("eii->e", A)[:, None, None] * Em - t[:, None, None] * dE)
        dt = 2 * np.einsum("eii->e", A)
        out.append((dN / t[:, None, None] ** 1.5 - 1.5 * N * dt[:, None, None] / t[:, None, None] ** 2.5).reshape(-1, 9))
    return out


def calibrate(edge_image, edge_F, edge_weight, pp, f0, group, G, solver="dense", **params):
    p = {**DEFAULTS, **params}
    ei, F, w = np.asarray(edge_image, np.int64).reshape(-1, 2), np.asarray(edge_F, np.float64), np.asarray(edge_weight)
    group = np.asarray(group, np.int64)
    E, n = len(ei), len(f0)
    out = dict(focal_scale=np.zeros(G), focal=np.zeros(n), edge_resid=np.zeros(E), edge_state=np.zeros(E, np.uint8),
               group_state=np.zeros(G, np.uint8), counts=np.zeros(16, np.int64), info=np.zeros(4))
    bits = 0
    if ((ei < 0) | (ei >= n)).any() or (ei[:, 0] == ei[:, 1]).any():
        bits |= 1
    if ((group < 0) | (group >= G)).any():
        bits |= 2
    if not (np.isfinite(f0).all() and (f0 > 0).all() and np.isfinite(pp).all()):
        bits |= 8
    if bits:
        out["counts"][1] = bits
        return out
    a, b = ei[:, 0], ei[:, 1]
    valid = (w > 0) & np.isfinite(F).all((1, 2))
    Fp = np.zeros((E, 3, 3))
    for e in range(E):
        if valid[e]:
            with np.errstate(all="ignore"):
                M = centred(F[e], pp[a[e]], pp[b[e]])
            valid[e] = np.isfinite(M).all()
            Fp[e] = M if valid[e] else 0
    v = np.nonzero(valid)[0]
    omega = np.minimum(w, p["weight_cap"]) / p["weight_cap"]
    ga, gb = group[a], group[b]
    inc = np.bincount(np.r_[ga[v], gb[v]], minlength=G)
    state = np.where(inc == 0, 0, np.where(inc >= p["min_edges"], 2, 1)).astype(np.uint8)
    free = state == 2
    fidx = np.nonzero(free)[0]
    col = -np.ones(G, np.int64)
    col[fidx] = np.arange(len(fidx))
    loss2, pw = p["loss"] ** 2, p["prior_weight"]

    def q_of(m):
        Em = essential(Fp[v], f0[a[v]] * m[ga[v]], f0[b[v]] * m[gb[v]])
        return resid_svd(Em) ** 2 if len(v) else np.zeros(0)

    def cost_of(m):
        q = q_of(m)
        return float((omega[v] * loss2 * q / (loss2 + q)).sum() + pw * ((m[free] - 1) ** 2).sum())

    m = np.ones(G)
    cost = cost0 = cost_of(m)
    lam, status, trials, accepted, n_pcg, n_bound, last_step = 1e-4, 1, 0, 0, 0, 0, 0.0
    done = False
    if len(v) == 0 or len(fidx) == 0:
        done, status = True, 3
    elif cost == 0.0:
        done, status = True, 0
    for _ in range(p["max_iters"]):
        if done:
            break
        Em = essential(Fp[v], f0[a[v]] * m[ga[v]], f0[b[v]] * m[gb[v]])
        rho, ja, jb = rho_and_jacobian(Em, m[ga[v]], m[gb[v]])
        q = (rho ** 2).sum(1)
        wgt = omega[v] * (loss2 / (loss2 + q)) ** 2
        J = np.zeros((len(v) * 9, G))
        rows = np.arange(len(v) * 9).reshape(-1, 9)
        np.add.at(J, (rows, ga[v][:, None]), ja)
        np.add.at(J, (rows, gb[v][:, None]), jb)
        sw = np.repeat(wgt, 9)
        Hm = (J * sw[:, None]).T @ J
        g = -(J * sw[:, None]).T @ rho.reshape(-1)
        Hf = Hm[np.ix_(fidx, fidx)] + pw * np.eye(len(fidx))
        gf = g[fidx] - pw * (m[fidx] - 1)
        d = np.diag(Hf).copy()
        dd = np.where(d == 0, lam, d * (1 + lam))
        A = Hf - np.diag(d) + np.diag(dd)
        bad = not (dd > 0).all()
        if solver == "dense":
            x = np.linalg.solve(A, gf) if not bad else np.zeros_like(gf)
        else:
            x, r = np.zeros_like(gf), gf.copy()
            z = r / dd
            pd = z.copy()
            rz = rz0 = float(r @ z)
            if rz > 0:
                for _k in range(p["pcg_iters"]):
                    Ap = A @ pd
                    pAp = float(pd @ Ap)
                    if not pAp > 0:
                        break
                    n_pcg += 1
                    alpha = rz / pAp
                    x, r = x + alpha * pd, r - alpha * Ap
                    z = r / dd
                    rz_new = float(r @ z)
                    beta, rz = rz_new / rz, rz_new
                    if rz <= p["pcg_tol"] ** 2 * rz0:
                        break
                    pd = z + beta * pd
        mt = m.copy()
        mt[fidx] = m[fidx] + x
        trials += 1
        oob = bool(((mt[fidx] <= p["bound_lo"]) | (mt[fidx] >= p["bound_hi"])).any())
        n_bound += oob
        bad = bad or not np.isfinite(mt).all()
        cost_t = cost_of(mt) if not bad else np.inf
        if not bad and not oob and cost_t < cost:
            gain, cost, m = cost - cost_t, cost_t, mt
            accepted += 1
            last_step = float(np.abs(x).max()) if len(x) else 0.0
            lam = max(lam / 10, 1e-10)
            if gain <= p["ftol"] * cost:
                done, status = True, 0
        else:
            lam *= 10
            if lam > 1e10:
                done, status = True, 2
    resid = np.zeros(E)
    resid[v] = np.sqrt(q_of(m))
    out["focal_scale"], out["focal"], out["edge_resid"] = m, f0 * m[group], resid
    out["edge_state"] = np.where(valid, np.where(resid > p["max_resid"], 2, 1), 0).astype(np.uint8)
    out["group_state"] = state
    out["counts"][:9] = [trials, 0, accepted, n_pcg, len(v), len(fidx), int((out["edge_state"] == 2).sum()), status, n_bound]
    out["info"][:] = [cost0, cost, lam, last_step]
    return out
