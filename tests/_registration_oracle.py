"""An independent statement of the correspondence table of the unposed images (rules 1-5): plain loops and dicts over numpy
arrays, no code shared with csrc/register_core.h.  The outputs have the library's shapes (sized by the bounds n and N, zero past P / C)."""
import math

import numpy as np


class BadInput(ValueError):
    def __init__(self, bits):
        super().__init__(f"error bits {bits}")
        self.bits = bits


def error_bits(offsets, obs_image, n, cam_offsets, cam_obs):
    """The three error bits: 1 an obs_image outside [0, n), 2 bad offsets, 4 a grouping that is not the stable one."""
    N, bits = len(obs_image), 0
    if any(not 0 <= int(i) < n for i in obs_image):
        bits |= 1
    off = [int(v) for v in offsets]
    if len(off) > 1 and (off[0] != 0 or off[-1] != N or any(b > e for b, e in zip(off, off[1:]))):
        bits |= 2
    want = {i: [] for i in range(n)}
    for o, i in enumerate(obs_image):
        if 0 <= int(i) < n:
            want[int(i)].append(o)
    co = [int(v) for v in cam_offsets]
    lists_ok = n == 0 or (co[0] == 0 and co[-1] == N and all(b <= e for b, e in zip(co, co[1:])))
    if lists_ok and not bits & 1:                                       # (with a bad image id there is no grouping to compare with)
        lists_ok = all([int(v) for v in cam_obs[co[i]:co[i + 1]]] == want[i] for i in range(n))
    if not lists_ok:
        bits |= 4
    return bits


def table(offsets, obs_image, obs_xy, xyz, status, posed, cam_offsets, cam_obs, min_corr):
    """-> dict of numpy arrays with the library's names, or raises BadInput(bits)."""
    n, N, T = len(posed), len(obs_image), len(offsets) - 1
    bits = error_bits(offsets, obs_image, n, cam_offsets, cam_obs)
    if bits:
        raise BadInput(bits)
    finite = lambda row: all(math.isfinite(float(v)) for v in row)
    per_image = {i: [] for i in range(n)}                               # image -> its correspondences (observation, track), ascending
    for j in range(T):
        for o in range(int(offsets[j]), int(offsets[j + 1])):
            i = int(obs_image[o])
            if posed[i] == 0 and status[j] == 0 and finite(xyz[j]) and finite(obs_xy[o]):
                per_image[i].append((o, j))
    for i in per_image:
        per_image[i].sort()
    out = dict(n_corr=np.zeros(n, np.int32), cand_rank=np.full(n, -1, np.int32), cand_image=np.zeros(n, np.int32),
               cand_offsets=np.zeros(n + 1, np.int64), corr_xyz=np.zeros((N, 3), np.float32), corr_xy=np.zeros((N, 2), np.float32),
               corr_bid=np.zeros(N, np.int64), corr_obs=np.zeros(N, np.int32), counts=np.zeros(8, np.int64))
    C = P = 0
    for i in range(n):
        out["n_corr"][i] = len(per_image[i])
        if posed[i] == 0 and len(per_image[i]) >= min_corr:
            out["cand_rank"][i], out["cand_image"][P], out["cand_offsets"][P] = P, i, C
            for o, j in per_image[i]:
                out["corr_xyz"][C], out["corr_xy"][C], out["corr_bid"][C], out["corr_obs"][C] = xyz[j], obs_xy[o], P, o
                C += 1
            P += 1
    out["cand_offsets"][P] = C
    unposed = [i for i in range(n) if posed[i] == 0]
    out["counts"][:] = [C, P, 0, len(unposed), sum(1 for i in unposed if per_image[i]), sum(len(v) for v in per_image.values()),
                        max([len(v) for v in per_image.values()], default=0), 0]
    return out


def groups(obs_image, n):
    """cam_offsets, cam_obs: the stable grouping by image, as the library's Python makes it."""
    obs_image = np.asarray(obs_image, np.int32)
    cam_obs = np.argsort(obs_image, kind="stable").astype(np.int32)
    cam_offsets = np.zeros(n + 1, np.int64)
    cam_offsets[1:] = np.cumsum(np.bincount(obs_image, minlength=n)[:n])
    return cam_offsets, cam_obs


def umeyama(src, dst):
    """Similarity (s, R, t) with dst ~ s R src + t, least squares (Umeyama 1991), float64."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    ms, md = src.mean(0), dst.mean(0)
    xs, xd = src - ms, dst - md
    U, D, Vt = np.linalg.svd(xd.T @ xs / len(src))
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    s = np.trace(np.diag(D) @ S) / (xs ** 2).sum() * len(src)
    return s, R, md - s * R @ ms


def aligned_errors(T, T_true, which):
    """Poses T [n,4,4] against T_true after the similarity that aligns the camera centres of `which` -> (largest rotation error in
    degrees, largest centre error)."""
    idx = np.nonzero(which)[0]
    centre = lambda M: -M[:3, :3].T @ M[:3, 3]
    c, c_true = np.stack([centre(T[i]) for i in idx]), np.stack([centre(T_true[i]) for i in idx])
    s, R, t = umeyama(c, c_true)
    rot = cen = 0.0
    for k, i in enumerate(idx):
        Rw = T[i, :3, :3] @ R.T                                         # camera from the true world
        dR = Rw @ T_true[i, :3, :3].T
        rot = max(rot, float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))))
        cen = max(cen, float(np.linalg.norm(s * R @ c[k] + t - c_true[k])))
    return rot, cen
