"""Global positioning: a centre for every camera of the view graph and a point for every track, all at once, from averaged rotations.

The incremental loop (registration.py) starts from one pair and registers images round by round, so a later pose inherits the drift of
the earlier ones.  With one rotation per image already fixed by rotation averaging (rotations.py), the camera centres ``c_i``, the
points ``X_k`` and one scale ``d_o`` per observation can be solved together from ``r_o = v_o - d_o (X_k - c_i)`` with ``v_o`` the
bearing of the observation in the world frame, under a Huber loss.  Unlike positions from pairwise translation directions, this is not
degenerate when the cameras move along a line::

    pos = global_positions(offsets, obs_image, obs_xy, K, rot.R, rot.in_graph, rot.root, tree_image, tree_t)   # GlobalPositions
    pos.centres, pos.xyz, pos.T_cam_from_world, pos.posed

    pos = sfm.global_positions(K, rot)                   # the same over the consistent tracks of a pair list (atlas.py)
    rec = sfm.reconstruct_global(K)                      # rotation averaging -> global positions -> triangulate / adjust

The rule (include/loftr_global.h): start values along the spanning tree that rotation averaging returns, Levenberg-Marquardt
with the scales eliminated first, then the points, and the reduced system over the centres solved by block-Jacobi preconditioned
conjugate gradients.  The host routine ``loftr_global_positions_host`` defines it in fp64 with every sum in a stated order (CPU tensors /
numpy arrays run it); the HIP kernels reproduce it bit for bit (GPU tensors run them; there is no silent fallback either way).

The defaults (``huber``, ``max_iters``, ``pcg_iters``, ``pcg_tol``, ``ftol``, ``min_cam_obs``) are those of a prototype on synthetic rings and
lines of 10 to 16 cameras; they are UNVALIDATED on real data.
"""
import numpy as np
import torch

from . import _tracks, ops_global

_ARGS = ("offsets", "obs_image", "obs_xy", "K", "R", "in_graph", "tree_image", "tree_t")


class GlobalPositions:
    """What ``global_positions`` returns (tensors on the device of the input).

    ``centres [n,3] f64`` (NaN outside the graph), ``xyz [T,3] f32`` (NaN for an inactive point), ``depth_scale [N] f64``, ``obs_state [N]
    u8`` (``ops_global.POSITION_OBS_STATES``), ``cam_state [n] u8`` (``ops_global.POSITION_CAM_STATES``: 0 outside, 1 chained only, 2
    solved, 3 root), ``point_active [T] bool``, ``T_cam_from_world [n,4,4] f64`` (``[R | -R c]``, NaN where ``cam_state < 2``), ``posed [n]
    bool`` (``cam_state >= 2``); ``stats``: the counts and info by name (``ops_global.POSITION_NAMES``, ``POSITION_INFO``).  The scale of
    the result is whatever the damping left."""

    FIELDS = ("centres", "xyz", "depth_scale", "obs_state", "cam_state", "point_active", "T_cam_from_world", "posed")

    def __init__(self, root, stats, **tensors):
        self.root, self.stats = root, stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])

    def to_host(self):
        """dict of numpy arrays (plus 'root' and 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out.update(root=self.root, stats=dict(self.stats))
        return out


def _integer(what, name, v, lo):
    if not isinstance(v, int) or isinstance(v, bool) or v < lo:
        raise ValueError(f"{what}: {name} must be an integer >= {lo}, got {v!r}")


def global_positions(offsets, obs_image, obs_xy, K, R, in_graph, root, tree_image, tree_t, huber=0.1, max_iters=50, pcg_iters=30,
                     pcg_tol=1e-2, ftol=1e-7, min_cam_obs=8, timings=None):
    """Camera centres, points and scales from tracks and fixed rotations -> ``GlobalPositions``.

    ``offsets [T+1]``, ``obs_image [N]``, ``obs_xy [N,2]``: the tracks in CSR form, as bundle adjustment takes them; ``K [n,3,3]``; ``R
    [n,3,3]`` camera-from-world, ``in_graph [n]`` and ``root`` from ``GlobalRotations``; ``tree_image [Et,2]`` (a, b) and ``tree_t [Et,3]``:
    the pairs of its spanning tree with the translation of each (``x_b = R_ab x_a + t``; only the direction counts).  CPU tensors or
    numpy arrays run the defining host routine; GPU tensors (all of them, on one device) run the kernels.  ``huber``: the scale of the
    loss, a chord between unit bearings (0: the square); ``max_iters``: trials of Levenberg-Marquardt; ``pcg_iters``, ``pcg_tol``: the
    conjugate gradients of a trial; ``ftol``: the relative gain that ends the call; ``min_cam_obs``: a camera with fewer active
    observations keeps its start value along the tree.  These defaults are a prototype's and UNVALIDATED on real data.  One readback
    (counts and info); a bad input raises ValueError.  timings: a list that receives (stage, ms) pairs of the GPU launches."""
    what = "global_positions"
    args = [offsets, obs_image, obs_xy, K, R, in_graph, tree_image, tree_t]
    gpu = _tracks.one_device(what, _ARGS, args)
    for name, a in (("offsets", offsets), ("obs_image", obs_image), ("tree_image", tree_image)):
        _tracks.integers(what, name, a)
    for name, v in (("root", root), ("max_iters", max_iters), ("pcg_iters", pcg_iters), ("min_cam_obs", min_cam_obs)):
        _integer(what, name, v, -(1 << 31) if name == "root" else 0)
    if not (float(huber) >= 0.0 and np.isfinite(float(huber))) or not 0.0 <= float(pcg_tol) < 1.0 or not (float(ftol) >= 0.0):
        raise ValueError(f"{what}: huber and ftol must be >= 0 and pcg_tol must lie in [0, 1), got {huber!r}, {ftol!r}, {pcg_tol!r}")
    tensor = lambda x: x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    off = tensor(offsets).to(torch.int64).reshape(-1)
    im = tensor(obs_image).to(torch.int32).reshape(-1)
    xy = tensor(obs_xy).to(torch.float32).reshape(-1, 2)
    Km = tensor(K).to(torch.float64).reshape(-1, 3, 3)
    Rm = tensor(R).to(torch.float64).reshape(-1, 3, 3)
    ing = tensor(in_graph).reshape(-1).to(torch.uint8)
    ti = tensor(tree_image).to(torch.int32).reshape(-1, 2)
    tt = tensor(tree_t).to(torch.float64).reshape(-1, 3)
    n = int(ing.shape[0])
    if n < 1 or Km.shape[0] != n or Rm.shape[0] != n or xy.shape[0] != im.shape[0] or tt.shape[0] != ti.shape[0] or off.shape[0] < 1:
        raise ValueError(f"{what}: expected offsets [T+1], obs_image [N], obs_xy [N,2], K [n,3,3], R [n,3,3], in_graph [n] with n >= 1, "
                         f"tree_image [Et,2] and tree_t [Et,3]")
    params = dict(huber=float(huber), max_iters=max_iters, pcg_iters=pcg_iters, pcg_tol=float(pcg_tol), ftol=float(ftol),
                  min_cam_obs=min_cam_obs)
    if gpu:
        cam_offsets, cam_obs = _tracks.group_by_image(im.clamp(0, n - 1), n)
        a = [x.contiguous() for x in (off, im, xy, cam_offsets, cam_obs, Km, Rm, ing, ti, tt)]
        out = ops_global.global_positions(*a, root, timings=timings, **params)
    else:
        cam_offsets, cam_obs = _tracks.group_by_image(im.clamp(0, n - 1).numpy(), n)
        a = [x.contiguous().numpy() for x in (off, im, xy)] + [cam_offsets, cam_obs] + [x.contiguous().numpy() for x in (Km, Rm, ing, ti, tt)]
        out = {k: torch.from_numpy(v) for k, v in ops_global.global_positions_host(*a, root, **params).items()}
    word = torch.cat([out["counts"], out["info"].view(torch.int64)]).cpu()  # the one readback
    counts = word[:ops_global.POSITION_COUNTS].tolist()
    info = word[ops_global.POSITION_COUNTS:].view(torch.float64).tolist()
    _tracks.raise_error_bits(what, counts[1], ops_global.POSITION_ERRORS)
    stats = {name: counts[i] for i, name in enumerate(ops_global.POSITION_NAMES) if name != "error_bits"}
    stats.update(zip(ops_global.POSITION_INFO, info))
    stats.update(status_name=ops_global.POSITION_STATUS[counts[9]], n_images=n, n_tracks=int(off.shape[0]) - 1, n_obs=int(im.shape[0]), **params)
    posed = out["cam_state"] >= 2
    c = out["centres"]                                                      # -R c in single multiplications and additions: no
    t = -((Rm[:, :, 0] * c[:, 0:1] + Rm[:, :, 1] * c[:, 1:2]) + Rm[:, :, 2] * c[:, 2:3])   # matrix product, so both devices give the same bits
    Tm = torch.eye(4, dtype=torch.float64, device=Rm.device).repeat(n, 1, 1)
    Tm[:, :3, :3], Tm[:, :3, 3] = Rm, t
    Tm = torch.where(posed[:, None, None], Tm, torch.full_like(Tm, float("nan")))          # (a mask, not an index list: nothing is read back)
    return GlobalPositions(root, stats, centres=out["centres"], xyz=out["xyz"], depth_scale=out["depth_scale"], obs_state=out["obs_state"],
                           cam_state=out["cam_state"], point_active=out["point_active"] != 0, T_cam_from_world=Tm, posed=posed)
