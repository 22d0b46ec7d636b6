"""Rotation averaging over the view graph: one rotation per image from the pairwise ones, and the pairs that disagree.

A wrongly matched pair (two sides of a symmetric facade, two similar corridors) has a five-point model with many inliers, so
verification passes it and its matches bend every track they touch.  The defence is at pair level: relative rotations around a cycle of
the view graph compose to the identity, so an edge that no cycle supports is suspect, and a robust average of all edges gives every
edge a residual::

    rot = average_rotations(edge_image, edge_R, edge_weight, n_images)      # GlobalRotations
    rot.R, rot.in_graph                                                     # camera-from-world rotations, gauge: R[root] = I
    rot.edge_ok, rot.edge_err_deg                                           # the verdict of every pair and its angle to the average

    rot = sfm.rotation_averaging(K)                                         # the same over the rows of a pair list (atlas.py)
    rec = sfm.reconstruct(K, rotations=True)                                # ... and the reconstruction without the rejected rows

The rule (include/loftr_hip.h): cycle support per edge, a maximum spanning tree that prefers supported then heavy edges,
start values along the tree, Gauss-Newton with a Geman-McClure loss on the chord of the residual rotation, the step solved by
Jacobi-preconditioned conjugate gradients.  The host routine ``loftr_rotation_averaging_host`` defines it in fp64 with every sum in a
stated order (CPU tensors / numpy arrays run it); the HIP kernels reproduce it bit for bit (GPU tensors run them; there is no silent
fallback either way).  Only the component of the root is solved, which need not be the largest one.

The defaults (``cycle_deg``, ``loss_deg``, ``max_err_deg``) come from synthetic view graphs (0.5 degrees of noise per axis, 8 to 30 % of
the edges replaced by random rotations); they are UNVALIDATED on real pair lists.
"""
import math

import numpy as np
import torch

from . import _tracks, ops

_ARGS = ("edge_image", "edge_R", "edge_weight")


class GlobalRotations:
    """What ``average_rotations`` returns (tensors on the device of the input).

    ``R [n,3,3] f64`` camera-from-world (identity at ``root``, NaN outside the graph), ``in_graph [n] bool``, ``edge_state [E] u8``
    (``ops.ROTATION_STATES``: 0 invalid, 1 an end outside the graph, 2 ok, 3 outlier), ``edge_chord [E] f64`` (the chord ``2 sin(err / 2)`` of
    an edge against the averaged rotations, NaN without a verdict), ``support [E] i32`` (cycles that vouch for a used edge), ``tree [E]
    bool``, ``edge_use [E] bool`` (the edge that stands for its pair), ``root``; ``stats``: the counts and info by name
    (``ops.ROTATION_NAMES``, ``ops.ROTATION_INFO``; ``n_tree_unsupported > 0`` is the warning sign: the tree had to cross an edge no cycle
    vouches for)."""

    FIELDS = ("R", "in_graph", "edge_state", "edge_chord", "support", "tree", "edge_use")

    def __init__(self, root, stats, **tensors):
        self.root, self.stats = root, stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])

    @property
    def edge_ok(self):
        return self.edge_state == 2

    @property
    def edge_err_deg(self):
        """The angle of every judged edge to the averaged rotations, degrees (derived here; not part of the bit-for-bit contract)."""
        return torch.rad2deg(2.0 * torch.asin((0.5 * self.edge_chord).clamp(max=1.0)))

    def to_host(self):
        """dict of numpy arrays (plus 'root' and 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out.update(root=self.root, stats=dict(self.stats))
        return out


def _integer(what, name, v, lo):
    if not isinstance(v, int) or isinstance(v, bool) or v < lo:
        raise ValueError(f"{what}: {name} must be an integer >= {lo}, got {v!r}")


def _valid(edge_R, edge_weight):
    """Rule 2 in torch, for the choice among duplicates only (the routine decides validity itself and clears the others)."""
    m = edge_R.reshape(-1, 9)
    det = (m[:, 0] * (m[:, 4] * m[:, 8] - m[:, 5] * m[:, 7]) - m[:, 1] * (m[:, 3] * m[:, 8] - m[:, 5] * m[:, 6])
           + m[:, 2] * (m[:, 3] * m[:, 7] - m[:, 4] * m[:, 6]))
    gram = edge_R.transpose(1, 2) @ edge_R - torch.eye(3, dtype=edge_R.dtype, device=edge_R.device)
    return (edge_weight > 0) & torch.isfinite(m).all(1) & (det > 0) & (gram.abs().reshape(-1, 9).amax(1) <= 1e-3)


def view_graph(edge_image, edge_R, edge_weight, n_images):
    """The integer plumbing of the call, stable sorts only -> (adj_offsets [n+1] i64, adj_edge [2E] i32, edge_use [E] u8) on the device of
    the input: the edges of every image ordered by (neighbour, edge), and the heaviest valid edge of every unordered pair (ties: the
    lowest index).  Bad image ids are caught by the routine, so they are only clamped here."""
    n, E, dev = n_images, edge_image.shape[0], edge_image.device
    im = edge_image.to(torch.int64).reshape(-1, 2)
    cl = im.clamp(0, max(n - 1, 0))
    node, nb = cl.reshape(-1), cl.flip(1).reshape(-1)                      # slot 2e is (a, b), slot 2e + 1 is (b, a): edges ascend
    order = torch.sort(node * max(n, 1) + nb, stable=True).indices
    adj_edge = (order // 2).to(torch.int32)
    adj_offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n > 0 and E > 0:
        adj_offsets[1:] = torch.cumsum(torch.bincount(node, minlength=n), 0)
    edge_use = torch.zeros(E, dtype=torch.uint8, device=dev)
    idx = torch.nonzero(_valid(edge_R, edge_weight)).reshape(-1)
    if idx.numel():
        key = cl.amin(1) * max(n, 1) + cl.amax(1)
        idx = idx[torch.sort(-edge_weight[idx].to(torch.int64), stable=True).indices]
        idx = idx[torch.sort(key[idx], stable=True).indices]
        first = torch.ones(idx.numel(), dtype=torch.bool, device=dev)
        first[1:] = key[idx][1:] != key[idx][:-1]
        edge_use[idx[first]] = 1
    return adj_offsets, adj_edge, edge_use


def average_rotations(edge_image, edge_R, edge_weight, n_images, root=-1, cycle_deg=5.0, loss_deg=5.0, max_err_deg=10.0, max_iters=20,
                      pcg_iters=30, pcg_tol=1e-4, step_tol_deg=1e-3, timings=None):
    """One rotation per image from the rotations of image pairs, and a verdict per pair -> ``GlobalRotations``.

    ``edge_image [E,2]`` (a, b); ``edge_R [E,3,3]`` with ``x_b = R x_a`` (so ``R_b = R_ab R_a`` for camera-from-world rotations);
    ``edge_weight [E]`` integers, for example inlier counts (an edge with weight 0, or with a matrix that is not a rotation to 1e-3, is
    invalid: no error).  CPU tensors or numpy arrays run the defining host routine; GPU tensors (all of them, on one device) run the
    kernels.  ``root``: the image whose rotation is the identity (-1: the image with the greatest sum of weights); only its component
    is solved.  ``cycle_deg``: a triangle vouches for its edges when its rotations compose to less than this; ``loss_deg``: the scale of
    the Geman-McClure loss; ``max_err_deg``: an edge further than this from the averaged rotations is an outlier; ``step_tol_deg``:
    the refinement ends when no rotation moves more.  One readback; a bad graph raises ValueError.  timings: a list that receives
    (stage, ms) pairs of the GPU launches."""
    what = "average_rotations"
    args = [edge_image, edge_R, edge_weight]
    gpu = _tracks.one_device(what, _ARGS, args)
    _tracks.integers(what, "edge_image", edge_image)
    _tracks.integers(what, "edge_weight", edge_weight)
    _integer(what, "n_images", n_images, 0)
    _integer(what, "root", root, -(1 << 31))
    _integer(what, "max_iters", max_iters, 0)
    _integer(what, "pcg_iters", pcg_iters, 0)
    for name, v, hi in (("cycle_deg", cycle_deg, 180.0), ("loss_deg", loss_deg, 180.0), ("max_err_deg", max_err_deg, 180.0),
                        ("step_tol_deg", step_tol_deg, 180.0)):
        if not (0.0 <= float(v) <= hi) or (name == "loss_deg" and float(v) == 0.0):
            raise ValueError(f"{what}: {name} must lie in [0, {hi}] degrees (loss_deg above 0), got {v!r}")
    if not 0.0 <= float(pcg_tol) < 1.0:
        raise ValueError(f"{what}: pcg_tol must lie in [0, 1), got {pcg_tol!r}")
    params = (math.cos(math.radians(cycle_deg) / 2.0), 2.0 * math.sin(math.radians(loss_deg) / 2.0),
              2.0 * math.sin(math.radians(max_err_deg) / 2.0), math.radians(step_tol_deg), max_iters, pcg_iters, float(pcg_tol))
    tensor = lambda x: x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    im = tensor(edge_image).to(torch.int32).reshape(-1, 2)
    Rm = tensor(edge_R).to(torch.float64).reshape(-1, 3, 3)
    wt = tensor(edge_weight).reshape(-1).to(torch.int64)
    if wt.numel() and (wt.max() >= (1 << 31) or wt.min() < -(1 << 31)):
        raise ValueError(f"{what}: edge_weight must fit 32 bits")
    wt = wt.to(torch.int32)
    if Rm.shape[0] != im.shape[0] or wt.shape[0] != im.shape[0]:
        raise ValueError(f"{what}: expected edge_image [E,2], edge_R [E,3,3] and edge_weight [E], got {tuple(edge_image.shape)}, "
                         f"{tuple(edge_R.shape)}, {tuple(edge_weight.shape)}")
    a = [im.contiguous(), Rm.contiguous(), wt.contiguous(), *view_graph(im, Rm, wt, n_images)]
    if gpu:
        out = ops.rotation_averaging(*a, n_images, root, *params, timings=timings)
    else:
        out = {k: torch.from_numpy(v) for k, v in ops.rotation_averaging_host(*[x.numpy() for x in a], n_images, root, *params).items()}
    word = torch.cat([out["counts"], out["info"].view(torch.int64)]).cpu()  # the one readback
    counts, info = word[:ops.ROTATION_COUNTS].tolist(), word[ops.ROTATION_COUNTS:].view(torch.float64).tolist()
    _tracks.raise_error_bits(what, counts[1], ops.ROTATION_ERRORS)
    stats = {name: counts[i] for i, name in enumerate(ops.ROTATION_NAMES) if name != "error_bits"}
    stats.update(zip(ops.ROTATION_INFO, info))
    stats.update(status_name=ops.ROTATION_STATUS[counts[14]], n_edges=int(im.shape[0]), n_images=n_images, cycle_deg=float(cycle_deg),
                 loss_deg=float(loss_deg), max_err_deg=float(max_err_deg))
    return GlobalRotations(counts[15], stats, R=out["R"], in_graph=out["in_graph"] != 0, edge_state=out["edge_state"],
                           edge_chord=out["edge_chord"], support=out["support"], tree=out["tree"] != 0, edge_use=out["edge_use"] != 0)
