"""View-graph calibration: a focal length for every image (or camera) from the fundamental matrices of all verified pairs at once.

Every stage after matching takes an intrinsics matrix per image, and ``refine_focal`` is validated for start values that are a few
per cent off.  Without EXIF nothing supplies that start.  A fundamental matrix needs no intrinsics, and an essential matrix has two
equal singular values and a zero one: the focal lengths are chosen so that ``K_b^T F K_a`` is as close to essential as possible on
all edges of the view graph together::

    cal = calibrate_view_graph(edge_image, edge_F, edge_weight, n_images, principal_point, f0)      # ViewGraphCalibration
    cal.focal, cal.K, cal.edge_ok, cal.focal_ok

    cal = sfm.calibrate()                              # the same over the rows of a pair list (atlas.py), F by RANSAC per row
    rec = sfm.reconstruct_uncalibrated()               # calibrate -> reconstruct with ba={'refine_focal': True}

The rule (include/loftr_calib.h): one scale ``m`` per camera on its start focal, a nine-component residual that is smooth
in the focals and whose norm is ``(s1^2 - s2^2) / (s1^2 + s2^2)``, a Geman-McClure loss, a weak prior ``m = 1``, Levenberg-Marquardt
with Jacobi-preconditioned conjugate gradients.  The host routine ``loftr_calibrate_view_graph_host`` defines it in fp64 with every
sum in a stated order (CPU tensors / numpy arrays run it); the HIP kernels reproduce it bit for bit (GPU tensors run them; there is
no silent fallback either way).

The defaults (``ops_calib.CALIB_DEFAULTS``) are those of a prototype on synthetic rings of 12 to 30 cameras; they are UNVALIDATED on
real data.  The principal point and a unit aspect ratio are ASSUMED, not estimated; optical axes that all meet in one point are the
known degenerate configuration of focal lengths from F, which only the prior keeps in check.
"""
import numpy as np
import torch

from . import _tracks, ops_calib

_ARGS = ("edge_image", "edge_F", "edge_weight", "principal_point", "f0")


class ViewGraphCalibration:
    """What ``calibrate_view_graph`` returns (tensors on the device of the input).

    ``focal_scale [G] f64``, ``focal [n] f64`` (``f0 * focal_scale[group]``), ``edge_resid [E] f64`` (0 for an invalid edge),
    ``edge_state [E] u8`` (``ops_calib.CALIB_EDGE_STATES``: 0 invalid, 1 ok, 2 outlier), ``group_state [G] u8``
    (``ops_calib.CALIB_GROUP_STATES``: 0 no valid edge, 1 held, 2 refined), ``group [n] i32`` (the camera of each image), ``K [n,3,3]
    f64`` (``focal`` and the assumed principal point); ``stats``: the counts and info by name (``ops_calib.CALIB_NAMES``,
    ``CALIB_INFO``)."""

    FIELDS = ("focal_scale", "focal", "edge_resid", "edge_state", "group_state", "group", "K")

    def __init__(self, stats, **tensors):
        self.stats = stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])

    @property
    def edge_ok(self):
        """[E] bool: the edge is valid and its residual is at most ``max_resid``."""
        return self.edge_state == 1

    @property
    def focal_ok(self):
        """[n] bool: the focal length of the image was refined (its camera had enough valid edges)."""
        return self.group_state[self.group.to(torch.int64)] == 2

    def to_host(self):
        """dict of numpy arrays (plus 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out.update(stats=dict(self.stats))
        return out


def default_focal(image_hw):
    """The usual guess without EXIF: 1.2 max(H, W)."""
    return 1.2 * float(max(image_hw[0], image_hw[1]))


def calibrate_view_graph(edge_image, edge_F, edge_weight, n_images, principal_point, f0, camera_ids=None, timings=None, **params):
    """Focal lengths from the fundamental matrices of a view graph -> ``ViewGraphCalibration``.

    ``edge_image [E,2]`` (a, b), ``edge_F [E,3,3]`` with ``x_b^T F x_a = 0`` in pixels, ``edge_weight [E]`` (inlier counts; an edge
    with weight <= 0 or an F that is not finite is invalid); ``principal_point [n,2]`` or one ``(cx, cy)`` for all images (ASSUMED);
    ``f0 [n]`` or one number: the start focals; ``camera_ids [n]``: any non-negative integers, images with one id share one scale
    (None: every image its own).  CPU tensors or numpy arrays run the defining host routine; GPU tensors (all of them, on one device)
    run the kernels.  ``params``: ``loss`` (scale of the Geman-McClure loss on the residual), ``max_resid`` (an edge above it is an
    outlier), ``prior_weight`` (of ``m = 1``), ``weight_cap`` (inlier counts above it weigh the same), ``bound_lo``, ``bound_hi`` (a
    trial that takes a scale outside is rejected), ``min_edges`` (a camera with fewer valid edge ends is held), ``max_iters``,
    ``pcg_iters``, ``pcg_tol``, ``ftol``; the defaults (``ops_calib.CALIB_DEFAULTS``) are a prototype's and UNVALIDATED on real
    data.  One readback (counts and info); a bad input raises ValueError.  timings: a list that receives (stage, ms) pairs of the GPU
    launches."""
    what = "calibrate_view_graph"
    if not isinstance(n_images, int) or isinstance(n_images, bool) or n_images < 1:
        raise ValueError(f"{what}: n_images must be an integer >= 1, got {n_images!r}")
    n = n_images
    unknown = set(params) - set(ops_calib.CALIB_DEFAULTS)
    if unknown:
        raise TypeError(f"{what}: unknown parameter(s) {sorted(unknown)}")
    p = {**ops_calib.CALIB_DEFAULTS, **params}
    ops_calib.check_params(what, **p)
    tensors = [x for x in (edge_image, edge_F, edge_weight, principal_point, f0, camera_ids)
               if isinstance(x, (torch.Tensor, np.ndarray))]
    names = [k for k, x in zip(_ARGS + ("camera_ids",), (edge_image, edge_F, edge_weight, principal_point, f0, camera_ids))
             if isinstance(x, (torch.Tensor, np.ndarray))]
    gpu = _tracks.one_device(what, names, tensors)
    dev = edge_image.device if gpu else torch.device("cpu")
    for name, a in (("edge_image", edge_image), ("edge_weight", edge_weight)) + ((("camera_ids", camera_ids),) if camera_ids is not None else ()):
        _tracks.integers(what, name, a)
    tensor = lambda x: x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ei = tensor(edge_image).to(torch.int32).reshape(-1, 2)
    F = tensor(edge_F).to(torch.float64).reshape(-1, 3, 3)
    ew = tensor(edge_weight).to(torch.int32).reshape(-1)
    E = int(ei.shape[0])
    if F.shape[0] != E or ew.shape[0] != E or E >= 1 << 30:
        raise ValueError(f"{what}: expected edge_image [E,2], edge_F [E,3,3] and edge_weight [E] with E < 2^30, got {tuple(ei.shape)}, "
                         f"{tuple(F.shape)}, {tuple(ew.shape)}")
    pp = tensor(np.asarray(principal_point, np.float64) if not isinstance(principal_point, torch.Tensor) else principal_point).to(torch.float64)
    pp = pp.reshape(1, 2).expand(n, 2) if pp.numel() == 2 else pp.reshape(-1, 2)
    fs = tensor(np.asarray(f0, np.float64) if not isinstance(f0, torch.Tensor) else f0).to(torch.float64)
    fs = fs.reshape(1).expand(n) if fs.numel() == 1 else fs.reshape(-1)
    if pp.shape[0] != n or fs.shape[0] != n:
        raise ValueError(f"{what}: expected principal_point [{n},2] (or one pair) and f0 [{n}] (or one number), got {tuple(pp.shape)}, "
                         f"{tuple(fs.shape)}")
    neg_id = torch.zeros(1, dtype=torch.int64, device=dev)
    if camera_ids is None:
        group, G = torch.arange(n, dtype=torch.int32, device=dev), n
    else:
        ids = tensor(camera_ids).reshape(-1)
        if ids.shape[0] != n:
            raise ValueError(f"{what}: expected camera_ids [{n}], got {tuple(ids.shape)}")
        neg_id = (ids < 0).any().to(torch.int64).reshape(1)               # read with the counts: the one readback
        groups = _tracks.group_by_camera(ids if gpu else ids.numpy())
        group = groups[0] if gpu else torch.from_numpy(groups[0])
        G = int(groups[1].shape[0]) - 1
    # the incidence lists: the codes 2e + side in a stable ascending grouping by the group of their image (integer sorts on the device
    # of the input; ids out of range are only clamped here, the routine reports them)
    key = group[ei.reshape(-1).to(torch.int64).clamp(0, n - 1)]
    if gpu:
        grp_offsets, grp_inc = _tracks.group_by_image(key, G)
        a = [x.contiguous() for x in (ei, F, ew, pp, fs, group, grp_offsets, grp_inc)]
        out = ops_calib.calibrate_view_graph(*a, timings=timings, **p)
    else:
        grp_offsets, grp_inc = _tracks.group_by_image(key.numpy(), G)
        a = [x.contiguous().numpy() for x in (ei, F, ew, pp, fs, group)] + [grp_offsets, grp_inc]
        out = {k: torch.from_numpy(v) for k, v in ops_calib.calibrate_view_graph_host(*a, **p).items()}
    word = torch.cat([out["counts"], out["info"].view(torch.int64), neg_id]).cpu()  # the one readback
    counts = word[:ops_calib.CALIB_COUNTS].tolist()
    info = word[ops_calib.CALIB_COUNTS:-1].view(torch.float64).tolist()
    if int(word[-1]):
        raise ValueError(f"{what}: camera_ids must be non-negative")
    _tracks.raise_error_bits(what, counts[1], ops_calib.CALIB_ERRORS)
    stats = {name: counts[i] for i, name in enumerate(ops_calib.CALIB_NAMES) if name != "error_bits"}
    stats.update(zip(ops_calib.CALIB_INFO, info))
    stats.update(status_name=ops_calib.CALIB_STATUS[counts[7]], n_images=n, n_groups=G, n_edges=E, **p)
    K = torch.zeros(n, 3, 3, dtype=torch.float64, device=dev)
    K[:, 0, 0] = K[:, 1, 1] = out["focal"]
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = pp[:, 0], pp[:, 1], 1.0
    return ViewGraphCalibration(stats, focal_scale=out["focal_scale"], focal=out["focal"], edge_resid=out["edge_resid"],
                                edge_state=out["edge_state"], group_state=out["group_state"], group=group, K=K)
