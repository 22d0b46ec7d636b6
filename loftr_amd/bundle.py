"""Bundle adjustment of the triangulated model: camera poses and points refined together over the reprojection error, on the device.

The step between two triangulations: database poses that come from pairwise estimates, a coarse SfM run, SLAM or GPS / IMU priors are
not exact, and the points triangulated from them carry the error into every localised query.  ``bundle_adjust`` minimises the pixel
reprojection error over the poses (6 DoF, intrinsics fixed) and the points::

    sfm = atlas.finalize()
    pts = sfm.triangulate(K, T_cam_from_world)
    res = sfm.adjust(pts, K, T_cam_from_world, fixed=known)                           # BundleResult, on the atlas's device
    pts = sfm.triangulate(K, res.T_cam_from_world)                                    # the refined poses admit more observations

The rule (include/loftr_hip.h): Levenberg-Marquardt with an optional Huber loss; the linear step is the point-eliminated
Schur system, solved by preconditioned conjugate gradients without forming it; every sum has a defined order.  The host routine
``loftr_bundle_adjust_host`` defines the result (CPU tensors / numpy arrays run it), the HIP kernels reproduce it bit for bit (GPU
tensors run them; there is no silent fallback either way).

Where the focal lengths are guesses (internet photos, EXIF), ``refine_focal`` adds one relative focal step per image to its six pose
parameters (``loftr_bundle_adjust_focal_host`` and its kernels); the result then carries ``K``::

    res = sfm.adjust(pts, K, T_cam_from_world, fixed=known, refine_focal=True)
    pts = sfm.triangulate(res.K, res.T_cam_from_world)

Where many images come from ONE camera (a video, a ScanNet sequence, a phone walk, a rig, a few bodies), ``camera_ids`` shares that
step between the images of a camera (``loftr_bundle_adjust_shared_host`` and its kernels): one parameter per camera,
estimated from every observation of every one of its images, the fixed-pose ones included::

    res = sfm.adjust(pts, K, T_cam_from_world, fixed=known, refine_focal=True, camera_ids=ids)     # ids [n]: equal ids, one camera
"""
import numpy as np
import torch

from . import _tracks, ops

_OUT = ("T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active")
_OUT_FOCAL = ("K", "cam_focal")
_OUT_SHARED = ("cam_group", "group_focal")
_ARGS = ("offsets", "obs_image", "obs_xy", "obs_mask", "xyz", "K", "T_cam_from_world")


class BundleResult:
    """What ``bundle_adjust`` returns (tensors on the device of the input).

    ``T_cam_from_world [n,4,4] f64`` (the input's bits for a camera that is not free), ``xyz [T,3] f32`` (the input's bits for a point
    that is not active), ``obs_active [N] bool``, ``cam_free [n] bool``, ``point_active [T] bool``; ``cost_before`` / ``cost_after`` (the
    sum of the loss over the active observations), ``rms_px_before`` / ``rms_px_after`` (root mean squared pixel error over them),
    ``n_iters`` (trials), ``n_accepted``, ``n_pcg`` (conjugate-gradient iterations), ``status`` (a name of ``ops.BUNDLE_STATUS``:
    converged, max_iters, stalled, nothing_to_adjust); ``stats``: dict of the counts.

    A call with ``refine_focal`` also carries ``K [n,3,3] f64`` (the input's bits for a camera that does not refine its focal),
    ``cam_focal [n] bool`` and ``stats['n_focal_cameras']``; ``FIELDS`` of that result names them too.  A call with ``camera_ids`` adds
    ``cam_group [n] i32`` (the dense group of each image, groups ordered by their smallest member), ``group_focal [G] bool`` (the group
    refined) and ``stats['n_focal_groups']``."""

    FIELDS = _OUT

    def __init__(self, stats, **tensors):
        self.stats = stats
        if "K" in tensors:                                               # a call with refine_focal: K and cam_focal as well
            self.FIELDS = _OUT + _OUT_FOCAL + (_OUT_SHARED if "cam_group" in tensors else ())
        for k in self.FIELDS:
            setattr(self, k, tensors[k])
        for k in ("cost_before", "cost_after", "rms_px_before", "rms_px_after", "n_iters", "n_accepted", "n_pcg", "status"):
            setattr(self, k, stats[k])

    def to_host(self):
        """dict of numpy arrays (plus 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out["stats"] = dict(self.stats)
        return out


def bundle_adjust(offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed=None, huber_px=0.0, max_iters=30, pcg_iters=30,
                  pcg_tol=1e-2, ftol=1e-9, timings=None, refine_focal=None, min_focal_obs=20, focal_bounds=(0.5, 2.0), camera_ids=None):
    """Refine poses and points over the reprojection error -> ``BundleResult``.

    ``offsets [T+1]``, ``obs_image [N]``, ``obs_xy [N,2]`` as for ``triangulate_tracks``; ``obs_mask [N]`` (bool or integers: which
    observations to use, e.g. ``Points3D.obs_inlier``), ``xyz [T,3]`` the starting points (NaN: the point is left out), ``K [n,3,3]``,
    ``T_cam_from_world [n,4,4]`` the starting poses.  CPU tensors or numpy arrays run the defining host routine; GPU tensors (all of them,
    on one device) run the kernels.

    ``fixed``: ``[n]`` bool, the cameras that keep their pose; ``None`` fixes image 0 only.  Fixing one camera removes six of the seven
    gauge freedoms; what remains of the gauge, the scale included, is held only by the damping, so a caller who knows two poses should
    fix both.  ``huber_px``: 0 for the squared loss, else the Huber radius in pixels.  ``max_iters`` trials at most, each solving its
    step with at most ``pcg_iters`` conjugate-gradient iterations to the relative tolerance ``pcg_tol``; the run stops as converged when
    an accepted trial lowers the cost by no more than ``ftol`` of it.  The active set is decided once, at the start; loop through
    ``triangulate`` to renew it.  One readback of the 16 counts; bad ``obs_image`` / ``offsets`` raise ValueError.

    ``refine_focal``: ``None`` keeps every ``K`` as given (the call above, unchanged); ``True`` or an ``[n]`` mask lets
    those images refine one relative focal step each -- fx, skew and fy scale together, cx and cy stay -- next to their pose.  An image
    refines only if it is free and has at least ``min_focal_obs`` active observations; a trial that takes a focal outside
    ``focal_bounds = (lo, hi)`` times its input value is rejected.  The result then carries ``K``, ``cam_focal`` and
    ``stats['n_focal_cameras']``.  Principal point, distortion and focal priors are not modelled.

    ``camera_ids`` (needs ``refine_focal``): ``[n]`` non-negative integers on the device of the other arguments; images with
    equal ids are one physical camera and share ONE relative step -- every member keeps its own fx, skew, fy (so images stored at different
    resize scales work) and all are multiplied by the same ``1 + delta``.  An image carries its camera's focal when it is valid, flagged in
    ``refine_focal`` and has an active observation, whether or not its pose is ``fixed``; a camera refines when its carrying images
    together have at least ``min_focal_obs`` active observations.  ``None`` is the per-image call above, unchanged bit for bit.  The
    result adds ``cam_group``, ``group_focal`` and ``stats['n_focal_groups']``."""
    what = "bundle_adjust"
    args = [offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world]
    params = ops._ba_params(what, huber_px, max_iters, pcg_iters, pcg_tol, ftol)
    focal = None
    if refine_focal is not None:
        if not (isinstance(focal_bounds, (tuple, list)) and len(focal_bounds) == 2):
            raise ValueError(f"{what}: focal_bounds must be a pair (lo, hi), got {focal_bounds!r}")
        focal = ops._ba_focal_params(what, min_focal_obs, *focal_bounds)
        if refine_focal is False:
            raise ValueError(f"{what}: refine_focal must be None, True or an [n] mask")
    if camera_ids is not None and focal is None:
        raise ValueError(f"{what}: camera_ids shares the focal step of refine_focal between images; pass refine_focal as well")
    gpu = _tracks.one_device(what, _ARGS + ("fixed",), args + ([] if fixed is None else [fixed]))   # ("fixed" is named only when given)
    neg_id = None
    if camera_ids is not None:
        on_gpu = isinstance(camera_ids, torch.Tensor) and camera_ids.is_cuda
        if on_gpu != gpu or (gpu and camera_ids.device != args[0].device):
            raise ValueError(f"{what}: camera_ids is on the {'GPU' if on_gpu else 'CPU'}, the other arguments are not; there is no "
                             "silent fallback: move it to their device")
        if not on_gpu:
            camera_ids = camera_ids.detach().numpy() if isinstance(camera_ids, torch.Tensor) else np.asarray(camera_ids)
        _tracks.integers(what, "camera_ids", camera_ids)
        if tuple(camera_ids.shape) != (len(K),):
            raise ValueError(f"{what}: camera_ids must have shape ({len(K)},), got {tuple(camera_ids.shape)}")
        if on_gpu:
            neg_id = (camera_ids.detach() < 0).any().to(torch.int64).reshape(1)          # read with the counts: the one readback
        elif camera_ids.size and camera_ids.min() < 0:
            raise ValueError(f"{what}: camera_ids must not be negative")
    if focal is not None and refine_focal is not True:
        on_gpu = isinstance(refine_focal, torch.Tensor) and refine_focal.is_cuda
        if on_gpu != gpu or (gpu and refine_focal.device != args[0].device):
            raise ValueError(f"{what}: refine_focal is on the {'GPU' if on_gpu else 'CPU'}, the other arguments are not; there is no "
                             "silent fallback: move it to their device")
        if not on_gpu:
            refine_focal = refine_focal.detach().numpy() if isinstance(refine_focal, torch.Tensor) else np.asarray(refine_focal)
        if tuple(refine_focal.shape) != (len(K),):
            raise ValueError(f"{what}: refine_focal must be None, True or a mask of shape ({len(K)},), got {tuple(refine_focal.shape)}")
    for n, a in zip(_ARGS[:2], args[:2]):
        _tracks.integers(what, n, a)
    # the arguments in the dtypes of the C call, on their side
    if gpu:
        dev = args[0].device
        dts = (torch.int64, torch.int32, torch.float32, None, torch.float32, torch.float64, torch.float64)
        a = [x.detach() if dt is None else x.detach().to(dt) for x, dt in zip(args, dts)]
        n = a[5].shape[0]
        flags = lambda x: (x.detach() != 0).to(torch.uint8)
        ones = torch.ones(n, dtype=torch.uint8, device=dev)
    else:
        dts = (np.int64, np.int32, np.float32, None, np.float32, np.float64, np.float64)
        host = lambda x: x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        a = [np.ascontiguousarray(host(x)) if dt is None else np.ascontiguousarray(host(x), dt) for x, dt in zip(args, dts)]
        n = a[5].shape[0]
        flags = lambda x: (host(x) != 0).astype(np.uint8)
        ones = np.ones(n, np.uint8)
        if a[0].ndim == 1 and a[1].ndim == 1 and a[5].ndim == 3:         # the errors the kernels report through counts[1]
            _tracks.check_host(what, a[0], a[1], n)
    a[3] = flags(a[3])
    fx = 0 * ones
    fx[:1] = 1                                                           # fixed = None: image 0 only
    if fixed is not None:
        fx = flags(fixed)
    # the mode, once: which pair of ops, and what it takes after the table of the observations grouped by image
    extra, mode = [], ""
    if focal is not None:
        extra, mode = [ones if refine_focal is True else flags(refine_focal)], "_focal"
    if camera_ids is not None:
        groups = _tracks.group_by_camera(camera_ids.detach() if gpu else camera_ids)
        extra, mode = extra + list(groups), "_shared"
    call = getattr(ops, "bundle_adjust" + mode + ("" if gpu else "_host"))
    out = call(*a, fx, *_tracks.group_by_image(a[1], n), *extra, *params, *(focal or ()), **({"timings": timings} if gpu else {}))
    if camera_ids is not None:
        out["cam_group"] = groups[0]
    if not gpu:
        out = {k: torch.from_numpy(v) for k, v in out.items()}
    counts = (out["counts"] if neg_id is None else torch.cat([out["counts"], neg_id])).cpu()      # the one readback
    reals = counts[8:13].view(torch.float64).tolist()
    counts = counts.tolist()
    if neg_id is not None and counts[16]:
        raise ValueError(f"{what}: camera_ids must not be negative")
    _tracks.raise_error_bits(what, counts[1], ops.BUNDLE_SHARED_ERRORS if camera_ids is not None else None)
    stats = {"status": ops.BUNDLE_STATUS[counts[0]], "n_iters": counts[2], "n_accepted": counts[3], "n_pcg": counts[4],
             "n_active_observations": counts[5], "n_active_points": counts[6], "n_free_cameras": counts[7],
             "n_tracks": out["point_active"].numel(), "n_observations": out["obs_active"].numel(), "n_images": out["cam_free"].numel(),
             "cost_before": reals[0], "cost_after": reals[1], "rms_px_before": reals[2], "rms_px_after": reals[3], "lambda": reals[4]}
    for k in ("obs_active", "cam_free", "point_active"):
        out[k] = out[k].view(torch.bool)
    if focal is None:
        return BundleResult(stats, **{k: out[k] for k in _OUT})
    stats["n_focal_cameras"] = counts[13]
    out["cam_focal"] = out["cam_focal"].view(torch.bool)
    if camera_ids is None:
        return BundleResult(stats, **{k: out[k] for k in _OUT + _OUT_FOCAL})
    stats["n_focal_groups"] = counts[14]
    out["group_focal"] = out["group_focal"].view(torch.bool)
    return BundleResult(stats, **{k: out[k] for k in _OUT + _OUT_FOCAL + _OUT_SHARED})
