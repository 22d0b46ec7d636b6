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

Where the camera positions were measured (GPS), ``position_prior`` holds every camera centre near its measurement in any of the three
modes (``loftr_bundle_adjust_prior_host`` and its kernels).  The model must already be in the frame of the measurements
(``Reconstruction.align``); the priors then fix the scale, remove the drift of the positions and hold the gauge without a fixed camera::

    rec2, al = rec.align(gps)                                                         # into the GPS frame
    none = torch.zeros(n, dtype=torch.bool, device=dev)
    res = sfm.adjust(pts2, K, rec2.T_cam_from_world, fixed=none, position_prior=gps, prior_mask=al.inliers, prior_sigma=2.0)

(``rec.align(gps, refine=dict(sfm=sfm, sigma=2.0))`` runs exactly that sequence and triangulates again.)

Where the lenses distort (internet photos, phones, action cameras), ``refine_radial`` adds one radial coefficient ``k`` per camera --
``x_d = x (1 + k r^2)`` on normalised coordinates -- next to its focal step (``loftr_bundle_adjust_radial_host`` and its
kernels).  The adjustment reads the stored (distorted) pixels; every other stage reads pinhole pixels, which ``undistort_points`` gives::

    res = sfm.adjust(pts, K, T_cam_from_world, fixed=known, refine_focal=True, refine_radial=True, camera_ids=ids)
    xy, ok = loftr_amd.undistort_points(obs_xy, obs_image, res.K, res.radial)            # what triangulation and registration read
"""
import numpy as np
import torch

from . import _tracks, ops

_OUT = ("T_cam_from_world", "xyz", "obs_active", "cam_free", "point_active")
_OUT_FOCAL = ("K", "cam_focal")
_OUT_SHARED = ("cam_group", "group_focal")
_OUT_PRIOR = ("cam_prior",)
_OUT_RADIAL = ("radial", "cam_radial", "group_radial")
_ARGS = ("offsets", "obs_image", "obs_xy", "obs_mask", "xyz", "K", "T_cam_from_world")


def _shaped(what, name, v, shape, must=None):
    if tuple(v.shape) != shape:
        raise ValueError(f"{what}: {name} must {must or f'have shape {shape}'}, got {tuple(v.shape)}")
    return v


def _beside(what, name, v, gpu, like, shape=None, must=None):
    """The optional argument ``v`` must live on the side of the others (``gpu``: on the device of ``like``) -> the tensor on the GPU, a
    numpy array on the host, of ``shape`` where one is given."""
    on_gpu = isinstance(v, torch.Tensor) and v.is_cuda
    if on_gpu != gpu or (gpu and v.device != like.device):
        raise ValueError(f"{what}: {name} is on the {'GPU' if on_gpu else 'CPU'}, the other arguments are not; there is no silent "
                         "fallback: move it to their device")
    v = v.detach() if isinstance(v, torch.Tensor) else np.asarray(v)
    if not on_gpu and isinstance(v, torch.Tensor):
        v = v.numpy()
    return v if shape is None else _shaped(what, name, v, shape, must)


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
    refined) and ``stats['n_focal_groups']``.  A call with ``position_prior`` adds ``cam_prior [n] bool`` (the camera had a prior) and
    ``stats['n_prior_cameras']``, ``prior_cost_before`` / ``prior_cost_after`` (the priors' part of the cost, in sigma^2) and
    ``prior_rms_before`` / ``prior_rms_after`` (root mean squared distance of the centres from their priors, in world units).  A call
    with ``refine_radial`` adds ``radial [n] f64`` (the input's bits for an image that does not refine it), ``cam_radial [n] bool``,
    ``group_radial [G] bool`` and ``stats['n_radial_cameras']``."""

    FIELDS = _OUT

    def __init__(self, stats, **tensors):
        self.stats = stats
        if "K" in tensors or "cam_prior" in tensors:                     # a call with refine_focal: K and cam_focal as well; with priors
            self.FIELDS = _OUT + (_OUT_FOCAL if "K" in tensors else ()) + (_OUT_SHARED if "cam_group" in tensors else ()) + \
                (_OUT_PRIOR if "cam_prior" in tensors else ()) + (_OUT_RADIAL if "radial" in tensors else ())
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
                  pcg_tol=1e-2, ftol=1e-9, timings=None, refine_focal=None, min_focal_obs=20, focal_bounds=(0.5, 2.0), camera_ids=None,
                  position_prior=None, prior_sigma=1.0, prior_mask=None, refine_radial=None, radial=None, radial_bounds=(-1.0, 1.0)):
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
    ``stats['n_focal_cameras']``.  Principal point and focal priors are not modelled.

    ``camera_ids`` (needs ``refine_focal``): ``[n]`` non-negative integers on the device of the other arguments; images with
    equal ids are one physical camera and share ONE relative step -- every member keeps its own fx, skew, fy (so images stored at different
    resize scales work) and all are multiplied by the same ``1 + delta``.  An image carries its camera's focal when it is valid, flagged in
    ``refine_focal`` and has an active observation, whether or not its pose is ``fixed``; a camera refines when its carrying images
    together have at least ``min_focal_obs`` active observations.  ``None`` is the per-image call above, unchanged bit for bit.  The
    result adds ``cam_group``, ``group_focal`` and ``stats['n_focal_groups']``.

    ``position_prior`` (any of the modes above): ``[n,3]`` measured camera centres in world units, on the device of the
    other arguments; a row with a NaN has no prior.  ``prior_sigma``: a positive scalar, ``[n]`` or ``[n,3]`` (per axis), in world units;
    an entry that is not finite and positive switches that camera's prior off.  ``prior_mask``: ``[n]``, which priors to use (default:
    the finite rows).  Each free camera with a prior adds ``|(c - g) / sigma|^2`` to the cost, ``c = -R^T t`` its centre.  The prior's
    loss is the square -- ``huber_px`` acts on the observations only -- so remove gross GPS errors with
    ``prior_mask=alignment.inliers``.  A camera that is not free has no prior (its term would be a constant).  ``fixed=None`` still
    fixes image 0; pass an all-false ``fixed`` to let the priors hold the gauge, which they do when at least three cameras with a
    prior are not collinear.  ``None`` makes the calls above exactly as before.  The result adds ``cam_prior`` and
    ``stats['n_prior_cameras']``, ``prior_cost_before`` / ``_after``, ``prior_rms_before`` / ``_after``.  Rotation priors, priors on
    points, a robust prior loss, lever arms and full covariances are not modelled.

    ``refine_radial`` (needs ``refine_focal``): ``None`` is every call above, bit for bit; ``True`` or an ``[n]`` mask lets
    the cameras of those images refine ONE radial coefficient each, ``x_d = x (1 + k r^2)`` on normalised coordinates, next to their focal
    step.  ``obs_xy`` are then the stored, distorted pixels.  ``radial``: ``[n]`` start values (default zeros), on the device of the other
    arguments.  Groups are those of ``camera_ids``; without it every image is a camera of its own (singleton groups: the group
    preconditioner is then one 2 x 2 block per image beside its 6 x 6 pose block, and §18.2 measured that such splitting of a camera's
    block costs conjugate-gradient iterations -- many singleton groups may end at ``pcg_iters``; give ``camera_ids`` where images share
    a camera).  An image refines its coefficient when it carries its camera's focal and is flagged here; a camera does when those images
    together have ``min_focal_obs`` active observations.  A trial that takes a ``k`` outside ``radial_bounds = (lo, hi)`` is rejected.
    The steps add: every member leaves with ``radial_in + a`` for ONE ``a`` of its camera.  The result adds ``radial``, ``cam_radial``,
    ``group_radial`` (and ``cam_group`` / ``group_focal``) and ``stats['n_radial_cameras']``.  Not modelled: priors together with
    ``refine_radial``, refining ``k`` with a trusted focal, k2, tangential and fisheye terms.  A KNOWN distortion is not an argument of
    the adjustment: ``undistort_points`` the observations, then make the pinhole call."""
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
    if refine_radial is None and radial is not None:
        raise ValueError(f"{what}: radial without refine_radial: a known distortion is not adjusted here; undistort the observations "
                         "(undistort_points), then make the pinhole call")
    if refine_radial is not None:
        if refine_radial is False:
            raise ValueError(f"{what}: refine_radial must be None, True or an [n] mask")
        if focal is None:
            raise ValueError(f"{what}: refine_radial refines a radial coefficient next to the focal step of refine_focal; pass refine_focal as well")
        if position_prior is not None:
            raise ValueError(f"{what}: position_prior together with refine_radial is not modelled")
        if not (isinstance(radial_bounds, (tuple, list)) and len(radial_bounds) == 2):
            raise ValueError(f"{what}: radial_bounds must be a pair (lo, hi), got {radial_bounds!r}")
        rbounds = ops._ba_radial_params(what, *radial_bounds)
    gpu = _tracks.one_device(what, _ARGS + ("fixed",), args + ([] if fixed is None else [fixed]))   # ("fixed" is named only when given)
    nK, beside = len(K), lambda name, v, *shape: _beside(what, name, v, gpu, args[0], *shape)
    if refine_radial is not None:
        if refine_radial is not True:
            refine_radial = beside("refine_radial", refine_radial, (nK,))
        if radial is not None:
            radial = beside("radial", radial, (nK,))
            radial = radial.to(torch.float64).contiguous() if gpu else np.ascontiguousarray(radial, np.float64)
        else:
            radial = torch.zeros(nK, dtype=torch.float64, device=args[0].device) if gpu else np.zeros(nK, np.float64)
        if camera_ids is None:                                           # every image a camera of its own
            camera_ids = torch.arange(nK, dtype=torch.int64, device=args[0].device) if gpu else np.arange(nK, dtype=np.int64)
    neg_id = None
    if camera_ids is not None:
        camera_ids = beside("camera_ids", camera_ids)
        _tracks.integers(what, "camera_ids", camera_ids)
        _shaped(what, "camera_ids", camera_ids, (nK,))
        if gpu:
            neg_id = (camera_ids < 0).any().to(torch.int64).reshape(1)                    # read with the counts: the one readback
        elif camera_ids.size and camera_ids.min() < 0:
            raise ValueError(f"{what}: camera_ids must not be negative")
    if focal is not None and refine_focal is not True:
        refine_focal = beside("refine_focal", refine_focal, (nK,), f"be None, True or a mask of shape ({nK},)")
    prior = None
    if position_prior is not None:
        pxyz = beside("position_prior", position_prior)
        if prior_sigma is not None and not isinstance(prior_sigma, (int, float)):
            prior_sigma = beside("prior_sigma", prior_sigma)
        if prior_mask is not None and not isinstance(prior_mask, (int, float)):
            prior_mask = beside("prior_mask", prior_mask)
        conv = (lambda v: v.to(torch.float64)) if gpu else (lambda v: np.asarray(v, np.float64))
        xp = torch if gpu else np
        pxyz = _shaped(what, "position_prior", conv(pxyz), (nK, 3))
        if isinstance(prior_sigma, (int, float)) and not isinstance(prior_sigma, bool):
            if not (prior_sigma > 0 and prior_sigma < float("inf")):
                raise ValueError(f"{what}: prior_sigma must be positive and finite, got {prior_sigma}")
            psig = xp.zeros_like(pxyz) + float(prior_sigma)
        else:
            if prior_sigma is None or isinstance(prior_sigma, bool):
                raise ValueError(f"{what}: prior_sigma must be a positive number or an array of shape ({nK},) or ({nK}, 3)")
            psig = conv(prior_sigma)
            if tuple(psig.shape) == (nK,):
                psig = psig.reshape(nK, 1) + xp.zeros_like(pxyz)
            if tuple(psig.shape) != (nK, 3):
                raise ValueError(f"{what}: prior_sigma must be a positive number or have shape ({nK},) or ({nK}, 3), got "
                                 f"{tuple(psig.shape)}")
        if prior_mask is None:
            pm = (xp.isfinite(pxyz).sum(1) == 3)
            pm = pm.to(torch.uint8) if gpu else pm.astype(np.uint8)
        else:
            pm = _shaped(what, "prior_mask", prior_mask if hasattr(prior_mask, "shape") else np.asarray(prior_mask), (nK,))
            pm = (pm != 0).to(torch.uint8) if gpu else (pm != 0).astype(np.uint8)
        prior = (pxyz.contiguous(), psig.contiguous(), pm) if gpu else (np.ascontiguousarray(pxyz), np.ascontiguousarray(psig), pm)
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
    if refine_radial is not None:
        extra, mode, focal = extra + [radial, ones if refine_radial is True else flags(refine_radial)], "_radial", focal + rbounds
    if prior is None:
        call = getattr(ops, "bundle_adjust" + mode + ("" if gpu else "_host"))
        out = call(*a, fx, *_tracks.group_by_image(a[1], n), *extra, *params, *(focal or ()), **({"timings": timings} if gpu else {}))
    else:                                                                # the one pair with priors: the mode's number, None below it
        call = ops.bundle_adjust_prior if gpu else ops.bundle_adjust_prior_host
        out = call(("", "_focal", "_shared").index(mode), *a, fx, *_tracks.group_by_image(a[1], n), *(extra + [None] * (4 - len(extra))), *prior,
                   *params, *(focal or ()), **({"timings": timings} if gpu else {}))
    if camera_ids is not None:
        out["cam_group"] = groups[0]
    if not gpu:
        out = {k: torch.from_numpy(v) for k, v in out.items()}
    counts = (out["counts"] if neg_id is None else torch.cat([out["counts"], neg_id])).cpu()      # the one readback
    reals = counts[8:13].view(torch.float64).tolist()
    counts = counts.tolist()
    if neg_id is not None and counts[-1]:
        raise ValueError(f"{what}: camera_ids must not be negative")
    _tracks.raise_error_bits(what, counts[1], ops.BUNDLE_SHARED_ERRORS if camera_ids is not None else None)
    stats = {"status": ops.BUNDLE_STATUS[counts[0]], "n_iters": counts[2], "n_accepted": counts[3], "n_pcg": counts[4],
             "n_active_observations": counts[5], "n_active_points": counts[6], "n_free_cameras": counts[7],
             "n_tracks": out["point_active"].numel(), "n_observations": out["obs_active"].numel(), "n_images": out["cam_free"].numel(),
             "cost_before": reals[0], "cost_after": reals[1], "rms_px_before": reals[2], "rms_px_after": reals[3], "lambda": reals[4]}
    for k in ("obs_active", "cam_free", "point_active"):
        out[k] = out[k].view(torch.bool)
    fields = _OUT
    if prior is not None:
        preals = torch.tensor(counts[17:21], dtype=torch.int64).view(torch.float64).tolist()
        stats.update(n_prior_cameras=counts[16], prior_cost_before=preals[0], prior_cost_after=preals[1], prior_rms_before=preals[2],
                     prior_rms_after=preals[3])
        out["cam_prior"] = out["cam_prior"].view(torch.bool)
    if focal is not None:
        stats["n_focal_cameras"] = counts[13]
        out["cam_focal"] = out["cam_focal"].view(torch.bool)
        fields += _OUT_FOCAL
        if camera_ids is not None:
            stats["n_focal_groups"] = counts[14]
            out["group_focal"] = out["group_focal"].view(torch.bool)
            fields += _OUT_SHARED
        if refine_radial is not None:
            stats["n_radial_cameras"] = counts[15]
            out["cam_radial"], out["group_radial"] = out["cam_radial"].view(torch.bool), out["group_radial"].view(torch.bool)
            fields += _OUT_RADIAL
    return BundleResult(stats, **{k: out[k] for k in fields + (_OUT_PRIOR if prior is not None else ())})
