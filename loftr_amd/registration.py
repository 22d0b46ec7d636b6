"""Image registration and incremental reconstruction from atlas tracks: the step that gives the images without a pose one, on the device.

``triangulate`` needs a pose for every image it uses and ``ops.estimate_poses`` only gives pairwise ones.  What joins them is the loop
of incremental structure from motion: triangulate from the images that have a pose, adjust, resect the images that do not from the 2D-3D
correspondences the tracks give them, repeat::

    sfm = atlas.finalize()
    rec = sfm.reconstruct(K)                                  # Reconstruction: poses of every image that could be registered, points
    pts = rec.points                                          # the final Points3D, ready for LocalizationModel

or piece by piece::

    pts = sfm.triangulate(K, T, posed=posed)                  # tolerates images without a pose
    reg = sfm.register(pts, K, T, posed, min_corr=15, min_inliers=15)          # Registration: poses of the newly registered images

The rule of the correspondence table (include/loftr_hip.h) is integer work and bit copies in a defined order: the host
routine ``loftr_register_corr_host`` defines it (CPU tensors / numpy arrays run it), the HIP kernels reproduce it bit for bit (GPU
tensors run them; there is no silent fallback either way).  The poses come from the batched P3P RANSAC of §14, one call for all
candidates, which is pinned bit for bit host against device as well; so are the triangulation (§16) and the bundle adjustment (§18), and
the whole chain therefore gives the same poses on both sides.
"""
import math

import numpy as np
import torch

from . import _tracks, ops
from ._lib import LoftrHipError

_ARGS = ("offsets", "obs_image", "obs_xy", "xyz", "status", "K", "T_cam_from_world", "posed")
_TABLE = ("cand_image", "cand_offsets", "corr_xyz", "corr_xy", "corr_obs")


class Registration:
    """What ``register_images`` returns (tensors on the device of the input).

    ``T_cam_from_world [n,4,4] f64`` (the input's bits for an image that was not registered in this call), ``registered [n] bool``,
    ``posed [n] bool`` (the input or registered), ``n_corr [n] i32`` (correspondences per unposed image), ``n_inliers [n] i64`` (-1
    where the image is not a candidate or has no model); the table of the ``P`` candidates: ``cand_image [P] i32``, ``cand_offsets
    [P+1] i64``, ``corr_xyz [C,3] f32``, ``corr_xy [C,2] f32``, ``corr_obs [C] i32`` (observation index), ``corr_inlier [C] bool``;
    ``stats``: dict of the counts."""

    FIELDS = ("T_cam_from_world", "registered", "posed", "n_corr", "n_inliers") + _TABLE + ("corr_inlier",)

    def __init__(self, stats, **tensors):
        self.stats = stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])

    def to_host(self):
        """dict of numpy arrays (plus 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out["stats"] = dict(self.stats)
        return out


class Reconstruction:
    """What ``reconstruct_tracks`` returns: ``T_cam_from_world [n,4,4] f64`` (NaN for an image that never got a pose), ``posed [n]
    bool``, ``round_registered [n] i32`` (the round in which the image got its pose; 0 for the initial pair; -1 for never), ``points``
    (the final ``Points3D``), ``bundle`` (the final ``BundleResult``), ``stats`` (dict; ``stats['rounds']`` holds the per-round counts),
    ``K [n,3,3] f64`` (the final intrinsics: the input's for an image that never refined its focal), ``radial [n] f64``
    (the final radial coefficients of a run with ``radial`` or ``ba['refine_radial']``; else None)."""

    def __init__(self, T_cam_from_world, posed, round_registered, points, bundle, stats, K=None, radial=None):
        self.T_cam_from_world, self.posed, self.round_registered = T_cam_from_world, posed, round_registered
        self.points, self.bundle, self.stats, self.K, self.radial = points, bundle, stats, K, radial
        self.sfm = None                                                 # the relabelled atlas of SfmResult.reconstruct(complete=True / merge=True)
        self.rotations = None                                           # the GlobalRotations of SfmResult.reconstruct(rotations=True)
        self.positions = None                                           # the GlobalPositions of SfmResult.reconstruct_global
        self.calibration = None                                         # the ViewGraphCalibration of SfmResult.reconstruct_uncalibrated

    def transformed(self, s, R, t):
        """A copy moved by the similarity X' = s R X + t (``ops.transform_model``): new ``T_cam_from_world`` and
        ``points.xyz``; every other tensor is shared with this one, and ``bundle`` is left in the old frame."""
        from .alignment import transformed
        return transformed(self, s, R, t)

    def align(self, ref_centres, known=None, thresh=1.0, with_scale=True, apply=True, conf=0.999, seed=0, refine=None):
        """Georegister against reference camera positions ``ref_centres [n,3]`` (``known [n]``: which rows hold one; default: the
        finite rows) -> ``(rec2, alignment)``: ``alignment`` is ``alignment.align_centres`` of the posed and known images at
        ``thresh`` (units of ``ref_centres``), ``rec2 = self.transformed(s, R, t)``.  ``bundle`` stays in the old frame.  Without a
        model (``alignment.n_inliers == -1``) nothing is raised and ``rec2`` is this reconstruction itself; likewise with
        ``apply=False``.

        ``refine=dict(sfm=..., sigma=..., **ba_kwargs)`` goes on from the aligned model: a bundle adjustment over the
        tracks of ``sfm`` (the ``SfmResult`` this reconstruction came from, or ``self.sfm``) with no camera fixed and the reference
        positions of ``alignment.inliers`` as position priors at ``sigma`` (a scalar, ``[n]`` or ``[n,3]``, units of ``ref_centres``),
        then a triangulation with the adjusted poses: align -> adjust -> triangulate.  ``rec2`` then carries the refined poses (an
        image without a pose keeps its NaN pose), ``K`` (when the focals are refined), ``points`` and ``bundle``.  ``ba_kwargs`` are
        ``bundle_adjust``'s.  Without ``refine`` the method is as before."""
        from .alignment import align
        return align(self, ref_centres, known, thresh, with_scale, apply, conf, seed, refine)

    def propose_pairs(self, sfm, top_k=5, min_shared=30, **kw):
        """The image pairs of ``sfm`` (the ``SfmResult`` this reconstruction came from) that were never matched but overlap, by
        projected-point overlap of the posed images (``proposals.propose_pairs``) -> ``(pairs [P,2] i64 with a < b, score
        [P] i64)``: what a second matching pass, and a loop closure of a sequentially matched set, start from."""
        from .proposals import propose_pairs
        return propose_pairs(self, sfm, top_k=top_k, min_shared=min_shared, **kw)


def register_images(offsets, obs_image, obs_xy, xyz, status, K, T_cam_from_world, posed, min_corr=15, min_inliers=15, thresh_px=4.0,
                    conf=0.999, seed=0, timings=None):
    """Resect the images that have no pose from the points their tracks already have -> ``Registration``.

    ``offsets [T+1]``, ``obs_image [N]``, ``obs_xy [N,2]`` as for ``triangulate_tracks``; ``xyz [T,3]`` and ``status [T]`` of a
    ``Points3D``; ``K [n,3,3]``; ``T_cam_from_world [n,4,4]`` (the poses of unposed images are never read); ``posed [n]`` (bool or
    integers).  CPU tensors or numpy arrays run the defining host routine and a loop over ``evaluation.estimate_absolute_pose_native``;
    GPU tensors (all of them, on one device) run the kernels and ONE ``ops.estimate_absolute_poses`` call over all candidates: the same
    result for one seed.

    An unposed image with at least ``min_corr`` (>= 4) correspondences is a candidate; a candidate whose estimate has at least
    ``min_inliers`` inliers at ``thresh_px`` pixels is registered: its pose is the estimator's f32 ``R``, ``t`` as float64.  One
    readback of the 8 counts; bad ``obs_image`` / ``offsets`` raise ValueError.  timings: a list that receives (stage, ms) pairs of the
    GPU stages."""
    what = "register_images"
    args = [offsets, obs_image, obs_xy, xyz, status, K, T_cam_from_world, posed]
    gpu = _tracks.one_device(what, _ARGS, args)
    for name, a in zip(_ARGS[:2], args[:2]):
        _tracks.integers(what, name, a)
    if not (isinstance(min_inliers, int) and not isinstance(min_inliers, bool) and math.isfinite(thresh_px) and thresh_px >= 0):
        raise ValueError(f"{what}: min_inliers must be an integer and thresh_px >= 0, got {min_inliers}, {thresh_px}")
    if gpu:
        dev = args[0].device
        dts = (torch.int64, torch.int32, torch.float32, torch.float32, torch.uint8, torch.float32, torch.float64, None)
        a = [x.detach() if dt is None else x.detach().to(dt) for x, dt in zip(args, dts)]
        a[7] = (a[7] != 0).to(torch.uint8)
    else:
        dev = torch.device("cpu")
        dts = (np.int64, np.int32, np.float32, np.float32, np.uint8, np.float32, np.float64, None)
        host = lambda x: x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        a = [np.ascontiguousarray(host(x)) if dt is None else np.ascontiguousarray(host(x), dt) for x, dt in zip(args, dts)]
        a[7] = (a[7] != 0).astype(np.uint8)
    n = a[7].shape[0] if a[7].ndim == 1 else -1
    if a[5].ndim != 3 or tuple(a[5].shape) != (n, 3, 3) or tuple(a[6].shape) != (n, 4, 4):
        raise LoftrHipError(f"{what}: expected K [n,3,3], T_cam_from_world [n,4,4] and posed [n], got {tuple(a[5].shape)}, {tuple(a[6].shape)}, "
                            f"{tuple(a[7].shape)}")
    if gpu:
        out = ops.register_corr(a[0], a[1], a[2], a[3], a[4], a[7], *_tracks.group_by_image(a[1], n), min_corr, timings=timings)
    else:
        if a[0].ndim == 1 and a[1].ndim == 1:                            # the errors the kernels report through counts[2]
            _tracks.check_host(what, a[0], a[1], n)
        out = ops.register_corr_host(a[0], a[1], a[2], a[3], a[4], a[7], *_tracks.group_by_image(a[1], n), min_corr)
        out = {k: torch.from_numpy(v) for k, v in out.items()}
        a = [torch.from_numpy(x) for x in a]
    counts = out["counts"].cpu().tolist()                               # the one readback
    _tracks.raise_error_bits(what, counts[2])
    C, P = counts[0], counts[1]
    cand = out["cand_image"][:P]
    cand64 = cand.to(torch.int64)
    table = {"cand_image": cand, "cand_offsets": out["cand_offsets"][:P + 1], "corr_xyz": out["corr_xyz"][:C], "corr_xy": out["corr_xy"][:C],
             "corr_obs": out["corr_obs"][:C]}
    Kc = a[5][cand64].contiguous()
    if P == 0:
        R, t = torch.zeros(0, 3, 3, device=dev), torch.zeros(0, 3, device=dev)
        inl, ninl = torch.zeros(0, dtype=torch.bool, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
    elif gpu:
        R, t, inl, ninl = ops.estimate_absolute_poses(table["corr_xyz"], table["corr_xy"], out["corr_bid"][:C], Kc, thresh_px, conf, seed)
    else:
        from .evaluation import estimate_absolute_pose_native
        R, t = torch.zeros(P, 3, 3), torch.zeros(P, 3)
        inl, ninl = torch.zeros(C, dtype=torch.bool), torch.full((P,), -1, dtype=torch.int64)
        off = table["cand_offsets"].tolist()
        for p in range(P):
            sl = slice(off[p], off[p + 1])
            est = estimate_absolute_pose_native(table["corr_xyz"][sl].numpy(), table["corr_xy"][sl].numpy(), Kc[p].numpy(), thresh_px, conf, seed)
            if est is not None:
                R[p], t[p] = torch.from_numpy(est[0]).float(), torch.from_numpy(est[1]).float()
                inl[sl] = torch.from_numpy(est[2])
                ninl[p] = int(est[2].sum())
    ok = ninl >= min_inliers                                            # [P]; a candidate is one image: no two writes meet below
    T_new = torch.zeros(P, 4, 4, dtype=torch.float64, device=dev)
    T_new[:, :3, :3], T_new[:, :3, 3], T_new[:, 3, 3] = R.to(torch.float64), t.to(torch.float64), 1.0
    T_out = a[6].clone()
    T_out[cand64] = torch.where(ok[:, None, None], T_new, a[6][cand64])
    registered = torch.zeros(n, dtype=torch.bool, device=dev)
    registered[cand64] = ok
    n_inliers = torch.full((n,), -1, dtype=torch.int64, device=dev)
    n_inliers[cand64] = ninl
    stats = {"n_correspondences": C, "n_candidates": P, "n_unposed": counts[3], "n_unposed_with_correspondences": counts[4],
             "n_correspondences_all": counts[5], "max_n_corr": counts[6], "n_images": n, "n_tracks": a[3].shape[0],
             "n_observations": a[1].shape[0]}
    return Registration(stats, T_cam_from_world=T_out, registered=registered, posed=(a[7] != 0) | registered, n_corr=out["n_corr"],
                        n_inliers=n_inliers, corr_inlier=inl, **table)


def triangulate_posed(offsets, obs_image, obs_xy, K, T_cam_from_world, posed, thresh_px=4.0, min_angle_deg=1.5, group=0):
    """``triangulate_tracks`` over the observations of the posed images only -> ``Points3D`` aligned with the FULL tracks: the CSR is
    filtered in torch (integer plumbing; a track keeps its row, so a track with fewer than 2 posed observations is ``too_short``), the
    poses of unposed images are never read, and ``obs_inlier`` is scattered back to the full observation order (false at the
    observations of unposed images).  Torch tensors on one device."""
    from .triangulation import triangulate_tracks
    dev = offsets.device
    posed = torch.as_tensor(posed).to(dev) != 0
    n, N, nt = K.shape[0], obs_image.shape[0], offsets.numel() - 1
    if tuple(posed.shape) != (n,):
        raise ValueError(f"triangulate: expected posed [{n}], got {tuple(posed.shape)}")
    image = obs_image.to(torch.int64)
    if n > 0:                                                          # an image id out of range stays in: triangulate_tracks reports it
        kept = torch.nonzero(posed[image.clamp(0, n - 1)] | (image < 0) | (image >= n)).reshape(-1)
    else:
        kept = torch.arange(N, device=dev)
    track = torch.repeat_interleave(torch.arange(nt, device=dev), offsets[1:] - offsets[:-1])
    sub = torch.zeros(nt + 1, dtype=torch.int64, device=dev)
    sub[1:] = torch.cumsum(torch.bincount(track[kept], minlength=nt), 0)
    T = torch.as_tensor(T_cam_from_world).to(dev, torch.float64)
    T = torch.where(posed[:, None, None], T, torch.eye(4, dtype=torch.float64, device=dev).expand(n, 4, 4))
    pts = triangulate_tracks(sub, obs_image[kept].to(torch.int32), obs_xy[kept], K, T, thresh_px=thresh_px, min_angle_deg=min_angle_deg, group=group)
    full = torch.zeros(N, dtype=torch.bool, device=dev)
    full[kept] = pts.obs_inlier
    pts.obs_inlier = full
    pts.stats["n_observations"], pts.stats["n_posed_observations"] = N, int(kept.numel())
    return pts


def _tensors(what, names, args):
    out = [a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)) for a in args]
    _tracks.one_device(what, names, out)
    return [a.detach() for a in out]


def _follow_group(K_in, K_out, group, cam_focal, G):
    """K_out with fx, skew, fy of the images without cam_focal scaled by the factor fx_out / fx_in of a member of their group that has it
    (1 where the group has none): integer indexing and one multiplication per entry, on the tensors' device."""
    ratio = torch.where(cam_focal, K_out[:, 0, 0] / K_in[:, 0, 0], torch.zeros_like(K_out[:, 0, 0]))
    per_group = torch.zeros(G, dtype=K_out.dtype, device=K_out.device).scatter_reduce(0, group, ratio, "amax")
    scale = torch.where(cam_focal | (per_group[group] == 0), torch.ones_like(ratio), per_group[group])
    K = K_out.clone()
    K[:, 0, 0], K[:, 0, 1], K[:, 1, 1] = K_out[:, 0, 0] * scale, K_out[:, 0, 1] * scale, K_out[:, 1, 1] * scale
    return K


def _follow_group_radial(k_in, k_out, group, cam_radial, G):
    """k_out with the k of the images without cam_radial moved by the step k_out - k_in of a member of their group that has it (0 where
    the group has none): the additive counterpart of _follow_group."""
    step = torch.where(cam_radial, k_out - k_in, torch.full_like(k_out, float("-inf")))
    per_group = torch.full((G,), float("-inf"), dtype=k_out.dtype, device=k_out.device).scatter_reduce(0, group, step, "amax")
    return torch.where(cam_radial | torch.isinf(per_group[group]), k_out, k_out + per_group[group])


def reconstruct_tracks(offsets, obs_image, obs_xy, K, init, max_rounds=50, ba=None, min_angle_deg=1.5, radial=None, start=None, **register_kw):
    """Incremental reconstruction from tracks and an initial pair -> ``Reconstruction``.

    ``offsets [T+1]``, ``obs_image [N]``, ``obs_xy [N,2]`` as for ``triangulate_tracks``, ``K [n,3,3]``; tensors on one device (GPU:
    the kernels; CPU: the host routines; the same result) or numpy arrays.  ``init`` = ``(a, b, R [3,3], t [3])`` with
    ``x_b = R x_a + t``, e.g. a five-point estimate: ``T[a] = I``, ``T[b] = [R | t / |t|]``; every other pose starts as NaN.

    A round is: triangulate over the posed images, ``bundle_adjust`` with image ``a`` fixed (``ba``: keyword arguments for
    ``bundle_adjust``; ``ba['fixed_extra']``: a ``[n]`` mask of further fixed images; ``position_prior`` and its keywords pass through
    as well, which makes sense only for a caller whose initial pair is already in the frame of the priors -- otherwise align first and
    use ``Reconstruction.align(refine=...)``), triangulate again with the adjusted poses,
    ``register_images`` (``register_kw``: its keyword arguments; ``thresh_px`` is also the triangulation's threshold).  The loop stops
    when a round registers nothing, when every image is posed, or after ``max_rounds``; then one more triangulate -> adjust ->
    triangulate.  An image is registered once: its pose changes afterwards only through the bundle adjustment.

    Only image ``a`` is fixed, which removes six of the seven gauge freedoms: the scale, set by ``|t| = 1`` at the start, is held only
    by the damping of the bundle adjustment and may drift slowly; fix ``b`` as well (``fixed_extra``) to pin it.

    With ``ba={'refine_focal': True}`` (or an ``[n]`` mask) every adjustment also refines the focal of the posed images
    named, and every step after an adjustment -- the triangulations, ``register_images``, the next adjustment -- uses the intrinsics it
    returned; ``Reconstruction.K`` holds the last.  The focal bounds of an adjustment are relative to the intrinsics it was given.

    With ``ba={'refine_focal': True, 'camera_ids': ids}`` the images of one camera share one relative focal step; the
    members of a camera that did not carry it in an adjustment (not posed yet, say) have their fx, skew, fy scaled by the factor their
    camera took, so that an image registered later starts from its camera's current focal.

    ``radial`` (``[n]``): the radial coefficients of the lenses, ``obs_xy`` being the stored, distorted pixels.  The
    triangulations and ``register_images`` then read ``undistort_points(obs_xy, obs_image, K, radial)``, recomputed after every
    adjustment.  With ``ba={'refine_focal': True, 'refine_radial': True[, 'camera_ids': ids]}`` the adjustment reads the stored pixels
    and refines the coefficients, starting from ``radial`` (default zeros); the members of a camera that did not carry it take their
    camera's step, as with the focal.  Without ``refine_radial`` the coefficients are taken as known: the adjustment is the pinhole
    call on the undistorted pixels.  ``Reconstruction.radial`` holds the final values.

    ``start = (T_cam_from_world [n,4,4], posed [n])`` or ``(T_cam_from_world, posed, fixed_image)`` instead of ``init`` (which must then
    be ``None``): the loop continues from poses somebody else found, for example ``global_positions`` (positions.py).
    ``fixed_image`` is the posed image the adjustments hold fixed (``SfmResult.reconstruct_global`` names the root of the rotation
    averaging); without it, it is the first posed image whose pose is exactly the identity, else the first posed one.  The images of
    ``start`` count as registered in round 0, and ``stats['init']`` is ``(fixed_image, None)``: there is no second image of a pair.  A
    start that holds exactly what ``init`` would have set gives the same result bit for bit."""
    from .bundle import bundle_adjust
    from .radial import undistort_points
    what = "reconstruct_tracks"
    offsets, obs_image, obs_xy, K = _tensors(what, ("offsets", "obs_image", "obs_xy", "K"), (offsets, obs_image, obs_xy, K))
    _tracks.integers(what, "offsets", offsets)
    _tracks.integers(what, "obs_image", obs_image)
    dev = offsets.device
    offsets, obs_image, obs_xy, K = offsets.to(torch.int64), obs_image.to(torch.int32), obs_xy.to(torch.float32), K.to(torch.float64)
    if K.dim() != 3 or tuple(K.shape[1:]) != (3, 3):
        raise LoftrHipError(f"{what}: expected K [n,3,3], got {tuple(K.shape)}")
    n = K.shape[0]
    if start is not None:
        if init is not None:
            raise ValueError(f"{what}: with start, init must be None")
        if len(start) not in (2, 3):
            raise ValueError(f"{what}: expected start = (T_cam_from_world, posed[, fixed_image]), got {len(start)} items")
        T0, posed0 = _tensors(what, ("start[0]", "start[1]"), tuple(start[:2]))
        T0, posed0 = T0.to(dev).to(torch.float64), posed0.to(dev) != 0
        if tuple(T0.shape) != (n, 4, 4) or tuple(posed0.shape) != (n,) or not bool(posed0.any()):
            raise ValueError(f"{what}: expected start = (T_cam_from_world [{n},4,4], posed [{n}]) with a posed image, got {tuple(T0.shape)}, "
                             f"{tuple(posed0.shape)}")
        if not bool(torch.isfinite(T0[posed0]).all()):
            raise ValueError(f"{what}: a posed image of start has a pose that is not finite")
        if len(start) == 3:
            a, b = int(start[2]), None
            if not 0 <= a < n or not bool(posed0[a]):
                raise ValueError(f"{what}: the fixed image of start must be a posed image in [0, {n}), got {start[2]!r}")
        else:
            gauge = posed0 & (T0 == torch.eye(4, dtype=torch.float64, device=dev)).reshape(n, 16).all(1)
            a, b = int(torch.nonzero(gauge if bool(gauge.any()) else posed0)[0]), None
    else:
        a, b, R, t = init
        a, b = int(a), int(b)
        R = torch.as_tensor(np.asarray(R.cpu() if isinstance(R, torch.Tensor) else R, np.float64)).reshape(3, 3)
        t = torch.as_tensor(np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t, np.float64)).reshape(3)
        if a == b or not (0 <= a < n and 0 <= b < n):
            raise ValueError(f"{what}: the initial pair must be two different images in [0, {n}), got a = {a}, b = {b}")
        norm = float(torch.linalg.norm(t))
        if not (bool(torch.isfinite(R).all()) and math.isfinite(norm) and norm > 0 and float(torch.linalg.det(R)) > 0):
            raise ValueError(f"{what}: init holds no relative pose (a refused five-point or P3P model returns zeros): det R = "
                             f"{float(torch.linalg.det(R))}, |t| = {norm}")
    ba = dict(ba or {})
    fixed = torch.zeros(n, dtype=torch.bool, device=dev)
    fixed[a] = True
    extra = ba.pop("fixed_extra", None)
    if extra is not None:
        fixed |= torch.as_tensor(extra).to(dev) != 0
    if "fixed" in ba:
        raise ValueError(f"{what}: image a is the fixed one; name further fixed images in ba['fixed_extra']")
    if ba.get("refine_focal") is not None and ba["refine_focal"] is not True:
        ba["refine_focal"] = torch.as_tensor(np.asarray(ba["refine_focal"].cpu() if isinstance(ba["refine_focal"], torch.Tensor)
                                                        else ba["refine_focal"])).to(dev)
    if ba.get("camera_ids") is not None:
        ba["camera_ids"] = torch.as_tensor(np.asarray(ba["camera_ids"].cpu() if isinstance(ba["camera_ids"], torch.Tensor)
                                                      else ba["camera_ids"])).to(dev)
    fits_lens = ba.get("refine_radial") is not None
    if fits_lens and ba["refine_radial"] is not True:
        ba["refine_radial"] = torch.as_tensor(np.asarray(ba["refine_radial"].cpu() if isinstance(ba["refine_radial"], torch.Tensor)
                                                         else ba["refine_radial"])).to(dev)
    if "radial" in ba:
        raise ValueError(f"{what}: the radial coefficients are an argument of the loop (radial=...), not of ba")
    rad = None
    if radial is not None or fits_lens:
        rad = torch.zeros(n, dtype=torch.float64, device=dev) if radial is None else \
            torch.as_tensor(np.asarray(radial.cpu() if isinstance(radial, torch.Tensor) else radial, np.float64)).to(dev)
        if tuple(rad.shape) != (n,):
            raise ValueError(f"{what}: expected radial [{n}], got {tuple(rad.shape)}")
    pinhole = lambda K, rad: obs_xy if rad is None else undistort_points(obs_xy, obs_image, K, rad)[0]
    thresh_px = register_kw.get("thresh_px", 4.0)
    T = torch.full((n, 4, 4), float("nan"), dtype=torch.float64, device=dev)
    posed = torch.zeros(n, dtype=torch.bool, device=dev)
    if start is not None:
        T[posed0] = T0[posed0]
        posed |= posed0
    else:
        T[a] = torch.eye(4, dtype=torch.float64)
        Tb = torch.eye(4, dtype=torch.float64)
        Tb[:3, :3], Tb[:3, 3] = R, t / norm
        T[b] = Tb
        posed[a] = posed[b] = True
    round_registered = torch.full((n,), -1, dtype=torch.int32, device=dev)
    round_registered[posed] = 0
    rounds = []

    def refine(T, posed, K, rad, first=False):
        """-> (points of the adjusted poses, the adjustment, the intrinsics and radial coefficients that hold from here on, the pinhole
        pixels under them)"""
        xy = pinhole(K, rad)
        pts = triangulate_posed(offsets, obs_image, xy, K, T, posed, thresh_px, min_angle_deg)
        if first and pts.stats["n_ok"] == 0:
            begun = f"the initial pair ({a}, {b}) triangulates" if start is None else \
                f"the {int(posed.sum())} posed images of start (fixed: {a}) triangulate"
            raise ValueError(f"{what}: {begun} nothing: {pts.stats['n_posed_observations']} observations in "
                             f"{pts.stats['n_tracks']} tracks, statuses {[pts.stats['n_' + s] for s in ops.TRI_STATUS]}")
        if fits_lens:                                                   # the adjustment fits the lens on the stored pixels
            res = bundle_adjust(offsets, obs_image, obs_xy, pts.obs_inlier, pts.xyz, K, T, fixed=fixed, radial=rad, **ba)
        else:
            res = bundle_adjust(offsets, obs_image, xy, pts.obs_inlier, pts.xyz, K, T, fixed=fixed, **ba)
        K_in, K = K, getattr(res, "K", K)                               # (a result without refine_focal carries no K)
        if hasattr(res, "cam_group"):                                   # an image posed later joins its camera at the camera's scale
            K = _follow_group(K_in, K, res.cam_group.long(), res.cam_focal, res.group_focal.numel())
        if fits_lens:
            rad = _follow_group_radial(rad, res.radial, res.cam_group.long(), res.cam_radial, res.group_focal.numel())
        xy = pinhole(K, rad)
        return triangulate_posed(offsets, obs_image, xy, K, res.T_cam_from_world, posed, thresh_px, min_angle_deg), res, K, rad, xy

    for r in range(1, int(max_rounds) + 1):
        pts, res, K, rad, xy = refine(T, posed, K, rad, first=r == 1)
        reg = register_images(offsets, obs_image, xy, pts.xyz, pts.status, K, res.T_cam_from_world, posed, **register_kw)
        n_new, n_posed = torch.stack([reg.registered.sum(), reg.posed.sum()]).tolist()
        round_registered[reg.registered] = r
        T, posed = reg.T_cam_from_world, reg.posed
        rounds.append({"round": r, "n_points": pts.stats["n_ok"], "rms_px_after": res.rms_px_after, "n_candidates": reg.stats["n_candidates"],
                       "n_registered": n_new, "n_posed": n_posed})
        if n_new == 0 or n_posed == n:
            break
    pts, res, K, rad, _ = refine(T, posed, K, rad, first=not rounds)
    stats = {"rounds": rounds, "n_rounds": len(rounds), "n_images": n, "n_posed": int(posed.sum()), "n_points": pts.stats["n_ok"],
             "rms_px_after": res.rms_px_after, "init": (a, b)}
    return Reconstruction(res.T_cam_from_world, posed, round_registered, pts, res, stats, K, rad)
