"""Triangulation of atlas tracks from known camera poses: one 3D point per track, on the device.

The step after ``KeypointAtlas``: with the poses of the database images (``T_cam_from_world``) and their intrinsics, every track becomes
a 3D point and every keypoint of the track learns whether it agrees with it -- the 2D-3D table that hloc-style localisation (Aachen,
InLoc) builds from database matches, without a depth map per image::

    sfm = atlas.finalize()
    pts = sfm.triangulate(K, T_cam_from_world, thresh_px=4.0, min_angle_deg=1.5)      # Points3D, on the atlas's device
    xyz, has = pts.keypoint_xyz(sfm)                                                  # [K,3] f32, [K] bool per atlas keypoint

The rule (include/loftr_hip.h) has no random numbers: two-ray midpoints over a fixed enumeration of at most 64 observation
pairs, scored by pixel reprojection error, the best one refitted by Gauss-Newton over its inliers, a minimum triangulation angle at the
end.  The host routine ``loftr_triangulate_tracks_host`` defines the result (CPU tensors / numpy arrays run it), the HIP kernels
reproduce it bit for bit (GPU tensors run them; there is no silent fallback either way).
"""
import math

import numpy as np
import torch

from . import _tracks, ops

_OUT = ("xyz", "n_inliers", "rms_px", "tri_cos", "status", "obs_inlier")


class Points3D:
    """What ``triangulate_tracks`` returns (tensors on the device of the input).

    ``xyz [T,3] f32`` (NaN unless the track is ok), ``n_inliers [T] i32``, ``rms_px [T] f32``, ``tri_cos [T] f32`` (cosine of the widest
    angle between two inlier rays of the enumerated pairs), ``status [T] u8`` (``ops.TRI_STATUS``: 0 ok, 1 too_short, 2 no_hypothesis,
    3 small_angle, 4 bad_camera), ``obs_inlier [N] bool`` (false for tracks that are not ok); ``stats``: dict of counts.
    ``SfmResult.triangulate`` also attaches the CSR arrays it triangulated: ``offsets [T+1]``, ``image [N]``, ``keypoint [N]`` (local)."""

    FIELDS = _OUT

    def __init__(self, stats, **tensors):
        self.stats = stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])
        self.offsets = self.image = self.keypoint = None

    @property
    def valid(self):
        """[T] bool: the track has a point (status ok)."""
        return self.status == 0

    def keypoint_xyz(self, sfm):
        """The 2D-3D table of the atlas ``sfm`` this result was triangulated from: (xyz [K,3] f32, has [K] bool) per atlas keypoint;
        ``has`` is true exactly at the inlier keypoints of valid tracks (xyz is NaN elsewhere)."""
        if self.offsets is None:
            raise ValueError("Points3D.keypoint_xyz: this result carries no tracks (use SfmResult.triangulate)")
        dev = self.xyz.device
        K = sfm.keypoints.shape[0]
        T = self.status.numel()
        track = torch.repeat_interleave(torch.arange(T, device=dev), self.offsets[1:] - self.offsets[:-1])
        sel = self.obs_inlier & self.valid[track]
        kp = (sfm.kp_offsets[self.image] + self.keypoint)[sel]
        xyz = torch.full((K, 3), float("nan"), dtype=torch.float32, device=dev)
        has = torch.zeros(K, dtype=torch.bool, device=dev)
        xyz[kp] = self.xyz[track[sel]]                                   # a keypoint belongs to one track: no two writes meet
        has[kp] = True
        return xyz, has

    def to_host(self):
        """dict of numpy arrays (plus 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out.update({k: getattr(self, k).cpu().numpy() for k in ("offsets", "image", "keypoint") if getattr(self, k) is not None})
        out["stats"] = dict(self.stats)
        return out


def triangulate_tracks(offsets, obs_image, obs_xy, K, T_cam_from_world, thresh_px=4.0, min_angle_deg=1.5, group=0, timings=None):
    """Triangulate tracks given in CSR form -> ``Points3D``.

    ``offsets [T+1]`` (integers), ``obs_image [N]`` (integers in [0, n_images)), ``obs_xy [N,2]`` pixels, ``K [n_images,3,3]`` and
    ``T_cam_from_world [n_images,4,4]`` (float32 or float64, passed as float64).  CPU tensors or numpy arrays run the defining host
    routine; GPU tensors (all of them, on one device) run the kernels.  ``thresh_px``: inlier threshold; ``min_angle_deg``: the smallest
    accepted triangulation angle; ``group``: 0, 8 or 64 lanes per track on the GPU (a tuning knob: the result does not depend on it).
    One readback of the 8 counts; bad ``obs_image`` / ``offsets`` raise ValueError."""
    what, names = "triangulate_tracks", ("offsets", "obs_image", "obs_xy", "K", "T_cam_from_world")
    args = (offsets, obs_image, obs_xy, K, T_cam_from_world)
    if not (math.isfinite(thresh_px) and thresh_px >= 0 and math.isfinite(min_angle_deg) and 0 <= min_angle_deg <= 180):
        raise ValueError(f"triangulate_tracks: thresh_px must be >= 0 and min_angle_deg in [0, 180], got {thresh_px}, {min_angle_deg}")
    if group not in (0, 8, 64):
        raise ValueError(f"triangulate_tracks: group must be 0, 8 or 64, got {group}")
    cos_min = math.cos(math.radians(float(min_angle_deg)))              # the host's libm, once: no trigonometry in the shared core
    gpu = _tracks.one_device(what, names, args)
    for n, a in zip(names[:2], args[:2]):
        _tracks.integers(what, n, a)
    if gpu:
        dts = (torch.int64, torch.int32, torch.float32, torch.float64, torch.float64)
        out = ops.triangulate_tracks(*[a.detach().to(dt) for a, dt in zip(args, dts)], float(thresh_px), cos_min, group=group, timings=timings)
    else:
        dts = (np.int64, np.int32, np.float32, np.float64, np.float64)
        a = [np.ascontiguousarray(x.detach().numpy() if isinstance(x, torch.Tensor) else x, dt) for x, dt in zip(args, dts)]
        if a[0].ndim == 1 and a[1].ndim == 1 and a[3].ndim == 3:         # the errors the kernels report through counts[5]
            _tracks.check_host(what, a[0], a[1], a[3].shape[0])
        out = {k: torch.from_numpy(v) for k, v in ops.triangulate_tracks_host(*a, float(thresh_px), cos_min).items()}
    counts = out["counts"].cpu().tolist()                               # the one readback
    _tracks.raise_error_bits(what, counts[5])
    stats = {"n_tracks": out["status"].numel(), "n_observations": out["obs_inlier"].numel(), "n_inlier_observations": counts[6]}
    stats.update({"n_" + name: counts[i] for i, name in enumerate(ops.TRI_STATUS)})
    out["obs_inlier"] = out["obs_inlier"].view(torch.bool)
    return Points3D(stats, **{k: out[k] for k in _OUT})
