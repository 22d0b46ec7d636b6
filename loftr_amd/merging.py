"""Track merging: rows whose points meet and agree become one track, on the device.

Track completion (completion.py) stops where two tracks both have a point and only counts those meetings.  Merging serves
them -- the step COLMAP runs next to ``CompleteTracks`` after every adjustment (``MergeTracks``)::

    rec = sfm.reconstruct(K, merge=True)                      # the loop, one merge, triangulate -> adjust -> triangulate
    rec.sfm, rec.stats["merge"]                               # the relabelled atlas and the counts

or piece by piece::

    pts = sfm.triangulate(K, T, posed=posed)
    sfm2, merge = sfm.merge(pts, K, T, posed=posed)           # merge: Merge; sfm2 shares every tensor with sfm except track_id
    pts2 = sfm2.triangulate(K, T, posed=posed)

The rule (include/loftr_hip.h) is fp64 arithmetic in a fixed operation order, integer searches and two unsigned 64-bit
minima per accepted meeting: the host routine ``loftr_merge_tracks_host`` defines it (CPU tensors / numpy arrays run it), the HIP
kernels reproduce it bit for bit (GPU tensors run them; there is no silent fallback either way).  Its whole result is a relabelled
``kp_row``.
"""
import math

import numpy as np
import torch

from . import _tracks, ops
from .completion import _raise, check_host_tables, default_reach

_ARGS = ("offsets", "obs_image", "obs_xy", "obs_mask", "kp_offsets", "keypoints", "kp_row", "xyz", "status", "K", "T_cam_from_world")


class Merge:
    """What ``merge_tracks`` returns (tensors on the device of the input).

    ``row_into [T] i32`` (the surviving row of every row: the lower row of a merged pair, the row itself elsewhere), ``merge_r2 [T] f32``
    (the pair's score -- the largest squared pixel error of a defining observation of either row against the weighted point -- for both
    rows of a merged pair, NaN elsewhere), ``merged [T] bool``, ``kp_row_new [K] i32``; ``stats``: the eight counts by name
    (``ops.MERGE_NAMES``)."""

    FIELDS = ("row_into", "merge_r2", "merged", "kp_row_new")

    def __init__(self, stats, **tensors):
        self.stats = stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])

    def to_host(self):
        """dict of numpy arrays (plus 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out["stats"] = dict(self.stats)
        return out


def merge_tracks(offsets, obs_image, obs_xy, obs_mask, kp_offsets, keypoints, kp_row, xyz, status, K, T_cam_from_world, image_hw, cell_px,
                 posed=None, thresh_px=4.0, reach=None, timings=None):
    """Merge the rows whose points meet and agree -> ``Merge``.

    The arguments of ``completion.complete_tracks`` plus ``obs_xy [N,2]`` (the pixel of every observation) and ``obs_mask [N]`` (the
    observations that define the row's point: ``Points3D.obs_inlier``).  CPU tensors or numpy arrays run the defining host routine;
    GPU tensors (all of them, on one device) run the kernels.

    A row with a point is projected into every posed image with a valid camera that it does not visit; where the nearest keypoint
    within ``thresh_px`` that another row WITH a point holds is found, the two rows meet.  The meeting is accepted when the rows share
    no image and every masked observation of both lies within ``thresh_px`` of the point weighted by their masked observations.  Two
    rows that are each other's best accepted partner (smallest worst error, then lowest row) merge into the lower one; a row merges
    with at most one other per call.  One readback; a bad table raises ValueError.  timings: a list that receives (stage, ms) pairs of
    the GPU stages."""
    from .atlas import _grid
    what = "merge_tracks"
    args = [offsets, obs_image, obs_xy, obs_mask, kp_offsets, keypoints, kp_row, xyz, status, K, T_cam_from_world]
    names = _ARGS if posed is None else _ARGS + ("posed",)
    gpu = _tracks.one_device(what, names, args if posed is None else args + [posed])
    for name, a in zip(names, args):
        if name in ("offsets", "obs_image", "kp_offsets", "kp_row"):
            _tracks.integers(what, name, a)
    if not (math.isfinite(thresh_px) and thresh_px >= 0):
        raise ValueError(f"{what}: thresh_px must be finite and >= 0, got {thresh_px}")
    inv, gh, gw = _grid(image_hw, cell_px)
    if reach is None:
        reach = default_reach(thresh_px, cell_px)
    if not isinstance(reach, int) or isinstance(reach, bool) or not 0 <= reach <= ops.COMPLETE_MAX_REACH:
        raise ValueError(f"{what}: reach = {reach} cells is outside [0, {ops.COMPLETE_MAX_REACH}]: thresh_px = {thresh_px} is too wide for "
                         f"cell_px = {cell_px}; pass a reach, a smaller threshold, or build the atlas with a larger cell_px")
    if gpu:
        dts = (torch.int64, torch.int32, torch.float32, None, torch.int64, torch.float32, torch.int32, torch.float32, torch.uint8,
               torch.float64, torch.float64)
        a = [(x.detach() != 0).to(torch.uint8) if dt is None else x.detach().to(dt) for x, dt in zip(args, dts)]
        n = a[4].numel() - 1
        p = torch.ones(max(n, 0), dtype=torch.uint8, device=a[0].device) if posed is None else (posed.detach() != 0).to(torch.uint8)
        T = a[0].numel() - 1
        kp_cell, cell_status = ops.model_cells(a[4], a[5], a[6], max(T, 0), gh, gw, inv)
        out = ops.merge_tracks(a[0], a[1], a[2], a[3], a[7], a[8], a[4], a[5], kp_cell, a[6], a[9], a[10], p, gh, gw, inv, float(thresh_px),
                               reach, timings=timings)
    else:
        dts = (np.int64, np.int32, np.float32, None, np.int64, np.float32, np.int32, np.float32, np.uint8, np.float64, np.float64)
        host = lambda x: x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        a = [np.ascontiguousarray(host(x) != 0).astype(np.uint8) if dt is None else np.ascontiguousarray(host(x), dt) for x, dt in zip(args, dts)]
        n = a[4].shape[0] - 1
        p = np.ones(max(n, 0), np.uint8) if posed is None else np.ascontiguousarray(host(posed) != 0).astype(np.uint8)
        T = a[0].shape[0] - 1
        check_host_tables(what, a[0], a[1], a[4], a[5], a[6], n, T)
        kp_cell, cells = ops.model_cells_host(a[4], a[5], a[6], max(T, 0), gh, gw, inv)
        out = ops.merge_tracks_host(a[0], a[1], a[2], a[3], a[7], a[8], a[4], a[5], kp_cell, a[6], a[9], a[10], p, gh, gw, inv,
                                    float(thresh_px), reach)
        out = {k: torch.from_numpy(v) for k, v in out.items()}
        cell_status = torch.tensor([cells], dtype=torch.int32)
    word = torch.cat([out["counts"], cell_status.to(torch.int64).reshape(1)]).cpu().tolist()                           # the one readback
    _raise(what, word[1], word[ops.MERGE_COUNTS])
    stats = {name: word[i] for i, name in enumerate(ops.MERGE_NAMES) if name != "error_bits"}
    stats.update(n_rows=max(T, 0), n_keypoints=int(out["kp_row_new"].numel()), thresh_px=float(thresh_px), reach=reach)
    return Merge(stats, row_into=out["row_into"], merge_r2=out["merge_r2"], merged=~torch.isnan(out["merge_r2"]), kp_row_new=out["kp_row_new"])
