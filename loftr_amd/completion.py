"""Track completion: points claim the atlas keypoints they project onto, on the device.

LoFTR has no detector, so a track exists only where the matches of different rows snapped to the same ``cell_px`` cell of an image: one
physical point tends to end as several short tracks plus loose keypoints.  After a reconstruction every track with a 3D point can be
projected into every posed image it does not visit yet and claim the keypoint it lands on -- the step COLMAP runs after every adjustment
(``CompleteTracks``)::

    rec = sfm.reconstruct(K, complete=True)                   # the loop, one completion, triangulate -> adjust -> triangulate
    rec.sfm, rec.stats["completion"]                          # the relabelled atlas and the counts

or piece by piece::

    pts = sfm.triangulate(K, T, posed=posed)
    sfm2, done = sfm.complete(pts, K, T, posed=posed)         # done: Completion; sfm2 shares every tensor with sfm except track_id
    pts2 = sfm2.triangulate(K, T, posed=posed)

The rule (include/loftr_hip.h) is fp64 arithmetic in a fixed operation order, integer searches and one unsigned 64-bit
minimum per keypoint: the host routine ``loftr_complete_tracks_host`` defines it (CPU tensors / numpy arrays run it), the HIP kernels
reproduce it bit for bit (GPU tensors run them; there is no silent fallback either way).  Its whole result is a relabelled ``kp_row``.
"""
import math

import numpy as np
import torch

from . import _tracks, ops

_ARGS = ("offsets", "obs_image", "kp_offsets", "keypoints", "kp_row", "xyz", "status", "K", "T_cam_from_world")
_CELLS_BAD = "keypoints outside the grid, or cells that do not ascend strictly within an image (kp_cell of ops.model_cells)"


class Completion:
    """What ``complete_tracks`` returns (tensors on the device of the input).

    ``kp_row_new [K] i32`` (the winner's row where a keypoint was claimed, ``kp_row`` elsewhere), ``link_r2 [K] f32`` (the squared pixel
    distance of the accepted link, NaN elsewhere), ``linked [K] bool``; ``stats``: the eight counts by name (``ops.COMPLETE_NAMES``) plus
    ``n_links_from_loose`` (the old ``kp_row`` was -1) and ``n_links_from_pointless_rows`` (taken from a row without a point).
    ``n_blocked`` counts the (row, image) pairs that found only keypoints owned by another row WITH a point: what merging points would
    serve."""

    FIELDS = ("kp_row_new", "link_r2", "linked")

    def __init__(self, stats, **tensors):
        self.stats = stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])

    def to_host(self):
        """dict of numpy arrays (plus 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out["stats"] = dict(self.stats)
        return out


def default_reach(thresh_px, cell_px):
    """Cells to search on each side of the projection's cell so that every keypoint within ``thresh_px`` is met."""
    return int(math.ceil(float(thresh_px) / float(cell_px)))


def _raise(what, bits, cells):
    for bit, text in ops.COMPLETE_ERRORS:
        if bits & bit:
            raise ValueError(f"{what}: {text} (found on the device)")
    if cells & 16:
        raise ValueError(f"{what}: {_CELLS_BAD}")


def check_host_tables(what, offsets, obs_image, kp_offsets, keypoints, kp_row, n, T):
    """The errors the kernels report through counts[1], raised on host arrays before the host routine runs (completion and merging)."""
    if not (all(x.ndim == 1 for x in (offsets, obs_image, kp_offsets, kp_row)) and keypoints.ndim == 2):
        return
    _tracks.check_host(what, offsets, obs_image, n)
    if kp_offsets.size and (kp_offsets[0] != 0 or kp_offsets[-1] != keypoints.shape[0] or (np.diff(kp_offsets) < 0).any()):
        raise ValueError(f"{what}: kp_offsets must start at 0, end at the number of keypoints and ascend")
    inner = np.ones(max(obs_image.shape[0] - 1, 0), bool)
    starts = offsets[1:-1]
    inner[starts[(starts > 0) & (starts < obs_image.shape[0])] - 1] = False               # a step across a row boundary may descend
    if (np.diff(obs_image)[inner] < 0).any():
        raise ValueError(f"{what}: " + ops.COMPLETE_ERRORS[2][1])
    if kp_row.size and (kp_row.min() < -1 or kp_row.max() >= T):
        raise ValueError(f"{what}: " + ops.COMPLETE_ERRORS[3][1])


def complete_tracks(offsets, obs_image, kp_offsets, keypoints, kp_row, xyz, status, K, T_cam_from_world, image_hw, cell_px, posed=None,
                    thresh_px=4.0, reach=None, timings=None):
    """Let the rows that have a point claim the keypoints they project onto -> ``Completion``.

    ``offsets [T+1]``, ``obs_image [N]`` (ascending within a row): the CSR of the rows a ``Points3D`` was triangulated from, with its
    ``xyz [T,3]`` and ``status [T]``; ``kp_offsets [n+1]``, ``keypoints [K,2]``: the keypoint pool of the atlas; ``kp_row [K]``: the row
    that holds a keypoint, or -1; ``K [n,3,3]``, ``T_cam_from_world [n,4,4]``; ``image_hw`` / ``cell_px``: the atlas's grid geometry;
    ``posed [n]`` (None: every image).  CPU tensors or numpy arrays run the defining host routine; GPU tensors (all of them, on one
    device) run the kernels.

    A row with a point (status ok, finite xyz) is projected into every posed image with a valid camera that it does not visit; there
    it proposes the nearest keypoint within ``thresh_px`` among the cells at most ``reach`` from the projection's (``None``:
    ``ceil(thresh_px / cell_px)``) that is free: loose, or held by a row WITHOUT a point.  A keypoint proposed by several rows goes to
    the nearest, then to the lowest row; the others get nothing in that image.  One readback; a bad table raises ValueError.
    timings: a list that receives (stage, ms) pairs of the GPU stages."""
    from .atlas import _grid
    what = "complete_tracks"
    args = [offsets, obs_image, kp_offsets, keypoints, kp_row, xyz, status, K, T_cam_from_world]
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
        dts = (torch.int64, torch.int32, torch.int64, torch.float32, torch.int32, torch.float32, torch.uint8, torch.float64, torch.float64)
        a = [x.detach().to(dt) for x, dt in zip(args, dts)]
        n = a[2].numel() - 1
        p = torch.ones(max(n, 0), dtype=torch.uint8, device=a[0].device) if posed is None else (posed.detach() != 0).to(torch.uint8)
        T = a[0].numel() - 1
        kp_cell, cell_status = ops.model_cells(a[2], a[3], a[4], max(T, 0), gh, gw, inv)
        out = ops.complete_tracks(a[0], a[1], a[5], a[6], a[2], a[3], kp_cell, a[4], a[7], a[8], p, gh, gw, inv, float(thresh_px), reach,
                                  timings=timings)
        kp_row_old = a[4]
    else:
        dts = (np.int64, np.int32, np.int64, np.float32, np.int32, np.float32, np.uint8, np.float64, np.float64)
        host = lambda x: x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        a = [np.ascontiguousarray(host(x), dt) for x, dt in zip(args, dts)]
        n = a[2].shape[0] - 1
        p = np.ones(max(n, 0), np.uint8) if posed is None else np.ascontiguousarray(host(posed) != 0).astype(np.uint8)
        T = a[0].shape[0] - 1
        check_host_tables(what, a[0], a[1], a[2], a[3], a[4], n, T)
        kp_cell, cells = ops.model_cells_host(a[2], a[3], a[4], max(T, 0), gh, gw, inv)
        out = ops.complete_tracks_host(a[0], a[1], a[5], a[6], a[2], a[3], kp_cell, a[4], a[7], a[8], p, gh, gw, inv, float(thresh_px), reach)
        out = {k: torch.from_numpy(v) for k, v in out.items()}
        kp_row_old, cell_status = torch.from_numpy(a[4]), torch.tensor([cells], dtype=torch.int32)
    linked = ~torch.isnan(out["link_r2"])
    n_loose = (linked & (kp_row_old == -1)).sum()
    word = torch.cat([out["counts"], cell_status.to(torch.int64).reshape(1), n_loose.reshape(1)]).cpu().tolist()      # the one readback
    _raise(what, word[1], word[ops.COMPLETE_COUNTS])
    stats = {name: word[i] for i, name in enumerate(ops.COMPLETE_NAMES) if name != "error_bits"}
    stats.update(n_links_from_loose=word[-1], n_links_from_pointless_rows=word[0] - word[-1], n_rows=max(T, 0), n_keypoints=int(linked.numel()),
                 thresh_px=float(thresh_px), reach=reach)
    return Completion(stats, kp_row_new=out["kp_row_new"], link_r2=out["link_r2"], linked=linked)
