"""Keypoint atlas: from the matches of a pair list to consolidated keypoints, index matches and tracks.

LoFTR has no detector.  ``mkpts1_f`` is a fresh sub-pixel point in every pair, ``mkpts0_f`` sits on the coarse grid, and an image is
side 0 in some rows of a pair list and side 1 in others, so two rows that share an image share no keypoint.  Multi-view consumers
(COLMAP / hloc-style SfM, triangulation, localisation from database poses) need the opposite: repeatable keypoints per image, matches
as index pairs, and tracks.  ``KeypointAtlas`` builds them on the device while the pair list is being matched::

    atlas = KeypointAtlas(n_images, image_hw, cell_px=2.0, device=dev)
    for rows, data in pairs.match_pair_list(model, pair_list, load, hw):
        atlas.add(pair_list[rows.start:rows.stop], data, mask=data.get("inliers"))     # no host synchronisation
    sfm = atlas.finalize(min_track_len=2)

The rules (include/loftr_hip.h):

1. every matched point falls into a ``cell_px`` cell of its image; a match whose mask bit is clear, whose numbers are not finite, whose
   confidence is negative or whose points leave the grid is counted in ``stats`` and otherwise ignored;
2. every occupied cell is one keypoint: position and score of its most confident observation (ties: the earliest), ordered by image,
   then row-major by cell;
3. within a row, a match is kept when it is the best of its keypoint on both sides (mutual best, one-to-one per row);
4. tracks are the connected components of the kept matches; ``track_ok`` is false when a track visits an image twice.

Everything is integer and order-defined: the host routine ``loftr_atlas_host`` defines the result (``device='cpu'`` runs it), the HIP
kernels reproduce it bit for bit.
"""
import numpy as np
import torch

from . import ops
from ._lib import LoftrHipError

_KEYS = ("mkpts0_f", "mkpts1_f", "mconf", "m_bids")


def _grid(image_hw, cell_px):
    """(inv, gh, gw): the fp32 reciprocal of the cell size that host and device multiply by, and the grid it gives."""
    H, W = float(image_hw[0]), float(image_hw[1])
    cell = np.float32(cell_px)
    if not (np.isfinite(cell) and cell > 0 and H > 0 and W > 0):
        raise ValueError(f"KeypointAtlas: image_hw and cell_px must be positive, got {tuple(image_hw)}, {cell_px}")
    inv = np.float32(1) / cell
    gh, gw = int(np.ceil(np.float32(H) * inv)), int(np.ceil(np.float32(W) * inv))
    if max(gh, gw) > 1 << 24:
        raise ValueError(f"KeypointAtlas: a {gh} x {gw} grid is beyond the supported 2^24 cells per side")
    return float(inv), gh, gw


class SfmResult:
    """What ``KeypointAtlas.finalize`` returns (tensors on the atlas's device).

    ``kp_offsets [n_images+1] i64`` delimits the images in ``keypoints [K,2] f32``, ``score [K] f32``, ``n_obs [K] i32``;
    ``row_offsets [R+1] i64`` delimits the rows in ``matches [Mk,2] i32`` (LOCAL keypoint indices of image a / image b of the row)
    and ``match_conf [Mk] f32``; ``track_id [K] i32`` (-1: none), ``track_len [T] i32``, ``track_ok [T] bool``; ``row_images [R,2] i32``;
    ``stats``: dict of counts.  ``image_hw`` / ``cell_px``: the atlas's grid geometry (None for a result built by hand)."""

    FIELDS = ("kp_offsets", "keypoints", "score", "n_obs", "row_offsets", "matches", "match_conf", "track_id", "track_len", "track_ok",
              "row_images")

    def __init__(self, stats, **tensors):
        self.stats = stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])
        self.image_hw = self.cell_px = None                            # set by KeypointAtlas.finalize
        self.is_undistorted = False                                     # True for the view that undistorted() returns
        self.is_refined = False                                         # True for the view that refine_tracks() returns

    def undistorted(self, K, radial):
        """The view of this result whose ``keypoints`` are the pinhole pixels of the stored ones under one radial coefficient per image
        (radial.undistort_points): ``K [n_images,3,3]``, ``radial [n_images]``.  Every other tensor is shared, and
        ``is_undistorted`` is True.  ``triangulate``, ``register``, ``adjust`` and ``pairwise_poses`` read it as they read any result (a
        keypoint that could not be undistorted is NaN and is left out by each of them); ``complete`` and ``merge`` raise ValueError on
        it: their cell lookup is in stored-pixel space.  A ``LocalizationModel`` is built from the ORIGINAL result with the points of
        this view: its lookups are by keypoint index, which the view does not change."""
        from .radial import undistort_points
        dev = self.keypoints.device
        n = self.kp_offsets.numel() - 1
        K, radial = (torch.as_tensor(x).detach().to(dev, torch.float64) for x in (K, radial))
        if tuple(K.shape) != (n, 3, 3) or tuple(radial.shape) != (n,):
            raise ValueError(f"SfmResult.undistorted: expected K [{n},3,3] and radial [{n}], got {tuple(K.shape)}, {tuple(radial.shape)}")
        xy, _ = undistort_points(self.keypoints, self.keypoint_image().to(torch.int32), K, radial)
        fields = {k: getattr(self, k) for k in self.FIELDS}
        fields.update(keypoints=xy)
        view = SfmResult(dict(self.stats), **fields)
        view.image_hw, view.cell_px, view.is_undistorted, view.is_refined = self.image_hw, self.cell_px, True, self.is_refined
        return view

    def refine_tracks(self, model, load, image_hw=None, obs_mask=None, max_std=None, max_shift_px=None, min_jobs_per_pair=1, **pair_list_kw):
        """Re-localise every observation of a consistent track against the track's reference view with the matcher's fine level
        (refinement.py) -> ``(view, refinement)``: the view shares every tensor with this result except ``keypoints`` and has
        ``is_refined`` True, the ``Refinement`` says what happened to every keypoint.  ``model``: a LoFTR in .eval() on a GPU; ``load``
        and the keyword arguments ``budget_bytes``, ``batch_size``, ``extract_batch`` as for ``pairs.match_pair_list``; ``image_hw``:
        the size of the loaded images (default: this result's); ``obs_mask`` [N] in the order of ``tracks(consistent_only=True)``,
        e.g. ``pts.obs_inlier``; a refined query is accepted when it is finite, inside the image, ``expec_f[:, 2] <= max_std`` and
        within ``max_shift_px`` of its old position (None: no limit).  ``triangulate``, ``register``, ``adjust`` and ``pairwise_poses``
        read the view as they read any result; ``complete``, ``merge`` and ``split`` raise ValueError on it (their cell lookups are
        in stored-pixel space), so refinement comes after the topology stages.  ``undistorted()`` of the view keeps ``is_refined``; an
        undistorted view is refused here, because the network saw the stored pixels.  A ``LocalizationModel`` is built from the
        ORIGINAL result with the points of the view."""
        from .refinement import refine_tracks
        return refine_tracks(self, model, load, image_hw=image_hw, obs_mask=obs_mask, max_std=max_std, max_shift_px=max_shift_px,
                             min_jobs_per_pair=min_jobs_per_pair, **pair_list_kw)

    def keypoint_image(self):
        """Image of every keypoint [K] i64."""
        n = self.kp_offsets.numel() - 1
        return torch.repeat_interleave(torch.arange(n, device=self.kp_offsets.device), self.kp_offsets[1:] - self.kp_offsets[:-1])

    def tracks(self, consistent_only=True):
        """CSR view of the tracks: (offsets [T'+1] i64, image [N] i64, local keypoint [N] i64), tracks in ascending id, the keypoints of
        a track in ascending global index (so by image).  consistent_only drops the tracks with track_ok false."""
        tid = self.track_id.to(torch.int64)
        use = tid >= 0
        ok = self.track_ok if consistent_only else torch.ones_like(self.track_ok)
        if tid.numel():
            use &= ok[tid.clamp(min=0)] if ok.numel() else torch.zeros_like(use)
        kp = torch.nonzero(use).reshape(-1)
        order = torch.sort(tid[kp], stable=True).indices
        kp = kp[order]
        image = self.keypoint_image()[kp]
        counts = torch.bincount(tid[kp], minlength=self.track_len.numel())[ok]
        offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=tid.device)
        offsets[1:] = torch.cumsum(counts, 0)
        return offsets, image, kp - self.kp_offsets[image]

    def triangulate(self, K, T_cam_from_world, thresh_px=4.0, min_angle_deg=1.5, consistent_only=True, group=0, posed=None):
        """One 3D point per track from the images' poses (triangulation.triangulate_tracks) -> Points3D on this result's
        device, with the CSR arrays of ``tracks(consistent_only)`` attached (``offsets``, ``image``, ``keypoint``).
        K [n_images,3,3], T_cam_from_world [n_images,4,4] (float32 or float64, tensors or arrays; moved to the device).
        posed: None, or [n_images] bool / integers: only the observations of these images are triangulated and the poses of the others
        are never read (registration.triangulate_posed); the result stays aligned with the full tracks, ``obs_inlier`` is
        false at the observations of unposed images and a track with fewer than 2 posed observations is too_short."""
        from .triangulation import triangulate_tracks
        dev = self.keypoints.device
        K, T = (torch.as_tensor(x).detach().to(dev, torch.float64) for x in (K, T_cam_from_world))
        n = self.kp_offsets.numel() - 1
        if tuple(K.shape) != (n, 3, 3) or tuple(T.shape) != (n, 4, 4):
            raise ValueError(f"SfmResult.triangulate: expected K [{n},3,3] and T_cam_from_world [{n},4,4], got {tuple(K.shape)}, {tuple(T.shape)}")
        offsets, image, local = self.tracks(consistent_only)
        xy = self.keypoints[self.kp_offsets[image] + local]
        if posed is None:
            pts = triangulate_tracks(offsets, image.to(torch.int32), xy, K, T, thresh_px=thresh_px, min_angle_deg=min_angle_deg, group=group)
        else:
            from .registration import triangulate_posed
            pts = triangulate_posed(offsets, image.to(torch.int32), xy, K, T, posed, thresh_px=thresh_px, min_angle_deg=min_angle_deg, group=group)
        pts.offsets, pts.image, pts.keypoint = offsets, image, local
        return pts

    def register(self, pts, K, T_cam_from_world, posed, **kwargs):
        """Resect the images without a pose from the points ``pts`` (a Points3D of ``triangulate`` on this result) that their tracks
        reach (registration.register_images) -> Registration on this result's device.  ``posed`` [n_images] and the keyword
        arguments are register_images'."""
        from .registration import register_images
        if pts.offsets is None:
            raise ValueError("SfmResult.register: this Points3D carries no tracks (use SfmResult.triangulate)")
        dev = self.keypoints.device
        K, T = (torch.as_tensor(x).detach().to(dev, torch.float64) for x in (K, T_cam_from_world))
        xy = self.keypoints[self.kp_offsets[pts.image] + pts.keypoint]
        return register_images(pts.offsets, pts.image.to(torch.int32), xy, pts.xyz, pts.status, K, T, torch.as_tensor(posed).to(dev), **kwargs)

    def pairwise_poses(self, K, thresh_px=4.0, conf=0.99999, seed=0):
        """Five-point poses of ALL rows from the kept matches: one ``ops.estimate_poses`` call on a GPU result, a loop over
        ``evaluation.estimate_pose_native`` on a CPU one (the same result for one seed).
        -> (R [R,3,3] f32, t [R,3] f32 with x_b = R x_a + t, n_inliers [R] i64, -1 without a model), on this result's device."""
        dev = self.keypoints.device
        n_rows = self.row_offsets.numel() - 1
        K32 = torch.as_tensor(K).detach().to(dev, torch.float32)
        row = torch.repeat_interleave(torch.arange(n_rows, device=dev), self.row_offsets[1:] - self.row_offsets[:-1])
        ims = self.row_images.to(torch.int64)
        m = self.matches.to(torch.int64)
        k0 = self.keypoints[self.kp_offsets[ims[row, 0]] + m[:, 0]].contiguous()
        k1 = self.keypoints[self.kp_offsets[ims[row, 1]] + m[:, 1]].contiguous()
        row_offsets = self.row_offsets
        if self.is_undistorted:                                          # a keypoint that could not be undistorted is NaN: its matches are left out
            keep = torch.isfinite(k0).all(1) & torch.isfinite(k1).all(1)
            k0, k1, row = k0[keep].contiguous(), k1[keep].contiguous(), row[keep]
            row_offsets = torch.zeros_like(self.row_offsets)
            row_offsets[1:] = torch.cumsum(torch.bincount(row, minlength=n_rows), 0)
        K0, K1 = K32[ims[:, 0]].contiguous(), K32[ims[:, 1]].contiguous()
        if dev.type == "cuda":
            R, t, _, ninl = ops.estimate_poses(k0, k1, row, K0, K1, thresh_px, conf, seed)
            return R, t, ninl
        from .evaluation import estimate_pose_native
        R, t, ninl = torch.zeros(n_rows, 3, 3), torch.zeros(n_rows, 3), torch.full((n_rows,), -1, dtype=torch.int64)
        off = row_offsets.tolist()
        for r in range(n_rows):
            sl = slice(off[r], off[r + 1])
            est = estimate_pose_native(k0[sl].numpy(), k1[sl].numpy(), K0[r].numpy(), K1[r].numpy(), thresh_px, conf, seed)
            if est is not None:
                R[r], t[r], ninl[r] = torch.from_numpy(est[0]).float(), torch.from_numpy(est[1]).float(), int(est[2].sum())
        return R, t, ninl

    def reconstruct(self, K, init_row=None, init_candidates=8, thresh_px=4.0, pose_conf=0.99999, consistent_only=True, complete=False, merge=False,
                    split=False, rotations=False, _candidate_rows=None, **kwargs):
        """Poses of the images and points of the tracks from intrinsics alone (registration.reconstruct_tracks) ->
        Reconstruction on this result's device, its ``points`` carrying the CSR arrays as ``triangulate`` attaches them.
        The initial pair is row ``init_row`` with its five-point pose (``pairwise_poses`` at ``thresh_px``).  With ``init_row=None``:
        of the ``init_candidates`` rows with the most five-point inliers (ties to the earliest row), the one whose two images alone
        triangulate the most points (ties to the earliest row); the selection is integer and order-defined.  ``thresh_px`` is also the
        triangulation's and the registration's threshold; the other keyword arguments are reconstruct_tracks'.
        ``radial`` ([n_images]): the coefficients of the lenses, known or a start for ``ba={'refine_radial': True, ...}``;
        the five-point poses and the choice of the initial pair then read the undistorted keypoints (``undistorted``), the loop is
        reconstruct_tracks' with that ``radial``, and ``complete`` / ``merge`` are refused (their cell lookup is in stored-pixel space).
        ``complete=True``: after the loop, one ``complete`` over the posed images with the final intrinsics, then triangulate -> adjust
        (the same fixed images and ``ba``) -> triangulate on the relabelled atlas; the Reconstruction then carries it as ``.sfm`` and the
        counts as ``stats['completion']``.  ``merge=True``: after the loop (and after the completion and one triangulation
        of it, when ``complete=True``), one ``merge`` of the tracks whose points meet and agree, then the same triangulate -> adjust ->
        triangulate; ``.sfm`` is the relabelled atlas and ``stats['merge']`` the counts.  ``split=True``: ``split`` runs first
        and everything after it, the five-point poses included, reads the split atlas, whose tracks are all consistent; ``.sfm`` is that
        atlas (or what ``complete`` / ``merge`` made of it) and ``stats['split']`` the counts.  ``rotations=True`` (or a dict
        of ``average_rotations`` keywords): ``rotation_averaging`` runs first, everything after it reads
        ``without_rows(ok rows | rows the graph could not judge)``, the initial pair is chosen among the ok rows only, and the
        Reconstruction carries the ``GlobalRotations`` as ``.rotations``, its counts as ``stats['rotations']`` and the atlas it was built
        on as ``.sfm``.  With the defaults nothing of this runs."""
        from .registration import reconstruct_tracks, triangulate_posed
        if rotations:
            view = self.undistorted(K, kwargs["radial"]) if kwargs.get("radial") is not None else self
            rot = view.rotation_averaging(K, thresh_px=thresh_px, pose_conf=pose_conf, seed=kwargs.get("seed", 0),
                                          **(rotations if isinstance(rotations, dict) else {}))
            sfm2, done = self.without_rows(rot.edge_ok | (rot.edge_state < 2))
            rec = sfm2.reconstruct(K, init_row=init_row, init_candidates=init_candidates, thresh_px=thresh_px, pose_conf=pose_conf,
                                   consistent_only=consistent_only, complete=complete, merge=merge, split=split,
                                   _candidate_rows=rot.edge_ok.cpu().tolist(), **kwargs)
            if rec.sfm is None:
                rec.sfm = sfm2
            rec.rotations = rot
            rec.stats.update(rotations=rot.stats, rows_removed=done.stats)
            return rec
        if split:
            sfm2, done = self.split()
            rec = sfm2.reconstruct(K, init_row=init_row, init_candidates=init_candidates, thresh_px=thresh_px, pose_conf=pose_conf,
                                   consistent_only=consistent_only, complete=complete, merge=merge, _candidate_rows=_candidate_rows, **kwargs)
            if rec.sfm is None:
                rec.sfm = sfm2
            rec.stats.update(split=done.stats)
            return rec
        dev = self.keypoints.device
        n = self.kp_offsets.numel() - 1
        K = torch.as_tensor(K).detach().to(dev, torch.float64)
        if tuple(K.shape) != (n, 3, 3):
            raise ValueError(f"SfmResult.reconstruct: expected K [{n},3,3], got {tuple(K.shape)}")
        lens = kwargs.get("radial") is not None or (kwargs.get("ba") or {}).get("refine_radial") is not None
        if lens and (complete or merge):
            raise ValueError("SfmResult.reconstruct: complete / merge under distortion are not modelled (their cell lookup is in stored-pixel space)")
        view = self.undistorted(K, kwargs["radial"]) if kwargs.get("radial") is not None else self
        R, t, ninl = view.pairwise_poses(K, thresh_px, pose_conf, kwargs.get("seed", 0))
        ninl_host, rows = ninl.cpu().tolist(), self.row_images.cpu().tolist()
        offsets, image, local = self.tracks(consistent_only)
        obs_image, xy = image.to(torch.int32), view.keypoints[self.kp_offsets[image] + local]
        if init_row is None:
            order = sorted((r for r in range(len(rows)) if ninl_host[r] >= 0 and (_candidate_rows is None or _candidate_rows[r])),
                           key=lambda r: (-ninl_host[r], r))[:max(int(init_candidates), 0)]
            if not order:
                raise ValueError(f"SfmResult.reconstruct: no row has a five-point model (inlier counts of the {len(rows)} rows: {ninl_host})")
            n_ok = []
            for r in sorted(order):
                a, b = rows[r]
                Tb, tb = torch.eye(4, dtype=torch.float64), t[r].cpu().to(torch.float64)       # on the host: one arithmetic for both devices
                Tb[:3, :3], Tb[:3, 3] = R[r].cpu().to(torch.float64), tb / torch.linalg.norm(tb)
                T = torch.eye(4, dtype=torch.float64, device=dev).repeat(n, 1, 1)
                T[b] = Tb.to(dev)
                posed = torch.zeros(n, dtype=torch.bool, device=dev)
                posed[a] = posed[b] = True
                n_ok.append((-triangulate_posed(offsets, obs_image, xy, K, T, posed, thresh_px, kwargs.get("min_angle_deg", 1.5)).stats["n_ok"], r))
            init_row = min(n_ok)[1]
        init_row = int(init_row)
        if not 0 <= init_row < len(rows) or ninl_host[init_row] < 0:
            raise ValueError(f"SfmResult.reconstruct: row {init_row} has no five-point model (rows: {len(rows)}, inliers: "
                             f"{ninl_host[init_row] if 0 <= init_row < len(rows) else None})")
        a, b = rows[init_row]
        xy = self.keypoints[self.kp_offsets[image] + local]              # the loop reads the stored pixels and undistorts them itself
        rec = reconstruct_tracks(offsets, obs_image, xy, K, (a, b, R[init_row], t[init_row]), thresh_px=thresh_px, **kwargs)
        rec.points.offsets, rec.points.image, rec.points.keypoint = offsets, image, local
        rec.stats["init_row"], rec.stats["pair_inliers"] = init_row, ninl_host
        if complete or merge:
            ba = dict(kwargs.get("ba") or {})
            fixed = torch.zeros(n, dtype=torch.bool, device=dev)
            fixed[a] = True
            extra = ba.pop("fixed_extra", None)
            if extra is not None:
                fixed |= torch.as_tensor(extra).to(dev) != 0
            tri = dict(thresh_px=thresh_px, min_angle_deg=kwargs.get("min_angle_deg", 1.5), consistent_only=consistent_only, posed=rec.posed)
            sfm2, pts = self, rec.points
            if complete:
                sfm2, done = sfm2.complete(pts, rec.K, rec.T_cam_from_world, posed=rec.posed, thresh_px=thresh_px)
                pts = sfm2.triangulate(rec.K, rec.T_cam_from_world, **tri)
                rec.stats.update(completion=done.stats)
            if merge:
                sfm2, merged = sfm2.merge(pts, rec.K, rec.T_cam_from_world, posed=rec.posed, thresh_px=thresh_px)
                pts = sfm2.triangulate(rec.K, rec.T_cam_from_world, **tri)
                rec.stats.update(merge=merged.stats)
            res = sfm2.adjust(pts, rec.K, rec.T_cam_from_world, fixed=fixed, **ba)
            K_in, rec.K = rec.K, getattr(res, "K", rec.K)                # (a result without refine_focal carries no K)
            if hasattr(res, "cam_group"):                                # (§18.2: an image without a pose keeps its camera's scale)
                from .registration import _follow_group
                rec.K = _follow_group(K_in, rec.K, res.cam_group.long(), res.cam_focal, res.group_focal.numel())
            rec.points = sfm2.triangulate(rec.K, res.T_cam_from_world, **tri)
            rec.T_cam_from_world, rec.bundle, rec.sfm = res.T_cam_from_world, res, sfm2
            rec.stats.update(n_points=rec.points.stats["n_ok"], rms_px_after=res.rms_px_after)
        return rec

    def _rows_of(self, who, pts, K, T_cam_from_world):
        """What ``complete`` and ``merge`` need of the rows of ``pts``: (the track id of every row, K and T on the device in fp64,
        kp_row [K] i32: the row that holds a keypoint, or -1)."""
        dev = self.keypoints.device
        n, n_kp, rows = self.kp_offsets.numel() - 1, self.keypoints.shape[0], pts.offsets.numel() - 1
        ok = self.track_ok.to(torch.bool)
        if rows == int(ok.sum()):                                        # tracks(consistent_only=True); the same list when every track is ok
            ids = torch.nonzero(ok).reshape(-1)
        elif rows == ok.numel():
            ids = torch.arange(rows, device=dev)
        else:
            raise ValueError(f"SfmResult.{who}: the Points3D has {rows} rows, this result {int(ok.sum())} consistent of {ok.numel()} tracks")
        K, T = (torch.as_tensor(x).detach().to(dev, torch.float64) for x in (K, T_cam_from_world))
        if tuple(K.shape) != (n, 3, 3) or tuple(T.shape) != (n, 4, 4):
            raise ValueError(f"SfmResult.{who}: expected K [{n},3,3] and T_cam_from_world [{n},4,4], got {tuple(K.shape)}, {tuple(T.shape)}")
        kp_row = torch.full((n_kp,), -1, dtype=torch.int32, device=dev)
        row = torch.repeat_interleave(torch.arange(rows, device=dev), pts.offsets[1:] - pts.offsets[:-1])
        kp_row[self.kp_offsets[pts.image] + pts.keypoint] = row.to(torch.int32)          # a keypoint belongs to one track: no two writes meet
        return ids, K, T, kp_row

    def _relabelled(self, track_id, **stats):
        """A new SfmResult that shares every tensor with this one except ``track_id`` and the ``track_len`` recomputed from it."""
        n_tracks = self.track_len.numel()
        track_len = torch.bincount(track_id[track_id >= 0].to(torch.int64), minlength=n_tracks).to(torch.int32)
        fields = {k: getattr(self, k) for k in self.FIELDS}
        fields.update(track_id=track_id, track_len=track_len)
        sfm2 = SfmResult(dict(self.stats, **stats), **fields)
        sfm2.image_hw, sfm2.cell_px = self.image_hw, self.cell_px
        return sfm2

    def edge_keypoints(self):
        """The kept matches as GLOBAL keypoint indices [Mk,2] i32 (integer indexing: the row of a match, its two images, their offsets)."""
        n_rows = self.row_offsets.numel() - 1
        row = torch.repeat_interleave(torch.arange(n_rows, device=self.row_offsets.device), self.row_offsets[1:] - self.row_offsets[:-1])
        base = self.kp_offsets[self.row_images.to(torch.int64)[row]]                         # [Mk,2]
        return (base + self.matches.to(torch.int64)).to(torch.int32).reshape(-1, 2)

    def split(self, min_track_len=2, max_rounds=32, timings=None):
        """Grow the keypoints of the tracks with ``track_ok`` false again into consistent tracks (splitting.split_tracks)
        -> ``(sfm2, split)``: a new SfmResult that shares every tensor with this one except ``track_id``, ``track_len`` and
        ``track_ok`` (all true), and the ``Split``.  A consistent track keeps its members; the tracks are numbered anew.  No pixel
        is read, so an undistorted view splits like the original.  This result is left untouched."""
        from .splitting import split_tracks
        if self.is_refined:
            raise ValueError("SfmResult.split: this is a refined view; the atlas's cells are in stored-pixel space (split the original result, then refine)")
        n = self.kp_offsets.numel() - 1
        done = split_tracks(self.edge_keypoints(), self.match_conf, self.keypoint_image().to(torch.int32), self.track_id,
                            self.track_ok, n, min_track_len=min_track_len, max_rounds=max_rounds, timings=timings)
        fields = {k: getattr(self, k) for k in self.FIELDS}
        fields.update(track_id=done.track_id_new, track_len=done.track_len_new, track_ok=torch.ones_like(done.track_len_new, dtype=torch.bool))
        sfm2 = SfmResult(dict(self.stats, n_tracks=done.stats["n_tracks"], n_split_rounds=done.stats["n_rounds"]), **fields)
        sfm2.image_hw, sfm2.cell_px, sfm2.is_undistorted = self.image_hw, self.cell_px, self.is_undistorted
        return sfm2, done

    def rotation_averaging(self, K, thresh_px=4.0, pose_conf=0.99999, seed=0, **kwargs):
        """The rows of the pair list as a view graph: the five-point rotations of ``pairwise_poses`` averaged into one rotation per image,
        the inlier counts as weights (rotations.average_rotations) -> ``GlobalRotations`` on this result's device.  Edge
        ``e`` is row ``e``: ``edge_ok[e]`` is the verdict of the row, a row without a model is invalid (state 0).  The keyword
        arguments are average_rotations'."""
        from .rotations import average_rotations
        R, _, ninl = self.pairwise_poses(K, thresh_px, pose_conf, seed)
        n = self.kp_offsets.numel() - 1
        return average_rotations(self.row_images, R.to(torch.float64), ninl.clamp(min=0).to(torch.int32), n, **kwargs)

    def global_positions(self, K, rot, thresh_px=4.0, pose_conf=0.99999, seed=0, **kwargs):
        """A centre for every camera of the view graph and a point for every consistent track, all at once, from the averaged rotations
        ``rot`` (a ``GlobalRotations`` of ``rotation_averaging`` on this pair list or on the one it was cut from; positions.global_positions;
        DESIGN §27) -> ``GlobalPositions`` on this result's device.  The start values walk the rows of ``rot.tree`` inside the root's
        component with the translation directions of ``pairwise_poses`` (the same seed gives the poses the averaging saw; a tree row
        that was removed since has no direction and is counted).  The keyword arguments are global_positions'."""
        from .positions import global_positions
        if self.is_refined:
            raise ValueError("SfmResult.global_positions: this is a refined view; position the original result, then refine")
        dev = self.keypoints.device
        n = self.kp_offsets.numel() - 1
        K = torch.as_tensor(K).detach().to(dev, torch.float64)
        if tuple(K.shape) != (n, 3, 3) or tuple(rot.R.shape) != (n, 3, 3) or rot.tree.numel() != self.row_images.shape[0]:
            raise ValueError(f"SfmResult.global_positions: expected K [{n},3,3] and the rotations of these {self.row_images.shape[0]} rows over "
                             f"{n} images, got {tuple(K.shape)}, {tuple(rot.R.shape)}, {rot.tree.numel()} rows")
        _, t, _ = self.pairwise_poses(K, thresh_px, pose_conf, seed)
        ims = self.row_images.to(torch.int64)
        in_graph = rot.in_graph.to(dev)
        rows = rot.tree.to(dev) & in_graph[ims[:, 0]] & in_graph[ims[:, 1]]
        offsets, image, local = self.tracks(consistent_only=True)
        xy = self.keypoints[self.kp_offsets[image] + local]
        return global_positions(offsets, image.to(torch.int32), xy, K, rot.R.to(dev), in_graph, int(rot.root), self.row_images[rows].to(torch.int32),
                                t[rows].to(torch.float64), **kwargs)

    def reconstruct_global(self, K, thresh_px=4.0, ba=None, rotations_kw=None, positions_kw=None, **register_kw):
        """Global reconstruction from intrinsics alone -> Reconstruction on this result's device: ``rotation_averaging``;
        everything after it reads ``without_rows(ok rows | rows the graph could not judge)``; ``global_positions`` gives every camera of
        the root's component with enough observations a pose at once; then registration.reconstruct_tracks continues from those poses
        (``start``): triangulate over the posed images, adjust with only the root fixed, triangulate again, and the images that still
        have no pose (chained only, or outside the graph) go through the existing rounds of register -> triangulate -> adjust ->
        triangulate.  ``ba``: bundle_adjust's keywords; ``rotations_kw`` / ``positions_kw``: average_rotations' / global_positions';
        ``register_kw``: reconstruct_tracks' other keywords.  The Reconstruction carries ``.rotations``, ``.positions``, the atlas it was
        built on as ``.sfm`` and the counts as ``stats['rotations']``, ``stats['positions']``."""
        from .registration import reconstruct_tracks
        dev = self.keypoints.device
        n = self.kp_offsets.numel() - 1
        K = torch.as_tensor(K).detach().to(dev, torch.float64)
        if tuple(K.shape) != (n, 3, 3):
            raise ValueError(f"SfmResult.reconstruct_global: expected K [{n},3,3], got {tuple(K.shape)}")
        rot = self.rotation_averaging(K, thresh_px=thresh_px, **(rotations_kw or {}))
        sfm2, done = self.without_rows(rot.edge_ok | (rot.edge_state < 2))
        pos = sfm2.global_positions(K, rot, thresh_px=thresh_px, **(positions_kw or {}))
        if not bool(pos.posed.any()):
            raise ValueError(f"SfmResult.reconstruct_global: global positioning posed no image ({pos.stats})")
        offsets, image, local = sfm2.tracks(consistent_only=True)
        xy = sfm2.keypoints[sfm2.kp_offsets[image] + local]
        rec = reconstruct_tracks(offsets, image.to(torch.int32), xy, K, None, start=(pos.T_cam_from_world, pos.posed, int(rot.root)), ba=ba,
                                 thresh_px=thresh_px, **register_kw)
        rec.points.offsets, rec.points.image, rec.points.keypoint = offsets, image, local
        rec.sfm, rec.rotations, rec.positions = sfm2, rot, pos
        rec.stats.update(rotations=rot.stats, rows_removed=done.stats, positions=pos.stats)
        return rec

    def pairwise_fundamentals(self, thresh_px=1.0, conf=0.999, seed=0):
        """Fundamental matrices of ALL rows from the kept matches, no intrinsics needed: one ``ops.estimate_geometry`` call on a GPU
        result, a loop over ``evaluation.estimate_fundamental_native`` on a CPU one (the same result for one seed).
        -> (F [R,3,3] f32 with x_b^T F x_a = 0 in pixels and unit norm, zero without a model; n_inliers [R] i64, -1 without a model), on
        this result's device."""
        dev = self.keypoints.device
        n_rows = self.row_offsets.numel() - 1
        row = torch.repeat_interleave(torch.arange(n_rows, device=dev), self.row_offsets[1:] - self.row_offsets[:-1])
        ims = self.row_images.to(torch.int64)
        m = self.matches.to(torch.int64)
        k0 = self.keypoints[self.kp_offsets[ims[row, 0]] + m[:, 0]].contiguous()
        k1 = self.keypoints[self.kp_offsets[ims[row, 1]] + m[:, 1]].contiguous()
        row_offsets = self.row_offsets
        if self.is_undistorted:                                          # a keypoint that could not be undistorted is NaN: its matches are left out
            keep = torch.isfinite(k0).all(1) & torch.isfinite(k1).all(1)
            k0, k1, row = k0[keep].contiguous(), k1[keep].contiguous(), row[keep]
            row_offsets = torch.zeros_like(self.row_offsets)
            row_offsets[1:] = torch.cumsum(torch.bincount(row, minlength=n_rows), 0)
        if dev.type == "cuda":
            F, _, ninl = ops.estimate_geometry(k0.to(torch.float32), k1.to(torch.float32), row, n_rows, "fundamental", thresh_px, conf, seed)
            return F, ninl
        from .evaluation import estimate_fundamental_native
        F, ninl = torch.zeros(n_rows, 3, 3), torch.full((n_rows,), -1, dtype=torch.int64)
        off = row_offsets.tolist()
        for r in range(n_rows):
            sl = slice(off[r], off[r + 1])
            est = estimate_fundamental_native(k0[sl].numpy(), k1[sl].numpy(), thresh_px, conf, seed)
            if est is not None:
                F[r], ninl[r] = torch.from_numpy(np.asarray(est[0])).float(), int(est[1].sum())
        return F, ninl

    def calibrate(self, f0=None, principal_point=None, camera_ids=None, thresh_px=1.0, seed=0, **params):
        """A focal length for every image from the fundamental matrices of all rows at once (calibration.calibrate_view_graph; DESIGN
        §28) -> ``ViewGraphCalibration`` on this result's device.  Edge ``e`` is row ``e`` with the F of ``pairwise_fundamentals`` at
        ``thresh_px`` and its inlier count as the weight; a row without a model is invalid (state 0).  ``f0=None``: 1.2 max(H, W) for
        every image, the usual guess without EXIF; ``principal_point=None``: (W / 2, H / 2), ASSUMED (both need the atlas's
        ``image_hw``).  ``camera_ids [n_images]``: images with one id share one focal scale.  ``params``: calibrate_view_graph's; the
        defaults are a prototype's, UNVALIDATED on real data."""
        from .calibration import calibrate_view_graph, default_focal
        if self.is_refined:
            raise ValueError("SfmResult.calibrate: this is a refined view; calibrate the original result, then refine")
        if (f0 is None or principal_point is None) and self.image_hw is None:
            raise ValueError("SfmResult.calibrate: f0=None and principal_point=None need the atlas's image_hw; this result carries none")
        dev = self.keypoints.device
        n = self.kp_offsets.numel() - 1
        if f0 is None:
            f0 = default_focal(self.image_hw)
        if principal_point is None:
            principal_point = (float(self.image_hw[1]) / 2.0, float(self.image_hw[0]) / 2.0)
        on = lambda x: x.to(dev) if isinstance(x, torch.Tensor) else (torch.as_tensor(np.asarray(x)).to(dev) if np.ndim(x) else x)
        F, ninl = self.pairwise_fundamentals(thresh_px=thresh_px, seed=seed)
        return calibrate_view_graph(self.row_images, F.to(torch.float64), ninl.clamp(min=0).to(torch.int32), n, on(principal_point), on(f0),
                                    camera_ids=None if camera_ids is None else on(camera_ids), **params)

    def reconstruct_uncalibrated(self, f0=None, camera_ids=None, global_=False, calibrate_kw=None, ba=None, **kw):
        """Reconstruction without intrinsics -> Reconstruction on this result's device: ``calibrate`` gives every image a
        focal length (the principal point is assumed), then ``reconstruct`` or, with ``global_=True``, ``reconstruct_global`` runs with
        that ``K``.  ``ba`` defaults to ``{'refine_focal': True}`` (plus ``camera_ids`` when given), so the bundle adjustment refines what
        the calibration left; ``calibrate_kw``: ``calibrate``'s other keywords; ``kw``: the reconstruction's.  The Reconstruction carries
        the ``ViewGraphCalibration`` as ``.calibration`` and its counts as ``stats['calibration']``."""
        cal = self.calibrate(f0=f0, camera_ids=camera_ids, **(calibrate_kw or {}))
        if ba is None:
            ba = {"refine_focal": True}
            if camera_ids is not None:
                ba["camera_ids"] = camera_ids
        rec = (self.reconstruct_global if global_ else self.reconstruct)(cal.K, ba=ba, **kw)
        rec.calibration = cal
        rec.stats.update(calibration=cal.stats)
        return rec

    def without_rows(self, rows_ok, min_track_len=2, max_rounds=32, timings=None):
        """This result without the matches of the rows where ``rows_ok [R]`` is false -> ``(sfm2, split)``.  Every track that holds a
        match of a rejected row loses its ``track_ok``; ``split_tracks`` then grows the keypoints of those tracks (and of the tracks
        that were inconsistent before) again over the matches of the kept rows only, so a consistent track that no rejected row touched
        keeps its members.  ``sfm2`` shares the keypoints with this result; its rejected rows are empty, its tracks are
        numbered anew and all consistent.  No kernel of its own.  This result is left untouched."""
        from .splitting import split_tracks
        if self.is_refined:
            raise ValueError("SfmResult.without_rows: this is a refined view; the atlas's cells are in stored-pixel space (drop the rows of the "
                             "original result, then refine)")
        dev = self.keypoints.device
        n, n_rows = self.kp_offsets.numel() - 1, self.row_offsets.numel() - 1
        rows_ok = torch.as_tensor(rows_ok).to(dev) != 0
        if tuple(rows_ok.shape) != (n_rows,):
            raise ValueError(f"SfmResult.without_rows: expected rows_ok [{n_rows}], got {tuple(rows_ok.shape)}")
        per_row = self.row_offsets[1:] - self.row_offsets[:-1]
        keep = rows_ok[torch.repeat_interleave(torch.arange(n_rows, device=dev), per_row)]
        edges = self.edge_keypoints()
        hit = self.track_id[edges[~keep].reshape(-1).to(torch.int64)].to(torch.int64)
        track_ok = self.track_ok.clone()
        track_ok[hit[hit >= 0]] = False
        done = split_tracks(edges[keep], self.match_conf[keep], self.keypoint_image().to(torch.int32), self.track_id, track_ok, n,
                            min_track_len=min_track_len, max_rounds=max_rounds, timings=timings)
        row_offsets = torch.zeros_like(self.row_offsets)
        row_offsets[1:] = torch.cumsum(torch.where(rows_ok, per_row, torch.zeros_like(per_row)), 0)
        fields = {k: getattr(self, k) for k in self.FIELDS}
        fields.update(matches=self.matches[keep], match_conf=self.match_conf[keep], row_offsets=row_offsets, track_id=done.track_id_new,
                      track_len=done.track_len_new, track_ok=torch.ones_like(done.track_len_new, dtype=torch.bool))
        sfm2 = SfmResult(dict(self.stats, n_tracks=done.stats["n_tracks"], n_kept=int(keep.sum()), n_rows_removed=int((~rows_ok).sum())), **fields)
        sfm2.image_hw, sfm2.cell_px, sfm2.is_undistorted = self.image_hw, self.cell_px, self.is_undistorted
        return sfm2, done

    def merge(self, pts, K, T_cam_from_world, posed=None, thresh_px=4.0, reach=None, timings=None):
        """Merge the tracks whose points ``pts`` (a Points3D of ``triangulate`` on this result) meet and agree (merging.merge_tracks;
        DESIGN §21) -> ``(sfm2, merge)``: a new SfmResult that shares every tensor with this one except ``track_id`` (the keypoints of
        an absorbed track carry the surviving track's id) and ``track_len`` (recomputed: an absorbed track has length 0; ``track_ok`` is
        unchanged, two merged tracks share no image), and the ``Merge`` whose rows are the tracks of ``pts``.  This result is left
        untouched.  The points are not re-estimated: triangulate ``sfm2`` next.  Calling again after that merges further."""
        from .merging import merge_tracks
        if self.is_refined:
            raise ValueError("SfmResult.merge: this is a refined view; the cell lookup is in stored-pixel space (merge the original result, then refine)")
        if self.is_undistorted:
            raise ValueError("SfmResult.merge: this is an undistorted view; the cell lookup is in stored-pixel space (merge the original result)")
        if pts.offsets is None:
            raise ValueError("SfmResult.merge: this Points3D carries no tracks (use SfmResult.triangulate)")
        if self.image_hw is None or self.cell_px is None:
            raise ValueError("SfmResult.merge: this result carries no grid geometry (image_hw / cell_px are set by KeypointAtlas.finalize)")
        dev = self.keypoints.device
        ids, K, T, kp_row = self._rows_of("merge", pts, K, T_cam_from_world)
        xy = self.keypoints[self.kp_offsets[pts.image] + pts.keypoint]
        done = merge_tracks(pts.offsets, pts.image.to(torch.int32), xy, pts.obs_inlier, self.kp_offsets, self.keypoints, kp_row, pts.xyz,
                            pts.status, K, T, self.image_hw, self.cell_px, posed=None if posed is None else torch.as_tensor(posed).to(dev),
                            thresh_px=thresh_px, reach=reach, timings=timings)
        track_id = self.track_id                                         # (without a row there is nothing to merge)
        if ids.numel() > 0:
            track_id = torch.where(done.kp_row_new != kp_row, ids[done.kp_row_new.to(torch.int64).clamp(min=0)].to(torch.int32), self.track_id)
        return self._relabelled(track_id, n_merges=done.stats["n_merges"]), done

    def complete(self, pts, K, T_cam_from_world, posed=None, thresh_px=4.0, reach=None, timings=None):
        """Let the points ``pts`` (a Points3D of ``triangulate`` on this result) claim the keypoints they project onto in the posed
        images their tracks do not visit (completion.complete_tracks) -> ``(sfm2, completion)``: a new SfmResult that
        shares every tensor with this one except ``track_id`` (the claimed keypoints carry the claiming track's id) and ``track_len``
        (recomputed: a track that yielded every keypoint has length 0 or 1 and triangulates as too_short; ``track_ok`` is unchanged),
        and the ``Completion`` whose rows are the tracks of ``pts`` (the r-th row is the r-th track that ``tracks()`` enumerated).
        This result is left untouched.

        Meant for AFTER the reconstruction loop: only a keypoint that is loose or held by a track WITHOUT a point can be claimed, and
        a track that has no point YET, because its images have no pose yet, would yield its keypoints as well."""
        from .completion import complete_tracks
        if self.is_refined:
            raise ValueError("SfmResult.complete: this is a refined view; the cell lookup is in stored-pixel space (complete the original result, then refine)")
        if self.is_undistorted:
            raise ValueError("SfmResult.complete: this is an undistorted view; the cell lookup is in stored-pixel space (complete the original result)")
        if pts.offsets is None:
            raise ValueError("SfmResult.complete: this Points3D carries no tracks (use SfmResult.triangulate)")
        if self.image_hw is None or self.cell_px is None:
            raise ValueError("SfmResult.complete: this result carries no grid geometry (image_hw / cell_px are set by KeypointAtlas.finalize)")
        dev = self.keypoints.device
        ids, K, T, kp_row = self._rows_of("complete", pts, K, T_cam_from_world)
        rows = ids.numel()
        done = complete_tracks(pts.offsets, pts.image.to(torch.int32), self.kp_offsets, self.keypoints, kp_row, pts.xyz, pts.status, K, T,
                               self.image_hw, self.cell_px, posed=None if posed is None else torch.as_tensor(posed).to(dev),
                               thresh_px=thresh_px, reach=reach, timings=timings)
        track_id = self.track_id                                         # (without a row there is no link)
        if rows > 0:
            track_id = torch.where(done.linked, ids[done.kp_row_new.to(torch.int64).clamp(min=0)].to(torch.int32), self.track_id)
        return self._relabelled(track_id, n_completion_links=done.stats["n_links"]), done

    def adjust(self, pts, K, T_cam_from_world, fixed=None, **kwargs):
        """Bundle adjustment of the poses and of the points ``pts`` (a Points3D of ``triangulate`` on this result) over the observations
        the triangulation kept (bundle.bundle_adjust) -> BundleResult on this result's device.  ``fixed`` and the keyword
        arguments are bundle_adjust's; the intended loop is triangulate -> adjust -> triangulate(K, res.T_cam_from_world).  With
        ``refine_focal`` (True or an [n] mask) the focal lengths are refined as well and the loop goes on with ``res.K``;
        with ``camera_ids`` ([n] integers) the images of one camera share that step; with ``position_prior`` ([n,3];
        ``prior_sigma``, ``prior_mask``) the camera centres are held near measured positions; with ``refine_radial``
        (``radial``, ``radial_bounds``; on the ORIGINAL result, whose keypoints are the stored pixels) every camera
        refines one radial coefficient as well."""
        from .bundle import bundle_adjust
        if pts.offsets is None:
            raise ValueError("SfmResult.adjust: this Points3D carries no tracks (use SfmResult.triangulate)")
        dev = self.keypoints.device
        K, T = (torch.as_tensor(x).detach().to(dev, torch.float64) for x in (K, T_cam_from_world))
        xy = self.keypoints[self.kp_offsets[pts.image] + pts.keypoint]
        if fixed is not None:
            fixed = torch.as_tensor(fixed).to(dev)
        if kwargs.get("refine_focal") is not None and kwargs["refine_focal"] is not True:
            kwargs["refine_focal"] = torch.as_tensor(kwargs["refine_focal"]).to(dev)
        if kwargs.get("camera_ids") is not None:                         # (images with equal ids share one focal step)
            kwargs["camera_ids"] = torch.as_tensor(kwargs["camera_ids"]).to(dev)
        for k in ("refine_radial", "radial"):                            # (one radial coefficient per camera)
            if kwargs.get(k) is not None and kwargs[k] is not True:
                kwargs[k] = torch.as_tensor(kwargs[k]).to(dev)
        for k in ("position_prior", "prior_sigma", "prior_mask"):        # (position priors on the camera centres)
            if kwargs.get(k) is not None and not isinstance(kwargs[k], (int, float)):
                kwargs[k] = torch.as_tensor(kwargs[k]).to(dev)
        return bundle_adjust(pts.offsets, pts.image.to(torch.int32), xy, pts.obs_inlier, pts.xyz, K, T, fixed=fixed, **kwargs)

    def to_host(self):
        """dict of numpy arrays (plus 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out["stats"] = dict(self.stats)
        return out


class KeypointAtlas:
    """Accumulates the matches of a pair list (``add``) and consolidates them (``finalize``); see the module docstring.

    ``image_hw``: extents (H, W) of the keypoint coordinates (after scale0 / scale1), the same for every image.  ``device='cpu'`` runs the
    defining host routine on host arrays; a GPU device keeps everything on it: one 8-byte word per cell of every image
    (``bytes_needed``; refused beyond ``max_bytes``, default half the free device memory) plus 29 bytes per match, grown geometrically
    from ``capacity`` matches."""

    def __init__(self, n_images, image_hw, cell_px=2.0, device="cuda", max_bytes=None, capacity=4096):
        self.n_images = int(n_images)
        if self.n_images < 1:
            raise ValueError(f"KeypointAtlas: n_images must be positive, got {n_images}")
        self.image_hw = (float(image_hw[0]), float(image_hw[1]))
        self.cell_px = float(cell_px)
        self.inv, self.gh, self.gw = _grid(image_hw, cell_px)
        if self.n_images * self.gh * self.gw >= 2 ** 31:
            raise ValueError(f"KeypointAtlas: {self.n_images} images of {self.gh} x {self.gw} cells are beyond the supported 2^31 cells")
        self.device = torch.device(device)
        self.n_rows = 0
        self.n_matches = 0
        self._done = False
        need = self.bytes_needed(n_images, image_hw, cell_px)
        if self.device.type != "cuda":
            if self.device.type != "cpu":
                raise LoftrHipError(f"KeypointAtlas: device must be a GPU or 'cpu' (the host routine), got {self.device}")
            self._chunks, self._row_images = [], []
            return
        if not torch.cuda.is_available():
            raise LoftrHipError("KeypointAtlas: no GPU here; device='cpu' runs the host routine (there is no silent fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if max_bytes is None:
            max_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
        if need > int(max_bytes):
            raise ValueError(f"KeypointAtlas: the cell grid needs {need} bytes ({self.n_images} images x {self.gh} x {self.gw} cells x 8), "
                             f"more than max_bytes = {int(max_bytes)}; use a larger cell_px")
        self.grid = torch.zeros(self.n_images * self.gh * self.gw, dtype=torch.int64, device=self.device)
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._cap = self._row_cap = 0
        self._store = {}
        self._rows_dev = None
        self._reserve(max(1, int(capacity)), 16)

    @staticmethod
    def bytes_needed(n_images, image_hw, cell_px=2.0):
        """Device bytes of the cell grid: one 64-bit word per cell of every image."""
        _, gh, gw = _grid(image_hw, cell_px)
        return 8 * int(n_images) * gh * gw

    # ---- storage: grows geometrically, like a list; the copies are stream-ordered --------------------------------------------------
    _LAYOUT = (("obs_xy", 4, torch.float32), ("obs_cell", 2, torch.int32), ("m_conf", 1, torch.float32), ("m_row", 1, torch.int32),
               ("m_reason", 1, torch.uint8))

    def _reserve(self, matches, rows):
        if matches > self._cap:
            cap = max(matches, 2 * self._cap)
            for name, width, dt in self._LAYOUT:
                new = torch.empty(cap * width, dtype=dt, device=self.device)
                if self.n_matches:
                    new[:self.n_matches * width].copy_(self._store[name][:self.n_matches * width])
                self._store[name] = new
            self._cap = cap
        if rows > self._row_cap:
            cap = max(rows, 2 * self._row_cap)
            new = torch.empty(cap, 2, dtype=torch.int32, device=self.device)
            if self.n_rows:
                new[:self.n_rows].copy_(self._rows_dev[:self.n_rows])
            self._rows_dev, self._row_cap = new, cap

    def add(self, image_ids, data, mask=None):
        """Add the matches of ``n`` pair-list rows.  ``image_ids`` [n,2]: images (a, b) of the rows; ``data``: the dict that ``forward`` /
        ``match_pairs`` leaves for them (``mkpts0_f``, ``mkpts1_f``, ``mconf``, ``m_bids``; ``m_bids`` in [0, n), ascending, as the matcher
        emits them); ``mask`` [M] bool: matches to use (e.g. ``data['inliers']`` of ``verify_matches``).  Rows get ids in arrival order.
        On a GPU nothing here waits for the device: ``m_bids`` that live there are checked by the kernel and reported by ``finalize``."""
        if self._done:
            raise ValueError("KeypointAtlas.add: the atlas is finalized; build a new one")
        ids = np.asarray(image_ids.cpu() if isinstance(image_ids, torch.Tensor) else image_ids)
        if ids.ndim != 2 or ids.shape[1] != 2 or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError(f"KeypointAtlas.add: image_ids must be an integer array [n, 2], got {ids.shape} {ids.dtype}")
        n = ids.shape[0]
        if n and (ids.min() < 0 or ids.max() >= self.n_images):
            raise ValueError(f"KeypointAtlas.add: image ids outside [0, {self.n_images}): {ids[((ids < 0) | (ids >= self.n_images)).any(1)][:8].tolist()}")
        if n and (ids[:, 0] == ids[:, 1]).any():
            raise ValueError(f"KeypointAtlas.add: rows that pair an image with itself: {np.nonzero(ids[:, 0] == ids[:, 1])[0][:8].tolist()}")
        missing = [k for k in _KEYS if k not in data]
        if missing:
            raise ValueError(f"KeypointAtlas.add: data lacks {missing} (pass the dict that forward / match_pairs leaves)")
        t = [torch.as_tensor(data[k]) for k in _KEYS]
        M = t[0].shape[0]
        if tuple(t[0].shape) != (M, 2) or tuple(t[1].shape) != (M, 2) or tuple(t[2].shape) != (M,) or tuple(t[3].shape) != (M,):
            raise ValueError(f"KeypointAtlas.add: expected mkpts0_f / mkpts1_f [M,2], mconf / m_bids [M], got {[tuple(x.shape) for x in t]}")
        if t[3].dtype.is_floating_point or t[3].dtype == torch.bool:
            raise ValueError(f"KeypointAtlas.add: m_bids must be integers, got {t[3].dtype}")
        if mask is not None:
            mask = torch.as_tensor(mask)
            if tuple(mask.shape) != (M,) or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"KeypointAtlas.add: mask must be bool [{M}], got {tuple(mask.shape)} {mask.dtype}")
        for x in t + ([mask] if mask is not None else []):
            if x.is_cuda and x.device != self.device:
                raise LoftrHipError(f"KeypointAtlas.add: data on {x.device}, the atlas on {self.device}")
        if M and n == 0:
            raise ValueError(f"KeypointAtlas.add: {M} matches but no row")
        if M and not t[3].is_cuda:                                 # host ids: checked here; device ids: by the kernel, reported by finalize
            self._check_bids(t[3].numpy(), n)
        if self.n_matches + M > 2 ** 31 - 2:
            raise ValueError("KeypointAtlas.add: more than 2^31 - 2 matches")
        ids32 = np.ascontiguousarray(ids, np.int32)
        if self.device.type == "cpu":
            k0, k1, c = (x.detach().to("cpu", torch.float32).numpy().copy() for x in t[:3])
            bids = t[3].detach().cpu().numpy()
            self._check_bids(bids, n)
            self._chunks.append((k0, k1, c, (self.n_rows + bids).astype(np.int32),
                                 np.ones(M, np.uint8) if mask is None else (mask.detach().cpu().numpy() != 0).astype(np.uint8)))
            self._row_images.append(ids32)
        else:
            self._reserve(self.n_matches + M, self.n_rows + n)
            with torch.cuda.device(self.device):
                if n:
                    self._rows_dev[self.n_rows:self.n_rows + n].copy_(torch.from_numpy(ids32), non_blocking=True)
                if M:
                    k0, k1, c = (x.detach().to(self.device, torch.float32, non_blocking=True).contiguous() for x in t[:3])
                    bids = t[3].detach().to(self.device, torch.int64, non_blocking=True).contiguous()
                    mk = None if mask is None else mask.detach().to(self.device, non_blocking=True).to(torch.uint8).contiguous()
                    s = self._store
                    ops.atlas_observe(k0, k1, c, bids, mk, n, self.n_matches, self.n_rows, self._rows_dev, self.n_images, self.gh, self.gw,
                                      self.inv, self.grid, s["obs_xy"], s["obs_cell"], s["m_conf"], s["m_row"], s["m_reason"], self._status)
        self.n_rows += n
        self.n_matches += M

    @staticmethod
    def _check_bids(bids, n):
        if bids.size and (bids.min() < 0 or bids.max() >= n):
            raise ValueError(f"KeypointAtlas.add: m_bids outside [0, {n})")
        if bids.size and (np.diff(bids) < 0).any():
            raise ValueError("KeypointAtlas.add: m_bids must ascend (matches grouped by row, as the matcher emits them)")

    def finalize(self, min_track_len=2, timings=None):
        """Consolidate: -> SfmResult.  One readback of a constant number of counts (K, Mk, T, status, reasons), whatever the number of
        rows or images.  The atlas accepts no ``add`` afterwards.  timings: a list that receives (stage, ms) pairs of the GPU stages."""
        if self._done:
            raise ValueError("KeypointAtlas.finalize: the atlas is already finalized")
        if int(min_track_len) < 1:
            raise ValueError(f"KeypointAtlas.finalize: min_track_len must be at least 1, got {min_track_len}")
        M, R = self.n_matches, self.n_rows
        if self.device.type == "cpu":
            cat = lambda i, shape, dt: np.concatenate([c[i] for c in self._chunks]) if self._chunks else np.zeros(shape, dt)
            rows = np.concatenate(self._row_images) if self._row_images else np.zeros((0, 2), np.int32)
            out = ops.atlas_host(cat(0, (0, 2), np.float32), cat(1, (0, 2), np.float32), cat(2, (0,), np.float32), cat(3, (0,), np.int32),
                                 cat(4, (0,), np.uint8), rows, self.n_images, self.gh, self.gw, self.inv, int(min_track_len))
            out = {k: torch.from_numpy(v) for k, v in out.items()}
            row_images = torch.from_numpy(rows)
        else:
            s = self._store
            out = ops.atlas_finalize(self.grid, s["obs_xy"], s["obs_cell"], s["m_conf"], s["m_row"], s["m_reason"], self._status, M, R,
                                     self.n_images, self.gh, self.gw, int(min_track_len), timings=timings)
            row_images = self._rows_dev[:R]
        self._done = True
        counts = out["counts"].cpu().tolist()                      # the one readback
        K, Mk, T, status = counts[:4]
        if status & 1:
            raise ValueError("KeypointAtlas: an add received m_bids outside [0, n) (found on the device)")
        if status & 2:
            raise ValueError("KeypointAtlas: an add received m_bids that do not ascend (found on the device)")
        stats = {"n_images": self.n_images, "n_rows": R, "n_matches": M, "n_keypoints": K, "n_kept": Mk, "n_tracks": T}
        stats.update({name: counts[4 + i] for i, name in enumerate(ops.ATLAS_REASONS) if name != "n_bad_row"})
        sfm = SfmResult(stats, kp_offsets=out["kp_offsets"], keypoints=out["keypoints"][:K], score=out["score"][:K], n_obs=out["n_obs"][:K],
                        row_offsets=out["row_offsets"], matches=out["matches"][:Mk], match_conf=out["match_conf"][:Mk],
                        track_id=out["track_id"][:K], track_len=out["track_len"][:T], track_ok=out["track_ok"][:T].to(torch.bool),
                        row_images=row_images)
        sfm.image_hw, sfm.cell_px = self.image_hw, self.cell_px       # the grid geometry (plain attributes: LocalizationModel.from_atlas)
        return sfm
