"""Localisation of query images against a triangulated model: from the matches of a query with its retrieved database images to
fused 2D-3D correspondences and one pose per query, on the device.

The last link of the hloc-style pipeline (feature banks -> ``KeypointAtlas`` -> ``SfmResult.triangulate`` -> here), the Aachen /
outdoor-InLoc case where no database image has a depth map::

    model = LocalizationModel.from_atlas(sfm, pts)                  # the atlas keypoints and the 3D point of each (built once)
    loc = QueryLocalizer(model, n_queries)
    for rows, data in pairs.match_pair_list(matcher, pair_list, load, hw):            # rows pair a query image with a database image
        loc.add(query_ids, db_image_ids, data, db_side=1, mask=data.get("inliers"))   # no host synchronisation
    res = loc.solve(K_query, thresh_px=3.0, conf=0.999, seed=0)     # QueryPoses: R, t, n_inliers per query + the correspondences

The rules (include/loftr_hip.h):

1. the database-side point of a match falls into a cell of the atlas's grid; the match is a candidate when its mask bit is set, its
   numbers are finite, its confidence is not negative, the cell holds a keypoint of that database image and the keypoint has a 3D
   point; every other match is counted in ``stats`` under the first reason that applies;
2. of the candidates of one (query, 3D point) the most confident is kept (ties: the earliest), the others are fused into it, so that
   no query uses a 3D point twice however many database images show it;
3. the kept correspondences stay in match order, which groups them by query;
4. the poses are ``ops.estimate_absolute_poses`` (P3P RANSAC + refit) over all queries at once.

Everything before the estimator is integer and order-defined: the host routine ``loftr_model_lookup_host`` defines the result (a CPU
model runs it, and ``evaluation.estimate_absolute_pose_native`` per query), the HIP kernels reproduce it bit for bit (a GPU model runs
them).  Devices are never mixed and there is no silent fallback either way.  Score the poses with ``evaluation.absolute_pose_error``
and ``evaluation.localization_recall``.
"""
import numpy as np
import torch

from . import ops
from ._lib import LoftrHipError
from .atlas import _KEYS, _grid


def _status_error(what, status, where=""):
    for bit, text in ops.MODEL_STATUS:
        if status & bit:
            raise ValueError(f"{what}: {text}{where}")


class LocalizationModel:
    """The 2D-3D table of a triangulated atlas in the form the lookup searches (tensors on one device; a CPU model runs the host routines).

    ``kp_offsets [n_images+1] i64`` delimits the images in ``keypoints [K,2] f32``; ``kp_point [K] i32`` is the row of ``xyz [P,3] f32`` of
    every keypoint or -1; ``image_hw`` / ``cell_px`` are the atlas's.  The constructor computes ``kp_cell [K] i32`` (the atlas cell of every
    keypoint) and checks, with one readback, that cells ascend strictly within an image (as the atlas orders its keypoints) and that
    ``kp_point`` stays in [-1, P)."""

    def __init__(self, kp_offsets, keypoints, kp_point, xyz, image_hw, cell_px):
        t = [torch.as_tensor(x).detach() for x in (kp_offsets, keypoints, kp_point, xyz)]
        names = ("kp_offsets", "keypoints", "kp_point", "xyz")
        devs = {x.device for x in t}
        if len(devs) != 1:
            raise LoftrHipError("LocalizationModel: arguments on different devices (" + ", ".join(f"{n}: {x.device}" for n, x in zip(names, t))
                                + "); there is no silent fallback: move them to one device")
        self.device = t[0].device
        if self.device.type not in ("cpu", "cuda"):
            raise LoftrHipError(f"LocalizationModel: device must be a GPU or the CPU (the host routine), got {self.device}")
        for n, x in zip(names[::2], t[::2]):
            if x.dtype.is_floating_point or x.dtype == torch.bool:
                raise ValueError(f"LocalizationModel: {n} must hold integers, got {x.dtype}")
        K, P = t[1].shape[0], t[3].shape[0]
        if t[0].dim() != 1 or t[0].numel() < 2 or tuple(t[1].shape) != (K, 2) or tuple(t[2].shape) != (K,) or tuple(t[3].shape) != (P, 3):
            raise ValueError(f"LocalizationModel: expected kp_offsets [n_images+1], keypoints [K,2], kp_point [K] and xyz [P,3], got "
                             f"{[tuple(x.shape) for x in t]}")
        self.image_hw = (float(image_hw[0]), float(image_hw[1]))
        self.cell_px = float(cell_px)
        self.inv, self.gh, self.gw = _grid(image_hw, cell_px)
        if self.gh * self.gw >= 2 ** 31 or K >= 2 ** 31 or P >= 2 ** 31:
            raise ValueError(f"LocalizationModel: {self.gh} x {self.gw} cells, {K} keypoints or {P} points are beyond the supported 2^31")
        self.kp_offsets = t[0].to(torch.int64).contiguous()
        self.keypoints = t[1].to(torch.float32).contiguous()
        self.kp_point = t[2].to(torch.int32).contiguous()
        self.xyz = t[3].to(torch.float32).contiguous()
        self.n_images, self.n_keypoints, self.n_points = self.kp_offsets.numel() - 1, K, P
        off = self.kp_offsets.cpu().numpy()                              # n_images + 1 numbers, once per model
        if off[0] != 0 or off[-1] != K or (np.diff(off) < 0).any():
            raise ValueError("LocalizationModel: kp_offsets must start at 0, end at the number of keypoints and ascend")
        if self.device.type == "cpu":
            cell, status = ops.model_cells_host(off, self.keypoints.numpy(), self.kp_point.numpy(), P, self.gh, self.gw, self.inv)
            self.kp_cell = torch.from_numpy(cell)
        else:
            self.kp_cell, status = ops.model_cells(self.kp_offsets, self.keypoints, self.kp_point, P, self.gh, self.gw, self.inv)
            status = int(status.cpu())                                   # the model's one readback
        _status_error("LocalizationModel", status)

    @classmethod
    def from_atlas(cls, sfm, pts):
        """The model of an atlas ``sfm`` (``KeypointAtlas.finalize``) and the points ``pts = sfm.triangulate(...)``: ``kp_point`` is the
        track's index at the inlier keypoints of valid tracks -- exactly where ``pts.keypoint_xyz(sfm)`` says ``has`` -- and -1 elsewhere."""
        if getattr(sfm, "image_hw", None) is None or getattr(sfm, "cell_px", None) is None:
            raise ValueError("LocalizationModel.from_atlas: this SfmResult carries no grid geometry (image_hw, cell_px); KeypointAtlas.finalize "
                             "sets them -- or call LocalizationModel(kp_offsets, keypoints, kp_point, xyz, image_hw, cell_px)")
        if pts.offsets is None:
            raise ValueError("LocalizationModel.from_atlas: these points carry no tracks (use SfmResult.triangulate)")
        dev = pts.xyz.device
        if sfm.keypoints.device != dev:
            raise LoftrHipError(f"LocalizationModel.from_atlas: the atlas on {sfm.keypoints.device}, the points on {dev}")
        T = pts.status.numel()
        track = torch.repeat_interleave(torch.arange(T, device=dev), pts.offsets[1:] - pts.offsets[:-1])
        sel = pts.obs_inlier & pts.valid[track]
        kp_point = torch.full((sfm.keypoints.shape[0],), -1, dtype=torch.int32, device=dev)
        kp_point[(sfm.kp_offsets[pts.image] + pts.keypoint)[sel]] = track[sel].to(torch.int32)   # a keypoint belongs to one track
        return cls(sfm.kp_offsets, sfm.keypoints, kp_point, pts.xyz, sfm.image_hw, sfm.cell_px)

    def propose_for_poses(self, K_db, T_db, K_query, T_query_prior, query_hw, top_k=10, **kw):
        """The database images to match each query against, chosen from a pose prior of the query by projected-point overlap
        (``proposals.propose_for_poses``) -> ``(ids [Q,top_k] i64, score [Q,top_k] i64)``, padded with -1."""
        from .proposals import propose_for_poses
        return propose_for_poses(self, K_db, T_db, K_query, T_query_prior, query_hw, top_k=top_k, **kw)


class QueryPoses:
    """What ``QueryLocalizer.solve`` returns (tensors on the model's device).

    Per query: ``R [Q,3,3] f32``, ``t [Q,3] f32`` (x_query = R X + t; zero without a model), ``n_inliers [Q] i64`` (-1: no model),
    ``n_corr [Q] i64``, ``q_offsets [Q+1] i64`` into the C correspondences ``pts3d [C,3] f32``, ``kpts [C,2] f32``, ``q_ids [C] i64``,
    ``match [C] i32`` (index into the matches in arrival order), ``point [C] i32`` (row of the model's xyz), ``conf [C] f32``,
    ``inliers [C] bool``.  Per match: ``match_reason [M] u8`` (``ops.MODEL_REASONS``: 0 kept, 2 masked, 3 non-finite, 4 negative
    confidence, 5 outside the grid, 6 no keypoint, 7 no 3D point, 8 fused), ``match_inlier [M] bool``.  ``stats``: dict of counts."""

    FIELDS = ("R", "t", "n_inliers", "n_corr", "q_offsets", "pts3d", "kpts", "q_ids", "match", "point", "conf", "inliers", "match_reason",
              "match_inlier")

    def __init__(self, stats, **tensors):
        self.stats = stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])

    def to_host(self):
        """dict of numpy arrays (plus 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out["stats"] = dict(self.stats)
        return out


class QueryLocalizer:
    """Accumulates the matches of ``n_queries`` query images against database images of ``model`` (``add``) and localises them
    (``solve``); see the module docstring.  Every tensor handed to it lives on the model's device."""

    def __init__(self, model, n_queries):
        if not isinstance(model, LocalizationModel):
            raise ValueError(f"QueryLocalizer: model must be a LocalizationModel, got {type(model).__name__}")
        self.model = model
        self.n_queries = int(n_queries)
        if not 0 <= self.n_queries < 2 ** 31:
            raise ValueError(f"QueryLocalizer: n_queries must lie in [0, 2^31), got {n_queries}")
        self.n_rows = 0
        self.n_matches = 0
        self._chunks, self._row_db, self._row_query = [], [], []
        self._last_query = 0

    def add(self, query_ids, db_image_ids, data, db_side=1, mask=None):
        """Add the matches of ``n`` rows.  ``query_ids`` [n]: the query of every row, in [0, n_queries), never descending, over all
        calls too (the rows of a query are contiguous, and may span calls); ``db_image_ids`` [n]: its database image, in [0, n_images);
        ``data``: the dict that ``forward`` / ``match_pairs`` leaves for the rows (``mkpts0_f``, ``mkpts1_f``, ``mconf``, ``m_bids`` in
        [0, n), ascending); ``db_side``: which image of the pair is the database image (0 or 1, for the whole call); ``mask`` [M] bool:
        matches to use (e.g. ``data['inliers']`` of ``verify_matches``).  The tensors are kept by reference and nothing here waits for
        the device: ``m_bids`` that live there are checked by the kernel and reported by ``solve``."""
        if db_side not in (0, 1):
            raise ValueError(f"QueryLocalizer.add: db_side must be 0 or 1, got {db_side!r}")
        ids = [np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x) for x in (query_ids, db_image_ids)]
        ids = [a.astype(np.int64) if a.size == 0 else a for a in ids]          # (an empty list has no integer dtype of its own)
        for name, a in zip(("query_ids", "db_image_ids"), ids):
            if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"QueryLocalizer.add: {name} must be an integer array [n], got {a.shape} {a.dtype}")
        q, d = ids
        n = q.shape[0]
        if d.shape[0] != n:
            raise ValueError(f"QueryLocalizer.add: {n} query ids but {d.shape[0]} database image ids")
        if n and (q.min() < 0 or q.max() >= self.n_queries):
            raise ValueError(f"QueryLocalizer.add: query ids outside [0, {self.n_queries}): {q[(q < 0) | (q >= self.n_queries)][:8].tolist()}")
        if n and (d.min() < 0 or d.max() >= self.model.n_images):
            raise ValueError(f"QueryLocalizer.add: database image ids outside [0, {self.model.n_images}): "
                             f"{d[(d < 0) | (d >= self.model.n_images)][:8].tolist()}")
        if n and ((np.diff(q) < 0).any() or q[0] < self._last_query):
            raise ValueError("QueryLocalizer.add: query ids must not descend, within a call and from one call to the next (the rows of a query "
                             "are contiguous)")
        missing = [k for k in _KEYS if k not in data]
        if missing:
            raise ValueError(f"QueryLocalizer.add: data lacks {missing} (pass the dict that forward / match_pairs leaves)")
        t = [torch.as_tensor(data[k]).detach() for k in _KEYS]
        M = t[0].shape[0]
        if tuple(t[0].shape) != (M, 2) or tuple(t[1].shape) != (M, 2) or tuple(t[2].shape) != (M,) or tuple(t[3].shape) != (M,):
            raise ValueError(f"QueryLocalizer.add: expected mkpts0_f / mkpts1_f [M,2], mconf / m_bids [M], got {[tuple(x.shape) for x in t]}")
        if t[3].dtype.is_floating_point or t[3].dtype == torch.bool:
            raise ValueError(f"QueryLocalizer.add: m_bids must be integers, got {t[3].dtype}")
        if mask is not None:
            mask = torch.as_tensor(mask).detach()
            if tuple(mask.shape) != (M,) or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"QueryLocalizer.add: mask must be bool [{M}], got {tuple(mask.shape)} {mask.dtype}")
        for name, x in zip(_KEYS + ("mask",), t + [mask]):
            if x is not None and x.device != self.model.device:
                raise LoftrHipError(f"QueryLocalizer.add: {name} on {x.device}, the model on {self.model.device}; there is no silent fallback: "
                                    "move them to one device")
        if M and n == 0:
            raise ValueError(f"QueryLocalizer.add: {M} matches but no row")
        if self.n_matches + M > 2 ** 31 - 2 or self.n_rows + n >= 2 ** 31:
            raise ValueError("QueryLocalizer.add: more than 2^31 - 2 matches or 2^31 - 1 rows")
        bids = t[3].to(torch.int64)
        if M and not bids.is_cuda:                                       # host ids: checked here; device ids: by the kernel, reported by solve
            b = bids.numpy()
            if b.min() < 0 or b.max() >= n:
                raise ValueError(f"QueryLocalizer.add: m_bids outside [0, {n})")
            if (np.diff(b) < 0).any():
                raise ValueError("QueryLocalizer.add: m_bids must ascend (matches grouped by row, as the matcher emits them)")
        # global rows; an id outside [0, n) becomes -1, which the lookup reports (elementwise and stream-ordered: no wait)
        rows = torch.where((bids >= 0) & (bids < n), bids + self.n_rows, torch.full_like(bids, -1)).to(torch.int32)
        self._chunks.append((t[db_side].to(torch.float32), t[1 - db_side].to(torch.float32), t[2].to(torch.float32), rows,
                             None if mask is None else mask.to(torch.uint8)))
        self._row_query.append(q.astype(np.int32))
        self._row_db.append(d.astype(np.int32))
        if n:
            self._last_query = int(q[-1])
        self.n_rows += n
        self.n_matches += M

    def correspondences(self, timings=None):
        """The lookup and the fusion without the poses -> (dict of trimmed tensors: pts3d, kpts, q_ids, match, point, conf, q_offsets,
        match_reason; stats).  One readback of the 16 counts; bad ``m_bids`` found on the device raise ValueError here."""
        m, dev = self.model, self.model.device
        M = self.n_matches
        cat = lambda i, shape, dt: torch.cat([c[i] for c in self._chunks]) if self._chunks else torch.zeros(shape, dtype=dt, device=dev)
        kd, kq, c, rows = cat(0, (0, 2), torch.float32), cat(1, (0, 2), torch.float32), cat(2, (0,), torch.float32), cat(3, (0,), torch.int32)
        mask = None
        if any(ch[4] is not None for ch in self._chunks):
            mask = torch.cat([torch.ones(ch[0].shape[0], dtype=torch.uint8, device=dev) if ch[4] is None else ch[4] for ch in self._chunks])
        row_db = np.concatenate(self._row_db) if self._row_db else np.zeros(0, np.int32)
        row_query = np.concatenate(self._row_query) if self._row_query else np.zeros(0, np.int32)
        if dev.type == "cpu":
            np_ = lambda x: None if x is None else x.numpy()
            out = ops.model_lookup_host(np_(m.kp_offsets), np_(m.kp_cell), np_(m.kp_point), np_(m.xyz), m.gh, m.gw, m.inv, np_(kd), np_(kq),
                                        np_(c), np_(rows), np_(mask), row_db, row_query, self.n_queries)
            out = {k: torch.from_numpy(v) for k, v in out.items()}
        else:
            with torch.cuda.device(dev):
                rd, rq = (torch.from_numpy(a).to(dev, non_blocking=True) for a in (row_db, row_query))
            out = ops.model_lookup(m.kp_offsets, m.kp_cell, m.kp_point, m.xyz, m.gh, m.gw, m.inv, kd, kq, c, rows, mask, rd, rq,
                                   self.n_queries, timings=timings)
        counts = out.pop("counts").cpu().tolist()                        # the one readback
        _status_error("QueryLocalizer", counts[3], " (found on the device)" if dev.type == "cuda" else "")
        C = counts[0]
        stats = {"n_queries": self.n_queries, "n_rows": self.n_rows, "n_matches": M, "n_correspondences": C}
        stats.update({name: counts[4 + i] for i, name in enumerate(ops.MODEL_REASONS) if name != "n_bad_row"})
        for k in ("pts3d", "kpts", "q_ids", "match", "point", "conf"):
            out[k] = out[k][:C]
        return out, stats

    def solve(self, K_query, thresh_px=3.0, conf=0.999, seed=0, timings=None, radial=None):
        """Localise every query -> ``QueryPoses``.  ``K_query`` [n_queries,3,3]: the queries' intrinsics (an array, or a tensor on the
        model's device).  The lookup, one readback of its counts, then ONE estimator call for all queries (``ops.estimate_absolute_poses``
        on a GPU model, a loop over ``evaluation.estimate_absolute_pose_native`` on a CPU model: the same result for one seed), whose
        inlier bits are scattered back to match order.  timings: a list that receives (stage, ms) pairs of the GPU lookup stages.
        ``radial`` [n_queries]: the radial coefficients of the queries' lenses; the query-side pixels are undistorted
        (``undistort_points``) before the estimator call, and a correspondence whose pixel cannot be is left out (``kpts`` of the result
        are then the undistorted pixels, and ``stats['n_not_undistorted']`` counts what was left out)."""
        dev, Q = self.model.device, self.n_queries
        if isinstance(K_query, torch.Tensor) and K_query.device != dev:
            raise LoftrHipError(f"QueryLocalizer.solve: K_query on {K_query.device}, the model on {dev}; there is no silent fallback")
        Kq = torch.as_tensor(K_query).detach().to(dev, torch.float32).contiguous()
        if tuple(Kq.shape) != (Q, 3, 3):
            raise ValueError(f"QueryLocalizer.solve: expected K_query [{Q},3,3], got {tuple(Kq.shape)}")
        out, stats = self.correspondences(timings=timings)
        C, M = stats["n_correspondences"], self.n_matches
        if radial is not None:
            from .radial import undistort_points
            if isinstance(radial, torch.Tensor) and radial.device != dev:
                raise LoftrHipError(f"QueryLocalizer.solve: radial on {radial.device}, the model on {dev}; there is no silent fallback")
            rad = torch.as_tensor(radial).detach().to(dev, torch.float64)
            if tuple(rad.shape) != (Q,):
                raise ValueError(f"QueryLocalizer.solve: expected radial [{Q}], got {tuple(rad.shape)}")
            K64 = torch.as_tensor(K_query).detach().to(dev, torch.float64)
            xy, ok = undistort_points(out["kpts"], out["q_ids"].to(torch.int32), K64, rad)
            for k in ("pts3d", "q_ids", "match", "point", "conf"):
                out[k] = out[k][ok].contiguous()
            out["kpts"] = xy[ok].contiguous()
            out["q_offsets"] = torch.zeros_like(out["q_offsets"])
            out["q_offsets"][1:] = torch.cumsum(torch.bincount(out["q_ids"].to(torch.int64), minlength=Q), 0)
            stats["n_not_undistorted"], C = C - int(out["q_ids"].numel()), int(out["q_ids"].numel())
            stats["n_correspondences"] = C
        if dev.type == "cuda":
            R, t, inl, n = ops.estimate_absolute_poses(out["pts3d"], out["kpts"], out["q_ids"], Kq, thresh_px, conf, seed)
        else:
            from .evaluation import estimate_absolute_pose_native
            R, t = torch.zeros(Q, 3, 3), torch.zeros(Q, 3)
            inl, n = torch.zeros(C, dtype=torch.bool), torch.full((Q,), -1, dtype=torch.int64)
            off = out["q_offsets"].tolist()
            for q in range(Q):
                sl = slice(off[q], off[q + 1])
                est = estimate_absolute_pose_native(out["pts3d"][sl].numpy(), out["kpts"][sl].numpy(), Kq[q].numpy(), thresh_px, conf, seed)
                if est is not None:
                    R[q], t[q] = torch.from_numpy(est[0]).float(), torch.from_numpy(est[1]).float()
                    inl[sl] = torch.from_numpy(est[2])
                    n[q] = int(est[2].sum())
        match_inlier = torch.zeros(M, dtype=torch.bool, device=dev)
        match_inlier[out["match"].to(torch.int64)] = inl                 # a match is kept once: no two writes meet
        return QueryPoses(stats, R=R, t=t, n_inliers=n, n_corr=out["q_offsets"][1:] - out["q_offsets"][:-1], inliers=inl,
                          match_inlier=match_inlier, **out)
