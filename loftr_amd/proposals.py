"""Pair proposals from the model: which image pairs are worth matching, by projected-point overlap, on the device.

Every stage after matching runs from a pair list that somebody else made.  Once a model exists, geometry proposes the pairs: two
images are worth matching when the points one of them observes project into the other within a viewing-angle and scale change LoFTR
can bridge (what hloc ships as ``pairs_from_covisibility`` / ``pairs_from_poses``)::

    rec = sfm.reconstruct(K)                                        # from a sparse pair list
    pairs, score = rec.propose_pairs(sfm, top_k=5, min_shared=30)   # [P,2] i64 (a < b): overlapping pairs that were never matched
    # match them, atlas.add(...), reconstruct again

    model = LocalizationModel.from_atlas(sfm, rec.points)
    db, score = model.propose_for_poses(K_db, T_db, K_query, T_query_prior, query_hw, top_k=10)    # [Q,top_k] i64, -1 padded

The rule (include/loftr_hip.h) is a per-point predicate in fp64 with a fixed operation order and an integer count: the host
routine ``loftr_view_overlap_host`` defines it (CPU tensors run it), the HIP kernels reproduce it exactly (GPU tensors run them; there is
no silent fallback either way).  The selection is integer work on keys without ties, so both sides select the same set.
"""
import math

import torch

from . import _tracks, ops
from ._lib import LoftrHipError

_ARGS = ("vis_offsets", "vis_point", "xyz", "point_ok", "K_src", "T_src", "src_ok", "K_tgt", "T_tgt", "tgt_ok", "tgt_hw")


class Overlap:
    """What ``view_overlap`` returns (tensors on the device of the input): ``overlap [n,m] i32`` (the points source image ``i`` observes
    that count for target view ``j``), ``n_vis [n] i32`` (the usable entries of each source's list), ``stats``: the counts by name
    (``ops.OVERLAP_NAMES`` less the error bits) plus the parameters."""

    FIELDS = ("overlap", "n_vis")

    def __init__(self, stats, **tensors):
        self.stats = stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])

    def to_host(self):
        """dict of numpy arrays (plus 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out["stats"] = dict(self.stats)
        return out


def view_overlap(vis_offsets, vis_point, xyz, point_ok, K_src, T_src, src_ok, K_tgt, T_tgt, tgt_ok, tgt_hw, max_angle_deg=45.0,
                 max_scale=2.0, border_px=0.0, timings=None):
    """Count, for every (source image, target view), the points the source observes that the target would see too -> ``Overlap``.

    ``vis_offsets [n+1]`` over ``vis_point [V]``: the point ids each source image observes; ``xyz [T,3]``, ``point_ok [T]``; ``K_src
    [n,3,3]``, ``T_src [n,4,4]`` (camera from world), ``src_ok [n]``; the ``m`` target views ``K_tgt``, ``T_tgt``, ``tgt_ok`` and
    ``tgt_hw [m,2]`` (H, W).  All tensors on one device: CPU tensors run the defining host routine, GPU tensors the kernels.

    A point counts when it lies in front of the target and inside its image less ``border_px``, the angle at the point between the two
    camera centres is at most ``max_angle_deg``, and the ratio of the apparent sizes focal / distance lies within ``max_scale`` either
    way (``inf``: no scale test).  The cosine is computed once here and handed to both sides as the same double.  One readback; a bad
    list raises ValueError.  timings: a list that receives (stage, ms) pairs of the GPU stages."""
    what = "view_overlap"
    args = [torch.as_tensor(a).detach() for a in (vis_offsets, vis_point, xyz, point_ok, K_src, T_src, src_ok, K_tgt, T_tgt, tgt_ok, tgt_hw)]
    _tracks.one_device(what, _ARGS, args)
    for name, a in zip(_ARGS[:2], args[:2]):
        _tracks.integers(what, name, a)
    max_angle_deg, max_scale, border_px = float(max_angle_deg), float(max_scale), float(border_px)
    if not 0.0 <= max_angle_deg <= 180.0:
        raise ValueError(f"{what}: max_angle_deg must lie in [0, 180], got {max_angle_deg}")
    if not max_scale >= 1.0:
        raise ValueError(f"{what}: max_scale must be >= 1 (inf disables the scale test), got {max_scale}")
    if not 0.0 <= border_px < math.inf:
        raise ValueError(f"{what}: border_px must be finite and >= 0, got {border_px}")
    n, m = args[6].shape[0] if args[6].dim() == 1 else -1, args[9].shape[0] if args[9].dim() == 1 else -1
    shapes = ((n, 3, 3), (n, 4, 4), (m, 3, 3), (m, 4, 4))
    if n < 0 or m < 0 or any(tuple(args[i].shape) not in (s, (s[0], s[1] * s[2])) for i, s in zip((4, 5, 7, 8), shapes)) or \
            tuple(args[10].shape) != (m, 2) or args[2].dim() != 2 or args[2].shape[1] != 3:
        raise ValueError(f"{what}: expected K_src [n,3,3], T_src [n,4,4], src_ok [n], K_tgt [m,3,3], T_tgt [m,4,4], tgt_ok [m], tgt_hw [m,2] "
                         f"and xyz [T,3], got {[tuple(a.shape) for a in args[2:]]}")
    if n * m > 2 ** 31:
        raise ValueError(f"{what}: {n} x {m} pairs are beyond the supported 2^31 entries (there is no sparse output)")
    flag = lambda a: (a != 0).to(torch.uint8)
    f64 = lambda a, w: a.to(torch.float64).reshape(a.shape[0], w)
    cos_min = math.cos(math.radians(max_angle_deg))
    out = ops.view_overlap(args[0].to(torch.int64), args[1].to(torch.int32), args[2].to(torch.float32), flag(args[3]), f64(args[4], 9),
                           f64(args[5], 16), flag(args[6]), f64(args[7], 9), f64(args[8], 16), flag(args[9]), f64(args[10], 2), border_px,
                           cos_min, max_scale * max_scale, timings=timings)
    word = out["counts"].cpu().tolist()                                                  # the one readback
    _tracks.raise_error_bits(what, word[1], ops.OVERLAP_ERRORS)
    stats = {name: word[i] for i, name in enumerate(ops.OVERLAP_NAMES) if name != "error_bits"}
    stats.update(n_images=n, n_views=m, max_angle_deg=max_angle_deg, max_scale=max_scale, border_px=border_px)
    return Overlap(stats, overlap=out["overlap"], n_vis=out["n_vis"])


def _table(what, overlap):
    o = overlap.overlap if isinstance(overlap, Overlap) else torch.as_tensor(overlap)
    if o.dim() != 2 or o.dtype.is_floating_point or o.dtype == torch.bool:
        raise ValueError(f"{what}: overlap must be an integer table [n,m], got {o.dtype} {tuple(o.shape)}")
    return o.detach().to(torch.int64)


def _count(what, name, v, lo):
    if not isinstance(v, int) or isinstance(v, bool) or v < lo:
        raise ValueError(f"{what}: {name} must be an integer >= {lo}, got {v}")
    return v


def _top(score, keep, top_k):
    """Per row of ``score [r,c]`` the ``top_k`` columns among ``keep`` by (score descending, column ascending) -> (columns [r,k] i64,
    -1 where there are fewer; their scores, 0 there).  The key score * c + (c - 1 - column) has no ties, so the choice does not depend
    on how topk breaks them."""
    r, c = score.shape
    k = min(top_k, c)
    if r == 0 or k == 0:
        return (torch.full((r, top_k), -1, dtype=torch.int64, device=score.device),
                torch.zeros((r, top_k), dtype=torch.int64, device=score.device))
    col = torch.arange(c, device=score.device)
    key = torch.where(keep, score * c + (c - 1 - col), torch.full_like(score, -1))
    best = torch.topk(key, k, dim=1).values
    found = best >= 0
    cols = torch.where(found, (c - 1) - best % c, torch.full_like(best, -1))
    vals = torch.where(found, torch.div(best, c, rounding_mode="floor"), torch.zeros_like(best))
    if k < top_k:
        pad = (r, top_k - k)
        cols = torch.cat([cols, torch.full(pad, -1, dtype=torch.int64, device=score.device)], 1)
        vals = torch.cat([vals, torch.zeros(pad, dtype=torch.int64, device=score.device)], 1)
    return cols, vals


def select_pairs(overlap, existing=None, top_k=5, min_shared=30):
    """Image pairs to match from a square overlap table (sources = targets) -> ``(pairs [P,2] i64, score [P] i64)``.

    The score of a pair is ``min(overlap[i,j], overlap[j,i])``.  ``i == j``, the pairs in ``existing [E,2]`` (in either order) and
    scores below ``min_shared`` are dropped; every image keeps its ``top_k`` partners by (score descending, partner ascending); the
    result is the union over the images, each pair once with ``a < b``, ascending by ``(a, b)``.  Integer work without ties: a CPU
    table and its GPU copy select the same set."""
    what = "select_pairs"
    o = _table(what, overlap)
    n = o.shape[0]
    if o.shape[1] != n:
        raise ValueError(f"{what}: overlap must be square (the sources are the targets), got {tuple(o.shape)}; see select_database")
    top_k, min_shared = _count(what, "top_k", top_k, 1), _count(what, "min_shared", min_shared, 0)
    score = torch.minimum(o, o.t())
    keep = (score >= min_shared) & ~torch.eye(n, dtype=torch.bool, device=o.device)
    if existing is not None:
        ex = torch.as_tensor(existing).detach()
        if ex.dim() != 2 or ex.shape[1] != 2 or ex.dtype.is_floating_point or ex.dtype == torch.bool:
            raise ValueError(f"{what}: existing must be an integer table [E,2], got {ex.dtype} {tuple(ex.shape)}")
        if ex.device != o.device:
            raise LoftrHipError(f"{what}: overlap on {o.device}, existing on {ex.device}; there is no silent fallback: move them to one device")
        ex = ex.to(torch.int64)
        ex = ex[((ex >= 0) & (ex < n)).all(1)]
        keep[ex[:, 0], ex[:, 1]] = False
        keep[ex[:, 1], ex[:, 0]] = False
    cols, _ = _top(score, keep, top_k)
    rows = torch.arange(n, device=o.device).unsqueeze(1).expand_as(cols)
    found = cols >= 0
    i, j = rows[found], cols[found]
    code = torch.unique(torch.minimum(i, j) * n + torch.maximum(i, j))                   # (sorted: ascending by (a, b))
    a, b = torch.div(code, max(n, 1), rounding_mode="floor"), code % max(n, 1)
    return torch.stack([a, b], 1), score[a, b]


def select_database(overlap, top_k=10, min_shared=30):
    """For every target view (query) of an overlap table ``[n,m]`` the source images (database) to match it against ->
    ``(ids [m,top_k] i64, score [m,top_k] i64)``: the ``top_k`` sources by (``overlap[i,j]`` descending, ``i`` ascending) among those
    with at least ``min_shared``; -1 (score 0) where there are fewer."""
    what = "select_database"
    o = _table(what, overlap)
    top_k, min_shared = _count(what, "top_k", top_k, 1), _count(what, "min_shared", min_shared, 0)
    score = o.t().contiguous()
    return _top(score, score >= min_shared, top_k)


def propose_pairs(rec, sfm, top_k=5, min_shared=30, **kw):
    """``Reconstruction.propose_pairs``: the unmatched image pairs of a reconstruction that overlap -> ``(pairs [P,2] i64, score [P])``.

    Sources and targets are the posed images of ``rec``; an image's visibility list holds the points of ``rec.points`` (status ok) that
    it observes as an inlier; ``existing`` is ``sfm.row_images`` and the image extents are ``sfm.image_hw``.  ``kw`` goes to
    ``view_overlap`` (``max_angle_deg``, ``max_scale``, ``border_px``, ``timings``)."""
    what = "propose_pairs"
    pts = rec.points
    if pts is None or pts.offsets is None or pts.image is None:
        raise ValueError(f"{what}: this reconstruction's points carry no tracks (use SfmResult.reconstruct)")
    if getattr(sfm, "image_hw", None) is None:
        raise ValueError(f"{what}: this SfmResult carries no image extents (image_hw is set by KeypointAtlas.finalize)")
    if rec.K is None:
        raise ValueError(f"{what}: this reconstruction carries no intrinsics (K)")
    dev = pts.xyz.device
    n, T = rec.posed.shape[0], pts.status.numel()
    track = torch.repeat_interleave(torch.arange(T, device=dev), pts.offsets[1:] - pts.offsets[:-1])
    sel = (pts.obs_inlier != 0) & pts.valid[track]
    image, point = pts.image[sel].to(torch.int32), track[sel].to(torch.int32)
    vis_offsets, order = _tracks.group_by_image(image, n)
    posed = rec.posed != 0
    hw = torch.tensor([float(sfm.image_hw[0]), float(sfm.image_hw[1])], dtype=torch.float64, device=dev).expand(n, 2)
    K, Tc = rec.K.to(dev), rec.T_cam_from_world.to(dev)
    ov = view_overlap(vis_offsets, point[order.to(torch.int64)], pts.xyz, pts.valid, K, Tc, posed, K, Tc, posed, hw, **kw)
    return select_pairs(ov, existing=sfm.row_images.to(dev), top_k=top_k, min_shared=min_shared)


def propose_for_poses(model, K_db, T_db, K_query, T_query_prior, query_hw, top_k=10, min_shared=30, **kw):
    """``LocalizationModel.propose_for_poses``: the database images to match each query against, from a pose prior (GPS plus compass,
    the previous frame of a sequence) -> ``(ids [Q,top_k] i64, score [Q,top_k] i64)``, -1 padded.

    ``K_db [n,3,3]`` / ``T_db [n,4,4]``: the database cameras of the model's images; ``K_query [Q,3,3]``, ``T_query_prior [Q,4,4]``,
    ``query_hw`` ((H, W) or ``[Q,2]``).  A database image's visibility list holds the 3D points of its keypoints (``kp_point >= 0``).
    ``kw`` goes to ``view_overlap``."""
    what = "propose_for_poses"
    dev = model.device
    t = [torch.as_tensor(a).detach() for a in (K_db, T_db, K_query, T_query_prior)]
    for name, a in zip(("K_db", "T_db", "K_query", "T_query_prior"), t):
        if a.device != dev:
            raise LoftrHipError(f"{what}: the model on {dev}, {name} on {a.device}; there is no silent fallback: move them to one device")
    n, Q = model.n_images, t[2].shape[0]
    if t[0].shape[0] != n:
        raise ValueError(f"{what}: K_db holds {t[0].shape[0]} cameras, the model {n} images")
    hw = torch.as_tensor(query_hw, dtype=torch.float64).to(dev)
    hw = hw.expand(Q, 2) if hw.dim() == 1 else hw
    has = model.kp_point >= 0
    before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(has.to(torch.int64), 0)])
    ones = lambda k: torch.ones(k, dtype=torch.uint8, device=dev)
    ov = view_overlap(before[model.kp_offsets], model.kp_point[has], model.xyz, ones(model.n_points), t[0], t[1], ones(n), t[2], t[3],
                      ones(Q), hw, **kw)
    return select_database(ov, top_k=top_k, min_shared=min_shared)
