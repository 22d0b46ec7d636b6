"""Track refinement: every observation of a track re-localised against one reference view with the matcher's fine level.

LoFTR has no detector: the atlas (atlas.py) snaps matched points to ``cell_px`` cells and keeps, per cell, the position of
its most confident observation.  Two rows that hit one cell matched two different physical points up to a cell apart, and the track that
links them claims that one 3D point projects onto both.  No later stage can remove that error.  The repair of detector-free SfM is a
pass after the coarse model: each track picks a reference view, every other observation is matched again against it with the fine
level, and all observations of the track then refer to one physical point::

    view, ref = sfm.refine_tracks(model, load, obs_mask=pts.obs_inlier, max_std=0.5, max_shift_px=4.0)
    pts = view.triangulate(K, T)                             # then adjust -> triangulate on the view, as on any result
    ref.kp_state, ref.kp_shift_px, ref.stats                 # what happened to every keypoint

``plan_track_refinement`` chooses references and orders the jobs, ``pairs.refine_pair_list`` runs them from feature banks
(``LoFTR.refine_points``), ``apply_refinement`` writes the accepted positions.  Planning and applying are integer and fp32 tensor work
with sorts on unique integer keys: the CPU and the GPU give the same result.

Not modelled: sub-pixel window centres (the reference moves to the fine grid instead, at most s/2 per axis), a multi-view transformer
over all views of a track, refinement inside ``reconstruct``, completion / merging / splitting on refined keypoints.
"""
import torch

STATE_NONE, STATE_REF_MOVED, STATE_QUERY_ACCEPTED, STATE_QUERY_REJECTED, STATE_REF_KEPT = range(5)
STATE_NAMES = ("n_untouched", "n_ref_moved", "n_query_accepted", "n_query_rejected", "n_ref_kept")


class RefinePlan:
    """What ``plan_track_refinement`` returns.

    ``pairs [P,2] i64`` (reference image, query image) and ``pair_offsets [P+1] i64``, host tensors: pair p holds the jobs
    ``pair_offsets[p] : pair_offsets[p+1]``; ``job_ref_kp [J] i64`` / ``job_query_kp [J] i64`` global keypoint indices and ``job_track [J]
    i64`` the track id of every job, on the result's device; ``stats``: n_tracks (tracks with a job), n_jobs, n_pairs, n_dropped_jobs,
    n_dropped_pairs."""

    FIELDS = ("pairs", "pair_offsets", "job_ref_kp", "job_query_kp", "job_track")

    def __init__(self, stats, **tensors):
        self.stats = stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])


class Refinement:
    """What ``SfmResult.refine_tracks`` / ``apply_refinement`` return beside the view.

    ``kp_state [K] i8``: 0 not in a job, 1 reference moved (to the fine-grid point the network matched against), 2 query accepted,
    3 query rejected, 4 reference kept (none of its jobs was accepted); ``kp_shift_px [K] f32``: how far the keypoint moved (0 where
    it kept its position); ``job_std [J] f32``: ``expec_f[:, 2]`` of every job; ``plan``: the RefinePlan; ``stats``: the counts per
    state (``STATE_NAMES``), ``mean_shift_px`` / ``max_shift_px`` over the accepted queries, and the plan's counts."""

    FIELDS = ("kp_state", "kp_shift_px", "job_std")

    def __init__(self, stats, plan, **tensors):
        self.stats, self.plan = stats, plan
        for k in self.FIELDS:
            setattr(self, k, tensors[k])


def _ordered_bits(x):
    """fp32 -> int64 in [0, 2^32) with the order of the floats (-0 below +0; NaNs at the ends)."""
    b = x.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(b < 0, -(b & 0x7FFFFFFF) - 1, b) + (1 << 31)


def plan_track_refinement(sfm, obs_mask=None, min_jobs_per_pair=1):
    """References and jobs of the refinement of ``sfm``'s tracks -> ``RefinePlan``.  The rules:

    1. only tracks with ``track_ok`` take part, read through ``sfm.tracks(consistent_only=True)``; ``obs_mask [N]`` (in that CSR order,
       e.g. ``pts.obs_inlier``) removes observations; a track left with fewer than two is skipped;
    2. the reference of a track is its remaining keypoint with the greatest ``score``, ties to the smallest global keypoint index;
    3. one job per other remaining keypoint: (reference image, query image, reference keypoint, query keypoint);
    4. jobs are ordered by (reference image, query image, query keypoint) -- a unique key, a keypoint lies in one track; the distinct
       (reference image, query image) in that order are the pair list; pairs with fewer than ``min_jobs_per_pair`` jobs are dropped
       with their jobs and counted."""
    if not isinstance(min_jobs_per_pair, int) or isinstance(min_jobs_per_pair, bool) or min_jobs_per_pair < 1:
        raise ValueError(f"plan_track_refinement: min_jobs_per_pair must be an integer >= 1, got {min_jobs_per_pair!r}")
    offsets, image, local = sfm.tracks(consistent_only=True)
    dev = image.device
    n_obs, n_tracks, n_kp = image.numel(), offsets.numel() - 1, sfm.keypoints.shape[0]
    n_images = sfm.kp_offsets.numel() - 1
    kp = sfm.kp_offsets[image] + local
    track = torch.repeat_interleave(torch.arange(n_tracks, device=dev), offsets[1:] - offsets[:-1])
    if obs_mask is None:
        keep = torch.ones(n_obs, dtype=torch.bool, device=dev)
    else:
        keep = torch.as_tensor(obs_mask).to(dev) != 0
        if tuple(keep.shape) != (n_obs,):
            raise ValueError(f"plan_track_refinement: obs_mask must be [{n_obs}] (the observations of tracks(consistent_only=True)), "
                             f"got {tuple(keep.shape)}")
    left = torch.bincount(track[keep], minlength=n_tracks)
    keep = keep & (left[track] >= 2)
    kp, track = kp[keep], track[keep]
    # rule 2 on one unique integer word per keypoint, (score bits in float order, 2^31 - 1 - keypoint): the greatest of its track
    word = (_ordered_bits(sfm.score[kp]) << 31) | ((1 << 31) - 1 - kp)
    by_word = torch.sort(word, descending=True).indices
    by_track = by_word[torch.sort(track[by_word], stable=True).indices]
    left = torch.bincount(track, minlength=n_tracks)
    ref_kp = torch.zeros(n_tracks, dtype=torch.int64, device=dev)
    ref_kp[left > 0] = kp[by_track][(torch.cumsum(left, 0) - left)[left > 0]]
    is_job = kp != ref_kp[track]
    q_kp, r_kp = kp[is_job], ref_kp[track[is_job]]
    kp_image = sfm.keypoint_image()
    r_im, q_im = kp_image[r_kp], kp_image[q_kp]
    # rule 4: keypoints are ordered by image, so (reference image, query keypoint) orders by the query image as well
    order = torch.sort(r_im * max(n_kp, 1) + q_kp, stable=True).indices
    q_kp, r_kp, r_im, q_im = q_kp[order], r_kp[order], r_im[order], q_im[order]
    pair_key, counts = torch.unique_consecutive(r_im * max(n_images, 1) + q_im, return_counts=True)
    good = counts >= min_jobs_per_pair
    job_good = torch.repeat_interleave(good, counts)
    q_kp, r_kp = q_kp[job_good], r_kp[job_good]
    pair_key, kept = pair_key[good], counts[good]
    job_track = sfm.track_id.to(torch.int64)[q_kp]
    P = int(pair_key.numel())
    key, kept_host = pair_key.cpu(), kept.cpu()                          # the scheduler needs the pair list on the host
    pairs = torch.stack([key // max(n_images, 1), key % max(n_images, 1)], 1).reshape(-1, 2)
    pair_offsets = torch.zeros(P + 1, dtype=torch.int64)
    pair_offsets[1:] = torch.cumsum(kept_host, 0)
    n_jobs = int(pair_offsets[-1])
    stats = dict(n_tracks=int(torch.unique(job_track).numel()), n_jobs=n_jobs, n_pairs=P, n_dropped_jobs=int(counts.sum()) - n_jobs,
                 n_dropped_pairs=int(good.numel()) - P, min_jobs_per_pair=min_jobs_per_pair)
    return RefinePlan(stats, pairs=pairs, pair_offsets=pair_offsets, job_ref_kp=r_kp, job_query_kp=q_kp, job_track=job_track)


def apply_refinement(sfm, plan, result, image_hw=None, max_std=None, max_shift_px=None):
    """Write the accepted positions of ``result`` (the outputs of ``LoFTR.refine_points`` for the jobs of ``plan``, in job order:
    ``pts0 [J,2]``, ``pts1 [J,2]``, ``expec_f [J,3]``, ``ok [J]``) -> ``(view, Refinement)``.

    A query keypoint takes ``pts1`` when its row is ok, ``pts1`` is finite and inside the image (0 <= x < W, 0 <= y < H),
    ``expec_f[:, 2] <= max_std`` and ``|pts1 - old position| <= max_shift_px`` (Euclidean; None: no limit); otherwise it keeps its
    position.  A reference keypoint takes ``pts0`` -- the point the network matched against -- when at least one of its jobs was
    accepted, otherwise it keeps its position.  Every keypoint has at most one writer: a keypoint lies in one track, is its reference
    or one of its queries, and the jobs of one reference carry the same ``pts0``.  ``view`` shares every tensor with ``sfm`` except
    ``keypoints`` and has ``is_refined = True``."""
    from .atlas import SfmResult
    image_hw = image_hw if image_hw is not None else sfm.image_hw
    if image_hw is None:
        raise ValueError("apply_refinement: image_hw is required (this result carries none)")
    dev = sfm.keypoints.device
    n_kp, J = sfm.keypoints.shape[0], plan.job_query_kp.numel()
    pts0, pts1, expec, ok = (result[k].to(dev) for k in ("pts0", "pts1", "expec_f", "ok"))
    if tuple(pts0.shape) != (J, 2) or tuple(pts1.shape) != (J, 2) or tuple(expec.shape) != (J, 3) or tuple(ok.shape) != (J,):
        raise ValueError(f"apply_refinement: expected the results of the plan's {J} jobs, got pts0 {tuple(pts0.shape)}, pts1 "
                         f"{tuple(pts1.shape)}, expec_f {tuple(expec.shape)}, ok {tuple(ok.shape)}")
    q_kp, r_kp = plan.job_query_kp, plan.job_ref_kp
    old = sfm.keypoints[q_kp]
    std = expec[:, 2].to(torch.float32)
    shift = torch.linalg.vector_norm(pts1 - old, dim=1)
    H, W = float(image_hw[0]), float(image_hw[1])
    accept = (ok != 0) & torch.isfinite(pts1).all(1) & (pts1[:, 0] >= 0) & (pts1[:, 0] < W) & (pts1[:, 1] >= 0) & (pts1[:, 1] < H)
    if max_std is not None:
        accept &= std <= float(max_std)
    if max_shift_px is not None:
        accept &= shift <= float(max_shift_px)
    keypoints = sfm.keypoints.clone()
    state = torch.zeros(n_kp, dtype=torch.int8, device=dev)
    moved = torch.zeros(n_kp, dtype=torch.float32, device=dev)
    state[r_kp] = STATE_REF_KEPT                                          # (equal values wherever two jobs write one reference)
    state[r_kp[accept]] = STATE_REF_MOVED
    state[q_kp] = torch.where(accept, STATE_QUERY_ACCEPTED, STATE_QUERY_REJECTED).to(torch.int8)
    keypoints[q_kp[accept]] = pts1[accept].to(torch.float32)
    moved[q_kp[accept]] = shift[accept]
    ref_new = pts0[accept].to(torch.float32)
    moved[r_kp[accept]] = torch.linalg.vector_norm(ref_new - sfm.keypoints[r_kp[accept]], dim=1)
    keypoints[r_kp[accept]] = ref_new
    n_acc = accept.sum()
    acc_shift = torch.where(accept, shift, torch.zeros_like(shift))
    word = torch.cat([torch.bincount(state.to(torch.int64), minlength=5).to(torch.float64),
                      torch.stack([n_acc.to(torch.float64), acc_shift.sum(dtype=torch.float64),
                                   acc_shift.max().to(torch.float64) if J else torch.zeros((), dtype=torch.float64, device=dev)])]).cpu().tolist()
    stats = dict(plan.stats)
    stats.update({name: int(word[i]) for i, name in enumerate(STATE_NAMES)})
    stats.update(mean_shift_px=word[6] / word[5] if word[5] else 0.0, max_shift_px=word[7], max_std=max_std, shift_limit_px=max_shift_px)
    fields = {k: getattr(sfm, k) for k in SfmResult.FIELDS}
    fields.update(keypoints=keypoints)
    view = SfmResult(dict(sfm.stats), **fields)
    view.image_hw, view.cell_px, view.is_undistorted, view.is_refined = sfm.image_hw, sfm.cell_px, sfm.is_undistorted, True
    return view, Refinement(stats, plan, kp_state=state, kp_shift_px=moved, job_std=std)


def refine_tracks(sfm, model, load, image_hw=None, obs_mask=None, max_std=None, max_shift_px=None, min_jobs_per_pair=1, **pair_list_kw):
    """SfmResult.refine_tracks (see there)."""
    from .pairs import refine_pair_list
    if sfm.is_undistorted:
        raise ValueError("SfmResult.refine_tracks: this is an undistorted view; the network saw the stored pixels (refine the original "
                         "result, then undistort the refined view)")
    image_hw = image_hw if image_hw is not None else sfm.image_hw
    if image_hw is None:
        raise ValueError("SfmResult.refine_tracks: image_hw is required (this result carries none)")
    plan = plan_track_refinement(sfm, obs_mask=obs_mask, min_jobs_per_pair=min_jobs_per_pair)
    dev = sfm.keypoints.device
    out = {"pts0": [], "pts1": [], "expec_f": [], "ok": []}
    if plan.stats["n_jobs"]:
        pts0, pts1 = sfm.keypoints[plan.job_ref_kp], sfm.keypoints[plan.job_query_kp]
        for _, res in refine_pair_list(model, plan.pairs.numpy(), plan.pair_offsets.numpy(), pts0, pts1, load, image_hw, **pair_list_kw):
            for k in out:
                out[k].append(res[k].to(dev))
    empty = {"pts0": (0, 2), "pts1": (0, 2), "expec_f": (0, 3), "ok": (0,)}
    result = {k: torch.cat(v) if v else torch.zeros(empty[k], dtype=torch.uint8 if k == "ok" else torch.float32, device=dev)
              for k, v in out.items()}
    return apply_refinement(sfm, plan, result, image_hw=image_hw, max_std=max_std, max_shift_px=max_shift_px)
