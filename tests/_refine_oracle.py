"""Restatements of the track-refinement rules for the tests: the fine-window centres in numpy fp32, the plan of
``plan_track_refinement`` with Python dicts and loops, and the apply rules of ``apply_refinement`` with a loop over the jobs."""
import math

import numpy as np

F = np.float32


def _centre(p, scale, s, extent):
    q = F(p)
    if scale is not None:
        q = F(q / F(scale))
    q = F(np.floor(F(F(q / F(s)) + F(0.5))))
    if not q > 0:
        return 0
    if q >= F(extent - 1):
        return extent - 1
    return int(q)


def _snapped(c, s, scale):
    v = F(F(c) * F(s))
    return v if scale is None else F(v * F(scale))


def centres(pts0, pts1, b_ids, n_pairs, hw0_f, hw1_f, hw0_c, hw1_c, stride, s, scale0=None, scale1=None):
    """loftr_refine_centres_host, one row after the other -> dict of numpy arrays."""
    M = len(b_ids)
    out = dict(c0=np.zeros((M, 2), np.int32), c1=np.zeros((M, 2), np.int32), i_ids=np.zeros(M, np.int64), j_ids=np.zeros(M, np.int64),
               pts0_s=np.zeros((M, 2), F), pts1_s=np.zeros((M, 2), F), ok=np.zeros(M, np.uint8))
    with np.errstate(all="ignore"):
        for m in range(M):
            b = int(b_ids[m])
            ok = 0 <= b < n_pairs and all(math.isfinite(float(v)) for v in (*pts0[m], *pts1[m]))
            out["ok"][m] = ok
            for pts, scale, (hf, wf), (hc, wc), c, ids, ps in ((pts0, scale0, hw0_f, hw0_c, "c0", "i_ids", "pts0_s"),
                                                             (pts1, scale1, hw1_f, hw1_c, "c1", "j_ids", "pts1_s")):
                if not ok:
                    continue                                            # centre 0, cell 0, snapped point (0, 0)
                sx, sy = (None, None) if scale is None else (scale[b][0], scale[b][1])
                cx, cy = _centre(pts[m][0], sx, s, wf), _centre(pts[m][1], sy, s, hf)
                out[c][m] = (cx, cy)
                out[ids][m] = min((cy + stride // 2) // stride, hc - 1) * wc + min((cx + stride // 2) // stride, wc - 1)
                out[ps][m] = (_snapped(cx, s, sx), _snapped(cy, s, sy))
    return out


def plan(host, obs_mask=None, min_jobs_per_pair=1):
    """plan_track_refinement on ``SfmResult.to_host()`` -> dict(pairs, pair_offsets, job_ref_kp, job_query_kp, job_track, stats)."""
    kp_offsets, track_id, track_ok, score = host["kp_offsets"], host["track_id"], host["track_ok"], host["score"]
    image_of = {}
    for im in range(len(kp_offsets) - 1):
        for k in range(int(kp_offsets[im]), int(kp_offsets[im + 1])):
            image_of[k] = im
    members = {}
    for k, t in enumerate(track_id.tolist()):                           # keypoints in ascending index
        if t >= 0 and track_ok[t]:
            members.setdefault(t, []).append(k)
    jobs, n = [], 0
    for t in sorted(members):                                           # the CSR order of tracks(consistent_only=True)
        left = []
        for k in members[t]:
            if obs_mask is None or obs_mask[n]:
                left.append(k)
            n += 1
        if len(left) < 2:
            continue
        ref = min(left, key=lambda k: (-float(score[k]), k))
        jobs += [(image_of[ref], image_of[k], k, ref, t) for k in left if k != ref]
    jobs.sort()
    by_pair = {}
    for j in jobs:
        by_pair.setdefault(j[:2], []).append(j)
    kept = {p: js for p, js in by_pair.items() if len(js) >= min_jobs_per_pair}
    pairs = sorted(kept)
    flat = [j for p in pairs for j in kept[p]]
    offsets = [0]
    for p in pairs:
        offsets.append(offsets[-1] + len(kept[p]))
    return dict(pairs=np.array(pairs, np.int64).reshape(-1, 2), pair_offsets=np.array(offsets, np.int64),
                job_ref_kp=np.array([j[3] for j in flat], np.int64), job_query_kp=np.array([j[2] for j in flat], np.int64),
                job_track=np.array([j[4] for j in flat], np.int64),
                stats=dict(n_tracks=len({j[4] for j in flat}), n_jobs=len(flat), n_pairs=len(pairs), n_dropped_jobs=len(jobs) - len(flat),
                           n_dropped_pairs=len(by_pair) - len(pairs)))


def apply(keypoints, job_ref_kp, job_query_kp, res, image_hw, max_std=None, max_shift_px=None):
    """apply_refinement -> (keypoints, kp_state, accepted [J] bool), a job after the other."""
    kp = np.array(keypoints, F, copy=True)
    state = np.zeros(len(kp), np.int8)
    H, W = image_hw
    accepted = np.zeros(len(job_query_kp), bool)
    for j, (r, q) in enumerate(zip(job_ref_kp.tolist(), job_query_kp.tolist())):
        p = res["pts1"][j]
        ok = bool(res["ok"][j]) and bool(np.isfinite(p).all()) and 0 <= p[0] < W and 0 <= p[1] < H
        if ok and max_std is not None:
            ok = bool(res["expec_f"][j][2] <= F(max_std))
        if ok and max_shift_px is not None:
            d = (p - keypoints[q]).astype(F)
            ok = bool(np.sqrt(F(d[0] * d[0]) + F(d[1] * d[1]), dtype=F) <= F(max_shift_px))
        accepted[j] = ok
        state[q] = 2 if ok else 3
        if state[r] != 1:
            state[r] = 1 if ok else 4
        if ok:
            kp[q] = p
            kp[r] = res["pts0"][j]
    return kp, state, accepted
