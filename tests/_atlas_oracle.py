"""Independent restatement of the keypoint atlas rules in plain Python / numpy: dicts and a textbook union-find.
Shares no code with loftr_amd; only the rules.

    chunks: list of (image_ids [n,2], mkpts0 [M,2], mkpts1 [M,2], mconf [M], m_bids [M], mask [M] bool or None), one per add
    -> dict with the arrays of SfmResult.to_host()
"""
import math

import numpy as np


def _cell(v, inv, g):
    """floor(v * inv) in float32, or None outside [0, g)."""
    f = np.floor(np.float32(v) * inv)
    if not (f >= 0 and f < g):
        return None
    return int(f)


def atlas_oracle(chunks, n_images, image_hw, cell_px, min_track_len=2):
    inv = np.float32(1) / np.float32(cell_px)
    gh = int(math.ceil(float(np.float32(image_hw[0]) * inv)))
    gw = int(math.ceil(float(np.float32(image_hw[1]) * inv)))
    stats = dict(n_images=n_images, n_rows=0, n_matches=0, n_valid=0, n_masked=0, n_nonfinite=0, n_negative_conf=0, n_outside=0)
    row_images, obs = [], []          # obs: per valid match (match index, row, conf, ((image, cy, cx, x, y) per side))
    m_index = 0
    for ids, k0, k1, conf, bids, mask in chunks:
        ids = np.asarray(ids).reshape(-1, 2)
        base = len(row_images)
        for a, b in ids:
            assert a != b and 0 <= a < n_images and 0 <= b < n_images
            row_images.append((int(a), int(b)))
        for i in range(len(conf)):
            m, m_index = m_index, m_index + 1
            assert 0 <= int(bids[i]) < len(ids)
            row = base + int(bids[i])
            vals = [np.float32(k0[i][0]), np.float32(k0[i][1]), np.float32(k1[i][0]), np.float32(k1[i][1]), np.float32(conf[i])]
            if mask is not None and not mask[i]:
                stats["n_masked"] += 1
                continue
            if not all(np.isfinite(v) for v in vals):
                stats["n_nonfinite"] += 1
                continue
            if not vals[4] >= 0:
                stats["n_negative_conf"] += 1
                continue
            cells = [_cell(vals[0], inv, gw), _cell(vals[1], inv, gh), _cell(vals[2], inv, gw), _cell(vals[3], inv, gh)]
            if any(c is None for c in cells):
                stats["n_outside"] += 1
                continue
            stats["n_valid"] += 1
            im = row_images[row]
            obs.append((m, row, vals[4], ((im[0], cells[1], cells[0], vals[0], vals[1]), (im[1], cells[3], cells[2], vals[2], vals[3]))))
    stats["n_rows"], stats["n_matches"] = len(row_images), m_index

    # rule 2: one keypoint per occupied (image, cy, cx); greatest conf, then smallest observation index 2 m + side
    best, count = {}, {}
    for m, row, c, sides in obs:
        for side, (im, cy, cx, x, y) in enumerate(sides):
            key = (im, cy, cx)
            cand = (-float(c), 2 * m + side, x, y, c)
            if key not in best or cand[:2] < best[key][:2]:
                best[key] = cand
            count[key] = count.get(key, 0) + 1
    order = sorted(best)
    kp = {key: k for k, key in enumerate(order)}
    K = len(order)
    keypoints = np.array([[best[key][2], best[key][3]] for key in order], np.float32).reshape(K, 2)
    score = np.array([best[key][4] for key in order], np.float32)
    n_obs = np.array([count[key] for key in order], np.int32)
    kp_image = [key[0] for key in order]
    kp_offsets = np.zeros(n_images + 1, np.int64)
    for im in kp_image:
        kp_offsets[im + 1] += 1
    kp_offsets = np.cumsum(kp_offsets)

    # rule 3: mutual best per row
    win = {}
    for m, row, c, sides in obs:
        for side in (0, 1):
            key = (row, side, kp[sides[side][:3]])
            cand = (-float(c), m)
            if key not in win or cand < win[key]:
                win[key] = cand
    kept = []
    for m, row, c, sides in obs:
        ka, kb = kp[sides[0][:3]], kp[sides[1][:3]]
        if win[(row, 0, ka)][1] == m and win[(row, 1, kb)][1] == m:
            kept.append((row, ka, kb, c))
    R = len(row_images)
    row_offsets = np.zeros(R + 1, np.int64)
    for row, _, _, _ in kept:
        row_offsets[row + 1] += 1
    row_offsets = np.cumsum(row_offsets)
    matches = np.array([[ka - kp_offsets[kp_image[ka]], kb - kp_offsets[kp_image[kb]]] for _, ka, kb, _ in kept], np.int32).reshape(-1, 2)
    match_conf = np.array([c for _, _, _, c in kept], np.float32)

    # rule 4: components
    parent = list(range(K))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for _, ka, kb, _ in kept:
        ra, rb = find(ka), find(kb)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    comps = {}
    for k in range(K):
        comps.setdefault(find(k), []).append(k)
    assert all(label == min(members) for label, members in comps.items())
    track_id = np.full(K, -1, np.int32)
    track_len, track_ok = [], []
    for label in sorted(comps):
        members = comps[label]
        if len(members) < min_track_len:
            continue
        track_id[members] = len(track_len)
        track_len.append(len(members))
        images = [kp_image[k] for k in members]
        track_ok.append(len(set(images)) == len(images))
    stats.update(n_keypoints=K, n_kept=len(kept), n_tracks=len(track_len))
    return {"kp_offsets": kp_offsets, "keypoints": keypoints, "score": score, "n_obs": n_obs, "row_offsets": row_offsets, "matches": matches,
            "match_conf": match_conf, "track_id": track_id, "track_len": np.array(track_len, np.int32), "track_ok": np.array(track_ok, bool),
            "row_images": np.array(row_images, np.int32).reshape(-1, 2), "stats": stats}
