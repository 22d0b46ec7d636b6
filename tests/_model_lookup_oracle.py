"""Independent oracle of the model lookup (include/loftr_hip.h): the rule in plain Python dictionaries, sharing no code with
the library -- its own cell function, its own per-image dictionaries instead of a binary search, tuples instead of the packed word.
It pins the host routine loftr_model_lookup_host, which in turn defines what the kernels must reproduce."""
import math

import numpy as np

KEPT, BAD_ROW, MASKED, NONFINITE, NEG_CONF, OUTSIDE, NO_KEYPOINT, NO_POINT, FUSED = range(9)
REASONS = ("kept", "bad_row", "masked", "nonfinite", "negative_conf", "outside", "no_keypoint", "no_point", "fused")
ST_ROW, ST_UNSORTED, ST_QUERY, ST_IMAGE, ST_CELLS, ST_POINT = 1, 2, 4, 8, 16, 32


def grid(image_hw, cell_px):
    """(inv, gh, gw) as the atlas computes them: the float32 reciprocal of the cell size and ceil(extent * inv)."""
    inv = np.float32(1) / np.float32(cell_px)
    return inv, int(math.ceil(np.float32(image_hw[0]) * inv)), int(math.ceil(np.float32(image_hw[1]) * inv))


def coord(x, inv, g):
    """floor of ONE float32 product; None outside [0, g)."""
    f = math.floor(float(np.float32(x) * np.float32(inv)))
    return f if 0 <= f < g else None


def cell_of(xy, inv, gh, gw):
    if not (math.isfinite(xy[0]) and math.isfinite(xy[1])):
        return None
    cx, cy = coord(xy[0], inv, gw), coord(xy[1], inv, gh)
    return None if cx is None or cy is None else cy * gw + cx


def model_cells(kp_offsets, keypoints, kp_point, P, image_hw, cell_px):
    """-> (kp_cell list with -1 for a keypoint outside the grid, status bits)."""
    inv, gh, gw = grid(image_hw, cell_px)
    cells, status = [], 0
    for i in range(len(kp_offsets) - 1):
        prev = None
        for k in range(int(kp_offsets[i]), int(kp_offsets[i + 1])):
            c = cell_of(keypoints[k], inv, gh, gw)
            if c is None or (prev is not None and prev >= c):
                status |= ST_CELLS
            c = -1 if c is None else c
            cells.append(c)
            prev = c
            if not -1 <= int(kp_point[k]) < P:
                status |= ST_POINT
    return cells, status


def lookup(model, queries):
    """model: dict(kp_offsets, keypoints, kp_point, xyz, image_hw, cell_px); queries: dict(kpts_db, kpts_q, conf, rows, mask or None,
    row_db, row_query, Q).  -> dict(status, and under status 0: pts3d, kpts, q_ids, match, point, conf, q_offsets, match_reason, counts
    = {reason name: n}, C)."""
    inv, gh, gw = grid(model["image_hw"], model["cell_px"])
    off, P = model["kp_offsets"], len(model["xyz"])
    n_images = len(off) - 1
    kp_of = [{cell_of(model["keypoints"][k], inv, gh, gw): k for k in range(int(off[i]), int(off[i + 1]))} for i in range(n_images)]
    q = queries
    M, R, Q = len(q["conf"]), len(q["row_db"]), int(q["Q"])
    status = 0
    for r in range(R):
        if not 0 <= q["row_db"][r] < n_images:
            status |= ST_IMAGE
        if not 0 <= q["row_query"][r] < Q or (r > 0 and q["row_query"][r] < q["row_query"][r - 1]):
            status |= ST_QUERY
    for m in range(M):
        if not 0 <= q["rows"][m] < R:
            status |= ST_ROW
        if m > 0 and q["rows"][m] < q["rows"][m - 1]:
            status |= ST_UNSORTED
    if status:
        return dict(status=status)
    reason, point, best = [None] * M, [None] * M, {}
    for m in range(M):
        db, qq, c = q["kpts_db"][m], q["kpts_q"][m], float(q["conf"][m])
        row = int(q["rows"][m])
        if q["mask"] is not None and not q["mask"][m]:
            reason[m] = MASKED
        elif not all(math.isfinite(float(v)) for v in (db[0], db[1], qq[0], qq[1], c)):
            reason[m] = NONFINITE
        elif c < 0:
            reason[m] = NEG_CONF
        else:
            cell = cell_of(db, inv, gh, gw)
            if cell is None:
                reason[m] = OUTSIDE
            elif cell not in kp_of[int(q["row_db"][row])]:
                reason[m] = NO_KEYPOINT
            elif model["kp_point"][kp_of[int(q["row_db"][row])][cell]] < 0:
                reason[m] = NO_POINT
            else:
                point[m] = int(model["kp_point"][kp_of[int(q["row_db"][row])][cell]])
                key = (int(q["row_query"][row]), point[m])
                if key not in best or (c, -m) > (float(q["conf"][best[key]]), -best[key]):
                    best[key] = m
    kept = []
    for m in range(M):
        if point[m] is not None:
            key = (int(q["row_query"][int(q["rows"][m])]), point[m])
            reason[m] = KEPT if best[key] == m else FUSED
            if best[key] == m:
                kept.append(m)
    q_of = [int(q["row_query"][int(q["rows"][m])]) for m in kept]
    q_offsets = np.zeros(Q + 1, np.int64)
    for x in q_of:
        q_offsets[x + 1] += 1
    return dict(status=0, C=len(kept),
                pts3d=np.array([model["xyz"][point[m]] for m in kept], np.float32).reshape(-1, 3),
                kpts=np.array([q["kpts_q"][m] for m in kept], np.float32).reshape(-1, 2),
                q_ids=np.array(q_of, np.int64), match=np.array(kept, np.int32), point=np.array([point[m] for m in kept], np.int32),
                conf=np.array([q["conf"][m] for m in kept], np.float32), q_offsets=np.cumsum(q_offsets),
                match_reason=np.array(reason, np.uint8).reshape(-1), counts={name: reason.count(i) for i, name in enumerate(REASONS)})
