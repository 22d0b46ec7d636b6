"""Inputs shared by the track-completion tests (tests/test_completion.py on the CPU, tests/test_hip_completion.py on the GPU): the split
scene with its exact expected result, the hand-written cases, the bad tables and the random / sized tables.

A table is a dict of numpy arrays in the order of NAMES (the arguments of ops.complete_tracks_host before the grid) plus 'grid' =
(gh, gw, inv), 'thresh_px' and 'reach'.  Every generator keeps margins: no r2 lies within 1e-6 relative of thr2 or of a rival's r2,
except the deliberate exact tie of two rows with identical xyz."""
import functools

import numpy as np

import _bundle_cases as BC
from _triangulation_cases import camera

NAMES = ("offsets", "obs_image", "xyz", "status", "kp_offsets", "keypoints", "kp_cell", "kp_row", "K", "T_cam_from_world", "posed")
HW, CELL, THRESH = (480.0, 640.0), 2.0, 4.0
OK, TOO_SHORT, NO_HYP, SMALL_ANGLE = 0, 1, 2, 3


def grid(hw=HW, cell=CELL):
    """(gh, gw, inv) as KeypointAtlas makes them"""
    inv = np.float32(1) / np.float32(cell)
    return int(np.ceil(np.float32(hw[0]) * inv)), int(np.ceil(np.float32(hw[1]) * inv)), float(inv)


def cell_of(xy, g):
    gh, gw, inv = g
    cx, cy = np.floor(np.float32(xy[0]) * np.float32(inv)), np.floor(np.float32(xy[1]) * np.float32(inv))
    return int(cy) * gw + int(cx) if 0 <= cx < gw and 0 <= cy < gh else -1


def project_all(K, T, X):
    """pixels [n,P,2] and depths [n,P] of the points X [P,3] in every camera"""
    Y = np.einsum("nij,pj->npi", T[:, :3, :3], X) + T[:, None, :3, 3]
    p = np.einsum("nij,npj->npi", K, Y)
    return p[..., :2] / p[..., 2:], Y[..., 2]


def assemble(n, rows, kps, K, T, posed, g, thresh=THRESH, reach=2):
    """rows: [(images, xyz, status)]; kps: [(image, (x, y), row or -1)] in any order -> the table, with 'kp_order' = the position of
    every entry of kps in the pool (ordered by image, then by cell)."""
    offsets, image = [0], []
    for ims, _, _ in rows:
        image += list(ims)
        offsets.append(len(image))
    xy32 = [np.asarray(k[1], np.float32) for k in kps]
    cell = [cell_of(p, g) for p in xy32]
    order = sorted(range(len(kps)), key=lambda k: (kps[k][0], cell[k]))
    per_image = np.bincount([k[0] for k in kps], minlength=n)[:n] if kps else np.zeros(n, np.int64)
    kp_offsets = np.zeros(n + 1, np.int64)
    kp_offsets[1:] = np.cumsum(per_image)
    where = np.empty(len(kps), np.int64)
    where[order] = np.arange(len(kps))
    return dict(offsets=np.array(offsets, np.int64), obs_image=np.array(image, np.int32),
                xyz=np.array([r[1] for r in rows], np.float32).reshape(len(rows), 3), status=np.array([r[2] for r in rows], np.uint8),
                kp_offsets=kp_offsets, keypoints=np.array([xy32[k] for k in order], np.float32).reshape(len(kps), 2),
                kp_cell=np.array([cell[k] for k in order], np.int32), kp_row=np.array([kps[k][2] for k in order], np.int32),
                K=np.ascontiguousarray(K, np.float64), T_cam_from_world=np.ascontiguousarray(T, np.float64), posed=np.asarray(posed, np.uint8),
                grid=g, thresh_px=thresh, reach=reach, kp_order=where)


def args(t, reach=None):
    """the positional arguments of ops.complete_tracks_host / oracle.complete"""
    gh, gw, inv = t["grid"]
    return [t[k] for k in NAMES] + [gh, gw, inv, t["thresh_px"], t["reach"] if reach is None else reach]


def check_margins(t, res):
    """no accepted or rejected distance near the threshold: asserts it of the oracle's proposals (r2 well below thr2)"""
    thr2 = t["thresh_px"] ** 2
    for _, bits in res["proposals"].values():
        r2 = float(np.array(bits, np.uint32).view(np.float32))
        assert abs(r2 - thr2) > 1e-4 * thr2


# ---- the split scene: every physical point is one row with a point, loose keypoints and pointless two-view rows ------------------------
@functools.lru_cache(maxsize=None)
def split_scene(seed=41, n_points=48):
    """12 ring cameras, 640 x 480, cell_px = 2, thresh_px = 4.  Points are accepted by rejection so that in every image all projections
    are more than 2 * 4 + 2 * 1.5 px apart, and a point is observed where it lies at least 12 px inside the border; keypoint noise is
    0.5 px, clipped at 1.5 px.  Every point's first 3-6 views form its row (xyz from the host triangulation with the true poses); of the
    remaining views half are loose keypoints and half form rows of two views given status small_angle.
    -> (table, expected kp_row_new [K], detached [K] bool)."""
    from loftr_amd import ops
    rng = np.random.default_rng(seed)
    n = 12
    K, T = BC.ring(n, seed + 1)
    g = grid()
    X, px = [], []
    while len(X) < n_points:
        x = rng.uniform([-1.2, -0.9, 4], [1.2, 0.9, 7])
        p, z = project_all(K, T, x[None])
        p, z = p[:, 0], z[:, 0]
        seen = (z > 0) & (p[:, 0] >= 12) & (p[:, 0] <= HW[1] - 12) & (p[:, 1] >= 12) & (p[:, 1] <= HW[0] - 12)
        if seen.sum() < 4 or (z <= 0).any():
            continue
        if px and min(np.linalg.norm(np.stack(px) - p[None], axis=2).min(), 1e9) <= 2 * THRESH + 2 * 1.5:
            continue
        X.append(x)
        px.append(p)
    rows, pointless, kps, owner = [], [], [], []                         # kps entries: (image, xy, row); owner: the point of each
    obs_xy = []
    for pt, (x, p) in enumerate(zip(X, px)):
        seen = [i for i in range(n) if 12 <= p[i, 0] <= HW[1] - 12 and 12 <= p[i, 1] <= HW[0] - 12]
        L = min(3 + pt % 4, len(seen) - 1)
        noisy = {}
        for i in seen:
            d = 0.5 * rng.standard_normal(2)
            d *= min(1.0, 1.5 / max(np.linalg.norm(d), 1e-12))
            noisy[i] = (p[i] + d).astype(np.float32)
        rows.append((seen[:L], pt, noisy))
        rest = seen[L:]
        for q in range(0, len(rest), 2):
            pair = rest[q:q + 2]
            if (q // 2) % 2 == 1 and len(pair) == 2:
                pointless.append((pair, pt))
            else:
                kps += [(i, noisy[i], -1) for i in pair]
                owner += [pt] * len(pair)
    all_rows = rows + [(ims, pt, rows[pt][2]) for ims, pt in pointless]
    for r, (ims, pt, noisy) in enumerate(all_rows):
        kps += [(i, noisy[i], r) for i in ims]
        owner += [pt] * len(ims)
        obs_xy += [noisy[i] for i in ims]
    t = assemble(n, [(ims, (0, 0, 0), OK) for ims, _, _ in all_rows], kps, K, T, np.ones(n, np.uint8), g)
    tri = ops.triangulate_tracks_host(t["offsets"], t["obs_image"], np.array(obs_xy, np.float32), t["K"], t["T_cam_from_world"], THRESH,
                                      float(np.cos(np.radians(1.5))))
    assert (tri["status"][:n_points] == OK).all(), tri["status"][:n_points]
    t["xyz"], t["status"] = tri["xyz"].copy(), tri["status"].copy()
    t["xyz"][n_points:], t["status"][n_points:] = np.nan, SMALL_ANGLE
    owner = np.array(owner)[np.argsort(t["kp_order"])]                   # the point of every keypoint of the pool
    detached = (t["kp_row"] == -1) | (t["kp_row"] >= n_points)
    expected = np.where(detached, owner, t["kp_row"]).astype(np.int32)  # (the row of point p is row p)
    assert len({(im, c) for im, c in zip(np.repeat(np.arange(n), np.diff(t["kp_offsets"])), t["kp_cell"])}) == len(kps)
    return t, expected, detached


# ---- hand-written cases, one call -------------------------------------------------------------------------------------------------------
N_HAND = 10
A, B, BEHIND, D, UNPOSED, FX0, EMPTY, H, I3, J = range(N_HAND)


def hand():
    """-> (table, notes): identity rotations, f = 500, principal point (320, 240), points at depth 4, so the projection of (x, y, 4) in
    a camera at centre c is (125 (x - cx) + 320, 125 (y - cy) + 240).  Every row visits all images except its targets, so a row meets
    keypoints only where its case wants it; points are at least 0.3 apart (37 px).  notes: name -> row / keypoint index, and
    'expect' = {keypoint name: row name or None} for reach 2."""
    cams = [camera(500, (0, 0, 0)), camera(500, (1, 0, 0)), camera(500, (0, 0, 10)), camera(500, (0.5, 0, 0)), camera(500, (0.5, 0.5, 0)),
            camera(500, (0.5, -0.5, 0)), camera(500, (0, 0.5, 0)), camera(500, (1, 0.5, 0)), camera(500, (-0.5, 0, 0)), camera(500, (0, -0.5, 0))]
    K, T = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    K[FX0, 0, 0] = 0.0
    posed = np.ones(N_HAND, np.uint8)
    posed[UNPOSED] = 0
    centre = [(0, 0), (1, 0), (0, 0), (0.5, 0), (0.5, 0.5), (0.5, -0.5), (0, 0.5), (1, 0.5), (-0.5, 0), (0, -0.5)]
    proj = lambda im, X, d=(0, 0): (125 * (X[0] - centre[im][0]) + 320 + d[0], 125 * (X[1] - centre[im][1]) + 240 + d[1])
    rows, kps, row_id, kp_id, expect = [], [], {}, {}, {}

    def row(name, X, status, targets):
        row_id[name] = len(rows)
        rows.append(([i for i in range(N_HAND) if i not in targets], X, status))

    def kp(name, image, xy, owner, taken_by):
        kp_id[name] = len(kps)
        kps.append((image, xy, -1 if owner is None else row_id[owner]))
        expect[name] = taken_by

    row("owner_ok", (-1.2, 1.5, 4), OK, ())
    row("owner_pointless", (-0.9, 1.5, 4), NO_HYP, ())
    X = (-1.0, -0.6, 4)
    row("behind", X, OK, (BEHIND,))                                       # z = 4 - 10 < 0 in that camera
    kp("behind", BEHIND, (125 * X[0] * 4 / -6 + 320, 125 * X[1] * 4 / -6 + 240), None, None)       # where it would land with |z|
    X = (4.0, -0.6, 4)
    row("outside", X, OK, (D,))                                           # u = 757.5
    kp("outside", D, (639.0, proj(D, X)[1]), None, None)
    X = (0.5 + 318.1 / 125, 238.1 / 125, 4)                               # (638.1, 478.1) in D: the last cell of a row and of a column
    row("corner", X, OK, (D,))
    kp("corner_two_cells", D, (635.9, 478.1), None, "corner")             # 2.2 px, two cells to the left: needs reach 2
    kp("corner_one_cell", D, (636.1, 476.1), None, None)                  # 2.83 px, one cell away: the winner at reach 1
    kp("next_row_start", D, (1.0, 479.0), None, None)                     # what an unclipped cell range would run into
    X = (-0.7, -0.6, 4)
    row("visits", X, OK, ())                                              # D is already in the row
    kp("visits", D, proj(D, X, (0.5, 0)), None, None)
    X = (-0.4, -0.6, 4)
    row("unposed", X, OK, (UNPOSED,))
    kp("unposed", UNPOSED, proj(UNPOSED, X, (0.5, 0)), None, None)
    X = (-0.1, -0.6, 4)
    row("fx0", X, OK, (FX0,))
    kp("fx0", FX0, (300.0, 200.0), None, None)
    row("nan", (np.nan, -0.3, 4), OK, (D,))
    X = (-1.0, -0.3, 4)
    row("not_ok", X, SMALL_ANGLE, (D,))
    kp("not_ok", D, proj(D, X, (0.5, 0)), None, None)
    X = (-0.7, -0.3, 4)
    row("blocked", X, OK, (D,))
    kp("blocked", D, proj(D, X, (1.0, 0)), "owner_ok", None)              # held by a row with a point: counts[7]
    X = (-0.4, -0.3, 4)
    row("takes", X, OK, (D,))
    kp("taken", D, proj(D, X, (-1.0, 0)), "owner_pointless", "takes")      # held by a row without a point
    X = (-0.1, -0.3, 4)
    row("two_free", X, OK, (D,))
    kp("two_free_near", D, proj(D, X, (0.8, 0.25)), None, "two_free")
    kp("two_free_far", D, proj(D, X, (-2.5, 0.25)), None, None)
    X = (0.2, -0.3, 4)
    row("tie_low", X, OK, (H,))
    row("tie_high", X, OK, (H,))                                          # identical xyz: equal key bits up to the row
    kp("tie", H, proj(H, X, (0.5, 0.25)), None, "tie_low")
    X = (0.5, -0.3, 4)
    row("three_a", X, OK, (I3,))
    row("three_b", (X[0] + 0.003, X[1], 4), OK, (I3,))                    # 0.375 px further right
    row("three_c", (X[0] + 0.006, X[1], 4), OK, (I3,))
    kp("three", I3, proj(I3, X, (0.45, 0.25)), None, "three_b")           # 0.45, 0.075 and 0.3 px to the right of a, b and c
    row("empty_image", (0.8, -0.3, 4), OK, (EMPTY,))
    t = assemble(N_HAND, rows, kps, K, T, posed, grid())
    notes = dict(row=row_id, kp={name: int(t["kp_order"][k]) for name, k in kp_id.items()}, expect=expect,
                 counts=dict(n_links=5, n_sources=sum(r[2] == OK and np.isfinite(r[1]).all() for r in rows), n_lost=3, n_blocked=1))
    return t, notes


def check_hand(t, notes, res, reach):
    """what hand() promises of a result (dict of numpy arrays) at reach 0, 1 or 2"""
    expect = dict(notes["expect"])
    if reach < 2:
        expect["corner_two_cells"] = None
    if reach == 1:
        expect["corner_one_cell"] = "corner"
    for name, by in expect.items():
        k = notes["kp"][name]
        want = t["kp_row"][k] if by is None else notes["row"][by]
        assert res["kp_row_new"][k] == want, (name, reach, int(res["kp_row_new"][k]), int(want))
        assert np.isnan(res["link_r2"][k]) == (by is None), (name, reach)
    c = res["counts"]
    want = notes["counts"]
    assert c[0] == want["n_links"] - (reach == 0) and c[1] == 0 and c[2] == want["n_sources"] and c[6] == want["n_lost"] and c[7] == want["n_blocked"], c
    assert c[3] == 12 and c[4] == 10 and c[5] == c[0] + c[6]                # 12 (source, target) pairs; behind and outside leave the grid
    assert abs(float(res["link_r2"][notes["kp"]["tie"]]) - (0.5 ** 2 + 0.25 ** 2)) < 1e-4


def empties():
    """T = 0, K = 0 and n = 0, each a table of its own"""
    t, _ = hand()
    n = N_HAND
    no_rows = assemble(n, [], [(D, (100.0, 100.0), -1)], t["K"], t["T_cam_from_world"], t["posed"], t["grid"])
    no_kps = assemble(n, [([A, B], (0, 0, 4), OK)], [], t["K"], t["T_cam_from_world"], t["posed"], t["grid"])
    nothing = assemble(0, [], [], np.zeros((0, 3, 3)), np.zeros((0, 4, 4)), np.zeros(0, np.uint8), t["grid"])
    return dict(no_rows=no_rows, no_keypoints=no_kps, no_images=nothing)


def bad_tables():
    """bit -> the hand table with that error alone; nothing can be read through the bad value before a check meets it"""
    out = {}
    for bit in (1, 2, 4, 8):
        t, _ = hand()
        t = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()}
        if bit == 1:
            t["obs_image"][t["offsets"][3] - 1] = N_HAND                 # the last observation of a row: no descent
        elif bit == 2:
            t["offsets"][-1] -= 1                                         # the last row no longer ends at N
        elif bit == 4:
            o = t["offsets"][4]
            t["obs_image"][o], t["obs_image"][o + 1] = t["obs_image"][o + 1], t["obs_image"][o]
        else:
            t["kp_row"][0] = len(t["status"])
        out[bit] = t
    return out


# ---- random and sized tables -------------------------------------------------------------------------------------------------------------
def random_table(seed, n_images=7, n_points=40, rows_per_point=2, kp_per_image=None, max_views=4, reach=2, thresh=THRESH, identical=False,
                 row_views=None, posed_rate=0.8):
    """ring cameras; every point gives rows_per_point rows (a split track) over random image subsets with slightly different xyz, random
    statuses (70 % ok, a few NaN points), keypoints near 80 % of the projections (1.5 px noise, one per cell), kp_row = the row of an
    observation, else -1 (60 %) or ANY row (40 %), random posed (80 %), the last camera invalid for odd seeds.
    kp_per_image: {image: number of keypoints} filled with (or cut down to) keypoints at random free cells.  identical: all rows share one
    xyz and image 0 holds one keypoint at its projection (the contention case).  row_views: observations of row 0."""
    rng = np.random.default_rng(seed)
    n, g = n_images, grid()
    gh, gw, _ = g
    K, T = BC.ring(n, seed + 1)
    X = rng.uniform([-1, -0.8, 4], [1, 0.8, 7], (n_points, 3))
    if identical:                                                        # on the optical axis of camera 0
        X[:] = -T[0, :3, :3].T @ T[0, :3, 3] + T[0, :3, :3].T @ np.array([0, 0, 5.0])
    p, z = project_all(K, T, X)
    rows, kps, taken = [], [], set()
    for pt in range(n_points):
        for r in range(rows_per_point):
            ims = sorted(rng.permutation(n)[:min(n - 1, rng.integers(1, max_views + 1))].tolist()) if not identical else ([1] if n > 1 else [])
            if row_views is not None and not rows:
                ims = sorted(rng.permutation(n)[:row_views].tolist())
            st = OK if identical or rng.random() < 0.7 else int(rng.integers(1, 5))
            xyz = X[pt] + (0 if identical else 0.002 * rng.standard_normal(3))
            if not identical and rng.random() < 0.05:
                xyz[rng.integers(3)] = np.nan
            rows.append((ims, xyz, st))
    n_rows = len(rows)
    for pt in range(n_points if not identical else 1):
        for i in range(n if not identical else 1):
            if z[i, pt] > 0 and (identical or rng.random() < 0.8):
                xy = (p[i, pt] + (0.25 if identical else 1.5 * rng.standard_normal(2))).astype(np.float32)
                c = cell_of(xy, g)
                if c >= 0 and (i, c) not in taken:
                    taken.add((i, c))
                    holders = [pt * rows_per_point + r for r in range(rows_per_point) if i in rows[pt * rows_per_point + r][0]]
                    u = rng.random()
                    kps.append((i, xy, -1 if identical else holders[0] if holders else -1 if u < 0.6 else int(rng.integers(n_rows))))
    for i, want in (kp_per_image or {}).items():
        kps = [k for k in kps if k[0] != i] + [k for k in kps if k[0] == i][:want]
        have = sum(k[0] == i for k in kps)
        while have < want:
            c = int(rng.integers(gh * gw))
            if (i, c) not in taken:
                taken.add((i, c))
                kps.append((i, np.array([(c % gw) * CELL + rng.uniform(0.2, 1.8), (c // gw) * CELL + rng.uniform(0.2, 1.8)], np.float32), -1))
                have += 1
    posed = np.ones(n, np.uint8) if identical else (rng.random(n) < posed_rate).astype(np.uint8)
    if seed % 2 == 1 and not identical:
        K[n - 1, 1, 1] = np.nan
    return assemble(n, rows, kps, K, T, posed, g, thresh, reach)


def corners(reach):
    """four rows whose points project into the four corner cells of image 1 (which they do not visit), keypoints in and around them"""
    cams = [camera(500, (0, 0, 0)), camera(500, (0.5, 0, 0))]
    K, T = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    rng = np.random.default_rng(7 + reach)
    rows, kps, used = [], [], set()
    g, spread = grid(), 2.0 * reach + 4
    for u, v in ((1.1, 0.9), (638.9, 1.1), (0.9, 478.9), (639.1, 479.1)):
        rows.append(([0], (0.5 + (u - 320) / 125, (v - 240) / 125, 4), OK))
        for _ in range(12):
            xy = np.array([u + rng.uniform(-spread, spread), v + rng.uniform(-spread, spread)], np.float32)
            c = cell_of(xy, g)
            if c >= 0 and c not in used:
                used.add(c)
                kps.append((1, xy, -1))
    return assemble(2, rows, kps, K, T, np.ones(2, np.uint8), g, max(THRESH, 2.0 * reach), reach)


# ---- a synthetic pair list whose tracks are split ------------------------------------------------------------------------------------------
SPLIT_EVERY = 3


def split_atlas(device):
    """KeypointAtlas over the pair list of _triangulation_cases.sfm_scene() (5 cameras, 60 points, every pair of images a row) with every
    third point cut in two: its matches stay in the rows among images 0-2 (a track of three views), and in row (3, 4) its true position
    in image 3 is matched to a position 60 px off in image 4 (a two-view track that triangulates nothing).  Its keypoint in image 3 is
    what a completion can give back to the point.  -> (SfmResult, scene, the cut points)."""
    import torch
    import _triangulation_cases as TC
    from loftr_amd import KeypointAtlas
    s = TC.sfm_scene()
    n_points = len(s["X"])
    cut = np.arange(n_points) % SPLIT_EVERY == 0
    snap = lambda p: (np.floor(p / TC.SFM_CELL) * TC.SFM_CELL + TC.SFM_CELL / 2).astype(np.float32)
    off = snap(s["px"][4] + np.array([0.0, 60.0], np.float32))
    assert len({tuple(q) for q in np.concatenate([s["px"][4][~cut], off[cut]]).tolist()}) == n_points and (off[:, 1] < TC.SFM_HW[0]).all()
    atlas = KeypointAtlas(5, TC.SFM_HW, TC.SFM_CELL, device=device)
    dev = torch.device(device)
    for a, b, k0, k1, c in s["rows"]:
        keep = np.ones(n_points, bool)
        if b >= 3:
            keep = ~cut if (a, b) != (3, 4) else keep
            k1 = np.where(cut[:, None], off, k1) if (a, b) == (3, 4) else k1
        data = {"mkpts0_f": torch.from_numpy(k0[keep]).to(dev), "mkpts1_f": torch.from_numpy(k1[keep]).to(dev),
                "mconf": torch.from_numpy(c[keep]).to(dev), "m_bids": torch.zeros(int(keep.sum()), dtype=torch.int64, device=dev)}
        atlas.add(np.array([[a, b]]), data)
    return atlas.finalize(), s, cut
