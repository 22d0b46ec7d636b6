"""Inputs shared by the track-merging tests (tests/test_merge.py on the CPU, tests/test_hip_merge.py on the GPU): the twin scene with its
exact expected result, the hand-written cases, the empty and the bad tables, the random / sized tables and the atlas of twin tracks.

A table is a table of _completion_cases (a dict of numpy arrays plus 'grid', 'thresh_px', 'reach') with 'obs_xy' [N,2] f32 and
'obs_mask' [N] u8 added; args() puts it in the order of ops.merge_tracks_host.  The generators assert conditions, not measurements: no
candidate distance and no pair score lies within 1e-4 relative of thr2 (check_margins)."""
import functools

import numpy as np

import _bundle_cases as BC
import _completion_cases as CC
import _triangulation_cases as TC

NAMES = ("offsets", "obs_image", "obs_xy", "obs_mask", "xyz", "status", "kp_offsets", "keypoints", "kp_cell", "kp_row", "K", "T_cam_from_world",
         "posed")
OK, NO_HYP = CC.OK, CC.NO_HYP
THRESH = CC.THRESH


def args(t, reach=None):
    """the positional arguments of ops.merge_tracks_host / oracle.merge"""
    gh, gw, inv = t["grid"]
    return [t[k] for k in NAMES] + [gh, gw, inv, t["thresh_px"], t["reach"] if reach is None else reach]


def check_margins(t, res):
    """of an oracle result: no candidate distance of a meeting and no score of an accepted pair near the threshold"""
    thr2 = t["thresh_px"] ** 2
    for bits in [m[3] for m in res["meetings"]] + list(res["scores"].values()):
        r2 = float(np.array(bits, np.uint32).view(np.float32))
        assert abs(r2 - thr2) > 1e-4 * thr2, r2


def with_observations(t, obs_xy, obs_mask):
    t = dict(t)
    t["obs_xy"] = np.ascontiguousarray(obs_xy, np.float32).reshape(len(t["obs_image"]), 2)
    t["obs_mask"] = np.ascontiguousarray(obs_mask, np.uint8).reshape(len(t["obs_image"]))
    return t


# ---- the twin scene: two thirds of the physical points are two rows, each with a point of its own ------------------------------------------
@functools.lru_cache(maxsize=None)
def twin_scene(seed=41, n_points=30):
    """split_scene's cameras (12 on a ring, 640 x 480), grid (cell_px = 2), separation (in every image all projections more than
    2 * 4 + 2 * 1.5 px apart), border (12 px) and noise (0.5 px, clipped at 1.5 px); only points seen in at least 6 views.  The views
    of two thirds of the points are split into a first and a second half: two rows, both triangulated by the host routine from the true
    poses and both ok; the other points are one row.  Row p < n_points is point p (its first half); the second halves follow.
    -> (table, expected row_into [T], expected kp_row_new [K], twins = [(lower row, higher row)])."""
    from loftr_amd import ops
    rng = np.random.default_rng(seed)
    n = 12
    K, T = BC.ring(n, seed + 1)
    g = CC.grid()
    hw = CC.HW
    inside = lambda p: (p[:, 0] >= 12) & (p[:, 0] <= hw[1] - 12) & (p[:, 1] >= 12) & (p[:, 1] <= hw[0] - 12)
    X, px = [], []
    while len(X) < n_points:
        x = rng.uniform([-1.2, -0.9, 4], [1.2, 0.9, 7])
        p, z = CC.project_all(K, T, x[None])
        p, z = p[:, 0], z[:, 0]
        if (inside(p) & (z > 0)).sum() < 6 or (z <= 0).any():
            continue
        if px and np.linalg.norm(np.stack(px) - p[None], axis=2).min() <= 2 * THRESH + 2 * 1.5:
            continue
        X.append(x)
        px.append(p)
    first, second = [], []
    for pt, p in enumerate(px):
        seen = [int(i) for i in np.nonzero(inside(p))[0]]
        noisy = {}
        for i in seen:
            d = 0.5 * rng.standard_normal(2)
            d *= min(1.0, 1.5 / max(np.linalg.norm(d), 1e-12))
            noisy[i] = (p[i] + d).astype(np.float32)
        half = len(seen) // 2
        if pt % 3 != 2:
            first.append((seen[:half], noisy))
            second.append((seen[half:], noisy, pt))
        else:
            first.append((seen, noisy))
    rows = first + [(ims, noisy) for ims, noisy, _ in second]
    twins = [(pt, n_points + k) for k, (_, _, pt) in enumerate(second)]
    kps = [(i, noisy[i], r) for r, (ims, noisy) in enumerate(rows) for i in ims]
    obs_xy = np.array([noisy[i] for ims, noisy in rows for i in ims], np.float32)
    t = CC.assemble(n, [(ims, (0, 0, 0), OK) for ims, _ in rows], kps, K, T, np.ones(n, np.uint8), g)
    tri = ops.triangulate_tracks_host(t["offsets"], t["obs_image"], obs_xy, t["K"], t["T_cam_from_world"], THRESH, float(np.cos(np.radians(1.5))))
    assert (tri["status"] == OK).all(), tri["status"]                       # both halves of every twin have a point
    t["xyz"], t["status"] = tri["xyz"].copy(), tri["status"].copy()
    t = with_observations(t, obs_xy, tri["obs_inlier"])
    row_into = np.arange(len(rows), dtype=np.int32)
    for lo, hi in twins:
        row_into[hi] = lo
    return t, row_into, row_into[t["kp_row"]].astype(np.int32), twins


def check_twins(t, res, row_into, kp_row_new, twins):
    """what twin_scene() promises of a result: every twin's higher row goes into the lower and nothing else changes"""
    c = res["counts"]
    assert np.array_equal(res["row_into"], row_into) and np.array_equal(res["kp_row_new"], kp_row_new)
    assert c[0] == len(twins) and c[1] == 0 and c[2] == len(row_into) and c[4] == c[5] == c[6] >= 2 * len(twins), c
    merged = np.zeros(len(row_into), bool)
    merged[[r for pair in twins for r in pair]] = True
    assert np.array_equal(~np.isnan(res["merge_r2"]), merged) and c[7] == (kp_row_new != t["kp_row"]).sum()
    for lo, hi in twins:
        assert res["merge_r2"][lo] == res["merge_r2"][hi] < t["thresh_px"] ** 2


# ---- hand-written cases, one call -------------------------------------------------------------------------------------------------------
CENTRES = [(0, 0, 0), (1, 0, 0), (0.5, 0, 0), (0.5, 0.5, 0), (0, 0.5, 0), (1, 0.5, 0), (-0.5, 0, 0), (-0.5, 0.5, 0), (0.5, -0.5, 0), (0, -0.5, 0)]
N_HAND = len(CENTRES)
UNPOSED, EMPTY = 8, 9


def hand():
    """-> (table, notes).  Identity rotations, f = 500, principal point (320, 240): (x, y, z) lands at (500 (x - cx) / z + 320,
    500 (y - cy) / z + 240) in a camera at centre c; the groups are at least 0.6 apart (75 px at depth 4), so rows meet only within their
    group.  Every observation has its keypoint, held by its row, at the projection of the row's point plus the offset given; nobody
    visits image 9 (an image without keypoints) and image 8 has no pose.
    notes: 'row' name -> index, 'into' name -> name of the surviving row, 'counts' the expected counts[0], [4], [5], [6]."""
    cams = [TC.camera(500, c) for c in CENTRES]
    K, T = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    posed = np.ones(N_HAND, np.uint8)
    posed[UNPOSED] = 0
    rows, kps, obs_xy, obs_mask, row_id, into = [], [], [], [], {}, {}

    def row(name, X, images, status=OK, offset=None, mask=None, xyz=None, survivor=None):
        r = row_id[name] = len(rows)
        rows.append((sorted(images), X if xyz is None else xyz, status))
        for i in sorted(images):
            p = (TC.project(K[i], T[i], X) + np.asarray((offset or {}).get(i, (0, 0)), np.float64)).astype(np.float32)
            kps.append((i, p, r))
            obs_xy.append(p)
            obs_mask.append((mask or {}).get(i, 1))
        into[name] = survivor or name

    # two points on the ray of camera 0 that meet in image 0 and disagree elsewhere: disjoint, not accepted
    row("ray_near", (-1.0, -0.9, 4), (1, 2))
    row("ray_far", (-1.5, -1.35, 6), (0, 3))
    # two rows that meet in images 0 and 1 and both visit image 2: not disjoint
    row("shared_a", (-0.4, -0.9, 4), (0, 2))
    row("shared_b", (-0.4, -0.9, 4), (1, 2), offset={2: (3.0, 0)})
    # a meeting found from one side only: the higher row projects 1 px outside the grid in the images of the lower; it still merges
    row("one_sided_in", (-319 / 125, 0.3, 4), (0, 4))
    row("one_sided_out", (-321 / 125, 0.3, 4), (6, 7), survivor="one_sided_in")
    # a chain A - B - C (2 px and 0.5 px apart) with B - C better: only B - C merges
    row("chain_a", (0.2 - 0.016, -0.9, 4), (0,))
    row("chain_b", (0.2, -0.9, 4), (1,))
    row("chain_c", (0.2 + 0.004, -0.9, 4), (2,), survivor="chain_b")
    # equal scores among three rows: both pairs' score is the error of equal_a's own observation; the key picks the lower partner
    row("equal_a", (0.8, -0.9, 4), (0,), offset={0: (3.0, 0)})
    row("equal_b", (0.8 + 0.004, -0.9, 4), (1,), survivor="equal_a")
    row("equal_c", (0.8 + 0.004, -0.9, 4), (1,), offset={1: (0, 2.2)})
    # a partner that is not a source: status ok, NaN xyz
    row("nan_meets", (-1.0, -0.3, 4), (0,))
    row("nan_point", (-1.0, -0.3, 4), (1,), xyz=(np.nan, -0.3, 4))
    # a row none of whose observations is masked in: w = 0
    row("weight_a", (-0.4, -0.3, 4), (0,))
    row("weight_0", (-0.4, -0.3, 4), (1,), mask={1: 0})
    # a masked observation in an image without a pose
    row("unposed_a", (0.2, -0.3, 4), (0, UNPOSED))
    row("unposed_b", (0.2, -0.3, 4), (1,))
    # a nearer free keypoint is ignored: the partner's keypoint is 2.5 px away, a loose one 0.5 px
    row("free_a", (0.8, -0.3, 4), (0,))
    row("free_b", (0.8, -0.3, 4), (1,), offset={1: (2.5, 0)}, survivor="free_a")
    kps.append((1, (TC.project(K[1], T[1], (0.8, -0.3, 4)) + np.array([0.5, 0])).astype(np.float32), -1))
    # a row without a point next to one with a point: its keypoint is completion's business
    row("pointless", (-1.0, 0.9, 4), (0,), status=NO_HYP)
    row("pointless_meets", (-1.0, 0.9, 4), (1,))
    t = with_observations(CC.assemble(N_HAND, rows, kps, K, T, posed, CC.grid()), obs_xy, obs_mask)
    return t, dict(row=row_id, into=into, counts=dict(n_merges=4, n_meetings=20, n_disjoint=18, n_accepted=13))


def check_hand(t, notes, res):
    """what hand() promises of a result (dict of numpy arrays) at reach 2"""
    row = notes["row"]
    for name, survivor in notes["into"].items():
        assert res["row_into"][row[name]] == row[survivor], (name, int(res["row_into"][row[name]]))
        partner = [other for other, s in notes["into"].items() if other != name and (s == name or (survivor != name and other == survivor))]
        assert np.isnan(res["merge_r2"][row[name]]) == (not partner), name
    c, want = res["counts"], notes["counts"]
    assert (c[0], c[1], c[4], c[5], c[6]) == (want["n_merges"], 0, want["n_meetings"], want["n_disjoint"], want["n_accepted"]), c
    assert c[2] == sum(1 for x, s in zip(t["xyz"], t["status"]) if s == OK and np.isfinite(x).all()) and c[7] == 5
    assert np.array_equal(res["kp_row_new"], np.where(t["kp_row"] < 0, t["kp_row"], res["row_into"][t["kp_row"]]))
    r2 = lambda name: float(res["merge_r2"][row[name]])
    assert abs(r2("free_a") - 6.25) < 1e-3 and abs(r2("chain_b") - 0.0625) < 1e-3 and r2("equal_a") == r2("equal_b")


def empties():
    """T = 0, K = 0 and n = 0, each a table of its own"""
    t, _ = hand()
    K, T, posed, g = t["K"], t["T_cam_from_world"], t["posed"], t["grid"]
    no_rows = with_observations(CC.assemble(N_HAND, [], [(3, (100.0, 100.0), -1)], K, T, posed, g), np.zeros((0, 2)), [])
    no_kps = with_observations(CC.assemble(N_HAND, [([0, 1], (0, 0, 4), OK)], [], K, T, posed, g), [[320, 240], [195, 240]], [1, 1])
    nothing = with_observations(CC.assemble(0, [], [], np.zeros((0, 3, 3)), np.zeros((0, 4, 4)), np.zeros(0, np.uint8), g), np.zeros((0, 2)), [])
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
            o = t["offsets"][0]
            t["obs_image"][o], t["obs_image"][o + 1] = t["obs_image"][o + 1], t["obs_image"][o]
        else:
            t["kp_row"][0] = len(t["status"])
        out[bit] = t
    return out


# ---- random and sized tables -------------------------------------------------------------------------------------------------------------
def random_table(seed, n_images=7, n_points=40, rows_per_point=2, max_views=3, noise=0.7, **kw):
    """_completion_cases.random_table (split tracks over random image subsets, random statuses, a few NaN points, keypoints held by a
    row of their point, loose or held by ANY row, random posed, an invalid camera for odd seeds) with the observations added: the
    projection of the row's own point plus `noise` px (the point's first coordinate where it is NaN), 85 % of them masked in."""
    t = CC.random_table(seed, n_images=n_images, n_points=n_points, rows_per_point=rows_per_point, max_views=max_views, **kw)
    rng = np.random.default_rng(1000 + seed)
    K, T = BC.ring(n_images, seed + 1)                                     # (the valid cameras of the table)
    row = np.repeat(np.arange(len(t["status"])), np.diff(t["offsets"]))
    X = np.nan_to_num(t["xyz"].astype(np.float64), nan=0.5)
    xy = np.zeros((len(row), 2))
    for o, (r, i) in enumerate(zip(row, t["obs_image"])):
        xy[o] = TC.project(K[i], T[i], X[r]) + noise * rng.standard_normal(2)
    return with_observations(t, xy, rng.random(len(row)) < 0.85)


def sized(n_rows, n_images, seed=0, views=(1, 2, 3), kp_per_image=None, thresh=THRESH, reach=2):
    """n_rows rows, all ok and fully masked, whose points lie within a fraction of a pixel of one point on the axis of the camera ring; row r
    visits views[r % len(views)] consecutive images from image 3 r mod n_images on (so rows straddle the chunk edge).  The keypoints of an image sit one per cell on the
    lattice of cells around the projection, nearest cells first: the first dozen rows of an image meet and agree, later ones meet and
    disagree (their own observation is too far from the point) or do not meet at all; rows that share an image are not disjoint.
    kp_per_image: {image: number of keypoints} filled up with loose keypoints at random free cells."""
    rng = np.random.default_rng(seed)
    g = CC.grid()
    gh, gw, _ = g
    K, T = BC.ring(max(n_images, 1), seed + 1)
    K, T = K[:n_images], T[:n_images]
    centre = np.array([0.0, 0.0, 6.0])                                     # on the axis of the ring: inside every image
    half = int(np.ceil(np.sqrt(n_rows * max(views)))) // 2 + 1
    lattice = sorted(((dx, dy) for dx in range(-half, half + 1) for dy in range(-half, half + 1)), key=lambda d: (d[0] ** 2 + d[1] ** 2, d))
    rows, kps, obs_xy, taken, used = [], [], [], set(), [0] * n_images
    for r in range(n_rows):
        ims = sorted({(3 * r + q) % n_images for q in range(min(views[r % len(views)], n_images))}) if n_images else []
        rows.append((ims, centre + 0.002 * rng.uniform(-1, 1, 3) * np.array([1, 1, 0]), OK))
        for i in ims:
            xy = ((np.floor(TC.project(K[i], T[i], centre) / CC.CELL) + np.array(lattice[used[i]])) * CC.CELL + rng.uniform(0.3, 1.7, 2)).astype(np.float32)
            used[i] += 1
            c = CC.cell_of(xy, g)
            assert c >= 0 and (i, c) not in taken
            taken.add((i, c))
            kps.append((i, xy, r))
            obs_xy.append(xy)
    for i, want in (kp_per_image or {}).items():
        have = sum(k[0] == i for k in kps)
        while have < want:
            c = int(rng.integers(gh * gw))
            if (i, c) not in taken:
                taken.add((i, c))
                kps.append((i, np.array([(c % gw) * CC.CELL + rng.uniform(0.2, 1.8), (c // gw) * CC.CELL + rng.uniform(0.2, 1.8)], np.float32), -1))
                have += 1
    t = CC.assemble(n_images, rows, kps, K, T, np.ones(n_images, np.uint8), g, thresh, reach)
    return with_observations(t, np.array(obs_xy, np.float32).reshape(-1, 2), np.ones(len(obs_xy), np.uint8))


def star(n_rows=512, per_image=8):
    """n_rows rows with one identical point seen by 130 identical cameras.  Row 0 visits image 0 alone, its observation 3 px off the
    projection; row r > 0 visits images 1 + (r - 1) // per_image and 65 + (r - 1) // per_image, its keypoints in the 8 cells around and
    under the projection and at most 2.7 px from it, and, masked out, image 129, which makes the rows r > 0 pairwise not disjoint.  So
    every pair (0, r) is accepted with the SAME score, row 0's own 9 px^2, and the key decides: row 1 wins, one merge.  Three image
    chunks of the meet kernel."""
    assert n_rows - 1 <= 64 * per_image and per_image <= 8
    n, hub = 130, 129
    g = CC.grid()
    K, T = (np.stack([x] * n) for x in TC.camera(500, (0, 0, 0)))
    X = (0.002, 0.002, 4)                                                  # (320.25, 240.25)
    p = TC.project(K[0], T[0], X)
    around = [(-1, -1), (0, -1), (1, -1), (-1, 0), (0, 0), (1, 0), (-1, 1), (0, 1)]
    rows, kps, obs_xy, obs_mask = [([0], X, OK)], [(0, (p + [3.0, 0.0]).astype(np.float32), 0)], [(p + [3.0, 0.0]).astype(np.float32)], [1]
    for r in range(1, n_rows):
        d = np.array(around[(r - 1) % per_image])
        corner = np.floor(p / CC.CELL) * CC.CELL + CC.CELL * d
        near = (corner + np.clip(p - corner, 0.1, CC.CELL - 0.1)).astype(np.float32)
        far = np.array([20.0 + CC.CELL * (r % 256), 20.0 + CC.CELL * (r // 256)], np.float32)
        ims = [1 + (r - 1) // per_image, 65 + (r - 1) // per_image, hub]
        rows.append((ims, X, OK))
        for i, xy in zip(ims, (near, near, far)):
            kps.append((i, xy, r))
            obs_xy.append(xy)
            obs_mask.append(i != hub)
    t = CC.assemble(n, rows, kps, K, T, np.ones(n, np.uint8), g, THRESH, 2)
    cells = set(zip(np.repeat(np.arange(n), np.diff(t["kp_offsets"])).tolist(), t["kp_cell"].tolist()))
    assert len(cells) == len(kps) and (t["kp_cell"] >= 0).all()           # distinct cells
    return with_observations(t, np.array(obs_xy, np.float32), obs_mask)


def long_and_short(seed=3):
    """a row of 70 observations (70 of 72 ring cameras) whose point merges with a row of 2 (the other two cameras)"""
    rng = np.random.default_rng(seed)
    n = 72
    K, T = BC.ring(n, seed)
    X = np.array([0.1, -0.05, 5.5])
    short = [17, 53]
    rows = [([i for i in range(n) if i not in short], X + np.array([0.002, 0, 0]), OK), (short, X - np.array([0.002, 0, 0]), OK)]
    kps, obs_xy = [], []
    for r, (ims, _, _) in enumerate(rows):
        for i in ims:
            xy = (TC.project(K[i], T[i], X) + rng.uniform(-0.7, 0.7, 2)).astype(np.float32)
            kps.append((i, xy, r))
            obs_xy.append(xy)
    t = CC.assemble(n, rows, kps, K, T, np.ones(n, np.uint8), CC.grid())
    return with_observations(t, np.array(obs_xy, np.float32), np.ones(len(obs_xy), np.uint8))


def corners(reach):
    """_completion_cases.corners (four points that project into the four corner cells of image 1) with every keypoint of image 1 held by
    a row of its own whose point is that corner's point moved by 1 mm: the corner rows meet them at the clipped edges of the grid"""
    c = CC.corners(reach)
    K, T, g = c["K"], c["T_cam_from_world"], c["grid"]
    rows = [([0], tuple(x), OK) for x in c["xyz"].astype(np.float64)]
    kps, obs_xy = [], []
    for r, (ims, X, _) in enumerate(rows):
        xy = TC.project(K[0], T[0], X).astype(np.float32)
        if CC.cell_of(xy, g) >= 0:
            kps.append((0, xy, r))
        obs_xy.append(xy)
    for k, xy in enumerate(c["keypoints"]):
        near = int(np.argmin([np.linalg.norm(TC.project(K[1], T[1], X) - xy) for _, X, _ in rows[:4]]))
        rows.append(([1], tuple(np.asarray(rows[near][1]) + np.array([0.001, 0, 0])), OK))
        kps.append((1, xy, len(rows) - 1))
        obs_xy.append(xy)
    t = CC.assemble(2, rows, kps, K, T, np.ones(2, np.uint8), g, c["thresh_px"], reach)
    mask = np.ones(len(rows), np.uint8)
    return with_observations(t, np.array(obs_xy, np.float32), mask)


# ---- a synthetic pair list whose tracks are twins ----------------------------------------------------------------------------------------
def twin_atlas(device):
    """KeypointAtlas over the pair list of _triangulation_cases.sfm_scene() (5 cameras, 60 points, every pair of images a row) with every
    third point cut in two PROPER tracks: its matches stay in the rows among images 0-2 and in row (3, 4), and are dropped from the six
    rows that join the two groups.  Both halves triangulate a point.  -> (SfmResult, scene, the cut points)."""
    import torch
    from loftr_amd import KeypointAtlas
    s = TC.sfm_scene()
    n_points = len(s["X"])
    cut = np.arange(n_points) % CC.SPLIT_EVERY == 0
    atlas = KeypointAtlas(5, TC.SFM_HW, TC.SFM_CELL, device=device)
    dev = torch.device(device)
    for a, b, k0, k1, c in s["rows"]:
        keep = ~cut if a < 3 <= b else np.ones(n_points, bool)
        data = {"mkpts0_f": torch.from_numpy(k0[keep]).to(dev), "mkpts1_f": torch.from_numpy(k1[keep]).to(dev),
                "mconf": torch.from_numpy(c[keep]).to(dev), "m_bids": torch.zeros(int(keep.sum()), dtype=torch.int64, device=dev)}
        atlas.add(np.array([[a, b]]), data)
    return atlas.finalize(), s, cut
