"""Inputs shared by the keypoint-atlas tests (tests/test_atlas.py on the CPU, tests/test_hip_atlas.py on the GPU).

A case is (n_images, image_hw, rows) with rows = [(a, b, mkpts0 [M,2] f32, mkpts1 [M,2] f32, mconf [M] f32, mask [M] bool or None)];
``chunks(rows, size)`` groups consecutive rows into the arguments of one ``KeypointAtlas.add`` each."""
import functools

import numpy as np
import torch

FIELDS = ("kp_offsets", "keypoints", "score", "n_obs", "row_offsets", "matches", "match_conf", "track_id", "track_len", "track_ok", "row_images")


def chunks(rows, size):
    """-> list of (image_ids [n,2], mkpts0, mkpts1, mconf, m_bids, mask or None)"""
    out = []
    for s in range(0, len(rows), size):
        part = rows[s:s + size]
        ids = np.array([[r[0], r[1]] for r in part], np.int64).reshape(-1, 2)
        cat = lambda i, shape: np.concatenate([r[i] for r in part]) if part else np.zeros(shape, np.float32)
        bids = np.concatenate([np.full(len(r[4]), i, np.int64) for i, r in enumerate(part)])
        masked = any(r[5] is not None for r in part)
        mask = np.concatenate([np.ones(len(r[4]), bool) if r[5] is None else r[5] for r in part]) if masked else None
        out.append((ids, cat(2, (0, 2)), cat(3, (0, 2)), cat(4, (0,)), bids, mask))
    return out


def run(n_images, image_hw, rows, cell_px=2.0, device="cpu", chunk=8, min_track_len=2, capacity=4096, **kw):
    """Feed a case to a KeypointAtlas on `device` -> to_host() dict."""
    from loftr_amd import KeypointAtlas
    atlas = KeypointAtlas(n_images, image_hw, cell_px, device=device, capacity=capacity, **kw)
    dev = torch.device(device)
    for ids, k0, k1, c, bids, mask in chunks(rows, chunk):
        data = {"mkpts0_f": torch.from_numpy(k0).to(dev), "mkpts1_f": torch.from_numpy(k1).to(dev), "mconf": torch.from_numpy(c).to(dev),
                "m_bids": torch.from_numpy(bids).to(dev)}
        atlas.add(ids, data, mask=None if mask is None else torch.from_numpy(mask).to(dev))
    return atlas.finalize(min_track_len=min_track_len).to_host()


def assert_same(got, want, what=""):
    for k in FIELDS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w), (what, k)
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])


# ---- (a) random: 12 images of 37 x 53 (cell 2: a 19 x 27 grid, its width no multiple of a wave), 30 rows of 0..500 matches, confidences
#      from {0, 0.25, 0.5, 1} (ties everywhere), a duplicated row, a reversed row, a row with no match
RANDOM_HW = (37, 53)


@functools.lru_cache(maxsize=None)
def random_case():
    rng = np.random.default_rng(20)
    H, W = RANDOM_HW
    rows = []
    for r in range(28):
        a = int(rng.integers(0, 12))
        b = int((a + rng.integers(1, 12)) % 12)
        M = 0 if r == 5 else int(rng.integers(1, 501))
        k0 = (rng.random((M, 2)) * [W, H]).astype(np.float32)
        if r % 3 == 0:
            k0 = (np.floor(k0 / 8) * 8).astype(np.float32)            # side 0 on the coarse grid, as LoFTR leaves it
        k1 = (rng.random((M, 2)) * [W, H]).astype(np.float32)
        c = rng.choice(np.array([0, 0.25, 0.5, 1.0], np.float32), M)
        rows.append((a, b, k0, k1, c, None))
    a, b, k0, k1, c, _ = rows[2]
    rows.insert(9, (a, b, k0.copy(), k1.copy(), c.copy(), None))      # duplicated row
    a, b, k0, k1, c, _ = rows[3]
    rows.insert(17, (b, a, k1.copy(), k0.copy(), c.copy(), None))     # reversed row
    assert len(rows) == 30
    return 12, RANDOM_HW, rows


# ---- (c) invalid observations, with the counts written out
def invalid_case():
    H, W = 20.0, 30.0
    nan, inf = np.nan, np.inf
    #          x0    y0    x1    y1    conf  mask
    table = [(1.0, 1.0, 2.0, 2.0, 0.9, 1),          # valid
             (nan, 1.0, 2.0, 2.0, 0.9, 1),          # NaN coordinate                  -> nonfinite
             (1.0, 1.0, 2.0, inf, 0.9, 1),          # inf coordinate                  -> nonfinite
             (-0.5, 1.0, 2.0, 2.0, 0.9, 1),         # negative coordinate             -> outside
             (1.0, 1.0, W, 2.0, 0.9, 1),            # x == W (W * inv == gw exactly)  -> outside
             (1.0, H, 2.0, 2.0, 0.9, 1),            # y == H                          -> outside
             (1.0, 1.0, 2.0, 2.0, nan, 1),          # NaN conf                        -> nonfinite
             (1.0, 1.0, 2.0, 2.0, -0.1, 1),         # negative conf                   -> negative_conf
             (5.0, 5.0, 6.0, 6.0, 0.8, 0),          # masked out                      -> masked
             (nan, 5.0, 6.0, 6.0, -1.0, 0),         # masked AND broken: the mask comes first
             (-1.0, 5.0, 6.0, 6.0, -1.0, 1),        # negative conf AND outside: the confidence comes first
             (29.99, 19.99, 0.0, 0.0, 0.0, 1),      # valid: the last cell, the first cell, confidence zero
             (3.0, 3.0, 4.0, 4.0, -0.0, 1)]         # valid: -0.0 is not negative
    t = np.array(table, np.float64)
    row0 = (0, 1, t[:, 0:2].astype(np.float32), t[:, 2:4].astype(np.float32), t[:, 4].astype(np.float32), t[:, 5] != 0)
    k = np.array([[7.0, 7.0], [9.0, 9.0]], np.float32)
    row1 = (1, 2, k, k + 2, np.array([0.5, 0.5], np.float32), np.zeros(2, bool))       # an empty mask: the row keeps nothing
    expect = dict(n_matches=15, n_valid=3, n_masked=4, n_nonfinite=3, n_negative_conf=2, n_outside=3, n_rows=2, n_images=3, n_keypoints=6,
                  n_kept=3, n_tracks=3)
    return 3, (H, W), [row0, row1], expect


# ---- (d) tracks with hand-written labels
def track_case():
    """19 images.  A chain over the ring of images 0..8 (one keypoint each; rows in a scrambled order so that roots get hooked under
    roots that move later), a star around image 9 (leaves 10, 11, 12), a component through images 13, 14, 15 that returns to image 13 in
    ANOTHER cell (two keypoints of image 13: inconsistent), and a plain pair 16-17.  Image 18 has no match.
    Global keypoints: image i < 13 -> i; image 13 -> 13 (5, 5) and 14 (11, 11); image 14 -> 15; 15 -> 16; 16 -> 17; 17 -> 18."""
    p, q = np.array([[5.0, 5.0]], np.float32), np.array([[11.0, 11.0]], np.float32)
    one = np.array([1.0], np.float32)
    rows = [(i, i + 1, p, p, one, None) for i in (3, 0, 6, 1, 7, 4, 2, 5)]
    rows += [(9, 10, p, p, one, None), (11, 9, p, p, one, None), (9, 12, p, p, one, None)]
    rows += [(13, 14, p, p, one, None), (14, 15, p, p, one, None), (15, 13, p, q, one, None)]
    rows += [(17, 16, p, p, one, None)]
    want = {2: dict(track_id=[0] * 9 + [1] * 4 + [2] * 4 + [3] * 2, track_len=[9, 4, 4, 2], track_ok=[True, True, False, True]),
            3: dict(track_id=[0] * 9 + [1] * 4 + [2] * 4 + [-1] * 2, track_len=[9, 4, 4], track_ok=[True, True, False])}
    return 19, (16.0, 16.0), rows, want


# ---- (e) table stress
STRESS_HW = (6002.0, 8192.0)          # cell 2: 3001 x 4096 cells per image


@functools.lru_cache(maxsize=None)
def stress_case():
    """Row 0: 3000 matches whose side-a cells are the multiples of 4096 of the image's grid (a column of points: keys and cells that
    differ only above bit 12), side b scattered.  Row 1: 3000 matches that all land in ONE cell on side b (one survives).  Rows 2..41:
    the same 40 keypoints matched in 40 rows (table keys that differ only in the row bits, above bit 33)."""
    rng = np.random.default_rng(7)
    n = 3000
    col = np.stack([np.full(n, 1.0), 2.0 * np.arange(n) + 1.0], 1).astype(np.float32)
    scat = (rng.random((n, 2)) * [8192, 6002]).astype(np.float32)
    conf = rng.choice(np.array([0.25, 0.5, 1.0], np.float32), n)
    rows = [(0, 1, col, scat, conf, None)]
    one_cell = (np.array([[100.0, 200.0]]) + rng.random((n, 2)) * 1.99).astype(np.float32)
    rows.append((1, 0, scat[::-1].copy(), one_cell, conf, None))
    grid = np.stack([16.0 * np.arange(40) + 3.0, np.full(40, 4001.0)], 1).astype(np.float32)
    for r in range(40):
        rows.append((r % 2, 1 - r % 2, grid, grid, np.full(40, 0.5, np.float32), None))
    return 2, STRESS_HW, rows
