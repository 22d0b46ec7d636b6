"""Inputs of the track-refinement tests: the point pairs of the centre rule, and hand-built SfmResults for the planner."""
import numpy as np
import torch

# geometry of the centre cases: two maps of different extents (fine 32 x 48 over coarse 8 x 12; fine 24 x 40 over coarse 6 x 10)
HW0_F, HW0_C, HW1_F, HW1_C, STRIDE, S = (32, 48), (8, 12), (24, 40), (6, 10), 4, 2.0
N_PAIRS = 3
SCALE0 = np.array([[1.9, 1.9], [1.0, 1.0], [1.25, 1.5]], np.float32)
SCALE1 = np.array([[1.25, 1.5], [1.0, 1.0], [0.7, 2.0]], np.float32)


def centre_points():
    """(pts0, pts1, b_ids): every row pairs a point of interest on side 0 with another on side 1; b_ids skip pair 1."""
    below = float(np.nextafter(np.float32(9.0), np.float32(0.0)))
    xs = [0.0, 8.0, 88.0, 56.0,                                         # exactly on cell centres (8 * cell)
          1.0, 9.0, below, 3.0, 61.0,                                   # x.5 fine pixels (the rounding rule) and just below one
          -0.9, -1.0, -3.0, -1e30,                                      # negative
          94.0, 95.0, 96.0, 1000.0, 1e30, 62.0, 63.9]                   # the far edge and beyond, on both maps
    ys = [8.0, 0.0, 56.0, 40.0, 5.0, 1.0, 9.0, below, 47.0, -2.5, 62.0, 63.0, 64.0, 46.0, 200.0, -1.0, 30.0, 31.0, 7.0, 1e30]
    pts0 = np.array(list(zip(xs, ys)), np.float32)
    pts1 = np.array(list(zip(ys, xs[::-1])), np.float32)
    bad = np.array([[np.nan, 4.0], [4.0, np.inf], [-np.inf, 4.0], [4.0, 4.0], [4.0, 4.0], [4.0, 4.0]], np.float32)
    bad1 = np.array([[4.0, 4.0], [4.0, 4.0], [4.0, 4.0], [4.0, np.nan], [np.inf, 4.0], [4.0, -np.inf]], np.float32)
    pts0, pts1 = np.concatenate([pts0, bad[:3], pts0[:8], bad[3:]]), np.concatenate([pts1, bad1[:3], pts1[:8], bad1[3:]])
    M = len(pts0)
    b_ids = np.where(np.arange(M) < M // 2, 0, 2).astype(np.int64)
    return pts0, pts1, b_ids


# ---- hand-built results: tracks as lists of (image, score); the keypoints of an image in the order they are listed ----------------
SCENE5 = dict(n_images=5, tracks=[
    ([(0, .30), (1, .40), (2, .95), (3, .20), (4, .10)], True),         # 0: a chain over the 5 images, reference in image 2
    ([(0, .90), (1, .50), (2, .60), (3, .70)], True),                   # 1: a star around image 0
    ([(1, .50), (2, .90), (3, .90)], True),                             # 2: a score tie: the smaller keypoint (image 2) is the reference
    ([(0, .80), (1, .70)], True),                                       # 3: obs_mask leaves one observation
    ([(0, .60), (0, .65), (1, .50)], False),                            # 4: visits image 0 twice
    ([(2, .85), (4, .15)], True),                                       # 5: a second job for the pair (2, 4)
], loose=[(0, .1), (3, .2), (4, .3), (4, .4)])

SCENE4 = dict(n_images=4, tracks=[
    ([(0, .30), (1, .40), (2, .95), (3, .20)], True),
    ([(0, .90), (1, .50), (2, .60), (3, .70)], True),
    ([(1, .50), (2, .90), (3, .90)], True),
    ([(0, .60), (0, .65), (1, .50)], False),
    ([(2, .85), (3, .15)], True),
    ([(1, .75), (0, .10)], True),
], loose=[(0, .1), (3, .2)])


def build_sfm(scene, device="cpu", image_hw=(64, 96), seed=0):
    """SfmResult with the tracks of `scene`; keypoint positions are seeded, inside the image, off the fine grid.  Without matches: the
    planner, the triangulation and the guards read keypoints and track arrays only."""
    from loftr_amd import SfmResult
    n = scene["n_images"]
    per_image = [[] for _ in range(n)]
    for t, (obs, _) in enumerate(scene["tracks"]):
        for im, sc in obs:
            per_image[im].append((t, sc))
    for im, sc in scene["loose"]:
        per_image[im].append((-1, sc))
    kp_offsets = np.cumsum([0] + [len(p) for p in per_image]).astype(np.int64)
    flat = [x for p in per_image for x in p]
    K = len(flat)
    rng = np.random.default_rng(seed)
    H, W = image_hw
    keypoints = np.stack([rng.uniform(3, W - 4, K), rng.uniform(3, H - 4, K)], 1).astype(np.float32)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(device)
    sfm = SfmResult({}, kp_offsets=t(kp_offsets, np.int64), keypoints=t(keypoints, np.float32), score=t([x[1] for x in flat], np.float32),
                    n_obs=t(np.ones(K), np.int32), row_offsets=t([0], np.int64), matches=t(np.zeros((0, 2)), np.int32),
                    match_conf=t(np.zeros(0), np.float32), track_id=t([x[0] for x in flat], np.int32),
                    track_len=t([len(o) for o, _ in scene["tracks"]], np.int32), track_ok=t([ok for _, ok in scene["tracks"]], bool),
                    row_images=t(np.zeros((0, 2)), np.int32))
    sfm.image_hw, sfm.cell_px = tuple(image_hw), 2.0
    return sfm
