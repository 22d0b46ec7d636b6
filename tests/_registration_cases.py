"""Inputs shared by the registration tests (tests/test_registration.py on the CPU, tests/test_hip_registration.py on the GPU): every
case is a dict of the numpy inputs of ops.register_corr_host (the grouping made by the oracle's groups()) plus min_corr."""
import numpy as np

import _bundle_cases as BC
import _registration_oracle as O

NAMES = ("offsets", "obs_image", "obs_xy", "xyz", "status", "posed", "cam_offsets", "cam_obs")
OUT = ("n_corr", "cand_rank", "cand_image", "cand_offsets", "corr_xyz", "corr_xy", "corr_bid", "corr_obs", "counts")
RANK_BLOCK = 256                                                        # b: the images reg_rank_kernel takes per step


def case(offsets, obs_image, obs_xy, xyz, status, posed, min_corr=4):
    obs_image = np.asarray(obs_image, np.int32).reshape(-1)
    N, n = len(obs_image), len(posed)
    cam_offsets, cam_obs = O.groups(obs_image, n) if N == 0 or (obs_image.min() >= 0 and obs_image.max() < n) else (np.zeros(n + 1, np.int64), np.zeros(N, np.int32))
    return dict(offsets=np.asarray(offsets, np.int64), obs_image=obs_image, obs_xy=np.asarray(obs_xy, np.float32).reshape(N, 2),
                xyz=np.asarray(xyz, np.float32).reshape(-1, 3), status=np.asarray(status, np.uint8), posed=np.asarray(posed, np.uint8),
                cam_offsets=cam_offsets, cam_obs=cam_obs, min_corr=min_corr)


def args(c):
    return [c[k] for k in NAMES] + [c["min_corr"]]


def from_scene(s, seed, min_corr, p_posed=0.4):
    """A bundle scene with a random posed mask, a tenth of the tracks not ok and a few NaN points."""
    rng = np.random.default_rng(seed)
    T, n = len(s["offsets"]) - 1, len(s["K"])
    status = np.where(rng.random(T) < 0.1, rng.integers(1, 5, T), 0)
    xyz = s["xyz"].copy()
    xyz[rng.random(T) < 0.03, rng.integers(0, 3)] = np.nan
    return case(s["offsets"], s["obs_image"], s["obs_xy"], xyz, status, rng.random(n) < p_posed, min_corr)


def random_case(seed, n, T, max_len, min_corr=4, p_posed=0.4):
    """T tracks of 0 .. max_len observations in random images (with repetition), some tracks not ok, some numbers not finite."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, T)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    N = int(offsets[-1])
    xy = rng.uniform(0, 640, (N, 2)).astype(np.float32)
    xy[rng.random(N) < 0.02, 0] = np.nan
    xy[rng.random(N) < 0.01, 1] = np.inf
    xyz = rng.uniform(-2, 8, (T, 3)).astype(np.float32)
    xyz[rng.random(T) < 0.03, 2] = -np.inf
    xyz[rng.random(T) < 0.03, 0] = np.nan
    return case(offsets, rng.integers(0, n, N), xy, xyz, np.where(rng.random(T) < 0.1, rng.integers(1, 5, T), 0), rng.random(n) < p_posed, min_corr)


def hand():
    """6 images: 0 and 5 posed.  min_corr = 4: image 1 ends with exactly 4 correspondences (a candidate), image 2 with 3 (not one), image 3
    with 5 of which two sit in one track, image 4 with none."""
    nan, inf = np.nan, np.inf
    tracks = [  # (status, xyz, [(image, xy)])
        (0, (0, 0, 4), [(0, (1, 1)), (1, (2, 2)), (2, (3, 3)), (3, (4, 4))]),
        (0, (1, 0, 4), [(0, (1, 2)), (1, (2, 3)), (2, (3, 4)), (3, (4, 5)), (3, (4.5, 5.5))]),          # image 3 twice in one track
        (0, (2, 0, 4), [(1, (5, 5)), (2, (6, 6)), (5, (7, 7))]),
        (0, (3, 0, 4), [(1, (8, 8)), (3, (9, 9)), (0, (9, 1))]),
        (3, (4, 0, 4), [(1, (1, 9)), (2, (2, 9)), (3, (3, 9))]),                                      # a status that is not ok
        (0, (5, nan, 4), [(1, (1, 8)), (2, (2, 8)), (3, (3, 8))]),                                    # NaN in xyz
        (0, (6, 0, inf), [(1, (1, 7)), (2, (2, 7))]),                                                 # an infinity in xyz
        (0, (7, 0, 4), [(1, (nan, 7)), (2, (2, nan)), (3, (3, 6)), (4, (inf, 1))]),                   # NaN / infinity in obs_xy
        (0, (8, 0, 4), []),                                                                           # no observation
        (1, (nan, nan, nan), [(4, (5, 5)), (0, (5, 6))]),
    ]
    offsets, image, xy = [0], [], []
    for _, _, obs in tracks:
        for im, p in obs:
            image.append(im); xy.append(p)
        offsets.append(len(image))
    c = case(offsets, image, xy, [t[1] for t in tracks], [t[0] for t in tracks], [1, 0, 0, 0, 0, 1], 4)
    c["expect_n_corr"] = [0, 4, 3, 5, 0, 0]
    return c


def list_case(k, seed=41):
    """Image 1 (unposed) with a list of exactly k observations: k tracks over images (0, 1), 9 more over images (0, 2); a few tracks
    not ok, so that the ballots have holes."""
    rng = np.random.default_rng(seed + k)
    T = k + 9
    image = np.array([[0, 1]] * k + [[0, 2]] * 9, np.int32).reshape(-1)
    status = np.where(rng.random(T) < 0.2, 2, 0)
    return case(np.arange(T + 1) * 2, image, rng.uniform(0, 640, (2 * T, 2)), rng.uniform(-2, 8, (T, 3)), status, [1, 0, 0], 4)


def images_case(n, seed=43):
    """n images, 3 n tracks over images (j mod n, (j + 1) mod n): 6 observations per image, min_corr 5."""
    rng = np.random.default_rng(seed + n)
    T = 3 * n
    image = np.stack([np.arange(T) % n, (np.arange(T) + 1) % n], 1).reshape(-1)
    status = np.where(rng.random(T) < 0.1, 1, 0)
    posed = rng.random(n) < 0.3
    posed[0] = False                                                    # (so that a single image is an unposed one)
    return case(np.arange(T + 1) * 2, image, rng.uniform(0, 640, (2 * T, 2)), rng.uniform(-2, 8, (T, 3)), status, posed, 5)


def long_track(seed=47):
    """One track of 70 observations among short ones, 5 images."""
    rng = np.random.default_rng(seed)
    lens = np.array([3, 70, 2, 4, 0, 5])
    N = int(lens.sum())
    return case(np.concatenate([[0], np.cumsum(lens)]), rng.integers(0, 5, N), rng.uniform(0, 640, (N, 2)), rng.uniform(-2, 8, (6, 3)),
                np.zeros(6), [1, 0, 0, 1, 0], 4)


def edge_cases():
    """name -> case: the hand-written ones of the issue."""
    h = hand()
    base = {k: h[k] for k in NAMES + ("min_corr",)}
    out = {"hand": base,
           "all_posed": case(h["offsets"], h["obs_image"], h["obs_xy"], h["xyz"], h["status"], np.ones(6), 4),
           "none_posed": case(h["offsets"], h["obs_image"], h["obs_xy"], h["xyz"], h["status"], np.zeros(6), 4),
           "no_candidate": case(h["offsets"], h["obs_image"], h["obs_xy"], h["xyz"], h["status"], h["posed"], 6),
           "min_corr_5": case(h["offsets"], h["obs_image"], h["obs_xy"], h["xyz"], h["status"], h["posed"], 5),
           "T=0": case([0], [], np.zeros((0, 2)), np.zeros((0, 3)), [], [0, 1, 0], 4),
           "N=0": case([0, 0, 0], [], np.zeros((0, 2)), np.ones((2, 3)), [0, 0], [0, 1, 0], 4),
           "n=0": case([0], [], np.zeros((0, 2)), np.zeros((0, 3)), [], [], 4)}
    return out


def bad_inputs():
    """[(name, case, bit)]: inputs that raise one error bit."""
    h = hand()
    base = {k: h[k] for k in NAMES + ("min_corr",)}
    out = []
    for name, image in (("image_high", 6), ("image_negative", -1)):
        c = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in base.items()}
        c["obs_image"][7] = image
        out.append((name, c, 1))
    for name, edit in (("offsets_start", (0, 1)), ("offsets_end", (-1, 99)), ("offsets_descend", (2, 3)), ("offsets_short", (-1, 20))):
        c = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in base.items()}
        c["offsets"][edit[0]] = edit[1]
        out.append((name, c, 2))
    for name, key, idx, val in (("groups_swapped", "cam_obs", None, None), ("groups_offsets", "cam_offsets", 2, 9), ("groups_start", "cam_offsets", 0, 1),
                                ("groups_end", "cam_offsets", -1, 5), ("groups_index", "cam_obs", 3, 999), ("groups_negative", "cam_obs", 3, -2),
                                ("groups_repeat", "cam_obs", 1, int(base["cam_obs"][0]))):
        c = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in base.items()}
        if idx is None:
            c[key][[0, 1]] = c[key][[1, 0]]
        else:
            c[key][idx] = val
        out.append((name, c, 4))
    return out


def trimmed(out):
    """The outputs with the table cut to C rows and P candidates, as Python hands them on."""
    C, P = int(out["counts"][0]), int(out["counts"][1])
    cut = {"cand_image": P, "cand_offsets": P + 1, "corr_xyz": C, "corr_xy": C, "corr_bid": C, "corr_obs": C}
    return {k: (v[:cut[k]] if k in cut else v) for k, v in out.items()}


def same(a, b):
    """Bit equality of two float arrays (NaN included) or plain equality of integer ones."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def scene_cases():
    return {"scene_a": from_scene(BC.scene_a(), 1, 30), "scene_a_min4": from_scene(BC.scene_a(), 2, 4, 0.6),
            "scene_b": from_scene(BC.scene_b(), 3, 55), "scene_b_min4": from_scene(BC.scene_b(), 4, 4, 0.2)}
