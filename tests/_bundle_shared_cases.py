"""Inputs of the shared-focal tests (tests/test_bundle_shared.py on the CPU, tests/test_hip_bundle_shared.py on the GPU): the
scenes of _bundle_cases with fx, skew and fy off by one factor per GROUP of images (one physical camera), the fixed-pose images 0 and 1
included: they stay at the true pose, but their K is as wrong as the rest of their group's."""
import functools

import numpy as np

import _bundle_cases as BC

# scene B's 12 images in three bodies of 5 / 4 / 3, interleaved, under sparse unsorted ids; images 0 and 1 are in different bodies
BODIES = np.array([7, 1000, 3, 7, 1000, 3, 7, 1000, 3, 7, 1000, 7], np.int64)
BODY_GROUP = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 0], np.int32)           # what the relabelling makes of them
THIN_CAP = 19                                                                   # active observations an image keeps at most in `thin`


def detune_groups(s, ids, seed=5):
    """A copy of scene dict s whose K[:,0,0], K[:,0,1] and K[:,1,1] are multiplied by one factor 1 +- U(0.04, 0.10) per distinct id (in
    the order of the ids' first images).  Adds K_true, fac [n], camera_ids."""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    rng, ids = np.random.default_rng(seed), np.asarray(ids, np.int64)
    order = list(dict.fromkeys(ids.tolist()))
    per = {i: 1 + rng.choice([-1, 1]) * rng.uniform(0.04, 0.10) for i in order}
    fac = np.array([per[i] for i in ids.tolist()])
    s["K_true"] = s["K"].copy()
    for r, c in ((0, 0), (0, 1), (1, 1)):
        s["K"][:, r, c] *= fac
    s["fac"], s["camera_ids"] = fac, ids
    return s


def thin_mask(s, cap=THIN_CAP):
    """The observation mask of s with whole tracks dropped, greedily in track order, so that no image keeps more than `cap`."""
    cnt, mask, off = np.zeros(len(s["K"]), int), np.zeros(len(s["obs_image"]), bool), s["offsets"]
    for t in range(len(off) - 1):
        ims = s["obs_image"][off[t]:off[t + 1]]
        if (cnt[ims] < cap).all():
            mask[off[t]:off[t + 1]] = True
            cnt[ims] += 1
    return mask


@functools.lru_cache(maxsize=None)
def shared_case(name):
    """'one_a' / 'one_b': scene A / B, every image one camera.  'bodies': scene B in BODIES.  'huber': scene_huber in BODIES.
    'thin': 'bodies' with thin_mask (every image keeps 16-19 observations: fewer than the default min_focal_obs = 20)."""
    if name in ("one_a", "one_b"):
        s = BC.scene_a() if name == "one_a" else BC.scene_b()
        return detune_groups(s, np.zeros(len(s["K"]), np.int64))
    if name == "bodies":
        return detune_groups(BC.scene_b(), BODIES)
    if name == "huber":
        return detune_groups(BC.scene_huber(), BODIES)
    if name == "thin":
        s = detune_groups(BC.scene_b(), BODIES)
        s["obs_mask"] = thin_mask(s)
        return s
    raise KeyError(name)


def thin_counts():
    s = shared_case("thin")
    return np.bincount(s["obs_image"][s["obs_mask"]], minlength=len(s["K"]))
