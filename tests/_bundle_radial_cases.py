"""Inputs of the radial tests (tests/test_bundle_radial.py on the CPU, tests/test_hip_bundle_radial.py on the GPU): the scenes
of _bundle_shared_cases -- fx, skew and fy off by one factor per camera -- observed again through a lens with one radial coefficient per
camera, x_d = x (1 + k r^2) on normalised coordinates.  The observation is computed here in numpy from the true cameras and points, not
with the library's distort routine."""
import functools

import numpy as np

import _bundle_shared_cases as SC

K_ONE = -0.12                                   # every image of one_a / one_b
K_BODIES = np.array([-0.12, 0.08, -0.05])       # groups 0, 1, 2 of BODIES


def observe(K, T, X, k):
    """The pixel of X [3] in the camera (K [3,3], T [4,4]) with the coefficient k."""
    Y = T[:3, :3] @ X + T[:3, 3]
    x = Y[:2] / Y[2]
    xd = x * (1.0 + k * (x @ x))
    return K[:2, :2] @ xd + K[:2, 2]


def distort_scene(s, k_per_image, seed=41):
    """A copy of the scene dict s (of _bundle_shared_cases: K_true, T_true, X_true) whose obs_xy are the true points seen by the true
    cameras through k_per_image [n], with 0.5 px Gaussian noise.  The outliers of scene_huber keep their displacement.  Adds k_true [n],
    radial (the start: zeros) and r_max, the largest undistorted radius of an observation."""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    rng, k_true = np.random.default_rng(seed), np.asarray(k_per_image, np.float64)
    track = np.repeat(np.arange(len(s["offsets"]) - 1), np.diff(s["offsets"]))
    xy, r_max = np.zeros((len(track), 2)), 0.0
    for o, (im, t) in enumerate(zip(s["obs_image"], track)):
        xy[o] = observe(s["K_true"][im], s["T_true"][im], s["X_true"][t], k_true[im]) + 0.5 * rng.standard_normal(2)
        Y = s["T_true"][im, :3, :3] @ s["X_true"][t] + s["T_true"][im, :3, 3]
        r_max = max(r_max, float(np.linalg.norm(Y[:2] / Y[2])))
    if "outlier" in s:                              # the displacement scene_huber gave them, on the new pixels
        import _bundle_cases as BC
        xy[s["outlier"]] += (s["obs_xy"].astype(np.float64) - BC.scene_b()["obs_xy"].astype(np.float64))[s["outlier"]]
    s["obs_xy"] = xy.astype(np.float32)
    s["k_true"], s["radial"], s["r_max"] = k_true, np.zeros(len(k_true)), r_max
    return s


@functools.lru_cache(maxsize=None)
def radial_case(name):
    """'one_a' / 'one_b': every image one camera with k = -0.12.  'bodies' / 'huber': scene B / its Huber variant in SC.BODIES with
    k = -0.12, 0.08, -0.05 for the groups 0, 1, 2.  Scene B reaches r = 1.58 in its widest view, where 1 + 3 k r^2 = 0.10 for k = -0.12:
    still on the monotone branch of r (1 + k r^2), so every observation has exactly one undistorted point."""
    s = SC.shared_case(name)
    k = np.full(len(s["K"]), K_ONE) if name in ("one_a", "one_b") else K_BODIES[SC.BODY_GROUP]
    return distort_scene(s, k)
