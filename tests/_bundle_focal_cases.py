"""Inputs of the focal-refinement tests (tests/test_bundle_focal.py on the CPU, tests/test_hip_bundle_focal.py on the GPU): the scenes of
_bundle_cases with the focal entries of every free camera's K off by 4-10 %."""
import functools

import numpy as np

import _bundle_cases as BC


def detune(s, seed=5):
    """A copy of scene dict s whose K[:,0,0], K[:,0,1] and K[:,1,1] are multiplied by fac: 1 for images 0 and 1, 1 +- U(0.04, 0.10) for
    the others.  Adds K_true (the K of s) and fac."""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    n, rng = len(s["K"]), np.random.default_rng(seed)
    fac = np.ones(n)
    fac[2:] = 1 + rng.choice([-1, 1], n - 2) * rng.uniform(0.04, 0.10, n - 2)
    s["K_true"] = s["K"].copy()
    s["K"][:, 0, 0] *= fac
    s["K"][:, 0, 1] *= fac
    s["K"][:, 1, 1] *= fac
    s["fac"] = fac
    return s


@functools.lru_cache(maxsize=None)
def focal_case(scene):
    """scene: 'scene_a', 'scene_b' or 'scene_huber' of _bundle_cases, detuned."""
    return detune(getattr(BC, scene)())


def focal_errors(K, K_true, which):
    """The largest relative error of fx over the cameras `which`."""
    which = np.asarray(which, bool)
    return float(np.abs(K[which, 0, 0] / K_true[which, 0, 0] - 1).max()) if which.any() else 0.0


def projections(s, K, T, xyz, use):
    """BC.projections under the intrinsics K."""
    return BC.projections(dict(s, K=K), T, xyz, use)
