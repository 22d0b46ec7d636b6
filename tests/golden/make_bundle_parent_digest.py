"""SHA-256 digests of what loftr_bundle_adjust_host (fixed intrinsics) returns on the scenes of tests/_bundle_cases.py.

    python tests/golden/make_bundle_parent_digest.py [--root CHECKOUT] [--write]

Run with --root pointing at a checkout (with its library built) of the commit BEFORE the camera block became a template, and --write,
it produced tests/golden/bundle_parent_digest.json; tests/test_bundle_focal.py recomputes the digests on the current build and compares:
the 6-wide path must return the same bits as it did then.  Every output tensor and the 16 counts are covered."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
OUT = os.path.join(HERE, "bundle_parent_digest.json")
CASES = (("scene_a", 0.0, 30), ("scene_b", 0.0, 30), ("scene_huber", 2.0, 100), ("hand_problem", 0.0, 30))    # scene, huber_px, max_iters


def raw(s):
    """The arguments of ops.bundle_adjust_host for scene dict s (the observations grouped by image with a stable sort)."""
    import _bundle_cases as BC
    a = [np.ascontiguousarray(s[k]) for k in BC.ARGS]
    a[3] = a[3].astype(np.uint8)
    n = len(s["K"])
    cam_obs = np.argsort(a[1], kind="stable").astype(np.int32)
    cam_offsets = np.zeros(n + 1, np.int64)
    cam_offsets[1:] = np.cumsum(np.bincount(a[1], minlength=n))
    return a + [s["fixed"].astype(np.uint8), cam_offsets, cam_obs]


def digests():
    """{case: {output name: sha256 hex}} with the loftr_amd that is importable now."""
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    import _bundle_cases as BC
    from loftr_amd import ops
    out = {}
    for name, huber, iters in CASES:
        s = getattr(BC, name)()
        s = s[0] if isinstance(s, tuple) else s
        args = raw(s)
        res = ops.bundle_adjust_host(*args, huber, iters, 30, 1e-2, 1e-9)
        out[name] = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(res.items())}
        out[name]["inputs"] = hashlib.sha256(b"".join(a.tobytes() for a in args)).hexdigest()     # (tells a changed scene from a changed result)
    return out


if __name__ == "__main__":
    root = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else os.path.dirname(TESTS)
    sys.path.insert(0, os.path.abspath(root))
    d = digests()
    text = json.dumps(d, indent=1, sort_keys=True) + "\n"
    if "--write" in sys.argv:
        with open(OUT, "w") as fh:
            fh.write(text)
    print(text, end="")
