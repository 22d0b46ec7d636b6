"""SHA-256 digests of what the two per-image host routines -- loftr_bundle_adjust_host (6-wide) and
loftr_bundle_adjust_focal_host (7-wide, §18.1) -- return on scenes A, B, Huber and the hand problem of tests/_bundle_cases.py.

    python tests/golden/make_bundle_focal_parent_digest.py [--root CHECKOUT] [--write]

Run with --root pointing at a checkout (with its library built) of the commit BEFORE the grouped focal step (§18.2) was added, and
--write, it produced tests/golden/bundle_focal_parent_digest.json; tests/test_bundle_shared.py recomputes the digests on the current
build and compares: both per-image paths must return the same bits as they did then.  Every output tensor and the 16 counts are covered."""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
OUT = os.path.join(HERE, "bundle_focal_parent_digest.json")
CASES = (("scene_a", 0.0, 30, 20), ("scene_b", 0.0, 30, 20), ("scene_huber", 2.0, 100, 20), ("hand_problem", 0.0, 30, 1))   # ..., min_focal_obs


def _sha(v):
    return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()


def digests():
    """{case: {'wide6' / 'wide7': {output name: sha256 hex}, 'inputs': sha256 hex}} with the loftr_amd that is importable now.  The 7-wide
    call runs on the detuned scene of tests/_bundle_focal_cases.py with every flag set."""
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    import _bundle_cases as BC
    import _bundle_focal_cases as FC
    from loftr_amd import ops
    spec = importlib.util.spec_from_file_location("make_bundle_parent_digest", os.path.join(HERE, "make_bundle_parent_digest.py"))
    old = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(old)
    out = {}
    for name, huber, iters, min_obs in CASES:
        s = getattr(BC, name)()
        s = s[0] if isinstance(s, tuple) else s
        args6, args7 = old.raw(s), old.raw(FC.detune(s))
        r6 = ops.bundle_adjust_host(*args6, huber, iters, 30, 1e-2, 1e-9)
        r7 = ops.bundle_adjust_focal_host(*args7, np.ones(len(s["K"]), np.uint8), huber, iters, 30, 1e-2, 1e-9, min_obs, 0.5, 2.0)
        out[name] = {"wide6": {k: _sha(v) for k, v in sorted(r6.items())}, "wide7": {k: _sha(v) for k, v in sorted(r7.items())},
                     "inputs": hashlib.sha256(b"".join(a.tobytes() for a in args6 + args7)).hexdigest()}
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
