"""SHA-256 digests of what the host routine with one radial coefficient per group -- loftr_bundle_adjust_radial_host, DESIGN §18.4 --
returns on the scenes of tests/_bundle_radial_cases.py and on the cases of its rule.

    python tests/golden/make_bundle_radial_parent_digest.py [--root CHECKOUT] [--write]

Run with --root pointing at a checkout (with its own library built) of the commit BEFORE a mode became a row of traits from the C entry
points down to the kernels, and --write, it produced tests/golden/bundle_radial_parent_digest.json; tests/test_bundle_radial.py
recomputes the digests on the current build and compares: the radial mode must return the same bits as it did then.  Every output tensor
(K, radial and the five decisions included), the 16 counts and a hash of the inputs are covered."""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
OUT = os.path.join(HERE, "bundle_radial_parent_digest.json")
# case: (scene, variant, huber_px, max_iters, (radial_lo, radial_hi))
CASES = {"one_a": ("one_a", None, 0.0, 30, (-1.0, 1.0)), "one_b": ("one_b", None, 0.0, 30, (-1.0, 1.0)),
         "bodies": ("bodies", None, 0.0, 30, (-1.0, 1.0)), "huber": ("huber", None, 2.0, 100, (-1.0, 1.0)),
         "singletons_a": ("one_a", "singletons", 0.0, 30, (-1.0, 1.0)),            # every image its own group
         "mixed_mask": ("bodies", "mixed", 0.0, 30, (-1.0, 1.0)),                  # distinct starts; images 3 and 4 do not refine
         "out_of_bounds": ("bodies", None, 0.0, 60, (-0.01, 0.01)),                # the first trial leaves the bounds and is rejected
         "known_poses": ("one_b", "known", 0.0, 30, (-1.0, 1.0))}                  # every pose fixed: zero free cameras, one group


def sibling(name):
    """The digest script `name` of this folder as a module (its raw() and groups() lay the arguments out)."""
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def digests(only=None):
    """{case: {output name: sha256 hex, 'inputs': sha256 hex}} with the loftr_amd that is importable now; every flag of refine_focal
    set.  only: the cases wanted."""
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    import _bundle_radial_cases as RC
    from loftr_amd import ops
    old, shared = sibling("make_bundle_parent_digest"), sibling("make_bundle_shared_parent_digest")
    out = {}
    for case, (name, variant, huber, iters, bounds) in CASES.items():
        if only is not None and case not in only:
            continue
        s = dict(RC.radial_case(name))
        n = len(s["K"])
        ids, start, mask = s["camera_ids"], s["radial"].astype(np.float64), np.ones(n, np.uint8)
        if variant == "singletons":
            ids = np.arange(n)[::-1].copy()
        if variant == "mixed":
            start = np.linspace(-0.02, 0.02, n)
            mask[[3, 4]] = 0
        if variant == "known":
            s.update(T_cam_from_world=s["T_true"].copy(), fixed=np.ones(n, bool))
        args = old.raw(s) + [np.ones(n, np.uint8)] + shared.groups(ids) + [np.ascontiguousarray(start), mask]
        res = ops.bundle_adjust_radial_host(*args, huber, iters, 30, 1e-2, 1e-9, 20, 0.5, 2.0, *bounds)
        out[case] = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(res.items())}
        out[case]["inputs"] = hashlib.sha256(b"".join(a.tobytes() for a in args) + np.float64(bounds).tobytes()).hexdigest()
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
