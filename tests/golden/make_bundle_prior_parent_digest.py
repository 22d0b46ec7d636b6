"""SHA-256 digests of what the host routine with position priors -- loftr_bundle_adjust_prior_host in its modes 0 (pose), 1 (focal per
image) and 2 (focal per group), DESIGN §18.3 -- returns on the scenes of tests/_bundle_prior_cases.py.

    python tests/golden/make_bundle_prior_parent_digest.py [--root CHECKOUT] [--write]

Run with --root pointing at a checkout (with its own library built) of the commit BEFORE a mode became a row of traits from the C entry
points down to the kernels, and --write, it produced tests/golden/bundle_prior_parent_digest.json; tests/test_bundle_prior.py recomputes
the digests on the current build and compares: the three modes with priors must return the same bits as they did then.  Every output
tensor (cam_prior included), the 24 counts and a hash of the inputs are covered."""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
OUT = os.path.join(HERE, "bundle_prior_parent_digest.json")
# case: (scene, mode, huber_px, max_iters, every second prior masked out)
CASES = {f"{name}_mode{mode}": (name, mode, 0.0, 30, False) for name in ("scene_a", "scene_b", "focal", "shared", "scaled") for mode in (0, 1, 2)}
CASES.update({"shared_partial_mask": ("shared", 2, 0.0, 30, True), "scene_b_partial_mask": ("scene_b", 0, 0.0, 30, True),
              "huber_mode1": ("huber", 1, 2.0, 100, False)})


def sibling(name):
    """The digest script `name` of this folder as a module (its raw() and groups() lay the arguments out)."""
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scene(name):
    import _bundle_cases as BC
    import _bundle_prior_cases as PC
    return PC.with_priors(BC.scene_huber()) if name == "huber" else PC.prior_case(name)


def digests(only=None):
    """{case: {output name: sha256 hex, 'inputs': sha256 hex}} with the loftr_amd that is importable now; every flag of refine_focal
    set; the groups are the scene's camera_ids where it has them and image i in group i % 3 where not.  only: the cases wanted."""
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    from loftr_amd import ops
    old, shared = sibling("make_bundle_parent_digest"), sibling("make_bundle_shared_parent_digest")
    out = {}
    for case, (name, mode, huber, iters, partial) in CASES.items():
        if only is not None and case not in only:
            continue
        s = scene(name)
        n = len(s["K"])
        mask = s["prior_mask"].astype(np.uint8)
        if partial:
            mask[1::2] = 0
        args = old.raw(s) + [np.ones(n, np.uint8)] + shared.groups(s.get("camera_ids", np.arange(n) % 3))
        prior = [np.ascontiguousarray(s["prior_xyz"], np.float64), np.full((n, 3), s["prior_sigma"], np.float64), mask]
        res = ops.bundle_adjust_prior_host(mode, *args, *prior, huber, iters, 30, 1e-2, 1e-9, 20, 0.5, 2.0)
        out[case] = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(res.items())}
        out[case]["inputs"] = hashlib.sha256(b"".join(a.tobytes() for a in args + prior) + bytes([mode])).hexdigest()
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
