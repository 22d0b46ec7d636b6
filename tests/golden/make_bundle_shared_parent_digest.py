"""SHA-256 digests of what the grouped host routine -- loftr_bundle_adjust_shared_host (one focal step per group of images)
-- returns on the scenes of tests/_bundle_shared_cases.py and on the cases of its rule.

    python tests/golden/make_bundle_shared_parent_digest.py [--root CHECKOUT] [--write]

Run with --root pointing at a checkout (with its library built) of the commit BEFORE the three modes became instantiations of one
sequence of phases, and --write, it produced tests/golden/bundle_shared_parent_digest.json; tests/test_bundle_shared.py recomputes the
digests on the current build and compares: the grouped path must return the same bits as it did then.  Every output tensor (K, cam_focal
and group_focal included) and the 16 counts are covered."""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
OUT = os.path.join(HERE, "bundle_shared_parent_digest.json")
# case: (scene, camera ids (None: the scene's), huber_px, max_iters, min_focal_obs)
CASES = {"one_a": ("one_a", None, 0.0, 30, 20), "one_b": ("one_b", None, 0.0, 30, 20), "bodies": ("bodies", None, 0.0, 30, 20),
         "thin": ("thin", None, 0.0, 30, 20), "huber": ("huber", None, 2.0, 100, 20),
         "hand_problem": ("hand_problem", [0, 0, 1, 1, 1, 2, 2, 3], 0.0, 30, 1),
         "singletons_a": ("one_a", "singletons", 0.0, 30, 20),                     # every image its own group
         "known_poses": ("known_poses", None, 0.0, 30, 20),                        # zero free cameras, one refining group
         "thin_at_min": ("thin", None, 0.0, 30, 51), "thin_above_min": ("thin", None, 0.0, 30, 52)}     # body 2 holds 51 observations


def groups(ids):
    """(cam_group [n] i32, group_offsets [G+1] i64, group_cams [n] i32): dense groups in the order of their first members, then a
    stable sort."""
    ids = np.asarray(ids, np.int64)
    uniq, first, inv = np.unique(ids, return_index=True, return_inverse=True)
    rank = np.empty(uniq.size, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(uniq.size)
    group = rank[inv.reshape(-1)]
    offsets = np.zeros(uniq.size + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(group, minlength=uniq.size))
    return [group.astype(np.int32), offsets, np.argsort(group, kind="stable").astype(np.int32)]


def scene(name):
    import _bundle_cases as BC
    import _bundle_shared_cases as SC
    if name == "hand_problem":
        return BC.hand_problem()[0]
    if name == "known_poses":
        s = SC.shared_case("one_b")
        return dict(s, T_cam_from_world=s["T_true"].copy(), fixed=np.ones(len(s["K"]), bool))
    return SC.shared_case(name)


def digests():
    """{case: {output name: sha256 hex, 'inputs': sha256 hex}} with the loftr_amd that is importable now; every flag of refine_focal set."""
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    from loftr_amd import ops
    spec = importlib.util.spec_from_file_location("make_bundle_parent_digest", os.path.join(HERE, "make_bundle_parent_digest.py"))
    old = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(old)
    out = {}
    for case, (name, ids, huber, iters, min_obs) in CASES.items():
        s = scene(name)
        n = len(s["K"])
        ids = s["camera_ids"] if ids is None else np.arange(n)[::-1].copy() if isinstance(ids, str) else ids
        args = old.raw(s) + [np.ones(n, np.uint8)] + groups(ids)
        res = ops.bundle_adjust_shared_host(*args, huber, iters, 30, 1e-2, 1e-9, min_obs, 0.5, 2.0)
        out[case] = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(res.items())}
        out[case]["inputs"] = hashlib.sha256(b"".join(a.tobytes() for a in args)).hexdigest()
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
