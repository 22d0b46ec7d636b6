#!/usr/bin/env python
"""Are the host estimators of two builds of libloftr_hip.so the same functions, bit for bit?

    python tools/host_estimators_ab.py OLD.so NEW.so
    python tools/host_estimators_ab.py --dump CASES.bin      (the same inputs as a file for tools/host_estimators_driver.cpp)

The batched GPU estimators are tested against the host estimators, so a change that moves both sides together is invisible to those
tests.  This tool calls loftr_five_point, loftr_estimate_pose, loftr_geometry_minimal, loftr_estimate_geometry (both models), loftr_p3p and
loftr_estimate_absolute_pose of the two libraries with identical inputs and requires byte-equal outputs (matrices as raw float64 / float32
bits, masks, counts, status).  Inputs are the seeded generators of tests/: per model, match counts {s - 1, s, s + 1, 37, 400, 1025} x noise
{0, 0.3, 1.0} px x outliers {0, 0.3, 0.6} x RANSAC seeds {0, 11}, the degenerate pairs of test_hip_pose and a make_scene batch.  Both
libraries run on this machine, so its libm (pow / log of the stopping rule, cos / sin of the root finder's start angles) is common to both.
Runs on the CPU; exit status 0 when every case is equal."""
import ctypes as C
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _absolute_pose_oracle as AO                                                     # noqa: E402
import _geometry_oracle as GO                                                          # noqa: E402
from _scenes import make_scene                                                         # noqa: E402
from test_hip_pose import _degenerate, _pair                                           # noqa: E402
from loftr_amd._lib import SIGNATURES                                                  # noqa: E402

NOISE, OUTLIERS, SEEDS = (0.0, 0.3, 1.0), (0.0, 0.3, 0.6), (0, 11)
counts = lambda s: (s - 1, s, s + 1, 37, 400, 1025)
ptr = lambda a: a.ctypes.data_as(C.c_void_p)
f32 = lambda a: np.ascontiguousarray(a, np.float32)
f64 = lambda a: np.ascontiguousarray(a, np.float64)


def load(path):
    lib = C.CDLL(os.path.abspath(path))
    for name in ("loftr_five_point", "loftr_estimate_pose", "loftr_geometry_minimal", "loftr_estimate_geometry", "loftr_p3p",
                 "loftr_estimate_absolute_pose"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = SIGNATURES[name]
    return lib


def outputs(*shapes):
    """Output arrays pre-filled with a pattern, so that what a call leaves unwritten compares equal too."""
    return [np.frombuffer(b"\x5a" * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).copy() for shape, dt in shapes]


def run(lib, kind, a):
    """One call -> bytes of (status, outputs)."""
    n = C.c_long(-7)
    ns = C.c_int(-7)
    if kind == "five_point":
        q0, q1 = a
        (E,) = outputs(((10, 9), np.float64))
        st = lib.loftr_five_point(ptr(q0), ptr(q1), len(q0), ptr(E), C.byref(ns))
        return bytes([st & 255]) + E.tobytes() + bytes(ns)
    if kind == "pose":
        p0, p1, K0, K1, seed = a
        R, t, inl = outputs(((9,), np.float32), ((3,), np.float32), ((max(len(p0), 1),), np.uint8))
        st = lib.loftr_estimate_pose(ptr(p0), ptr(p1), len(p0), ptr(K0), ptr(K1), 0.5, 0.99999, seed, ptr(R), ptr(t), ptr(inl), C.byref(n))
        return bytes([st & 255]) + R.tobytes() + t.tobytes() + inl.tobytes() + bytes(n)
    if kind == "geometry_minimal":
        p0, p1, model = a
        (mats,) = outputs(((3, 9), np.float64))
        st = lib.loftr_geometry_minimal(ptr(p0), ptr(p1), model, ptr(mats), C.byref(ns))
        return bytes([st & 255]) + mats.tobytes() + bytes(ns)
    if kind == "geometry":
        p0, p1, model, seed = a
        mat, inl = outputs(((9,), np.float32), ((max(len(p0), 1),), np.uint8))
        st = lib.loftr_estimate_geometry(ptr(p0), ptr(p1), len(p0), model, (3.0, 1.0)[model], 0.999, seed, ptr(mat), ptr(inl), C.byref(n))
        return bytes([st & 255]) + mat.tobytes() + inl.tobytes() + bytes(n)
    if kind == "p3p":
        X, f = a
        R, t = outputs(((4, 9), np.float64), ((4, 3), np.float64))
        st = lib.loftr_p3p(ptr(X), ptr(f), ptr(R), ptr(t), C.byref(ns))
        return bytes([st & 255]) + R.tobytes() + t.tobytes() + bytes(ns)
    X, kpts, K, seed = a
    R, t, inl = outputs(((9,), np.float32), ((3,), np.float32), ((max(len(X), 1),), np.uint8))
    st = lib.loftr_estimate_absolute_pose(ptr(X), ptr(kpts), len(X), ptr(K), 3.0, 0.999, seed, ptr(R), ptr(t), ptr(inl), C.byref(n))
    return bytes([st & 255]) + R.tobytes() + t.tobytes() + inl.tobytes() + bytes(n)


def cases():
    """(kind, label, arguments) of every call."""
    grid = lambda s: itertools.product(counts(s), NOISE, OUTLIERS)
    normalised = lambda p, K: f64((p.astype(np.float64) - K[:2, 2]) / [K[0, 0], K[1, 1]])
    # relative pose: test_hip_pose's pairs, its degenerate ones, a make_scene batch
    rng = np.random.default_rng(2024)
    pairs = [((n, noise, out), _pair(rng, n, noise, out)) for n, noise, out in grid(5)]
    pairs += [(("degenerate", i), p) for i, p in enumerate(_degenerate(rng))]
    sc = make_scene(77, [300, 1200, 5, 0, 900], noise_px=0.5, outlier_frac=0.3)
    pairs += [(("scene", b), tuple(sc[k][sc["m_bids"] == b] for k in ("mkpts0_f", "mkpts1_f")) + (sc["K0"][b], sc["K1"][b])) for b in range(5)]
    for tag, (p0, p1, K0, K1) in pairs:
        p0, p1, K0, K1 = f32(p0), f32(p1), f32(K0), f32(K1)
        for seed in SEEDS:
            yield "pose", (tag, seed), (p0, p1, K0, K1, seed)
        if len(p0) >= 5:                                                               # the solver on the first five points and on all
            q0, q1 = normalised(p0, K0), normalised(p1, K1)
            yield "five_point", (tag, 5), (f64(q0[:5]), f64(q1[:5]))
            yield "five_point", (tag, len(q0)), (q0, q1)
    # homography / fundamental matrix: _geometry_oracle's pairs
    for model, name in enumerate(("homography", "fundamental")):
        s = (4, 7)[model]
        rng = np.random.default_rng(2025 + model)
        for n, noise, out in grid(s):
            p0, p1 = (f32(x) for x in GO.make_pair(rng, name, n, noise, out, (3.0, 1.0)[model])[:2])
            for seed in SEEDS:
                yield "geometry", (name, n, noise, out, seed), (p0, p1, model, seed)
            if n >= s:
                yield "geometry_minimal", (name, n, noise, out), (f64(p0[:s]), f64(p1[:s]), model)
    # absolute pose: _absolute_pose_oracle's scenes
    rng = np.random.default_rng(2026)
    for n, noise, out in grid(3):
        sc = AO.make_scene(rng, n, noise, out)
        X, kpts, K = f32(sc["X"]), f32(sc["kpts"]), f32(sc["K"])
        for seed in SEEDS:
            yield "absolute_pose", (n, noise, out, seed), (X, kpts, K, seed)
        if n >= 3:
            rays = np.c_[(kpts[:3].astype(np.float64) - sc["K"][:2, 2]) / [sc["K"][0, 0], sc["K"][1, 1]], np.ones(3)]
            yield "p3p", (n, noise, out), (f64(X[:3]), f64(rays))
    sc = AO.make_collinear_scene()
    yield "absolute_pose", ("collinear",), (f32(sc["X"]), f32(sc["kpts"]), f32(sc["K"]), 0)
    yield "p3p", ("collinear",), (f64(sc["X"][:3]), f64(np.c_[sc["kpts"][:3], np.ones(3)]))


KINDS = ("five_point", "pose", "geometry_minimal", "geometry", "p3p", "absolute_pose")


def dump(path):
    """Every case as: int32 kind (index into KINDS), n, model, seed, then the input arrays in argument order."""
    with open(path, "wb") as fh:
        for kind, _, args in cases():
            arrays = [a for a in args if isinstance(a, np.ndarray)]
            ints = [a for a in args if not isinstance(a, np.ndarray)]
            model = ints[0] if kind.startswith("geometry") else 0
            seed = ints[-1] if kind in ("pose", "geometry", "absolute_pose") else 0
            n = 3 if kind == "p3p" else len(arrays[0])
            fh.write(np.array([KINDS.index(kind), n, model, seed], np.int32).tobytes() + b"".join(a.tobytes() for a in arrays))


def main(old_path, new_path):
    old, new = load(old_path), load(new_path)
    if old._handle == new._handle:
        sys.exit("the two paths name one library")
    total, bad = {}, []
    for kind, label, args in cases():
        total[kind] = total.get(kind, 0) + 1
        if run(old, kind, args) != run(new, kind, args):
            bad.append((kind, label))
    n = sum(total.values())
    for kind, label in bad[:20]:
        print("DIFFERENT", kind, label)
    print(f"{'FAIL' if bad else 'PASS'}: {n - len(bad)} of {n} host calls byte-equal ("
          + ", ".join(f"{k} {v}" for k, v in sorted(total.items())) + ")")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    if sys.argv[1] == "--dump":
        sys.exit(dump(sys.argv[2]))
    sys.exit(main(sys.argv[1], sys.argv[2]))
