"""Golden vectors for the lifting of matched keypoints to 3D (loftr_lift_keypoints, evaluation.localize), produced by the REAL
reference's warp_kpts (src/loftr/utils/geometry.py, imported through oracle/ref_shim.py).  Authoring container only:

    python tests/golden/make_golden_lift.py        ->  tests/golden/lift_warp.npz

Inputs are synthetic and seeded: 3 pairs with 60 x 80 depth maps (a smooth surface at depths 2-8 with a block of zero depth),
200 keypoints per pair inside the map, some of them at exact .5 coordinates (torch.round rounds those to the even pixel), intrinsics of
an 80 x 60 frame and a random relative pose.  warp_kpts is run in float32 and in float64; stored: the inputs, both w_kpts0 and
depth0[b, round(y), round(x)] != 0.  The distance between the two runs is the reference's own float32 error, the yardstick of the tests.
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_shim import import_reference_training   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N, L, DH, DW = 3, 200, 60, 80


def _rot(axis, ang):
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def main():
    import_reference_training()
    warp_kpts = importlib.import_module("src.loftr.utils.geometry").warp_kpts
    rng = np.random.default_rng(2031)
    yy, xx = np.mgrid[0:DH, 0:DW]
    depth0 = np.stack([5 + 2.5 * np.sin(0.07 * xx + b) * np.cos(0.09 * yy - b) + 0.3 * rng.random((DH, DW)) for b in range(N)])
    depth0[:, 20:32, 30:50] = 0.0                                          # a block without depth
    depth1 = rng.uniform(2, 8, (N, DH, DW))
    kpts0 = np.stack([np.c_[rng.uniform(0, DW - 1, L), rng.uniform(0, DH - 1, L)] for _ in range(N)])
    kpts0[:, :24] = np.floor(kpts0[:, :24]) + 0.5                          # exact halves: 10.5 -> 10, 11.5 -> 12
    kpts0[:, 24:32] = np.floor(kpts0[:, 24:32])                            # exact pixel centres
    kpts0[:, :, 0] = np.minimum(kpts0[:, :, 0], DW - 1.5)                  # the rounded keypoint stays inside the map
    kpts0[:, :, 1] = np.minimum(kpts0[:, :, 1], DH - 1.5)
    K0 = np.stack([np.array([[66.0 + b, 0, 40.5 - b], [0, 65.0 - b, 29.5 + b], [0, 0, 1]]) for b in range(N)])
    K1 = np.stack([np.array([[64.0 - b, 0, 39.0 + b], [0, 67.0 + b, 30.5 - b], [0, 0, 1]]) for b in range(N)])
    T = np.tile(np.eye(4), (N, 1, 1))
    for b in range(N):
        T[b, :3, :3] = _rot(rng.standard_normal(3), 0.1 + 0.2 * rng.random())
        T[b, :3, 3] = rng.uniform(-0.5, 0.5, 3)
    f32 = [a.astype(np.float32) for a in (kpts0, depth0, depth1, T, K0, K1)]
    out = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        _, w = warp_kpts(*[torch.from_numpy(a).to(dt) for a in f32])       # float64 run on the float32 inputs
        out["w_kpts0_" + name] = w.numpy()
    r = np.rint(f32[0]).astype(np.int64)
    nonzero = np.stack([f32[1][b, r[b, :, 1], r[b, :, 0]] != 0 for b in range(N)])
    np.savez_compressed(os.path.join(HERE, "lift_warp.npz"), kpts0=f32[0], depth0=f32[1], T_0to1=f32[3], K0=f32[4], K1=f32[5], nonzero=nonzero, **out)
    d = np.abs(out["w_kpts0_f32"].astype(np.float64) - out["w_kpts0_f64"])[nonzero]
    print(f"wrote lift_warp.npz: {int(nonzero.sum())} of {N * L} keypoints with depth, reference fp32 vs fp64 max {d.max():.3e} px")


if __name__ == "__main__":
    main()
