#!/usr/bin/env python
"""Absolute pose from 2D-3D matches: the host estimator (loftr_estimate_absolute_pose, one call per pair) against the batched GPU
estimator (ops.estimate_absolute_poses, one call per batch).  One JSON line per workload.

    python tools/micro/absolute_pose_bench.py [--pairs 64] [--counts 500,2000,5000] [--outliers 0.1,0.3,0.5] [--repeats 5] [--out FILE]

Workloads: seeded tests/_absolute_pose_oracle.make_scene batches of --pairs pairs with M matches each, 0.5 px noise, the given outlier
fraction; threshold 3.0 px, confidence 0.999, seed 0 (evaluation.localize's defaults).  The host estimator runs once over every pair
(per-pair ms = total / pairs); the GPU estimator gets one warm-up call, then --repeats calls of the whole batch timed with device
events (median reported, per pair = median / pairs).  Every run asserts that the GPU result equals the host result pair by pair:
n_inliers, mask, and R, t after the float32 rounding."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from loftr_amd import evaluation as EV, ops                            # noqa: E402
import _absolute_pose_oracle as O                                       # noqa: E402

DEV = "cuda:0"
THR, CONF = 3.0, 0.999


def run(P, M, outl, repeats):
    rng = np.random.default_rng(1000 + M + int(100 * outl))
    scenes = [O.make_scene(rng, M, 0.5, outl) for _ in range(P)]
    t0 = time.perf_counter()
    host = [EV.estimate_absolute_pose_native(s["X"], s["kpts"], s["K"], THR, CONF, 0) for s in scenes]
    host_s = time.perf_counter() - t0
    X = torch.from_numpy(np.concatenate([s["X"] for s in scenes])).to(DEV)
    k = torch.from_numpy(np.concatenate([s["kpts"] for s in scenes])).to(DEV)
    K = torch.from_numpy(np.stack([s["K"] for s in scenes]).astype(np.float32)).to(DEV)
    bids = torch.arange(P, device=DEV).repeat_interleave(M)
    call = lambda: ops.estimate_absolute_poses(X, k, bids, K, THR, CONF, 0)
    call()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = call()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1))
    R, t, inl, n = (x.cpu().numpy() for x in got)
    for b, ref in enumerate(host):
        if ref is None:
            assert n[b] == -1, b
            continue
        assert n[b] == ref[2].sum() and np.array_equal(inl[b * M:(b + 1) * M], ref[2]), b
        assert np.array_equal(R[b], ref[0].astype(np.float32)) and np.array_equal(t[b], ref[1].astype(np.float32)), b
    gpu_ms = float(np.median(runs))
    return {"workload": f"absolute_pose_P{P}_M{M}_out{outl}", "pairs": P, "matches_per_pair": M, "outliers": outl, "noise_px": 0.5,
            "identical_to_host": True, "pairs_without_model": int((n < 0).sum()), "mean_inlier_ratio": round(float(inl.mean()), 4),
            "host_ms_per_pair": round(host_s * 1e3 / P, 3), "gpu_ms_per_batch": {"median": round(gpu_ms, 3), "min": round(min(runs), 3),
                                                                                 "max": round(max(runs), 3)},
            "gpu_ms_per_pair": round(gpu_ms / P, 4), "speedup": round(host_s * 1e3 / gpu_ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--counts", default="500,2000,5000")
    ap.add_argument("--outliers", default="0.1,0.3,0.5")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    for M in [int(x) for x in a.counts.split(",")]:
        for o in [float(x) for x in a.outliers.split(",")]:
            line = json.dumps(run(a.pairs, M, o, a.repeats))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
