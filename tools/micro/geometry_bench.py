#!/usr/bin/env python
"""Geometric verification of uncalibrated pairs: the host estimator (loftr_estimate_geometry, one call per pair) against the batched
GPU estimator (ops.estimate_geometry, one call per batch), for both models.  One JSON line per workload.

    python tools/micro/geometry_bench.py [--pairs 64] [--counts 500,2000,5000] [--outliers 0.1,0.3,0.5] [--repeats 5] [--out FILE]

Workloads: seeded tests/_geometry_oracle.make_pair batches of --pairs pairs with M matches each, 0.5 px noise, the given outlier
fraction; thresholds 3.0 px (homography) / 1.0 px (fundamental), confidence 0.999, seed 0 (evaluation.verify_matches' defaults).  The
host estimator runs once over every pair (per-pair ms = total / pairs); the GPU estimator gets one warm-up call, then --repeats
device-synchronised calls of the whole batch (median reported, per pair = median / pairs).  Every run asserts that the GPU result equals
the host result pair by pair: n_inliers, mask, and the matrix after the float32 rounding."""
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
import _geometry_oracle as O                                            # noqa: E402

DEV = "cuda:0"
CONF = 0.999
THR = {"homography": 3.0, "fundamental": 1.0}
HOST = {"homography": EV.estimate_homography_native, "fundamental": EV.estimate_fundamental_native}


def run(model, P, M, outl, repeats):
    rng = np.random.default_rng(1000 + M + int(100 * outl))
    pairs = [O.make_pair(rng, model, M, 0.5, outl, THR[model])[:2] for _ in range(P)]
    t0 = time.perf_counter()
    host = [HOST[model](p0, p1, THR[model], CONF, 0) for p0, p1 in pairs]
    host_s = time.perf_counter() - t0
    k0 = torch.from_numpy(np.concatenate([p[0] for p in pairs])).to(DEV)
    k1 = torch.from_numpy(np.concatenate([p[1] for p in pairs])).to(DEV)
    bids = torch.arange(P, device=DEV).repeat_interleave(M)
    call = lambda: ops.estimate_geometry(k0, k1, bids, P, model, THR[model], CONF, 0)
    call()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        s = time.perf_counter()
        got = call()
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - s)
    mat, inl, n = (x.cpu().numpy() for x in got)
    for b, ref in enumerate(host):
        if ref is None:
            assert n[b] == -1, b
            continue
        assert n[b] == ref[1].sum() and np.array_equal(inl[b * M:(b + 1) * M], ref[1]), b
        assert np.array_equal(mat[b], ref[0].astype(np.float32)), b
    gpu_ms = float(np.median(runs)) * 1e3
    return {"workload": f"{model}_P{P}_M{M}_out{outl}", "model": model, "pairs": P, "matches_per_pair": M, "outliers": outl, "noise_px": 0.5,
            "identical_to_host": True, "pairs_without_model": int((n < 0).sum()), "mean_inlier_ratio": round(float(inl.mean()), 4),
            "host_ms_per_pair": round(host_s * 1e3 / P, 3), "gpu_ms_per_batch": {"median": round(gpu_ms, 3), "min": round(min(runs) * 1e3, 3),
                                                                                 "max": round(max(runs) * 1e3, 3)},
            "gpu_ms_per_pair": round(gpu_ms / P, 4), "speedup": round(host_s * 1e3 / gpu_ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--counts", default="500,2000,5000")
    ap.add_argument("--outliers", default="0.1,0.3,0.5")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--models", default="homography,fundamental")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    for model in a.models.split(","):
        for M in [int(x) for x in a.counts.split(",")]:
            for o in [float(x) for x in a.outliers.split(",")]:
                line = json.dumps(run(model, a.pairs, M, o, a.repeats))
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as fh:
                        fh.write(line + "\n")


if __name__ == "__main__":
    main()
