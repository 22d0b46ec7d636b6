#!/usr/bin/env python
"""3D similarity RANSAC and moving a model on the GPU, timed.  One JSON line per workload.

    python tools/micro/similarity_bench.py [--repeats 5] [--only rgbd|alignment|transform] [--out FILE]

Workloads:
  rgbd       64 problems x 1000 correspondences, rigid (evaluation.register_depth's shape): tests/_similarity_oracle.make_scene, noise
             0.008, 30 % outliers, thresh 0.05;
  alignment  one problem of 800 centres with scale, 25 % outliers (Reconstruction.align's shape);
  transform  ops.transform_model at 250 000 points / 806 images.
Each GPU call gets one warm-up call, then --repeats calls timed with device events (median reported).  The estimator workloads assert
that the GPU result equals the host estimator's problem by problem (n_inliers, mask, the float64 bits of s, R, t), the transform that it
equals the host routine's bits.  Next to each estimator workload stands the one yardstick there is: ops.estimate_absolute_poses (P3P
RANSAC, the same scaffold) at the same M and P, on tests/_absolute_pose_oracle.make_scene with the same outlier share.
The entry point has no stage_ms argument (the scaffold's run() takes no timer), so there is no stage split here; per-kernel times come
from a kernel trace of one workload (`rocprofv3 --kernel-trace --stats -- python tools/micro/similarity_bench.py --only rgbd`, summarised
by tools/rocpd_summary.py)."""
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
import _absolute_pose_oracle as AO                                      # noqa: E402
import _similarity_cases as SC                                          # noqa: E402
import _similarity_oracle as O                                          # noqa: E402

DEV = "cuda:0"
THR, CONF = 0.05, 0.999


def timed(call, repeats):
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
    return got, {"median": round(float(np.median(runs)), 3), "min": round(min(runs), 3), "max": round(max(runs), 3)}


def estimator(name, P, M, outl, with_scale, repeats):
    rng = np.random.default_rng(3000 + M + P)
    scenes = [O.make_scene(rng, M, 0.008, outl, with_scale=with_scale, thresh=THR) for _ in range(P)]
    t0 = time.perf_counter()
    host = [EV.estimate_similarity_native(s["src"], s["dst"], with_scale, THR, CONF, 0) for s in scenes]
    host_s = time.perf_counter() - t0
    src = torch.from_numpy(np.concatenate([s["src"] for s in scenes])).to(DEV)
    dst = torch.from_numpy(np.concatenate([s["dst"] for s in scenes])).to(DEV)
    bids = torch.arange(P, device=DEV).repeat_interleave(M)
    got, ms = timed(lambda: ops.estimate_similarities(src, dst, bids, P, with_scale, THR, CONF, 0), repeats)
    s, R, t, inl, n = (x.cpu().numpy() for x in got)
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    for b, ref in enumerate(host):
        assert ref is not None and n[b] == ref[3].sum() and np.array_equal(inl[b * M:(b + 1) * M], ref[3]), b
        assert np.array_equal(bits(s[b]), bits(ref[0])) and np.array_equal(bits(R[b]), bits(ref[1])) and np.array_equal(bits(t[b]), bits(ref[2])), b
    # the yardstick: the absolute-pose estimator at the same M, P and outlier share
    ab = [AO.make_scene(rng, M, 0.5, outl) for _ in range(P)]
    X = torch.from_numpy(np.concatenate([a["X"] for a in ab])).to(DEV)
    k = torch.from_numpy(np.concatenate([a["kpts"] for a in ab])).to(DEV)
    K = torch.from_numpy(np.stack([a["K"] for a in ab]).astype(np.float32)).to(DEV)
    _, ms_abs = timed(lambda: ops.estimate_absolute_poses(X, k, bids, K, 3.0, CONF, 0), repeats)
    return {"workload": name, "problems": P, "correspondences_per_problem": M, "outliers": outl, "with_scale": with_scale,
            "identical_to_host": True, "mean_inlier_ratio": round(float(inl.mean()), 4), "host_ms_per_problem": round(host_s * 1e3 / P, 3),
            "gpu_ms_per_batch": ms, "absolute_pose_gpu_ms_per_batch_same_M_P": ms_abs, "speedup_over_host": round(host_s * 1e3 / ms["median"], 1)}


def transform(N, n, repeats):
    case = [torch.from_numpy(np.ascontiguousarray(a)) for a in SC.model_case(N, n)]
    t0 = time.perf_counter()
    want = ops.transform_model(*case)
    host_ms = (time.perf_counter() - t0) * 1e3
    dev = [a.to(DEV) for a in case]
    got, ms = timed(lambda: ops.transform_model(*dev), repeats)
    assert all(g.cpu().numpy().tobytes() == w.numpy().tobytes() for g, w in zip(got, want))
    return {"workload": "transform", "points": N, "images": n, "identical_to_host": True, "host_ms": round(host_ms, 3), "gpu_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--only", default=None, choices=["rgbd", "alignment", "transform"], help="run one workload (for a kernel trace)")
    a = ap.parse_args()
    jobs = {"rgbd": lambda: estimator("rgbd", 64, 1000, 0.3, False, a.repeats), "alignment": lambda: estimator("alignment", 1, 800, 0.25, True, a.repeats),
            "transform": lambda: transform(250_000, 806, a.repeats)}
    for name, job in jobs.items():
        if a.only not in (None, name):
            continue
        line = json.dumps(job())
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
