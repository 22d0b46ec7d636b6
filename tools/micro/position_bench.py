#!/usr/bin/env python
"""Global positioning (loftr_amd/positions.py, csrc/position_gpu.hip): what it costs.

    python tools/micro/position_bench.py [--sizes 200 2000 10000] [--no-host] [--out profiles/position_bench.txt]        (needs a GPU)

Load: a street.  n cameras on a straight line, half a unit apart, all looking the same way (the case pairwise directions cannot solve);
40 n points, each seen by 5 consecutive cameras, so a camera holds about 200 observations; 0.5 px noise at f = 500; the tree is the path,
which is the deepest one the start-value workgroup can meet.  max_iters = 10 trials, the other parameters at their defaults; then the
same at the defaults (50 trials of 30 iterations), and at the defaults with ftol = 1, which ends the refinement after its first trials:
the schedule is fixed, so that line is the cost of the idle launches of a call that converges early.

One JSON line per size: the wall time of global_positions on GPU tensors with its one readback (median of 5 after a warm-up), the stages
by device events inside loftr_global_positions, the host routine on one core, and whether the two results are identical.  The figures
are recorded, not judged."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import loftr_amd                                                       # noqa: E402
from loftr_amd import ops_global                                       # noqa: E402

PARAMS = dict(max_iters=10)
IDLE = dict(ftol=1.0)                                                  # ends after the first trials: what is left of the default schedule is idle launches


def street(n, seed, per_cam=40, span=5):
    rng = np.random.default_rng(seed)
    c = np.stack([0.5 * np.arange(n), np.zeros(n), np.zeros(n)], 1)
    T = per_cam * n
    first = np.minimum(np.arange(T) // per_cam, max(n - span, 0))
    X = np.stack([0.5 * (first + rng.uniform(0, span - 1, T)), rng.uniform(-1, 1, T), rng.uniform(4, 8, T)], 1)
    k = min(span, n)
    image = (first[:, None] + np.arange(k)[None]).reshape(-1).astype(np.int32)
    p = np.repeat(X, k, 0) - c[image]
    xy = (500.0 * p[:, :2] / p[:, 2:3] + np.array([320.0, 240.0]) + rng.normal(size=(T * k, 2)) * 0.5).astype(np.float32)
    offsets = (k * np.arange(T + 1)).astype(np.int64)
    K = np.tile(np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]), (n, 1, 1))
    R = np.tile(np.eye(3), (n, 1, 1))
    tree_image = np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.int32)
    tree_t = np.tile(np.array([-0.5, 0.0, 0.0]), (n - 1, 1))              # x_b = x_a + (c_a - c_b)
    return [offsets, image, xy, K, R, np.ones(n, np.uint8), 0, tree_image, tree_t], c


def bench(sizes, host):
    return [line for params in (PARAMS, {}, IDLE) for line in bench_with(sizes, host, params)]


def bench_with(sizes, host, params):
    dev = torch.device("cuda")
    lines = []
    for n in sizes:
        args, c_gt = street(n, n)
        gpu_args = [torch.from_numpy(x).to(dev) if isinstance(x, np.ndarray) else x for x in args]
        loftr_amd.global_positions(*gpu_args, **params)                   # warm-up (kernel load)
        wall, stages = [], []
        for _ in range(5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            pos = loftr_amd.global_positions(*gpu_args, **params)
            wall.append(1e3 * (time.perf_counter() - t))
            timed = []
            loftr_amd.global_positions(*gpu_args, timings=timed, **params)
            stages.append([v for _, v in timed])
        out = {"workload": "global_positions_street", "params": params or "defaults", "images": n, "points": int(args[0].shape[0] - 1),
               "observations": int(args[1].shape[0]),
               "call_wall_ms_with_readback": round(float(np.median(wall)), 3),
               "stage_ms": {k: round(float(v), 4) for k, v in zip(ops_global.POSITION_STAGES, np.median(np.array(stages), 0))},
               "stats": {k: pos.stats[k] for k in ("n_trials", "n_accepted", "n_pcg_iters", "n_free", "tree_depth", "cost_start", "cost_end",
                                                   "status_name")}}
        if host:
            t = time.perf_counter()
            want = loftr_amd.global_positions(*args, **params)
            out["host_routine_ms"] = round(1e3 * (time.perf_counter() - t), 1)
            a, b = want.to_host(), pos.to_host()
            out["identical_to_host"] = bool(all(a[k].tobytes() == b[k].tobytes() for k in loftr_amd.GlobalPositions.FIELDS) and a["stats"] == b["stats"])
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="*", default=[200, 2000, 10000])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    lines = bench(args.sizes, not args.no_host)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
