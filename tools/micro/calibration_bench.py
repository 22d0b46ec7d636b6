#!/usr/bin/env python
"""View-graph calibration (loftr_amd/calibration.py, csrc/calib_gpu.hip): what it costs.

    python tools/micro/calibration_bench.py [--sizes 200 2000 10000] [--no-host] [--out profiles/calibration_bench.txt]      (needs a GPU)

Load: a seeded sequential graph.  n cameras along a street, half a unit apart, each turned by its own small random rotation (so the
optical axes do not meet), focals 600 to 1100 at 1000 x 750 pixels; every image is joined to the next 5, so there are about 5 n
edges and an image holds about 10 edge ends.  The F of an edge is the exact one of the two cameras with every entry disturbed by
1e-3 of its size, unit norm, through float32.  Start 1.2 * 1000 for every image, one group per image, every parameter at its default
(50 trials of 30 iterations); then the same with one camera for all images, whose single incidence list is about 10 n long; then
both again with max_iters = 10 and pcg_iters = 15, which is enough for these scenes (6 or 7 trials of at most 15 iterations): the
schedule is fixed, so the difference to the defaults is the cost of the launches that return at once after convergence.

One JSON line per size: the wall time of calibrate_view_graph on GPU tensors with its one readback (median of 5 after a warm-up), the
stages by device events inside loftr_calibrate_view_graph, the host routine on one core, and whether the two results are identical.
The figures are recorded, not judged: no target exists."""
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
from loftr_amd import ops_calib                                        # noqa: E402

W, H = 1000.0, 750.0


def rodrigues(v):
    th = np.linalg.norm(v, axis=1)[:, None, None]
    k = v / np.linalg.norm(v, axis=1, keepdims=True)
    Kx = np.zeros((len(v), 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def street(n, seed, k=5, one_camera=False):
    rng = np.random.default_rng(seed)
    f = np.full(n, 850.0) if one_camera else rng.uniform(600.0, 1100.0, n)
    c = np.stack([0.5 * np.arange(n), rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n)], 1)
    R = rodrigues(rng.uniform(-0.25, 0.25, (n, 3)))
    a = np.repeat(np.arange(n), k)
    b = a + np.tile(np.arange(1, k + 1), n)
    a, b = a[b < n], b[b < n]
    Rab = R[b] @ R[a].transpose(0, 2, 1)
    t = np.einsum("eij,ej->ei", R[b], c[a] - c[b])
    tx = np.zeros((len(a), 3, 3))
    tx[:, 0, 1], tx[:, 0, 2], tx[:, 1, 0], tx[:, 1, 2], tx[:, 2, 0], tx[:, 2, 1] = -t[:, 2], t[:, 1], t[:, 2], -t[:, 0], -t[:, 1], t[:, 0]
    Kinv = np.zeros((n, 3, 3))
    Kinv[:, 0, 0] = Kinv[:, 1, 1] = 1 / f
    Kinv[:, 0, 2], Kinv[:, 1, 2], Kinv[:, 2, 2] = -W / 2 / f, -H / 2 / f, 1.0
    F = Kinv[b].transpose(0, 2, 1) @ (tx @ Rab) @ Kinv[a]
    F = F * (1 + 1e-3 * rng.standard_normal(F.shape))
    F = (F / np.linalg.norm(F, axis=(1, 2), keepdims=True)).astype(np.float32).astype(np.float64)
    args = [np.stack([a, b], 1).astype(np.int32), F, rng.integers(30, 300, len(a)).astype(np.int32), n, np.tile([W / 2, H / 2], (n, 1)),
            np.full(n, 1.2 * W)]
    return args, f, (np.zeros(n, np.int64) if one_camera else None)


SHORT = dict(max_iters=10, pcg_iters=15)


def bench(sizes, host):
    return [line for params in ({}, SHORT) for line in bench_with(sizes, host, params)]


def bench_with(sizes, host, params):
    dev = torch.device("cuda")
    lines = []
    for one_camera in (False, True):
        for n in sizes:
            args, f_true, ids = street(n, n, one_camera=one_camera)
            gpu_args = [torch.from_numpy(x).to(dev) if isinstance(x, np.ndarray) else x for x in args]
            gpu_ids = None if ids is None else torch.from_numpy(ids).to(dev)
            loftr_amd.calibrate_view_graph(*gpu_args, camera_ids=gpu_ids, **params)    # warm-up (kernel load)
            wall, stages = [], []
            for _ in range(5):
                torch.cuda.synchronize()
                t = time.perf_counter()
                cal = loftr_amd.calibrate_view_graph(*gpu_args, camera_ids=gpu_ids, **params)
                wall.append(1e3 * (time.perf_counter() - t))
                timed = []
                loftr_amd.calibrate_view_graph(*gpu_args, camera_ids=gpu_ids, timings=timed, **params)
                stages.append([v for _, v in timed])
            err = np.abs(cal.focal.cpu().numpy() / f_true - 1)
            out = {"workload": "calibrate_view_graph_street", "params": params or "defaults", "groups": "one camera" if one_camera else "per image", "images": n,
                   "edges": int(args[0].shape[0]), "call_wall_ms_with_readback": round(float(np.median(wall)), 3),
                   "stage_ms": {k: round(float(v), 4) for k, v in zip(ops_calib.CALIB_STAGES, np.median(np.array(stages), 0))},
                   "focal_error_median_max": [round(float(np.median(err)), 5), round(float(err.max()), 5)],
                   "stats": {k: cal.stats[k] for k in ("n_trials", "n_accepted", "n_pcg_iters", "n_free_groups", "n_outlier_edges", "cost_start",
                                                       "cost_end", "status_name")}}
            if host:
                t = time.perf_counter()
                want = loftr_amd.calibrate_view_graph(*args, camera_ids=ids, **params)
                out["host_routine_ms"] = round(1e3 * (time.perf_counter() - t), 1)
                a, b = want.to_host(), cal.to_host()
                out["identical_to_host"] = bool(all(a[k].tobytes() == b[k].tobytes() for k in loftr_amd.ViewGraphCalibration.FIELDS)
                                                and a["stats"] == b["stats"])
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
