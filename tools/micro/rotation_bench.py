#!/usr/bin/env python
"""Rotation averaging over the view graph (loftr_amd/rotations.py, csrc/rotation_gpu.hip): what it costs and what it finds.

    python tools/micro/rotation_bench.py [--sizes 200 2000 10000] [--no-host] [--out profiles/rotation_bench.txt]        (needs a GPU)
    python tools/micro/rotation_bench.py --accuracy [--out profiles/rotation_accuracy.txt]                                (CPU only)

Load: the seeded view graphs of tests/_rotation_cases.py (random rotations, pairs (i, j) with j - i <= win plus chords, 0.5 degrees of
noise per axis, a share of the edges replaced by random rotations carrying the same weights): sequential graphs are the deep-tree case,
which is what the start-value workgroup and the conjugate gradients feel.

Without --accuracy, one JSON line per size: the wall time of average_rotations on GPU tensors with its one readback (median of 5 after
a warm-up), the stages by device events inside loftr_rotation_averaging, the host routine on one core, and whether the two results are
identical.  With --accuracy, the host routine against the numpy oracle (tests/_rotation_oracle.py) on the scenes of the tests: the
distances the test tolerances are ten times of, the margins of the planted-outlier scenes, and averaging against chaining."""
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

import _rotation_cases as RC                                          # noqa: E402
import loftr_amd                                                       # noqa: E402
from loftr_amd import ops                                              # noqa: E402
from loftr_amd.evaluation import global_rotation_errors               # noqa: E402

SHAPES = {200: dict(win=3, chords=200), 2000: dict(win=3, chords=4000), 10000: dict(win=4, chords=10000)}      # 4 to 10 edges per image


def bench(sizes, host):
    dev = torch.device("cuda")
    lines = []
    for n in sizes:
        sc = RC.make_scene(f"bench_{n}", n, seed=n, planted=0.1, **SHAPES.get(n, dict(win=3, chords=n)))
        gpu_args = [torch.from_numpy(x).to(dev) for x in sc.args[:3]]
        loftr_amd.average_rotations(*gpu_args, n)                          # warm-up (kernel load)
        wall, stages = [], []
        for _ in range(5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            rot = loftr_amd.average_rotations(*gpu_args, n)
            wall.append(1e3 * (time.perf_counter() - t))
            timed = []
            loftr_amd.average_rotations(*gpu_args, n, timings=timed)
            stages.append([v for _, v in timed])
        out = {"workload": "rotation_averaging_sequential_graph", "images": n, "edges": int(sc.edge_weight.shape[0]),
               "planted": int(sc.planted.sum()), "call_wall_ms_with_readback": round(float(np.median(wall)), 3),
               "stage_ms": {k: round(float(v), 4) for k, v in zip(ops.ROTATION_STAGES, np.median(np.array(stages), 0))},
               "stats": {k: rot.stats[k] for k in ("n_in_graph", "tree_depth", "n_tree_unsupported", "n_iters", "n_pcg_iters", "n_ok", "n_outlier",
                                                   "status_name")},
               "outliers_are_the_planted": bool(np.array_equal((rot.edge_state == 3).cpu().numpy(), sc.planted))}
        if host:
            t = time.perf_counter()
            want = loftr_amd.average_rotations(*sc.args)
            out["host_routine_ms"] = round(1e3 * (time.perf_counter() - t), 1)
            a, b = want.to_host(), rot.to_host()
            out["identical_to_host"] = bool(all(a[k].tobytes() == b[k].tobytes() for k in loftr_amd.GlobalRotations.FIELDS) and a["stats"] == b["stats"])
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    return lines


def accuracy():
    import _rotation_oracle as RO
    deg = lambda chord: np.degrees(2.0 * np.arcsin(np.clip(chord / 2.0, 0.0, 1.0)))
    lines = ["scene                images edges | max |R - oracle|  max |chord - oracle|   (host routine, pcg_tol 1e-12, against the dense-solve oracle)"]
    scenes = RC.outlier_scenes() + RC.chain_scenes() + [RC.hub_scene(), RC.two_components(), RC.with_duplicates(RC.make_scene("d", 20, 3, 5))[0]]
    worst = [0.0, 0.0]
    runs = {}
    for sc in scenes:
        o = runs[sc.name] = RO.average(*sc.args, solver="dense")
        h = loftr_amd.average_rotations(*sc.args, pcg_iters=500, pcg_tol=1e-12).to_host()
        m, j = o["in_graph"], ~np.isnan(o["edge_chord"])
        d = [float(np.abs(h["R"][m] - o["R"][m]).max()), float(np.abs(h["edge_chord"][j] - o["edge_chord"][j]).max())]
        worst = [max(a, b) for a, b in zip(worst, d)]
        lines.append(f"{sc.name:20s} {sc.n:6d} {sc.edge_weight.shape[0]:5d} | {d[0]:15.3e}  {d[1]:20.3e}")
    lines.append(f"largest: {worst[0]:.3e} (R), {worst[1]:.3e} (edge_chord); tests/test_rotation.py asserts ten times MEASURED_R / MEASURED_CHORD")
    lines.append("")
    lines.append("planted outliers (oracle alone; max_err_deg = 10: good edges must end below 5 degrees, planted ones above 20)")
    lines.append("scene                planted | good edges <= deg  planted >= deg | host routine: outliers == planted, planted edges in the tree")
    for sc in RC.outlier_scenes() + [RC.hub_scene()]:
        e = deg(runs[sc.name]["edge_chord"])
        rot = loftr_amd.average_rotations(*sc.args)
        lines.append(f"{sc.name:20s} {int(sc.planted.sum()):7d} | {e[~sc.planted].max():17.2f}  {e[sc.planted].min():14.2f} | "
                     f"{np.array_equal((rot.edge_state == 3).numpy(), sc.planted)}, {int((rot.tree.numpy() & sc.planted).sum())}")
    lines.append("")
    lines.append("averaging against chaining (1 degree of noise per axis, nothing planted): largest error to the true rotations, degrees")
    lines.append("scene                | oracle: tree  averaged | host routine: tree  averaged  outer iterations")
    for sc in RC.chain_scenes():
        o = runs[sc.name]
        start, rot = loftr_amd.average_rotations(*sc.args, max_iters=0), loftr_amd.average_rotations(*sc.args)
        e = [float(global_rotation_errors(x, sc.R_gt).max()) for x in (o["R_start"], o["R"], start.R, rot.R)]
        lines.append(f"{sc.name:20s} | {e[0]:12.2f}  {e[1]:8.2f} | {e[2]:18.2f}  {e[3]:8.2f}  {rot.stats['n_iters']:16d}")
    print("\n".join(lines))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="*", default=[200, 2000, 10000])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--accuracy", action="store_true", help="CPU: the host routine against the numpy oracle")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    lines = accuracy() if args.accuracy else bench(args.sizes, not args.no_host)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
