#!/usr/bin/env python
"""View overlap (loftr_amd/proposals.py, csrc/overlap_gpu.hip) at the MegaDepth-1500 shape of DESIGN §19.  One JSON line.

    python tools/micro/overlap_bench.py [--images 806] [--points 250000] [--visible 800] [--no-host] [--no-torch] [--out FILE]

Load: --images cameras (f in [450, 650], rotations up to 20 degrees, tools/micro/completion_bench.py's) that are sources and targets
(m = n), --points points in front of them, and per image a list of --visible random points among those that project into it.

Reported: the three launches (device events inside loftr_view_overlap, medians of 5 calls after a warm-up), the counts, point tests per
second; next to it the same table from a chunked torch composition (the entries of a block of sources projected into all targets as
[E, m] fp64 tensors in the rule's operation order, boolean masks, index_add_ per source), compared equal inside the tool; and the host
routine on one core, compared equal as well."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from loftr_amd import ops, proposals                                   # noqa: E402
from tools.micro.completion_bench import cameras                       # noqa: E402

DEV = "cuda:0"
HW = (480.0, 640.0)
BORDER, MAX_ANGLE, MAX_SCALE = 0.0, 45.0, 2.0


def tables(K, T):
    fx, sk, cx, fy, cy = K[:, 0, 0], K[:, 0, 1], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2]
    P0 = (fx[:, None] * T[:, 0] + sk[:, None] * T[:, 1]) + cx[:, None] * T[:, 2]
    P1 = fy[:, None] * T[:, 1] + cy[:, None] * T[:, 2]
    C = torch.stack([-((T[:, 0, r] * T[:, 0, 3] + T[:, 1, r] * T[:, 1, 3]) + T[:, 2, r] * T[:, 2, 3]) for r in range(3)], 1)
    return P0, P1, T[:, 2], C, fx * fx


def visibility(K, T, X, per_image, g, block=32):
    """Per image `per_image` random points among those that project into it -> (vis_offsets [n+1] i64, vis_point [V] i32)."""
    P0, P1, P2, _, _ = tables(K, T)
    Xd = X.double()
    dot = lambda P: ((P[:, None, 0] * Xd[None, :, 0] + P[:, None, 1] * Xd[None, :, 1]) + P[:, None, 2] * Xd[None, :, 2]) + P[:, None, 3]
    lists = []
    for b in range(0, K.shape[0], block):
        s = slice(b, b + block)
        x, y, z = dot(P0[s]), dot(P1[s]), dot(P2[s])
        seen = (z > 0) & (x / z >= 0) & (x / z < HW[1]) & (y / z >= 0) & (y / z < HW[0])
        score = torch.where(seen, torch.rand(seen.shape, device=DEV, generator=g), torch.full(seen.shape, -1.0, device=DEV))
        top = torch.topk(score, min(per_image, X.shape[0]), dim=1)
        lists += [top.indices[r][top.values[r] >= 0] for r in range(seen.shape[0])]
    offsets = torch.zeros(K.shape[0] + 1, dtype=torch.int64, device=DEV)
    offsets[1:] = torch.cumsum(torch.tensor([len(v) for v in lists], device=DEV), 0)
    return offsets, torch.cat(lists).to(torch.int32)


def torch_overlap(vis_offsets, vis_point, xyz, point_ok, K, T, hw, border, cos_min, max_scale2, block=8):
    """The same table from existing torch ops -> overlap [n, n] i32.  fp64 element-wise ops in the rule's operation order."""
    n = K.shape[0]
    P0, P1, P2, C, f2 = tables(K, T)
    valid = torch.isfinite(P0).all(1) & torch.isfinite(P1).all(1) & torch.isfinite(P2).all(1) & torch.isfinite(C).all(1)
    source = torch.repeat_interleave(torch.arange(n, device=DEV), vis_offsets[1:] - vis_offsets[:-1])
    p = vis_point.long()
    usable = (point_ok[p] != 0) & torch.isfinite(xyz[p]).all(1) & valid[source]
    overlap = torch.zeros(n, n, dtype=torch.int32, device=DEV)
    dot = lambda P, X: ((P[None, :, 0] * X[:, None, 0] + P[None, :, 1] * X[:, None, 1]) + P[None, :, 2] * X[:, None, 2]) + P[None, :, 3]
    dot3 = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    hi_u, hi_v = hw[:, 1] - border, hw[:, 0] - border
    for b in range(0, n, block):
        e = torch.nonzero(usable & (source >= b) & (source < b + block)).reshape(-1)
        X, src = xyz[p[e]].double(), source[e]
        a = [C[src, k] - X[:, k] for k in range(3)]
        aa = dot3(a, a)
        x, y, z = dot(P0, X), dot(P1, X), dot(P2, X)                                     # [E, n]
        u, v = x / z, y / z
        good = valid[None] & (z > 0) & (u >= border) & (u < hi_u[None]) & (v >= border) & (v < hi_v[None])
        bv = [C[None, :, k] - X[:, None, k] for k in range(3)]
        bb, d = dot3(bv, bv), dot3([t[:, None] for t in a], bv)
        good &= d >= cos_min * torch.sqrt(aa[:, None] * bb)
        sj, si = f2[None] * aa[:, None], f2[src][:, None] * bb
        good &= (sj <= max_scale2 * si) & (si <= max_scale2 * sj)
        overlap.index_add_(0, src, good.to(torch.int32))
    return overlap


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=806)
    ap.add_argument("--points", type=int, default=250000)
    ap.add_argument("--visible", type=int, default=800)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    n = args.images
    g = torch.Generator(device=DEV).manual_seed(1)
    K, T = cameras(n, g)
    X = torch.rand(args.points, 3, device=DEV, generator=g) * torch.tensor([4.0, 3.0, 5.0], device=DEV) + torch.tensor([-2.0, -1.5, 3.0], device=DEV)
    vis_offsets, vis_point = visibility(K, T, X, args.visible, g)
    ok = torch.ones(n, dtype=torch.uint8, device=DEV)
    point_ok = torch.ones(args.points, dtype=torch.uint8, device=DEV)
    hw = torch.tensor(HW, dtype=torch.float64, device=DEV).expand(n, 2).contiguous()
    cos_min, max_scale2 = math.cos(math.radians(MAX_ANGLE)), MAX_SCALE * MAX_SCALE
    a = (vis_offsets, vis_point, X, point_ok, K.reshape(n, 9), T.reshape(n, 16), ok, K.reshape(n, 9), T.reshape(n, 16), ok, hw, BORDER, cos_min,
         max_scale2)
    out = {"workload": "view_overlap_megadepth1500_shape", "images": n, "views": n, "points": args.points, "entries": int(vis_point.numel()),
           "max_angle_deg": MAX_ANGLE, "max_scale": MAX_SCALE, "border_px": BORDER}
    ops.view_overlap(*a)                                                # warm-up (kernel load)
    runs = []
    for _ in range(5):
        stages = []
        res = ops.view_overlap(*a, timings=stages)
        runs.append([v for _, v in stages])
    med = np.median(np.array(runs), 0)
    out["kernel_ms"] = {k: round(float(v), 4) for k, v in zip(ops.OVERLAP_STAGES, med)}
    out["kernels_total_ms"] = round(float(med.sum()), 4)
    counts = res["counts"].cpu().tolist()
    out["counts"] = {k: counts[i] for i, k in enumerate(ops.OVERLAP_NAMES)}
    tests = counts[0] * counts[3]
    out["point_tests"] = tests
    out["point_tests_per_s"] = round(tests / (1e-3 * float(med[ops.OVERLAP_STAGES.index("count")])), 1)
    pairs, _ = proposals.select_pairs(res["overlap"], top_k=5, min_shared=30)
    out["pairs_selected_top5_min30"] = int(pairs.shape[0])

    if not args.no_torch:
        t_args = (vis_offsets, vis_point, X, point_ok, K, T, hw, BORDER, cos_min, max_scale2)
        torch_overlap(*t_args)
        ev = []
        for _ in range(3):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            want = torch_overlap(*t_args)
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1))
        out["torch_composition_gpu_ms"] = round(float(np.median(ev)), 3)
        out["identical_to_torch_composition"] = bool(torch.equal(want, res["overlap"]))

    if not args.no_host:
        torch.set_num_threads(1)
        host = [x.cpu() if isinstance(x, torch.Tensor) else x for x in a]
        t = time.perf_counter()
        want = ops.view_overlap(*host)
        out["host_routine_ms"] = round(1e3 * (time.perf_counter() - t), 1)
        out["identical_to_host"] = bool(all(torch.equal(res[k].cpu(), want[k]) for k in ("overlap", "n_vis", "counts")))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
    assert out.get("identical_to_torch_composition", True), "the kernels and the torch composition disagree"
    assert out.get("identical_to_host", True), "the kernels and the host routine disagree"


if __name__ == "__main__":
    main()
