#!/usr/bin/env python
"""Track completion (loftr_amd/completion.py, csrc/complete_gpu.hip) on a MegaDepth-1500-shaped load.  One JSON line.

    python tools/micro/completion_bench.py [--rows 1500] [--matches 1000] [--posed 422] [--points 0.437] [--no-host] [--out FILE]

Load: the keypoint pool and the tracks of tools/micro/atlas_bench.py's atlas (806 images of 640 x 480, 2 px cells); its consistent tracks
are the rows.  The atlas's points have no geometry, so the cameras (f in [450, 650], rotations up to 20 degrees, tools/micro/
registration_bench.py's) and the points are made here: --posed images have a pose, a --points share of the rows has a point (status ok)
at a random place in front of the cameras, the others are too_short.  What a projection meets is then a pool of the real density, which
is what the search costs depend on.

Reported: the four launches (device events inside loftr_complete_tracks, medians of 5 calls after a warm-up), the counts, projections
per second and the fp64 rate of the projections alone (20 operations each: three 3-term dot products with their offsets, two
divisions); next to it the same links from a chunked torch composition (a block of rows projected into all images, searchsorted over
kp_cell + image * gh * gw for every cell of the window, an amin over the window, scatter_reduce(amin) of the packed key), compared equal
inside the tool; and the host routine on one core."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from loftr_amd import KeypointAtlas, ops                               # noqa: E402
from loftr_amd.completion import default_reach                         # noqa: E402
from tools.micro.atlas_bench import HW, make_chunks                    # noqa: E402

DEV = "cuda:0"
CELL, THRESH = 2.0, 4.0


def cameras(n, g):
    f = 450 + 200 * torch.rand(n, device=DEV, generator=g)
    K = torch.zeros(n, 3, 3, device=DEV, dtype=torch.float64)
    K[:, 0, 0] = K[:, 1, 1] = f.double()
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 320.0, 240.0, 1.0
    w = torch.randn(n, 3, device=DEV, generator=g, dtype=torch.float64)
    w = w / w.norm(dim=1, keepdim=True) * torch.deg2rad(20 * torch.rand(n, 1, device=DEV, generator=g, dtype=torch.float64))
    Wx = torch.zeros(n, 3, 3, device=DEV, dtype=torch.float64)
    Wx[:, 0, 1], Wx[:, 0, 2], Wx[:, 1, 0], Wx[:, 1, 2], Wx[:, 2, 0], Wx[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    R = torch.linalg.matrix_exp(Wx)
    centre = (torch.rand(n, 3, device=DEV, generator=g, dtype=torch.float64) - 0.5) * torch.tensor([4.0, 2.0, 1.0], device=DEV)
    T = torch.eye(4, device=DEV, dtype=torch.float64).repeat(n, 1, 1)
    T[:, :3, :3], T[:, :3, 3] = R, -(R @ centre[:, :, None])[:, :, 0]
    return K, T


def torch_links(a, gh, gw, inv, thr2, reach, block=512):
    """The same claims from existing torch ops -> claim [K] i64 (2^63 - 1: none).  fp64 elementwise ops in the rule's operation order."""
    offsets, image, xyz, status, kp_offsets, kp, kp_cell, kp_row, K, T, posed = a
    n, n_rows, n_kp = posed.numel(), status.numel(), kp_cell.numel()
    fx, sk, cx, fy, cy = K[:, 0, 0], K[:, 0, 1], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2]
    P0 = (fx[:, None] * T[:, 0] + sk[:, None] * T[:, 1]) + cx[:, None] * T[:, 2]
    P1 = fy[:, None] * T[:, 1] + cy[:, None] * T[:, 2]
    P2 = T[:, 2]
    kp_image = torch.repeat_interleave(torch.arange(n, device=DEV), kp_offsets[1:] - kp_offsets[:-1])
    gkey = kp_cell.to(torch.int64) + kp_image * (gh * gw)                                # ascends over the whole pool
    free = (kp_row == -1) | (status[kp_row.clamp(min=0).long()] != 0)
    src = torch.nonzero((status == 0) & torch.isfinite(xyz).all(1)).reshape(-1)
    track = torch.repeat_interleave(torch.arange(n_rows, device=DEV), offsets[1:] - offsets[:-1])
    none = torch.iinfo(torch.int64).max
    claim = torch.full((n_kp,), none, dtype=torch.int64, device=DEV)
    target_image = (posed != 0) & torch.isfinite(P0).all(1) & torch.isfinite(P1).all(1) & torch.isfinite(P2).all(1)
    dot = lambda P, X: ((P[None, :, 0] * X[:, None, 0] + P[None, :, 1] * X[:, None, 1]) + P[None, :, 2] * X[:, None, 2]) + P[None, :, 3]
    steps = torch.arange(-reach, reach + 1, device=DEV)
    for b in range(0, src.numel(), block):
        rows = src[b:b + block]
        X = xyz[rows].double()
        visited = torch.zeros(n_rows, dtype=torch.long, device=DEV)
        visited[rows] = torch.arange(rows.numel(), device=DEV) + 1
        sel = visited[track] > 0
        seen = torch.zeros(rows.numel(), n, dtype=torch.bool, device=DEV)
        seen[visited[track[sel]] - 1, image[sel].long()] = True
        x, y, z = dot(P0, X), dot(P1, X), dot(P2, X)                                     # [B, n]
        u, v = x / z, y / z
        fu, fv = torch.floor(u.float() * inv), torch.floor(v.float() * inv)
        ok = target_image[None] & ~seen & (z > 0) & (fu >= 0) & (fu < gw) & (fv >= 0) & (fv < gh)
        r, i = torch.nonzero(ok, as_tuple=True)
        cxs, cys, uu, vv = fu[r, i].long(), fv[r, i].long(), u[r, i], v[r, i]
        best = torch.full((r.numel(),), none, dtype=torch.int64, device=DEV)
        for dy in steps:
            for dx in steps:
                xx, yy = cxs + dx, cys + dy
                inside = (xx >= 0) & (xx < gw) & (yy >= 0) & (yy < gh)
                want = (yy * gw + xx + i * (gh * gw)).clamp(min=0)
                k = torch.searchsorted(gkey, want).clamp(max=n_kp - 1)
                hit = inside & (gkey[k] == want)
                du, dv = uu - kp[k, 0].double(), vv - kp[k, 1].double()
                r2 = du * du + dv * dv
                good = hit & (r2 <= thr2) & free[k]
                word = (r2.float().view(torch.int32).long() << 32) | k
                best = torch.where(good & (word < best), word, best)
        has = best != none
        k = best[has] & 0xFFFFFFFF
        key = (best[has] >> 32 << 32) | rows[r[has]]
        claim.scatter_reduce_(0, k, key, "amin")
    return claim


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--posed", type=int, default=422)
    ap.add_argument("--points", type=float, default=0.437, help="share of the rows with a point (254 370 of 582 152 in DESIGN §19)")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    pairs = np.load(os.path.join(ROOT, "tests", "golden", "pair_lists.npz"))["megadepth_pairs"][:args.rows].astype(np.int64)
    n, chunks = make_chunks(pairs, args.matches)
    atlas = KeypointAtlas(n, HW, CELL, device=DEV)
    for ids, data in chunks:
        atlas.add(ids, data)
    sfm = atlas.finalize(min_track_len=2)
    inv, gh, gw = atlas.inv, atlas.gh, atlas.gw
    g = torch.Generator(device=DEV).manual_seed(1)
    K, T = cameras(n, g)
    offsets, image, local = sfm.tracks()
    n_rows, n_kp = offsets.numel() - 1, sfm.keypoints.shape[0]
    posed = torch.zeros(n, dtype=torch.uint8, device=DEV)
    posed[torch.randperm(n, device=DEV, generator=g)[:args.posed]] = 1
    has = torch.rand(n_rows, device=DEV, generator=g) < args.points
    status = torch.where(has, 0, 1).to(torch.uint8)
    X = torch.rand(n_rows, 3, device=DEV, generator=g) * torch.tensor([4.0, 3.0, 5.0], device=DEV) + torch.tensor([-2.0, -1.5, 3.0], device=DEV)
    xyz = torch.where(has[:, None], X, torch.full_like(X, float("nan")))
    kp_row = torch.full((n_kp,), -1, dtype=torch.int32, device=DEV)
    kp_row[sfm.kp_offsets[image] + local] = torch.repeat_interleave(torch.arange(n_rows, device=DEV), offsets[1:] - offsets[:-1]).to(torch.int32)
    kp_cell, cells = ops.model_cells(sfm.kp_offsets, sfm.keypoints, kp_row, n_rows, gh, gw, inv)
    assert int(cells) == 0
    reach = default_reach(THRESH, CELL)
    a = (offsets, image.to(torch.int32), xyz, status, sfm.kp_offsets, sfm.keypoints, kp_cell, kp_row, K, T, posed)
    tail = (gh, gw, inv, THRESH, reach)
    out = {"workload": "completion_megadepth1500_shape", "images": n, "rows": n_rows, "observations": int(image.numel()), "keypoints": n_kp,
           "rows_with_a_point": int(has.sum()), "posed_images": int(posed.sum()), "thresh_px": THRESH, "cell_px": CELL, "reach": reach}
    ops.complete_tracks(*a, *tail)                                       # warm-up (kernel load)
    runs = []
    for _ in range(5):
        stages = []
        res = ops.complete_tracks(*a, *tail, timings=stages)
        runs.append([v for _, v in stages])
    med = np.median(np.array(runs), 0)
    out["kernel_ms"] = {k: round(float(v), 4) for k, v in zip(ops.COMPLETE_STAGES, med)}
    out["kernels_total_ms"] = round(float(med.sum()), 4)
    counts = res["counts"].cpu().tolist()
    out["counts"] = dict(zip(ops.COMPLETE_NAMES, counts))
    link_s = 1e-3 * float(med[ops.COMPLETE_STAGES.index("link")])
    out["projections_per_s"] = round(counts[3] / link_s, 1)
    out["projection_fp64_gflops"] = round(20 * counts[3] / link_s / 1e9, 3)

    if not args.no_torch:
        thr2 = THRESH * THRESH
        torch_links(a, gh, gw, inv, thr2, reach)
        ev = []
        for _ in range(3):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            claim = torch_links(a, gh, gw, inv, thr2, reach)
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1))
        out["torch_composition_gpu_ms"] = round(float(np.median(ev)), 3)
        won = claim != torch.iinfo(torch.int64).max
        rows_t = torch.where(won, (claim & 0xFFFFFFFF).to(torch.int32), kp_row)
        bits_t = torch.where(won, (claim >> 32).to(torch.int32), torch.full_like(kp_row, 0x7FC00000))
        out["identical_to_torch_composition"] = bool(torch.equal(rows_t, res["kp_row_new"]) and torch.equal(bits_t, res["link_r2"].view(torch.int32)))

    if not args.no_host:
        host = [x.cpu().numpy() for x in a]
        t = time.perf_counter()
        want = ops.complete_tracks_host(*host, *tail)
        out["host_routine_ms"] = round(1e3 * (time.perf_counter() - t), 1)
        out["identical_to_host"] = bool(np.array_equal(res["kp_row_new"].cpu().numpy(), want["kp_row_new"])
                                        and np.array_equal(res["link_r2"].cpu().numpy().view(np.int32), want["link_r2"].view(np.int32))
                                        and np.array_equal(res["counts"].cpu().numpy(), want["counts"]))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
    assert out.get("identical_to_torch_composition", True), "the kernels and the torch composition disagree"
    assert out.get("identical_to_host", True), "the kernels and the host routine disagree"


if __name__ == "__main__":
    main()
