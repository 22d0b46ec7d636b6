#!/usr/bin/env python
"""Track triangulation (loftr_amd/triangulation.py, csrc/triangulate_gpu.hip) on a MegaDepth-1500-shaped load.  One JSON line.

    python tools/micro/triangulation_bench.py [--rows 1500] [--matches 1000] [--outliers 0.1] [--out FILE]

Load: tools/micro/atlas_bench.py's synthetic atlas (1500 rows over 806 images) gives the TRACK LENGTHS -- its points carry no consistent
geometry (every image has its own random points), so the observations are synthetic: one exact camera per image (f in [450, 650],
rotations up to 20 degrees, centres in [-2,2] x [-1,1] x [-0.5,0.5]), one 3D point per track in [-2,2] x [-1.5,1.5] x [3,8], every
observation in a random image, projected, with 0.5 px of noise; --outliers of the observations at positions >= 2 are displaced 15-80 px.

Reported: the track-length histogram, the device-event time of each kernel (events inside loftr_triangulate_tracks; median of 5 calls
after a warm-up) for the shipped rule (group 0: 8 lanes per track of at most 64 observations, 64 lanes beyond) and with one group size forced
for every track, the wall time of triangulate_tracks with its one readback, the host routine (loftr_triangulate_tracks_host, one core)
on the same input for orientation, and whether every output compared equal inside the tool."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from loftr_amd import KeypointAtlas, Points3D, triangulate_tracks        # noqa: E402
from tools.micro.atlas_bench import DEV, HW, make_chunks                 # noqa: E402


def rotations(rng, n, max_deg):
    axis = rng.standard_normal((n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = np.radians(rng.uniform(0, max_deg, n))[:, None, None]
    A = np.zeros((n, 3, 3))
    A[:, 0, 1], A[:, 0, 2], A[:, 1, 0], A[:, 1, 2], A[:, 2, 0], A[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    return np.eye(3) + np.sin(ang) * A + (1 - np.cos(ang)) * (A @ A)


def make_load(track_len, n_images, outliers, seed=0):
    rng = np.random.default_rng(seed)
    R = rotations(rng, n_images, 20.0)
    c = rng.uniform([-2, -1, -0.5], [2, 1, 0.5], (n_images, 3))
    K = np.tile(np.eye(3), (n_images, 1, 1))
    K[:, 0, 0] = K[:, 1, 1] = rng.uniform(450, 650, n_images)
    K[:, 0, 2], K[:, 1, 2] = 320.0, 240.0
    T = np.tile(np.eye(4), (n_images, 1, 1))
    T[:, :3, :3] = R
    T[:, :3, 3] = -(R @ c[:, :, None])[:, :, 0]
    K, T = torch.from_numpy(K).to(DEV), torch.from_numpy(T).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    lens = track_len.to(DEV, torch.int64)
    n_tracks = lens.numel()
    offsets = torch.zeros(n_tracks + 1, dtype=torch.int64, device=DEV)
    offsets[1:] = torch.cumsum(lens, 0)
    N = int(offsets[-1])
    track = torch.repeat_interleave(torch.arange(n_tracks, device=DEV), lens)
    pos = torch.arange(N, device=DEV) - offsets[track]
    lo, hi = torch.tensor([-2, -1.5, 3.0], device=DEV, dtype=torch.float64), torch.tensor([2, 1.5, 8.0], device=DEV, dtype=torch.float64)
    X = lo + (hi - lo) * torch.rand(n_tracks, 3, device=DEV, dtype=torch.float64, generator=g)
    image = torch.randint(0, n_images, (N,), device=DEV, generator=g)
    p = torch.einsum("nij,nj->ni", K[image], torch.einsum("nij,nj->ni", T[image, :3, :3], X[track]) + T[image, :3, 3])
    xy = p[:, :2] / p[:, 2:] + 0.5 * torch.randn(N, 2, device=DEV, dtype=torch.float64, generator=g)
    out = (pos >= 2) & (torch.rand(N, device=DEV, generator=g) < outliers)
    ang = 2 * np.pi * torch.rand(N, device=DEV, dtype=torch.float64, generator=g)
    r = 15 + 65 * torch.rand(N, device=DEV, dtype=torch.float64, generator=g)
    xy = xy + out[:, None] * r[:, None] * torch.stack([torch.cos(ang), torch.sin(ang)], 1)
    return offsets, image.to(torch.int32), xy.to(torch.float32), K, T


def histogram(lens):
    lens = lens.cpu().numpy()
    bins = [("2", 2, 2), ("3", 3, 3), ("4", 4, 4), ("5-8", 5, 8), ("9-16", 9, 16), ("17-64", 17, 64), (">64", 65, 1 << 40)]
    return {name: int(((lens >= a) & (lens <= b)).sum()) for name, a, b in bins}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--outliers", type=float, default=0.1)
    ap.add_argument("--thresh", type=float, default=4.0)
    ap.add_argument("--min-angle", type=float, default=1.5)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    pairs = np.load(os.path.join(ROOT, "tests", "golden", "pair_lists.npz"))["megadepth_pairs"][:args.rows].astype(np.int64)
    n_images, chunks = make_chunks(pairs, args.matches)
    atlas = KeypointAtlas(n_images, HW, 2.0, device=DEV)
    for ids, data in chunks:
        atlas.add(ids, data)
    sfm = atlas.finalize(min_track_len=2)
    lens = sfm.track_len[sfm.track_ok]
    del atlas, chunks
    inputs = make_load(lens, n_images, args.outliers)
    out = {"workload": "triangulation_megadepth1500_shape", "images": n_images, "tracks": int(lens.numel()), "observations": int(inputs[0][-1]),
           "longest_track": int(lens.max()), "track_length_histogram": histogram(lens), "outlier_rate": args.outliers, "thresh_px": args.thresh,
           "min_angle_deg": args.min_angle}
    run = lambda group, timings=None: triangulate_tracks(*inputs, args.thresh, args.min_angle, group=group, timings=timings)
    results = {}
    for group in (0, 8, 64):
        run(group)                                                      # warm-up (kernel load)
        stages, wall = [], []
        for _ in range(5):
            timings = []
            torch.cuda.synchronize()
            t = time.perf_counter()
            results[group] = run(group, timings)
            wall.append(1e3 * (time.perf_counter() - t))
            stages.append([ms for _, ms in timings])
        med = np.median(np.array(stages), 0)
        out[f"group_{group}_kernel_ms"] = {name: round(float(v), 4) for (name, _), v in zip(timings, med)}
        out[f"group_{group}_wall_ms"] = round(float(np.median(wall)), 3)
    out["stats"] = results[0].stats
    t = time.perf_counter()
    host = triangulate_tracks(*[x.cpu() for x in inputs], args.thresh, args.min_angle)
    out["host_routine_ms"] = round(1e3 * (time.perf_counter() - t), 1)

    def same(a, b):
        eq = lambda x, y: torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0))
        return all(eq(getattr(a, k).cpu().float(), getattr(b, k).cpu().float()) for k in Points3D.FIELDS) and a.stats == b.stats
    out["identical_to_host"] = bool(all(same(results[g], host) for g in (0, 8, 64)))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
