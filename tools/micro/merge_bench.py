#!/usr/bin/env python
"""Track merging (loftr_amd/merging.py, csrc/merge_gpu.hip) on a MegaDepth-1500-shaped load.  One JSON line.

    python tools/micro/merge_bench.py [--rows 1500] [--matches 1000] [--posed 422] [--points 0.437] [--no-host] [--out FILE]

Load: exactly that of tools/micro/completion_bench.py (the keypoint pool and the consistent tracks of tools/micro/atlas_bench.py's atlas,
its cameras, posed images and random points, the same seed), with what merging adds: obs_xy is the keypoint of every observation and
obs_mask is 1 at every observation of a row with a point.  That load has NO geometry: a row's point is a random place, not where its
keypoints say, so a projection meets another row's keypoint by the pool's density alone, the meeting rows' points are far apart and the
agreement test fails at the first observation it looks at.  The figures therefore describe the search and the disjoint walk, not a
reconstruction; what merging is worth on a real scene is not measured here.

Reported: the five launches (device events inside loftr_merge_tracks, medians of 5 calls after a warm-up), the eight counts, projections
per second, and the host routine on one core, compared equal inside the tool."""
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
from tools.micro.completion_bench import CELL, DEV, THRESH, cameras    # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--posed", type=int, default=422)
    ap.add_argument("--points", type=float, default=0.437, help="share of the rows with a point (254 370 of 582 152 in DESIGN §19)")
    ap.add_argument("--no-host", action="store_true")
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
    row = torch.repeat_interleave(torch.arange(n_rows, device=DEV), offsets[1:] - offsets[:-1])
    kp = sfm.kp_offsets[image] + local
    kp_row = torch.full((n_kp,), -1, dtype=torch.int32, device=DEV)
    kp_row[kp] = row.to(torch.int32)
    obs_xy, obs_mask = sfm.keypoints[kp].contiguous(), has[row].to(torch.uint8)
    kp_cell, cells = ops.model_cells(sfm.kp_offsets, sfm.keypoints, kp_row, n_rows, gh, gw, inv)
    assert int(cells) == 0
    reach = default_reach(THRESH, CELL)
    a = (offsets, image.to(torch.int32), obs_xy, obs_mask, xyz, status, sfm.kp_offsets, sfm.keypoints, kp_cell, kp_row, K, T, posed)
    tail = (gh, gw, inv, THRESH, reach)
    out = {"workload": "merge_megadepth1500_shape", "images": n, "rows": n_rows, "observations": int(image.numel()), "keypoints": n_kp,
           "rows_with_a_point": int(has.sum()), "posed_images": int(posed.sum()), "thresh_px": THRESH, "cell_px": CELL, "reach": reach}
    ops.merge_tracks(*a, *tail)                                          # warm-up (kernel load)
    runs = []
    for _ in range(5):
        stages = []
        res = ops.merge_tracks(*a, *tail, timings=stages)
        runs.append([v for _, v in stages])
    med = np.median(np.array(runs), 0)
    out["kernel_ms"] = {k: round(float(v), 4) for k, v in zip(ops.MERGE_STAGES, med)}
    out["kernels_total_ms"] = round(float(med.sum()), 4)
    counts = res["counts"].cpu().tolist()
    out["counts"] = dict(zip(ops.MERGE_NAMES, counts))
    out["projections_per_s"] = round(counts[3] / (1e-3 * float(med[ops.MERGE_STAGES.index("meet")])), 1)
    # completion's link kernel on the same load, in the same run: the meet kernel does its search plus the inline tests
    ca = (a[0], a[1], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12])
    ops.complete_tracks(*ca, *tail)
    link = []
    for _ in range(5):
        stages = []
        ops.complete_tracks(*ca, *tail, timings=stages)
        link.append(dict(stages)["link"])
    out["complete_link_ms_same_run"] = round(float(np.median(link)), 4)
    out["meet_over_link"] = round(out["kernel_ms"]["meet"] / out["complete_link_ms_same_run"], 3)
    if not args.no_host:
        host = [x.cpu().numpy() for x in a]
        t = time.perf_counter()
        want = ops.merge_tracks_host(*host, *tail)
        out["host_routine_ms"] = round(1e3 * (time.perf_counter() - t), 1)
        out["identical_to_host"] = bool(np.array_equal(res["row_into"].cpu().numpy(), want["row_into"])
                                        and np.array_equal(res["kp_row_new"].cpu().numpy(), want["kp_row_new"])
                                        and np.array_equal(res["merge_r2"].cpu().numpy().view(np.int32), want["merge_r2"].view(np.int32))
                                        and np.array_equal(res["counts"].cpu().numpy(), want["counts"]))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
    assert out.get("identical_to_host", True), "the kernels and the host routine disagree"


if __name__ == "__main__":
    main()
