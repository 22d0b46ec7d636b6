#!/usr/bin/env python
"""Track splitting (loftr_amd/splitting.py, csrc/split_gpu.hip) on a MegaDepth-1500-shaped load.  One JSON line.

    python tools/micro/split_bench.py [--rows 1500] [--matches 1000] [--share 0.3] [--rounds 32] [--no-host] [--out FILE]

Load: the atlas of tools/micro/atlas_bench.py (806 images of 640 x 480, 2 px cells, 1500 rows of about 1000 matches, the same seed): its
kept matches as edges between global keypoints, its tracks and its own track_ok.  That atlas has few inconsistent tracks of its own
(its rows share points by a random draw, not by geometry), so the tool also marks a random `--share` of the consistent tracks
inconsistent: the rule is defined on the flags, and such a track grows back to what it was.  The figures therefore describe the
rounds over a load of this size, not what splitting is worth on a scene; that is profiles/split_accuracy.txt.

Reported: the launch classes (device events inside loftr_split_tracks, a round's four launches summed over the rounds, medians of 5 calls
after a warm-up), the counts, the rounds used, and the host routine on one core, compared equal inside the tool."""
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
from tools.micro.atlas_bench import HW, make_chunks                    # noqa: E402

CELL, DEV = 2.0, torch.device("cuda")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--share", type=float, default=0.3, help="share of the consistent tracks that is marked inconsistent as well")
    ap.add_argument("--rounds", type=int, default=32)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    pairs = np.load(os.path.join(ROOT, "tests", "golden", "pair_lists.npz"))["megadepth_pairs"][:args.rows].astype(np.int64)
    n, chunks = make_chunks(pairs, args.matches)
    atlas = KeypointAtlas(n, HW, CELL, device=DEV)
    for ids, data in chunks:
        atlas.add(ids, data)
    sfm = atlas.finalize(min_track_len=2)
    g = torch.Generator(device=DEV).manual_seed(1)
    own = int((~sfm.track_ok).sum())
    ok = (sfm.track_ok & (torch.rand(sfm.track_ok.numel(), device=DEV, generator=g) >= args.share)).to(torch.uint8)
    a = (sfm.edge_keypoints().contiguous(), sfm.match_conf.contiguous(), sfm.keypoint_image().to(torch.int32), sfm.track_id.contiguous(), ok)
    tail = (n, 2, args.rounds)
    out = {"workload": "split_megadepth1500_shape", "images": n, "keypoints": int(a[2].numel()), "edges": int(a[1].numel()),
           "tracks": int(ok.numel()), "inconsistent_in_the_atlas": own, "marked_inconsistent": int((ok == 0).sum()), "max_rounds": args.rounds}
    ops.split_tracks(*a, *tail)                                          # warm-up (kernel load)
    runs, wall = [], []
    for _ in range(5):
        stages = []
        res = ops.split_tracks(*a, *tail, timings=stages)
        runs.append([v for _, v in stages])
        torch.cuda.synchronize()
        t = time.perf_counter()
        ops.split_tracks(*a, *tail)
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t))
    med = np.median(np.array(runs), 0)
    out["kernel_ms"] = {k: round(float(v), 4) for k, v in zip(ops.SPLIT_STAGES, med)}
    out["kernels_total_ms"] = round(float(med.sum()), 4)
    out["call_wall_ms_untimed"] = round(float(np.median(wall)), 4)
    counts = res["counts"].cpu().tolist()
    out["counts"] = dict(zip(ops.SPLIT_NAMES, counts))
    out["round_accepted"] = [v for v in res["round_accepted"].cpu().tolist() if v]
    if not args.no_host:
        host = [x.cpu().numpy() for x in a]
        t = time.perf_counter()
        want = ops.split_tracks_host(*host, *tail)
        out["host_routine_ms"] = round(1e3 * (time.perf_counter() - t), 1)
        out["identical_to_host"] = bool(all(np.array_equal(res[k].cpu().numpy(), want[k]) for k in want))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
    assert out.get("identical_to_host", True), "the kernels and the host routine disagree"


if __name__ == "__main__":
    main()
