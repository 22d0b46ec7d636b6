#!/usr/bin/env python
"""LoFTR.refine_points (loftr_amd/pairs.py, csrc/refine_gpu.hip) beside LoFTR.match_pairs on one 8-pair chunk.  One JSON line.

    python tools/micro/refine_bench.py [--jobs 1000] [--repeats 7] [--out FILE]

Load: a chunk of MegaDepth-1500's shape, as tools/micro/pairs_bench.py workload (c) builds it: 8 pairs over 16 distinct seeded images of
840 x 840 in a feature bank, rows >= 560 zero, coarse masks, scale 1.9, temp_bug_fix False, border_rm 2, the bench's seeded weights.
The jobs are synthetic: --jobs point pairs per image pair (default 1000, about what a MegaDepth row keeps), uniform over the valid part
of both images, so the fine windows sit anywhere, not on coarse cells.  With seeded weights the refined positions mean nothing; the
tool times the path.

Reported, all from one run, after a warm-up of every shape, medians of --repeats alternating passes with the spread (device events
around each call, ended by a synchronise): ms per chunk of refine_points and of match_pairs on the same chunk; ms of
ops.fine_preprocess_gather_at (the window gather at given centres with the coarse gather and the two projections behind it) and of its
twin ops.fine_preprocess_gather on the same number of windows; the bytes the window gather moves.  The time of the gather kernel alone
(refine_windows_at_kernel) comes from a kernel trace of this tool in a run of its own (rocprofv3 --kernel-trace --stats -- python
tools/micro/refine_bench.py --repeats 3); profiles/refine_bench.txt holds both.  Recorded, not judged: nobody had timed this path."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from loftr_amd import FeatureBank, ops                                 # noqa: E402
from tools.micro.pairs_bench import BATCH, DEV, Images, build          # noqa: E402

HW = (840, 840)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--jobs", type=int, default=1000, help="point pairs per image pair")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("refine_bench: needs a GPU (a timing taken elsewhere says nothing)")
    model = build(outdoor=True)
    load = Images(HW, outdoor=True)
    bank = FeatureBank(model, 2 * BATCH, HW)
    batch = load(list(range(2 * BATCH)))
    slots = bank.add(batch["image"], mask=batch["mask"], scale=batch["scale"])
    ids0, ids1 = slots[:BATCH], slots[BATCH:]
    g = torch.Generator(device=DEV).manual_seed(3)
    M = BATCH * args.jobs
    b_ids = torch.repeat_interleave(torch.arange(BATCH), args.jobs)      # on the host: checked there, no readback
    span = torch.tensor([HW[1] * 1.9 - 1, 560 * 1.9 - 1], device=DEV)    # the valid part, in the scaled coordinates forward returns
    pts0, pts1 = (torch.rand(M, 2, device=DEV, generator=g) * span for _ in range(2))

    refine = lambda: model.refine_points(bank, ids0, bank, ids1, b_ids, pts0, pts1)
    match = lambda: model.match_pairs(bank, ids0, bank, ids1)
    res, data = refine(), match()                                        # warm-up of every shape
    torch.cuda.synchronize()
    # the fine preprocess at given centres and its twin on the same number of windows, from the tensors of one refine_points call
    hw_c, hw_f = (bank.h_c, bank.w_c), (bank.h_f, bank.w_f)
    at = ops.refine_centres(pts0, pts1, b_ids.to(DEV), BATCH, hw_f, hw_f, hw_c, hw_c, 4, 2.0, batch["scale"][:BATCH], batch["scale"][:BATCH])
    feat = torch.randn(2 * BATCH, bank.h_c * bank.w_c, bank.coarse.shape[3], device=DEV, generator=g)
    fp = model.fine_preprocess
    w = dict(down_w=fp.down_proj.weight, down_b=fp.down_proj.bias, merge_w=fp.merge_feat.weight, merge_b=fp.merge_feat.bias)
    bd = b_ids.to(DEV)
    f = bank.fine_map()
    gather_at = lambda: ops.fine_preprocess_gather_at(f, ids0, f, ids1, feat[:BATCH], feat[BATCH:], bd, at["i_ids"], at["j_ids"], at["c0"],
                                                      at["c1"], hw_c, hw_c, fp.W, 4, **w)
    gather = lambda: ops.fine_preprocess_gather(f, ids0, f, ids1, feat[:BATCH], feat[BATCH:], bd, at["i_ids"], at["j_ids"], hw_c, hw_c,
                                                fp.W, 4, **w)
    gather_at(), gather()
    torch.cuda.synchronize()
    runs = {"refine_points": [], "match_pairs": [], "fine_preprocess_gather_at": [], "fine_preprocess_gather": []}
    for _ in range(args.repeats):                                        # alternating passes
        for name, fn in (("refine_points", refine), ("match_pairs", match), ("fine_preprocess_gather_at", gather_at),
                         ("fine_preprocess_gather", gather)):
            runs[name].append(timed(fn)[0])
    stat = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)}
    cf = bank.fine.shape[3]
    window_bytes = 2 * M * fp.W * fp.W * cf * (4 + 4)                    # fp32 read, one SP dword written per element
    out = {"workload": "refine_megadepth1500_chunk", "pairs": BATCH, "image_hw": list(HW), "jobs_per_pair": args.jobs, "windows_per_side": M,
           "matches_of_match_pairs": int(data["b_ids"].shape[0]), "ok_rows": int(res["ok"].sum()), "repeats": args.repeats,
           **{k: stat(v) for k, v in runs.items()}, "window_gather_bytes": window_bytes}
    r = out["refine_points"]["median_ms"]
    out["refine_over_match"] = round(r / out["match_pairs"]["median_ms"], 4)
    out["fine_preprocess_at_share_of_refine"] = round(out["fine_preprocess_gather_at"]["median_ms"] / r, 4)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
