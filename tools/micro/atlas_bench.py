#!/usr/bin/env python
"""Keypoint atlas (loftr_amd/atlas.py, csrc/atlas_gpu.hip) on a synthetic MegaDepth-1500-shaped load.  One JSON line.

    python tools/micro/atlas_bench.py [--rows 1500] [--matches 1000] [--cell-px 2] [--oracle-rows N] [--no-match-step] [--out FILE]

Load: the pair structure of MegaDepth-1500 (tests/golden/pair_lists.npz: 1500 rows over 806 images), keypoint extents 640 x 480, about
--matches matches per row.  Every image has 3000 fixed "scene points"; a row (a, b) draws its matches among the point ids, side 0 is the
point of image a snapped to the 8 px coarse grid (as LoFTR leaves mkpts0_f), side 1 the point of image b plus 0.5 px of noise, confidences
uniform in (0.2, 1] -- so points repeat across the rows of an image and tracks form.  The matches are made on the GPU, 8 rows per add.

Reported: add per 8-row chunk (device events around every add; the storage is pre-sized, then a second pass grows from 4096 matches),
finalize in total (wall, with its one readback) and per stage (device events inside loftr_atlas_finalize), the grid bytes, the wall time
of the host routine (loftr_atlas_host, one core) and of the numpy / Python oracle (tests/_atlas_oracle.py: what callers write today,
--oracle-rows rows of the same data, 0 = all) with the copy of every chunk off the device, and add per chunk as a fraction of the 8-pair
match step (LoFTR.match_pairs of 8 pairs of 640 x 480 images from a FeatureBank, tools/micro/pairs_bench.py's model) of the same run.
The result is checked equal to the host routine's inside the tool."""
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

from loftr_amd import KeypointAtlas                                    # noqa: E402

DEV = "cuda:0"
HW = (480, 640)
BATCH = 8


def make_chunks(pairs, matches, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    n_images, n_pts = int(pairs.max()) + 1, 3000
    pts = torch.rand(n_images, n_pts, 2, device=DEV, generator=g) * torch.tensor([HW[1] - 1.0, HW[0] - 1.0], device=DEV)
    chunks = []
    for s in range(0, len(pairs), BATCH):
        ids = pairs[s:s + BATCH]
        k0, k1, conf, bids = [], [], [], []
        for i, (a, b) in enumerate(ids):
            m = int(matches * (0.5 + torch.rand(1, device=DEV, generator=g).item()))
            j = torch.randint(0, n_pts, (m,), device=DEV, generator=g)
            k0.append(torch.floor(pts[a, j] / 8) * 8)
            k1.append(pts[b, j] + 0.5 * torch.randn(m, 2, device=DEV, generator=g))
            conf.append(0.2 + 0.8 * torch.rand(m, device=DEV, generator=g))
            bids.append(torch.full((m,), i, dtype=torch.long, device=DEV))
        chunks.append((ids, {"mkpts0_f": torch.cat(k0), "mkpts1_f": torch.cat(k1), "mconf": torch.cat(conf), "m_bids": torch.cat(bids)}))
    return n_images, chunks


def add_all(atlas, chunks):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in chunks]
    host = []
    torch.cuda.synchronize()
    for (ids, data), (e0, e1) in zip(chunks, ev):
        t = time.perf_counter()
        e0.record()
        atlas.add(ids, data)
        e1.record()
        host.append(time.perf_counter() - t)
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev]), 1e3 * np.array(host)


def spread(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(np.min(x)), 4), "max": round(float(np.max(x)), 4)}


def match_step_ms():
    from tools.micro.pairs_bench import Images, build
    from loftr_amd import FeatureBank
    model, load = build(False), Images(HW, False)
    bank = FeatureBank(model, 16, HW)
    bank.add(load(list(range(16)))["image"], slots=list(range(16)))
    ms = []
    for k in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        data = model.match_pairs(bank, list(range(8)), bank, list(range(8, 16)))
        e1.record()
        torch.cuda.synchronize()
        if k >= 2:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), int(data["mconf"].shape[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--cell-px", type=float, default=2.0)
    ap.add_argument("--oracle-rows", type=int, default=0, help="rows given to the Python oracle (0: all)")
    ap.add_argument("--no-match-step", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    pairs = np.load(os.path.join(ROOT, "tests", "golden", "pair_lists.npz"))["megadepth_pairs"][:args.rows].astype(np.int64)
    n_images, chunks = make_chunks(pairs, args.matches)
    M = sum(d["mconf"].numel() for _, d in chunks)
    out = {"workload": "atlas_megadepth1500_shape", "rows": len(pairs), "images": n_images, "extent_hw": list(HW), "cell_px": args.cell_px,
           "matches": M, "grid_bytes": KeypointAtlas.bytes_needed(n_images, HW, args.cell_px)}

    # warm-up (kernel load), then the timed passes: storage pre-sized / grown from the default capacity
    a = KeypointAtlas(n_images, HW, args.cell_px, device=DEV)
    add_all(a, chunks[:4])
    a.finalize()
    a = KeypointAtlas(n_images, HW, args.cell_px, device=DEV, capacity=M)
    dev_ms, host_ms = add_all(a, chunks)
    out["add_ms_per_chunk"] = spread(dev_ms)
    out["add_host_ms_per_chunk"] = spread(host_ms)
    stages = []
    torch.cuda.synchronize()
    t = time.perf_counter()
    sfm = a.finalize(min_track_len=2, timings=stages)
    torch.cuda.synchronize()
    out["finalize_wall_ms"] = round(1e3 * (time.perf_counter() - t), 3)
    out["finalize_stage_ms"] = {k: round(v, 4) for k, v in stages}
    out["finalize_gpu_ms"] = round(sum(v for _, v in stages), 3)
    out["stats"] = sfm.stats
    a = KeypointAtlas(n_images, HW, args.cell_px, device=DEV)
    dev_ms, _ = add_all(a, chunks)
    out["add_ms_per_chunk_growing"] = spread(dev_ms)
    out["add_ms_growing_total"] = round(float(dev_ms.sum()), 3)
    t = time.perf_counter()
    sfm2 = a.finalize(min_track_len=2)
    torch.cuda.synchronize()
    out["finalize_wall_ms_untimed"] = round(1e3 * (time.perf_counter() - t), 3)
    got = sfm.to_host()

    # the host routine on the same data (what defines the result), the chunks copied off the device first
    t = time.perf_counter()
    host_chunks = [(ids, {k: v.cpu() for k, v in d.items()}) for ids, d in chunks]
    out["copy_chunks_off_device_ms"] = round(1e3 * (time.perf_counter() - t), 3)
    h = KeypointAtlas(n_images, HW, args.cell_px, device="cpu")
    for ids, d in host_chunks:
        h.add(ids, d)
    t = time.perf_counter()
    want = h.finalize(min_track_len=2).to_host()
    out["host_routine_ms"] = round(1e3 * (time.perf_counter() - t), 3)
    same = all(np.array_equal(got[k], want[k]) for k in want if k != "stats") and got["stats"] == want["stats"]
    same2 = all(np.array_equal(v, want[k]) for k, v in sfm2.to_host().items() if k != "stats")
    out["identical_to_host"] = bool(same and same2)

    # what callers write today: numpy / Python on the host (the tests' oracle)
    from _atlas_oracle import atlas_oracle
    n_or = len(host_chunks) if args.oracle_rows <= 0 else max(1, args.oracle_rows // BATCH)
    sub = [(ids, d["mkpts0_f"].numpy(), d["mkpts1_f"].numpy(), d["mconf"].numpy(), d["m_bids"].numpy(), None) for ids, d in host_chunks[:n_or]]
    t = time.perf_counter()
    ref = atlas_oracle(sub, n_images, HW, args.cell_px, 2)
    out["python_oracle_ms"] = round(1e3 * (time.perf_counter() - t), 1)
    out["python_oracle_rows"] = int(sum(len(ids) for ids, *_ in sub))
    if n_or == len(host_chunks):
        out["identical_to_oracle"] = bool(all(np.array_equal(got[k], ref[k]) for k in ref if k != "stats"))

    if not args.no_match_step:
        ms, m8 = match_step_ms()
        out["match_step_8_pairs_ms"] = round(ms, 3)
        out["match_step_matches"] = m8
        out["add_fraction_of_match_step"] = round(out["add_ms_per_chunk"]["median"] / ms, 5)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
