#!/usr/bin/env python
"""Localisation against a triangulated model (loftr_amd/localization.py, csrc/model_lookup_gpu.hip) on a synthetic Aachen-shaped load.
One JSON line.

    python tools/micro/model_lookup_bench.py [--queries 1000] [--rows 20] [--matches 1000] [--images 800] [--host-queries N]
                                             [--oracle-queries N] [--out FILE]

Load: a model of --images images with extents 640 x 480 and 2 px cells, about 2300 keypoints per image at random cells, 70 % of them
with a 3D point; the points of image i are drawn from a window of point ids that overlaps its neighbours', so that the database images
of a query share points and the fusion has work.  Query q has its own camera and --rows database rows (consecutive images); a row has
about --matches matches: 80 % sit in the cell of a keypoint of the database image (the query point is then the projection of that
keypoint's 3D point plus 0.5 px of noise, 15 % of them displaced as outliers), 20 % are random positions.  Everything is made on the
GPU; one add per query.

Reported: add per query (host time; nothing waits), the lookup stages on the device (events inside loftr_model_lookup: lookup with the
clearing of the table, keep + scans, write), the estimator (device events around ops.estimate_absolute_poses), solve in total (wall,
with its one readback), and on the same data the wall time of the host routine (loftr_model_lookup_host, one core; the first
--host-queries queries, 0 = all) and of the Python oracle (tests/_model_lookup_oracle.py: what callers write today; the first
--oracle-queries queries), each compared equal to the kernels' result inside the tool."""
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

from loftr_amd import LocalizationModel, QueryLocalizer, ops        # noqa: E402

DEV = "cuda:0"
HW, CELL = (480.0, 640.0), 2.0
GH, GW = 240, 320
KP_PER_IMAGE, WINDOW, STRIDE = 2300, 3000, 600
FIELDS = ("pts3d", "kpts", "q_ids", "match", "point", "conf", "match_reason")


def make_model(n_images, g):
    P = STRIDE * n_images + WINDOW
    xyz = torch.rand(P, 3, device=DEV, generator=g) * torch.tensor([8.0, 6.0, 4.0], device=DEV) + torch.tensor([-4.0, -3.0, 4.0], device=DEV)
    kp, pt = [], []
    for i in range(n_images):
        cells = torch.sort(torch.randperm(GH * GW, device=DEV, generator=g)[:KP_PER_IMAGE]).values
        frac = 0.05 + 0.9 * torch.rand(KP_PER_IMAGE, 2, device=DEV, generator=g)
        kp.append((torch.stack([cells % GW, cells // GW], 1) + frac) * CELL)
        p = i * STRIDE + torch.randperm(WINDOW, device=DEV, generator=g)[:KP_PER_IMAGE]
        pt.append(torch.where(torch.rand(KP_PER_IMAGE, device=DEV, generator=g) < 0.3, torch.full_like(p, -1), p))
    off = torch.arange(n_images + 1, device=DEV, dtype=torch.int64) * KP_PER_IMAGE
    return LocalizationModel(off, torch.cat(kp).float(), torch.cat(pt).to(torch.int32), xyz, HW, CELL)


def make_queries(model, n_queries, n_rows, matches, g):
    """-> (K_query [Q,3,3], chunks: one (query_ids, db_ids, data) per query)."""
    Kq = torch.tensor([[520.0, 0, 320], [0, 520, 240], [0, 0, 1]], device=DEV).repeat(n_queries, 1, 1)
    chunks = []
    for q in range(n_queries):
        t = (torch.rand(3, device=DEV, generator=g) - 0.5) * torch.tensor([1.0, 0.5, 0.5], device=DEV)
        first = (q * 7) % max(1, model.n_images - n_rows + 1)
        dbs = list(range(first, first + n_rows))
        kd, kq, conf, bids = [], [], [], []
        for r, d in enumerate(dbs):
            m = int(matches * (0.5 + torch.rand(1, device=DEV, generator=g).item()))
            k = d * KP_PER_IMAGE + torch.randint(0, KP_PER_IMAGE, (m,), device=DEV, generator=g)
            hit = torch.rand(m, device=DEV, generator=g) < 0.8
            cell_pos = torch.floor(model.keypoints[k] / CELL) * CELL + CELL * torch.rand(m, 2, device=DEV, generator=g) * 0.999
            rand_pos = torch.rand(m, 2, device=DEV, generator=g) * torch.tensor([HW[1], HW[0]], device=DEV)
            kd.append(torch.where(hit[:, None], cell_pos, rand_pos))
            X = model.xyz[model.kp_point[k].clamp(min=0).long()] + t
            proj = X[:, :2] / X[:, 2:] * 520.0 + torch.tensor([320.0, 240.0], device=DEV) + 0.5 * torch.randn(m, 2, device=DEV, generator=g)
            out = torch.rand(m, device=DEV, generator=g) < 0.15
            kq.append(torch.where(out[:, None], proj + 40.0 * torch.randn(m, 2, device=DEV, generator=g), proj))
            conf.append(0.2 + 0.8 * torch.rand(m, device=DEV, generator=g))
            bids.append(torch.full((m,), r, dtype=torch.long, device=DEV))
        chunks.append(([q] * n_rows, dbs, {"mkpts0_f": torch.cat(kq), "mkpts1_f": torch.cat(kd), "mconf": torch.cat(conf), "m_bids": torch.cat(bids)}))
    return Kq, chunks


def fill(model, n_queries, chunks):
    loc = QueryLocalizer(model, n_queries)
    host = []
    for q_ids, d_ids, data in chunks:
        t = time.perf_counter()
        loc.add(q_ids, d_ids, data, db_side=1)
        host.append(time.perf_counter() - t)
    return loc, 1e3 * np.array(host)


def prefix_arrays(chunks, n):
    """The first n queries as the numpy arrays of ops.model_lookup_host."""
    sub = chunks[:n]
    cat = lambda k: torch.cat([c[2][k] for c in sub]).cpu().numpy()
    rows = np.concatenate([c[2]["m_bids"].cpu().numpy() + i * len(c[0]) for i, c in enumerate(sub)]).astype(np.int32)
    return dict(kpts_db=cat("mkpts1_f"), kpts_q=cat("mkpts0_f"), conf=cat("mconf"), rows=rows, mask=None,
                row_db=np.concatenate([c[1] for c in sub]).astype(np.int32), row_query=np.concatenate([c[0] for c in sub]).astype(np.int32), Q=n)


def same_prefix(res, want, n_matches):
    """want: trimmed arrays of the first queries; res: the QueryPoses of all of them."""
    C = len(want["match"])
    ok = all(np.array_equal(getattr(res, k)[:C].cpu().numpy(), want[k]) for k in FIELDS[:-1])
    return bool(ok and np.array_equal(res.match_reason[:n_matches].cpu().numpy(), want["match_reason"])
                and np.array_equal(res.q_offsets[:len(want["q_offsets"])].cpu().numpy(), want["q_offsets"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=20)
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--images", type=int, default=800)
    ap.add_argument("--host-queries", type=int, default=0, help="queries given to the host routine (0: all)")
    ap.add_argument("--oracle-queries", type=int, default=10, help="queries given to the Python oracle (0: all)")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(0)
    model = make_model(args.images, g)
    Kq, chunks = make_queries(model, args.queries, args.rows, args.matches, g)
    M = sum(c[2]["mconf"].numel() for c in chunks)
    out = {"workload": "model_lookup_aachen_shape", "queries": args.queries, "rows_per_query": args.rows, "images": args.images,
           "keypoints": model.n_keypoints, "points": model.n_points, "matches": M, "extent_hw": list(HW), "cell_px": CELL}

    # warm-up (kernel load) on a few queries, then the timed pass
    fill(model, args.queries, chunks[:4])[0].solve(Kq)
    loc, add_ms = fill(model, args.queries, chunks)
    out["add_host_ms_per_query"] = {"median": round(float(np.median(add_ms)), 4), "max": round(float(add_ms.max()), 4)}
    stages = []
    torch.cuda.synchronize()
    t = time.perf_counter()
    corr, stats = loc.correspondences(timings=stages)
    torch.cuda.synchronize()
    out["lookup_wall_ms_timed"] = round(1e3 * (time.perf_counter() - t), 3)
    out["lookup_stage_ms"] = {k: round(v, 4) for k, v in stages}
    out["lookup_gpu_ms"] = round(sum(v for _, v in stages), 4)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ops.estimate_absolute_poses(corr["pts3d"], corr["kpts"], corr["q_ids"], Kq, 3.0, 0.999, 0)
    e1.record()
    torch.cuda.synchronize()
    out["pose_gpu_ms"] = round(e0.elapsed_time(e1), 3)
    t = time.perf_counter()
    res = loc.solve(Kq, thresh_px=3.0, conf=0.999, seed=0)
    torch.cuda.synchronize()
    out["solve_wall_ms"] = round(1e3 * (time.perf_counter() - t), 3)
    out["stats"] = res.stats
    out["localized"] = int((res.n_inliers >= 3).sum())
    out["median_inliers"] = float(res.n_inliers.float().median())

    # the host routine on the same data (what defines the result)
    np_ = lambda x: x.cpu().numpy()
    mo = (np_(model.kp_offsets), np_(model.kp_cell), np_(model.kp_point), np_(model.xyz), model.gh, model.gw, model.inv)
    trim = lambda o: {k: (o[k][:int(o["counts"][0])] if k not in ("match_reason", "q_offsets") else o[k]) for k in FIELDS + ("q_offsets",)}
    n_host = args.queries if args.host_queries <= 0 else min(args.queries, args.host_queries)
    a = prefix_arrays(chunks, n_host)
    t = time.perf_counter()
    want = ops.model_lookup_host(*mo, a["kpts_db"], a["kpts_q"], a["conf"], a["rows"], None, a["row_db"], a["row_query"], n_host)
    out["host_routine_ms"] = round(1e3 * (time.perf_counter() - t), 3)
    out["host_routine_queries"], out["host_routine_matches"] = n_host, len(a["conf"])
    out["identical_to_host"] = same_prefix(res, trim(want), len(a["conf"]))
    assert out["identical_to_host"], "the kernels and the host routine disagree"

    # what callers write today: Python on the host (the tests' oracle)
    import _model_lookup_oracle as O
    n_or = args.queries if args.oracle_queries <= 0 else min(args.queries, args.oracle_queries)
    a = prefix_arrays(chunks, n_or)
    md = dict(kp_offsets=mo[0], keypoints=np_(model.keypoints), kp_point=mo[2], xyz=mo[3], image_hw=HW, cell_px=CELL)
    t = time.perf_counter()
    ref = O.lookup(md, a)
    out["python_oracle_ms"] = round(1e3 * (time.perf_counter() - t), 1)
    out["python_oracle_queries"], out["python_oracle_matches"] = n_or, len(a["conf"])
    out["identical_to_oracle"] = ref["status"] == 0 and same_prefix(res, ref, len(a["conf"]))
    assert out["identical_to_oracle"], "the kernels and the oracle disagree"
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
