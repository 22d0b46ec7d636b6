#!/usr/bin/env python
"""The correspondence table of the unposed images (loftr_amd/registration.py, csrc/register_gpu.hip) on a
MegaDepth-1500-shaped load.  One JSON line.

    python tools/micro/registration_bench.py [--images 806] [--keypoints 2000] [--posed 0.5] [--min-corr 15] [--out FILE]

Load: --images exact cameras (f in [450, 650], rotations up to 20 degrees), about --keypoints observations per image in tracks of 2-12
observations (lengths weighted towards 2, as the atlas's tracks are), one 3D point per track, every observation in a random image,
projected, 0.5 px of noise; a --posed share of the images has a pose; a track has a point (status ok) when at least two of its
observations lie in posed images.  Everything is made on the GPU.

Reported: the four kernels (device events inside loftr_register_corr, median of 5 calls after a warm-up), the readback of the 8 counts
(wall), the one P3P call over all candidates (device events around ops.estimate_absolute_poses), register_images in total (wall); next to
it the same table built from existing torch ops (repeat_interleave, boolean masks, bincount, nonzero, a stable sort; device events, and
wall with its hidden host synchronisations), compared equal to the kernels' table inside the tool; and the host routine on one core."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from loftr_amd import ops, register_images                           # noqa: E402

DEV = "cuda:0"


def make_load(n, per_image, posed_share, g):
    N_target = n * per_image
    lens = 2 + torch.floor(-torch.log(torch.rand(N_target // 2, device=DEV, generator=g)) * 1.2).clamp(max=10).long()
    lens = lens[torch.cumsum(lens, 0) <= N_target]
    T, N = lens.numel(), int(lens.sum())
    offsets = torch.zeros(T + 1, dtype=torch.int64, device=DEV)
    offsets[1:] = torch.cumsum(lens, 0)
    track = torch.repeat_interleave(torch.arange(T, device=DEV), lens)
    image = torch.randint(0, n, (N,), device=DEV, generator=g)
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
    Tcw = torch.eye(4, device=DEV, dtype=torch.float64).repeat(n, 1, 1)
    Tcw[:, :3, :3], Tcw[:, :3, 3] = R, -(R @ centre[:, :, None])[:, :, 0]
    X = torch.rand(T, 3, device=DEV, generator=g, dtype=torch.float64) * torch.tensor([4.0, 3.0, 5.0], device=DEV) + torch.tensor([-2.0, -1.5, 3.0], device=DEV)
    Y = (R[image] @ X[track][:, :, None])[:, :, 0] + Tcw[image, :3, 3]
    uv = torch.stack([K[image, 0, 0] * Y[:, 0] / Y[:, 2] + 320.0, K[image, 1, 1] * Y[:, 1] / Y[:, 2] + 240.0], 1)
    xy = (uv + 0.5 * torch.randn(N, 2, device=DEV, generator=g, dtype=torch.float64)).float()
    posed = torch.rand(n, device=DEV, generator=g) < posed_share
    seen = torch.bincount(track[posed[image]], minlength=T)
    status = torch.where(seen >= 2, 0, 1).to(torch.uint8)
    xyz = torch.where((status == 0)[:, None], X.float(), torch.full((T, 3), float("nan"), device=DEV))
    return dict(offsets=offsets, obs_image=image.to(torch.int32), obs_xy=xy, xyz=xyz, status=status, K=K, T=Tcw, posed=posed)


def groups(image, n):
    im = image.to(torch.int64)
    cam_obs = torch.sort(im, stable=True).indices.to(torch.int32)
    cam_offsets = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    cam_offsets[1:] = torch.cumsum(torch.bincount(im, minlength=n), 0)
    return cam_offsets, cam_obs


def torch_table(L, min_corr):
    """The same table from existing torch ops -> (corr_xyz, corr_xy, corr_bid, corr_obs, cand_image, cand_offsets)."""
    n, T = L["posed"].numel(), L["status"].numel()
    image = L["obs_image"].to(torch.int64)
    track = torch.repeat_interleave(torch.arange(T, device=DEV), L["offsets"][1:] - L["offsets"][:-1])
    corr = ~L["posed"][image] & (L["status"][track] == 0) & torch.isfinite(L["xyz"][track]).all(1) & torch.isfinite(L["obs_xy"]).all(1)
    n_corr = torch.bincount(image[corr], minlength=n)
    cand = ~L["posed"] & (n_corr >= min_corr)
    rank = torch.cumsum(cand, 0) - 1
    obs = torch.nonzero(corr & cand[image]).reshape(-1)               # (a host synchronisation inside)
    obs = obs[torch.sort(image[obs], stable=True).indices]
    cand_image = torch.nonzero(cand).reshape(-1)                       # (and another)
    cand_offsets = torch.zeros(cand_image.numel() + 1, dtype=torch.int64, device=DEV)
    cand_offsets[1:] = torch.cumsum(n_corr[cand_image], 0)
    return L["xyz"][track[obs]], L["obs_xy"][obs], rank[image[obs]], obs.to(torch.int32), cand_image.to(torch.int32), cand_offsets


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=806)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--posed", type=float, default=0.5)
    ap.add_argument("--min-corr", type=int, default=15)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(0)
    L = make_load(args.images, args.keypoints, args.posed, g)
    n = args.images
    cam_offsets, cam_obs = groups(L["obs_image"], n)
    a = (L["offsets"], L["obs_image"], L["obs_xy"], L["xyz"], L["status"], L["posed"].to(torch.uint8), cam_offsets, cam_obs)
    out = {"workload": "registration_megadepth1500_shape", "images": n, "tracks": L["status"].numel(), "observations": L["obs_image"].numel(),
           "posed_images": int(L["posed"].sum()), "points": int((L["status"] == 0).sum()), "min_corr": args.min_corr}
    ops.register_corr(*a, args.min_corr)                              # warm-up (kernel load)
    runs = []
    for _ in range(5):
        stages = []
        res = ops.register_corr(*a, args.min_corr, timings=stages)
        runs.append([v for _, v in stages])
    med = np.median(np.array(runs), 0)
    out["kernel_ms"] = {k: round(float(v), 4) for k, v in zip(ops.REGISTER_STAGES, med)}
    out["kernels_total_ms"] = round(float(med.sum()), 4)
    torch.cuda.synchronize()
    t = time.perf_counter()
    counts = res["counts"].cpu().tolist()
    out["readback_wall_ms"] = round(1e3 * (time.perf_counter() - t), 4)
    C, P = counts[0], counts[1]
    out["counts"] = counts
    Kc = L["K"].float()[res["cand_image"][:P].long()].contiguous()
    ops.estimate_absolute_poses(res["corr_xyz"][:C], res["corr_xy"][:C], res["corr_bid"][:C], Kc, 4.0, 0.999, 0)
    p3p = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.estimate_absolute_poses(res["corr_xyz"][:C], res["corr_xy"][:C], res["corr_bid"][:C], Kc, 4.0, 0.999, 0)
        e1.record()
        torch.cuda.synchronize()
        p3p.append(e0.elapsed_time(e1))
    out["p3p_gpu_ms"] = round(float(np.median(p3p)), 3)
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        reg = register_images(L["offsets"], L["obs_image"], L["obs_xy"], L["xyz"], L["status"], L["K"], L["T"], L["posed"], min_corr=args.min_corr,
                              min_inliers=args.min_corr)
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t))
    out["register_images_wall_ms"] = round(float(np.median(walls)), 3)
    out["registered"] = int(reg.registered.sum())

    # the same table from existing torch ops
    torch_table(L, args.min_corr)
    ev, wall = [], []
    for _ in range(5):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        tab = torch_table(L, args.min_corr)
        e1.record()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t))
        ev.append(e0.elapsed_time(e1))
    out["torch_composition_gpu_ms"] = round(float(np.median(ev)), 4)
    out["torch_composition_wall_ms"] = round(float(np.median(wall)), 4)
    names = ("corr_xyz", "corr_xy", "corr_bid", "corr_obs")
    same = all(torch.equal(torch.nan_to_num(res[k][:C]), torch.nan_to_num(v)) for k, v in zip(names, tab[:4]))
    out["identical_to_torch_composition"] = bool(same and torch.equal(res["cand_image"][:P], tab[4]) and torch.equal(res["cand_offsets"][:P + 1], tab[5]))
    assert out["identical_to_torch_composition"], "the kernels and the torch composition disagree"

    host = [x.cpu().numpy() for x in a]
    t = time.perf_counter()
    want = ops.register_corr_host(*host, args.min_corr)
    out["host_routine_ms"] = round(1e3 * (time.perf_counter() - t), 3)
    out["identical_to_host"] = all(np.array_equal(res[k].cpu().numpy(), want[k], equal_nan=k in ("corr_xyz", "corr_xy")) for k in want)
    assert out["identical_to_host"], "the kernels and the host routine disagree"
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
