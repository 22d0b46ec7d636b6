#!/usr/bin/env python
"""Bundle adjustment (loftr_amd/bundle.py, csrc/bundle_gpu.hip) on a MegaDepth-1500-shaped load.  One JSON line.

    python tools/micro/bundle_bench.py [--rows 1500] [--matches 1000] [--max-iters 30] [--pcg-iters 30] [--huber 0] [--refine-focal] [--camera-groups G[,G...]] [--radial] [--prior] [--no-host] [--out FILE]

Load: the track lengths of tools/micro/atlas_bench.py's synthetic atlas (1500 rows over 806 images), observations as in
tools/micro/triangulation_bench.py without outliers (one exact camera per image, one 3D point per track, every observation in a random
image, projected, 0.5 px of noise).  The start: every pose but those of images 0 and 1 (fixed) rotated by 1 degree about a random axis
and its centre moved by N(0, 0.05) per axis, every point moved by N(0, 0.05).

Reported: per kernel class the median device time over all launches of the class (those that returned at once on a stop flag
included), the total and the launches issued (events around every launch inside loftr_bundle_adjust, one call after a warm-up); a lower
bound of the launches that returned at once (from the counts: trials and conjugate-gradient iterations not run); the wall time of bundle_adjust with its one readback (median of 3 calls without events); trials,
accepted trials and conjugate-gradient iterations; the host routine (loftr_bundle_adjust_host, one core) on the same input; and the
assertion that every run's output tensors and counts equal the host routine's.  With --refine-focal the focal of every
free camera starts 4-10 % off and the line holds two such legs on that load: "fixed_intrinsics" (the 6-wide kernels) and "refine_focal"
(the 7-wide kernels, refine_focal=True), with the largest relative focal error before and after.  With --camera-groups 1,8,806 (DESIGN
§18.2) the line holds that per-image leg as the reference point ("per_image") and one leg per G ("groups_G"): image i is of camera
i mod G, every camera's focal -- the fixed-pose images' too -- starts off by one factor of 4-10 %, and the call is
refine_focal=True, camera_ids=ids; per leg the trials, conjugate-gradient iterations, rms before and after, the largest focal error
over all images and the wall time.  With --camera-groups 1,8,806 --radial the load of every G is observed through one
radial coefficient per camera, k drawn from U(-0.08, 0.08), and the line holds per G the shared-focal call of §18.2 on that load as the
reference point ("groups_G_shared": today's best pinhole model; its equality with the host routine is §18.2's, not repeated here) and
the radial call ("groups_G_radial": refine_focal=True, refine_radial=True, camera_ids=ids, start k = 0), with the largest focal and
radial error over all images next to the figures above.  With --prior the line holds three legs on the default load, run in alternation
--rounds times (no_prior, prior_masked, prior, no_prior, ...) after one warm-up of each: "no_prior" (the default call: images 0 and 1
fixed), "prior_masked" (the kernels with priors and an all-zero prior_mask: the same result as no_prior, asserted), "prior" (no camera
fixed, position_prior = the true centres + N(0, 0.05) per axis at prior_sigma = 0.05); per leg every wall time with its median and
spread, the trials, accepted trials and conjugate-gradient iterations, the class times of one call with events, and for "prior" the
rms distance of the centres from their priors before and after."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from loftr_amd import BundleResult, KeypointAtlas, bundle_adjust         # noqa: E402
from tools.micro.atlas_bench import DEV, HW, make_chunks                 # noqa: E402
from tools.micro.triangulation_bench import rotations                    # noqa: E402


def make_load(track_len, n_images, seed=0, radial=None):
    """-> (offsets, obs_image, obs_xy, obs_mask, xyz start, K, T start, fixed) on the device.  radial: None, or [n_images] coefficients
    k of the lens the observations are made through, x_d = x (1 + k r^2) on normalised coordinates."""
    rng = np.random.default_rng(seed)
    R = rotations(rng, n_images, 20.0)
    c = rng.uniform([-2, -1, -0.5], [2, 1, 0.5], (n_images, 3))
    K = np.tile(np.eye(3), (n_images, 1, 1))
    K[:, 0, 0] = K[:, 1, 1] = rng.uniform(450, 650, n_images)
    K[:, 0, 2], K[:, 1, 2] = 320.0, 240.0
    T = np.tile(np.eye(4), (n_images, 1, 1))
    T[:, :3, :3] = R
    T[:, :3, 3] = -(R @ c[:, :, None])[:, :, 0]
    axis_turn = rotations_fixed(rng, n_images, 1.0) @ R
    c0 = c + 0.05 * rng.standard_normal((n_images, 3))
    T0 = T.copy()
    T0[2:, :3, :3] = axis_turn[2:]
    T0[2:, :3, 3] = -(axis_turn[2:] @ c0[2:, :, None])[:, :, 0]
    K, T, T0 = (torch.from_numpy(a).to(DEV) for a in (K, T, T0))
    g = torch.Generator(device=DEV).manual_seed(seed)
    lens = track_len.to(DEV, torch.int64)
    n_tracks = lens.numel()
    offsets = torch.zeros(n_tracks + 1, dtype=torch.int64, device=DEV)
    offsets[1:] = torch.cumsum(lens, 0)
    N = int(offsets[-1])
    track = torch.repeat_interleave(torch.arange(n_tracks, device=DEV), lens)
    lo, hi = torch.tensor([-2, -1.5, 3.0], device=DEV, dtype=torch.float64), torch.tensor([2, 1.5, 8.0], device=DEV, dtype=torch.float64)
    X = lo + (hi - lo) * torch.rand(n_tracks, 3, device=DEV, dtype=torch.float64, generator=g)
    image = torch.randint(0, n_images, (N,), device=DEV, generator=g)
    Y = torch.einsum("nij,nj->ni", T[image, :3, :3], X[track]) + T[image, :3, 3]
    if radial is not None:                                              # the lens acts on the normalised point; its depth stays
        x = Y[:, :2] / Y[:, 2:]
        Y = torch.cat([x * (1 + radial.to(DEV)[image][:, None] * (x * x).sum(1, keepdim=True)), torch.ones_like(Y[:, 2:])], 1)
    p = torch.einsum("nij,nj->ni", K[image], Y)
    xy = p[:, :2] / p[:, 2:] + 0.5 * torch.randn(N, 2, device=DEV, dtype=torch.float64, generator=g)
    xyz = (X + 0.05 * torch.randn(n_tracks, 3, device=DEV, dtype=torch.float64, generator=g)).to(torch.float32)
    fixed = torch.zeros(n_images, dtype=torch.bool, device=DEV)
    fixed[:2] = True
    return offsets, image.to(torch.int32), xy.to(torch.float32), torch.ones(N, dtype=torch.bool, device=DEV), xyz, K, T0, fixed


def rotations_fixed(rng, n, deg):
    """Rotations by exactly `deg` degrees about random axes."""
    axis = rng.standard_normal((n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    A = np.zeros((n, 3, 3))
    A[:, 0, 1], A[:, 0, 2], A[:, 1, 0], A[:, 1, 2], A[:, 2, 0], A[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * A + (1 - np.cos(t)) * (A @ A)


def same(a, b):
    eq = lambda x, y: torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0))
    return a.FIELDS == b.FIELDS and all(eq(getattr(a, k).cpu().double(), getattr(b, k).cpu().double()) for k in a.FIELDS) and a.stats == b.stats


def detune(K, fixed, seed=5):
    """K with fx, skew and fy of every camera that is not fixed multiplied by 1 +- U(0.04, 0.10)."""
    rng = np.random.default_rng(seed)
    n = K.shape[0]
    fac = torch.from_numpy(1 + rng.choice([-1, 1], n) * rng.uniform(0.04, 0.10, n)).to(K.device)
    fac = torch.where(fixed, torch.ones_like(fac), fac)
    K = K.clone()
    K[:, 0, 0], K[:, 0, 1], K[:, 1, 1] = K[:, 0, 0] * fac, K[:, 0, 1] * fac, K[:, 1, 1] * fac
    return K


def detune_groups(K, ids, seed=5):
    """K with fx, skew and fy of every image multiplied by the factor 1 +- U(0.04, 0.10) of its camera ids[i]."""
    rng = np.random.default_rng(seed)
    G = int(ids.max()) + 1
    fac = torch.from_numpy(1 + rng.choice([-1, 1], G) * rng.uniform(0.04, 0.10, G)).to(K.device)[ids]
    K = K.clone()
    K[:, 0, 0], K[:, 0, 1], K[:, 1, 1] = K[:, 0, 0] * fac, K[:, 0, 1] * fac, K[:, 1, 1] * fac
    return K


def leg(inputs, fixed, kw, n_tracks, args, host=True):
    """One timed leg: a warm-up, 3 timed calls, one call with events, the host routine and the equality assertion (host=False: neither)
    -> dict."""
    out = {}
    run = lambda timings=None: bundle_adjust(*inputs, fixed=fixed, timings=timings, **kw)
    results = [run()]                                                   # warm-up (kernel load)
    wall = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        results.append(run())
        wall.append(1e3 * (time.perf_counter() - t))
    timings = {}
    results.append(run(timings))
    res = results[-1]
    out["wall_ms"] = round(float(np.median(wall)), 3)
    out["class_median_ms"] = {k: round(v[0], 4) for k, v in timings.items()}
    out["class_total_ms"] = {k: round(v[1], 3) for k, v in timings.items()}
    out["class_launches"] = {k: v[2] for k, v in timings.items()}
    issued = sum(v[2] for v in timings.values())
    levels_t = 1 if n_tracks <= 4096 else 2
    per_pcg, per_trial = 6, 3 + 2 + 1 + 2 + 2 * levels_t + 1                # the launches of one iteration / of a trial without them
    if "camera_ids" in kw:                                              # §18.2: the group kernels, and a dot product is two sums
        per_pcg, per_trial = 9, 4 + 3 + 2 + 2 + 2 * levels_t + 1
    skipped = (args.max_iters - res.n_iters) * (per_trial + per_pcg * args.pcg_iters) + per_pcg * (res.n_iters * args.pcg_iters - res.n_pcg)
    out["launches_issued"], out["launches_skipped_at_least"] = issued, int(skipped)
    if "position_prior" in kw:                                          # §18.3: an evaluation has three more launches per level of the cameras' sum
        del out["launches_skipped_at_least"]
    out["stats"] = res.stats
    if host and not args.no_host:
        t = time.perf_counter()
        host_kw = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        host = bundle_adjust(*[x.cpu() for x in inputs], fixed=fixed.cpu(), **host_kw)
        out["host_routine_ms"] = round(1e3 * (time.perf_counter() - t), 1)
        out["identical_to_host"] = bool(all(same(r, host) for r in results))
        assert out["identical_to_host"], "a GPU run differs from the host routine"
    print(f"[bundle_bench] leg {sorted(k for k in kw if k not in ('huber_px', 'max_iters', 'pcg_iters'))}: {res.n_iters} trials, {res.n_pcg} pcg, "
          f"wall {out['wall_ms']} ms, host {out.get('host_routine_ms')} ms", file=sys.stderr, flush=True)     # (the host routine takes minutes)
    return out, res


def true_centres(n_images, seed=0):
    """The camera centres make_load(.., seed) draws before it perturbs them."""
    rng = np.random.default_rng(seed)
    rotations(rng, n_images, 20.0)
    return rng.uniform([-2, -1, -0.5], [2, 1, 0.5], (n_images, 3))


def prior_legs(inputs, fixed, kw, n_images, args):
    """--prior: the three legs in alternation -> dict of legs."""
    sigma = 0.05
    g = torch.from_numpy(true_centres(n_images) + sigma * np.random.default_rng(7).standard_normal((n_images, 3))).to(DEV)
    none = torch.zeros_like(fixed)
    legs = {"no_prior": dict(fixed=fixed, **kw),
            "prior_masked": dict(fixed=fixed, position_prior=g, prior_sigma=sigma, prior_mask=none, **kw),
            "prior": dict(fixed=none, position_prior=g, prior_sigma=sigma, **kw)}
    res, wall = {}, {k: [] for k in legs}
    for k, a in legs.items():
        res[k] = bundle_adjust(*inputs, **a)                             # warm-up (kernel load)
    for _ in range(args.rounds):
        for k, a in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = bundle_adjust(*inputs, **a)
            wall[k].append(round(1e3 * (time.perf_counter() - t), 3))
            assert same_fields(r, res[k]), f"{k}: two runs differ"
    plain, masked = res["no_prior"], res["prior_masked"]
    assert all(torch.equal(torch.nan_to_num(getattr(plain, f).double()), torch.nan_to_num(getattr(masked, f).double())) for f in plain.FIELDS) and \
        all(masked.stats[f] == v for f, v in plain.stats.items()), "an all-zero prior_mask differs from the call without priors"
    out = {}
    for k, a in legs.items():
        timings = {}
        bundle_adjust(*inputs, timings=timings, **a)
        st = res[k].stats
        out[k] = {"wall_ms": wall[k], "wall_median_ms": round(float(np.median(wall[k])), 3), "wall_min_ms": min(wall[k]), "wall_max_ms": max(wall[k]),
                  "n_iters": st["n_iters"], "n_accepted": st["n_accepted"], "n_pcg": st["n_pcg"], "status": st["status"],
                  "rms_px_before": st["rms_px_before"], "rms_px_after": st["rms_px_after"],
                  "class_total_ms": {c: round(v[1], 3) for c, v in timings.items()}, "class_launches": {c: v[2] for c, v in timings.items()}}
        if "prior_rms_after" in st:
            out[k].update(n_prior_cameras=st["n_prior_cameras"], prior_rms_before=st["prior_rms_before"], prior_rms_after=st["prior_rms_after"])
    out["prior_masked"]["identical_to_no_prior"] = True
    return out


def same_fields(a, b):
    return a.FIELDS == b.FIELDS and all(torch.equal(torch.nan_to_num(getattr(a, k).double()), torch.nan_to_num(getattr(b, k).double())) for k in a.FIELDS) \
        and a.stats == b.stats


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--max-iters", type=int, default=30)
    ap.add_argument("--pcg-iters", type=int, default=30)
    ap.add_argument("--huber", type=float, default=0.0)
    ap.add_argument("--refine-focal", action="store_true",
                    help="the focal of every free camera off by 4-10 %%: a fixed-intrinsics leg and a refine_focal=True leg on that load")
    ap.add_argument("--camera-groups", default=None,
                    help="comma-separated group counts G (image i is of camera i mod G): a per-image refine_focal leg and one shared leg per G")
    ap.add_argument("--radial", action="store_true",
                    help="(with --camera-groups; DESIGN §18.4) one radial coefficient per camera: a shared-focal leg and a radial leg per G")
    ap.add_argument("--prior", action="store_true", help="position priors (DESIGN §18.3): the no_prior, prior_masked and prior legs in alternation")
    ap.add_argument("--rounds", type=int, default=5, help="(--prior) timed calls per leg")
    ap.add_argument("--no-host", action="store_true", help="skip the host routine (and the equality assertion)")
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
    *inputs, fixed = make_load(lens, n_images)
    kw = dict(huber_px=args.huber, max_iters=args.max_iters, pcg_iters=args.pcg_iters)
    out = {"workload": "bundle_megadepth1500_shape", "images": n_images, "tracks": int(lens.numel()), "observations": int(inputs[0][-1]),
           "fixed_cameras": 2, **kw}
    if args.prior:
        out["workload"] += "_position_priors"
        out.update(prior_legs(inputs, fixed, kw, n_images, args))
    elif args.camera_groups and args.radial:
        out["workload"] += "_camera_groups_radial"
        for G in (int(g) for g in args.camera_groups.split(",")):
            ids = torch.arange(n_images, device=DEV) % G
            k_true = torch.from_numpy(np.random.default_rng(9).uniform(-0.08, 0.08, G)).to(DEV)[ids]
            *inputs, fixed = make_load(lens, n_images, radial=k_true)
            K_true = inputs[5]
            err = lambda K: float((K[:, 0, 0] / K_true[:, 0, 0] - 1).abs().max())
            inputs[5] = detune_groups(K_true, ids)
            d, res = leg(inputs, fixed, dict(kw, refine_focal=True, camera_ids=ids), lens.numel(), args, host=False)
            out[f"groups_{G}_shared"] = dict(d, focal_error_before=round(err(inputs[5]), 5), focal_error_after=round(err(res.K), 5))
            d, res = leg(inputs, fixed, dict(kw, refine_focal=True, refine_radial=True, camera_ids=ids), lens.numel(), args)
            out[f"groups_{G}_radial"] = dict(d, focal_error_before=round(err(inputs[5]), 5), focal_error_after=round(err(res.K), 5),
                                             radial_error_before=round(float(k_true.abs().max()), 5),
                                             radial_error_after=round(float((res.radial - k_true).abs().max()), 5))
    elif args.camera_groups:
        K_true = inputs[5]
        err = lambda K: float((K[:, 0, 0] / K_true[:, 0, 0] - 1).abs().max())
        brief = lambda d, res, K0: dict(d, focal_error_before=round(err(K0), 5), focal_error_after=round(err(res.K), 5))
        out["workload"] += "_camera_groups"
        inputs[5] = detune(K_true, fixed)
        out["per_image"] = brief(*leg(inputs, fixed, dict(kw, refine_focal=True), lens.numel(), args), inputs[5])
        for G in (int(g) for g in args.camera_groups.split(",")):
            ids = torch.arange(n_images, device=DEV) % G
            inputs[5] = detune_groups(K_true, ids)
            out[f"groups_{G}"] = brief(*leg(inputs, fixed, dict(kw, refine_focal=True, camera_ids=ids), lens.numel(), args), inputs[5])
    elif not args.refine_focal:
        out.update(leg(inputs, fixed, kw, lens.numel(), args)[0])
    else:
        K_true = inputs[5]
        inputs[5] = detune(K_true, fixed)
        err = lambda K: float(((K[:, 0, 0] / K_true[:, 0, 0] - 1).abs()[~fixed]).max())
        out["workload"] += "_focal_off_4_to_10_percent"
        out["focal_error_before"] = round(err(inputs[5]), 5)
        out["fixed_intrinsics"], _ = leg(inputs, fixed, kw, lens.numel(), args)
        out["refine_focal"], res = leg(inputs, fixed, dict(kw, refine_focal=True), lens.numel(), args)
        out["focal_error_after"] = round(err(res.K), 5)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
