#!/usr/bin/env python
"""What track splitting (loftr_amd/splitting.py) is worth on noisy synthetic pair lists, on the CPU (the host routines).

    python tools/split_accuracy.py [--points 1500] [--out FILE]

Loads (tests/_split_cases.noisy_scene): cameras on a 6-unit baseline, f = 500, 640 x 480 images, `--points` points, every pair of images
a row (or the rows (i, i+1 .. i+3)) that observes 70 % of the co-visible points with independent Gaussian noise on both sides, 2 px
cells, mutual best per row: the atlas's own rules 1-4, then SfmResult.split.  Per load: the share of the keypoints that lie in
consistent tracks before and after, the tracks of length >= 3 before and after, the rounds used, n_open, and the share of the tracks
after the split whose keypoints all belong to one physical point (a keypoint belongs to the point whose projection is nearest).
Then SfmResult.reconstruct on the test scene of tests/test_split.py with and without split=True: images posed, points, rms, and the
rotation and centre errors of evaluation.trajectory_errors."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _split_cases as SC                                              # noqa: E402
import _triangulation_cases as TC                                      # noqa: E402
from loftr_amd import evaluation                                       # noqa: E402

LOADS = (dict(n_cams=8, noise_px=0.5), dict(n_cams=12, noise_px=0.5), dict(n_cams=12, noise_px=1.0), dict(n_cams=20, noise_px=0.5),
         dict(n_cams=20, noise_px=0.5, window=3))


def owner(sfm, scene):
    """The physical point of every keypoint: the one whose projection into the keypoint's image is nearest."""
    image = sfm.keypoint_image().numpy()
    xy = sfm.keypoints.numpy().astype(np.float64)
    out = np.zeros(len(image), np.int64)
    for i in range(scene["n"]):
        px = np.stack([TC.project(scene["K"][i], scene["T"][i], x) for x in scene["X"]])
        ks = np.flatnonzero(image == i)
        for s in range(0, len(ks), 512):
            k = ks[s:s + 512]
            out[k] = np.argmin(((xy[k, None, :] - px[None, :, :]) ** 2).sum(-1), 1)
    return out


def figures(n_points, **load):
    scene = SC.noisy_scene(seed=11, n_points=n_points, **load)
    t = time.perf_counter()
    sfm = SC.run_atlas("cpu", seed=11, n_points=n_points, **load)
    atlas_s = time.perf_counter() - t
    t = time.perf_counter()
    sfm2, done = sfm.split()
    split_s = time.perf_counter() - t
    K = sfm.track_id.numel()
    ok = sfm.track_ok[sfm.track_id.clamp(min=0).long()] & (sfm.track_id >= 0)
    own = owner(sfm, scene)
    tid = sfm2.track_id.numpy()
    first = {}
    pure = np.ones(sfm2.track_len.numel(), bool)
    for k in np.flatnonzero(tid >= 0):
        pure[tid[k]] &= first.setdefault(tid[k], own[k]) == own[k]
    bad = ~sfm.track_ok
    return dict(load=load, rows=len(scene["rows"]), keypoints=K, kept_matches=int(sfm.match_conf.numel()),
                share_in_consistent_tracks_before=round(float(ok.sum()) / K, 4),
                share_in_tracks_after=round(float((sfm2.track_id >= 0).sum()) / K, 4),
                tracks_len3_before=int(((sfm.track_len >= 3) & sfm.track_ok).sum()), tracks_len3_after=int((sfm2.track_len >= 3).sum()),
                inconsistent_tracks=int(bad.sum()), mean_inconsistent_track_len=round(float(sfm.track_len[bad].float().mean()), 1) if bad.any() else 0.0,
                rounds=done.stats["n_rounds"], n_open=done.stats["n_open"], n_conflict=done.stats["n_conflict"],
                largest_component=done.stats["largest_component"], share_of_tracks_with_one_point=round(float(pure.mean()), 4),
                atlas_host_s=round(atlas_s, 2), split_host_s=round(split_s, 3))


def reconstruction():
    scene = SC.noisy_scene()
    sfm = SC.run_atlas("cpu")
    out = {}
    for name, kw in (("without_split", {}), ("with_split", dict(split=True))):
        rec = sfm.reconstruct(scene["K"], **kw)
        rot, cen = evaluation.trajectory_errors(rec.T_cam_from_world, rec.posed, scene["T"])
        out[name] = dict(images_posed=int(rec.posed.sum()), n_ok=rec.points.stats["n_ok"], tracks=int(rec.points.offsets.numel() - 1),
                         rms_px_after=rec.stats.get("rms_px_after"), max_rot_deg=round(float(np.nanmax(rot)), 5),
                         max_centre_err=round(float(np.nanmax(cen)), 5), median_rot_deg=round(float(np.nanmedian(rot)), 5),
                         median_centre_err=round(float(np.nanmedian(cen)), 5))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=1500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [json.dumps(figures(args.points, **load)) for load in LOADS]
    lines.append(json.dumps({"reconstruct_test_scene_8_cameras_300_points": reconstruction()}))
    for line in lines:
        print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
