#!/usr/bin/env python
"""Pair lists through a feature bank (loftr_amd/pairs.py) against LoFTR.forward per chunk of 8 pairs.  One JSON line per workload.

    python tools/micro/pairs_bench.py [--workloads abcd] [--pairs N] [--budget-gb 32] [--repeats 3] [--frames 40]

Weights: bench.py's seeded state dict (matcher seed 0, backbone seed 7, BatchNorm strength 0.3).  Images: bench.py's seeded synthetic
pairs (synth.make_images, seed 1234) as a pool of 32; image id x is pool[x % 32] rolled by (x // 32) px, made on the GPU when loaded,
so a list has as many distinct images as it names.  Both paths load their images through the same function.

  (a) 8 pairs over 16 distinct images (no reuse): forward vs match_pair_list.
  (b) ScanNet-1500's pair structure (tests/golden/pair_lists.npz: 1500 pairs, 2596 images) at 640 x 480.
  (c) MegaDepth-1500's structure (1500 pairs, 806 images) at 840 x 840, bench.py's outdoor setting: rows >= 560 zero, coarse masks,
      scale 1.9, temp_bug_fix False, border_rm 2.  --pairs N takes the first N pairs.
  --budget-gb caps the bank of (b) and (c) (default 32: all of (c)'s images fit, (b)'s 2596 do not).
  (d) the demo loop at N = 1: ms per frame of forward(reference, frame) vs FeatureBank.add(frame) + match_pairs with the reference
      frame kept in the bank.
Each path gets a warm-up pass, then --repeats alternating timed passes (median and spread reported).  Also reported: backbone images
run and backbone calls of the bank path, bank bytes, and the share of extraction time spent copying the backbone output into the bank
(FeatureBank.add of 16 images against the bare backbone on them)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from loftr_amd import FeatureBank, LoFTR, get_cfg                     # noqa: E402
from loftr_amd.pairs import match_pair_list                            # noqa: E402
from loftr_amd.synth import make_backbone_weights, make_images, make_weights   # noqa: E402

DEV = "cuda:0"
BATCH = 8


def build(outdoor):
    torch.manual_seed(0)
    cfg = get_cfg(thr=0.0, border_rm=2) if outdoor else get_cfg(thr=0.0)
    cfg["coarse"]["temp_bug_fix"] = not outdoor
    model = LoFTR(cfg).eval()
    sd = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(v))) for k, v in make_weights(0, cfg).items()}
    for k, v in make_backbone_weights(7, model.backbone, 0.3).items():
        sd["backbone." + k] = v
    model.load_state_dict(sd, strict=True)
    return model.to(DEV)


class Images:
    """load(ids) -> {"image": [k,1,H,W], "mask", "scale"} of synthetic images; outdoor: bench.py's 840 x 840 padded setting."""

    def __init__(self, hw, outdoor):
        a, b = make_images(1234, 16, *hw)
        self.pool = torch.from_numpy(np.concatenate([a, b])).to(DEV)
        self.outdoor, self.hw = outdoor, hw
        if outdoor:
            self.pool[:, :, 560:] = 0
            self.mask = torch.zeros(hw[0] // 8, hw[1] // 8, dtype=torch.bool, device=DEV)
            self.mask[:70] = True

    def image(self, x):
        img = self.pool[x % len(self.pool)]
        img = torch.roll(img, x // len(self.pool), dims=2)
        if self.outdoor:
            img = img.clone()
            img[:, 560:] = 0
        return img

    def __call__(self, ids):
        out = {"image": torch.stack([self.image(int(x)) for x in ids])}
        if self.outdoor:
            k = len(ids)
            out.update(mask=self.mask.expand(k, -1, -1).contiguous(), scale=torch.full((k, 2), 1.9, device=DEV))
        return out


def run_forward(model, pairs, load):
    n = 0
    for r in range(0, len(pairs), BATCH):
        p = pairs[r:r + BATCH]
        a, b = load(p[:, 0]), load(p[:, 1])
        data = {"image0": a["image"], "image1": b["image"]}
        if "mask" in a:
            data.update(mask0=a["mask"], mask1=b["mask"], scale0=a["scale"], scale1=b["scale"])
        model(data)
        n += int(data["mconf"].shape[0])
    return n


def run_bank(model, pairs, load, hw, budget, stats):
    n = 0
    for _, data in match_pair_list(model, pairs, load, hw, budget_bytes=budget, stats=stats):
        n += int(data["mconf"].shape[0])
    return n


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def copy_share(model, load, hw):
    """Share of FeatureBank.add(16 images) spent on the copy into the bank: 1 - t(bare backbone) / t(add)."""
    x = load(list(range(16)))["image"]
    bank = FeatureBank(model, 16, hw)
    cl = x.contiguous(memory_format=torch.channels_last)
    run = model.backbone.forward_hip if model.backbone_impl == "hip" else model.backbone
    with torch.no_grad():
        for _ in range(2):
            bank.add(x, slots=list(range(16)))
            run(cl)
        tb, ta = [], []
        for _ in range(5):
            tb.append(timed(lambda: run(cl))[0])
            ta.append(timed(lambda: bank.add(x, slots=list(range(16))))[0])
    tb, ta = float(np.median(tb)), float(np.median(ta))
    return {"add16_ms": round(ta * 1e3, 3), "backbone16_ms": round(tb * 1e3, 3), "extract_copy_share": round(max(0.0, 1 - tb / ta), 4)}


def spread(xs):
    return {"median": round(float(np.median(xs)), 2), "min": round(float(min(xs)), 2), "max": round(float(max(xs)), 2),
            "runs": [round(float(x), 2) for x in xs]}


def pair_list_workload(tag, pairs, hw, outdoor, budget, repeats):
    model = build(outdoor)
    load = Images(hw, outdoor)
    U = len(np.unique(pairs))
    stats = {}
    m_fwd = run_forward(model, pairs, load)                               # warm-up (and match counts)
    m_bank = run_bank(model, pairs, load, hw, budget, stats)
    fwd, bank = [], []
    for _ in range(repeats):
        fwd.append(len(pairs) / timed(lambda: run_forward(model, pairs, load))[0])
        stats = {}
        bank.append(len(pairs) / timed(lambda: run_bank(model, pairs, load, hw, budget, stats))[0])
    out = {"workload": tag, "image_hw": list(hw), "pairs": len(pairs), "distinct_images": U, "uses_per_image": round(2 * len(pairs) / U, 2),
           "forward_pairs_per_s": spread(fwd), "bank_pairs_per_s": spread(bank),
           "speedup": round(float(np.median(bank) / np.median(fwd)), 3),
           "forward_backbone_images": 2 * len(pairs), "bank_backbone_images": stats["images_extracted"],
           "bank_backbone_calls": stats["backbone_calls"], "bank_slots": stats["n_slots"], "bank_bytes": stats["bank_bytes"],
           "matches_forward": m_fwd, "matches_bank": m_bank}
    out.update(copy_share(model, load, hw))
    print(json.dumps(out), flush=True)
    del model
    torch.cuda.empty_cache()


def demo_loop(frames, repeats):
    hw = (480, 640)
    model = build(False)
    load = Images(hw, False)
    ref = load([0])["image"]
    seq = [load([1 + k])["image"] for k in range(frames)]
    bank = FeatureBank(model, 2, hw)
    bank.add(ref, slots=[0])

    def fwd():
        for f in seq:
            model({"image0": ref, "image1": f})

    def banked():
        for f in seq:
            bank.add(f, slots=[1])
            model.match_pairs(bank, [0], bank, [1])
    fwd(); banked()
    a, b = [], []
    for _ in range(repeats):
        a.append(1e3 * timed(fwd)[0] / frames)
        b.append(1e3 * timed(banked)[0] / frames)
    print(json.dumps({"workload": "d_demo_loop", "image_hw": list(hw), "frames": frames, "forward_ms_per_frame": spread(a),
                      "bank_ms_per_frame": spread(b), "speedup": round(float(np.median(a) / np.median(b)), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workloads", default="abcd")
    ap.add_argument("--pairs", type=int, default=1500, help="(c) first N pairs of the MegaDepth-1500 structure")
    ap.add_argument("--budget-gb", type=float, default=32.0, help="(b), (c) bank budget")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=40)
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = True
    g = np.load(os.path.join(ROOT, "tests", "golden", "pair_lists.npz"))
    if "a" in args.workloads:
        pairs = np.stack([np.arange(8), np.arange(8, 16)], 1)
        pair_list_workload("a_no_reuse", pairs, (480, 640), False, None, args.repeats)
    if "b" in args.workloads:
        pair_list_workload("b_scannet1500", g["scannet_pairs"], (480, 640), False, int(args.budget_gb * 2 ** 30), args.repeats)
    if "c" in args.workloads:
        pairs = g["megadepth_pairs"][:args.pairs]
        pair_list_workload("c_megadepth1500", pairs, (840, 840), True, int(args.budget_gb * 2 ** 30), args.repeats)
    if "d" in args.workloads:
        demo_loop(args.frames, args.repeats)


if __name__ == "__main__":
    main()
