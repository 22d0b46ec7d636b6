#!/usr/bin/env python
"""fine_pair_kernel at op level: four waves per workgroup against eight (debug switch fine_waves), over match counts, the two forms
alternating call by call.  The table is what the launch rule in csrc/fine_fused.hip (FINE_WAVES8_MIN_M) is read from.
    python tools/micro/fine_waves_crossover.py [M ...]        (default: 256 765 1024 2048 4096 6120 12240)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from loftr_amd import LoFTR, get_cfg, ops     # noqa: E402
from loftr_amd.synth import make_weights      # noqa: E402

MS = [int(a) for a in sys.argv[1:]] or [256, 765, 1024, 2048, 4096, 6120, 12240]
REPS, WARM = 40, 5
cfg = get_cfg(thr=0.0)
w = make_weights(0, cfg)
model = LoFTR(cfg).eval()
model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(np.asarray(v))) for k, v in w.items()}, strict=False)
model = model.cuda()
print(f"{'M':>6s}  {'4 waves: median (min) us':>26s}  {'8 waves: median (min) us':>26s}  {'8 / 4':>6s}  same bits")
for M in MS:
    g = torch.Generator(device="cpu").manual_seed(M)
    f0 = torch.randn(M, 25, 128, generator=g).cuda()
    f1 = (0.6 * f0 + 0.8 * torch.randn(M, 25, 128, generator=g).cuda()).contiguous()
    times, outs = {4: [], 8: []}, {}
    with torch.no_grad():
        for r in range(WARM + REPS):
            for waves in (4, 8):
                a, b = f0.clone(), f1.clone()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with ops.debug_switch(fine_waves=waves):
                    e0.record()
                    model.loftr_fine(a, b, inplace=True)
                    e1.record()
                torch.cuda.synchronize()
                if r >= WARM:
                    times[waves].append(e0.elapsed_time(e1) * 1e3)
                outs[waves] = (a, b)
    same = torch.equal(outs[4][0], outs[8][0]) and torch.equal(outs[4][1], outs[8][1])
    m4, m8 = np.median(times[4]), np.median(times[8])
    print(f"{M:6d}  {m4:16.1f} ({min(times[4]):7.1f})  {m8:16.1f} ({min(times[8]):7.1f})  {m8 / m4:6.3f}  {same}", flush=True)
