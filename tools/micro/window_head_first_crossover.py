"""Op-level crossover of the two forms of the fine head's FIRST convolution (csrc/window_head_first.hip, ops.WINDOW_HEAD_FIRST_MAX_FILL).

    python -m tools.micro.window_head_first_crossover [--out profiles/window_head_first_crossover.txt]

On the bench's maps (2 x 8 images, 240 x 320 x 196 SP in, 196 -> 128 channels out) with random distinct cells per image at 0.5x / 1x / 1.5x / 2x
the bench's 765 matches per pair, it times
  dense pair  = conv_bn_act of the head's first layer (two 8-image launches, as the forward runs them) + window_head
  window pair = window_head_first + window_head_last (kernel A + kernel B)
and, alone, the dense launches against kernel A.  Medians of hipEvent times over --reps launches after a warm-up; the spread (min .. max)
of the dense pair's repeated timings is the noise a win has to exceed.
"""
import argparse
import sys

import numpy as np
import torch


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    from loftr_amd import ops
    dev = "cuda:0"
    N, H, W, cin, cmid, cout, hc, wc, stride = 8, 240, 320, 196, 196, 128, 60, 80, 4
    g = torch.Generator().manual_seed(0)
    conv0 = torch.nn.Conv2d(cin, cmid, 3, padding=1, bias=False).to(dev).eval()
    bn = torch.nn.BatchNorm2d(cmid).to(dev).eval()
    conv1 = torch.nn.Conv2d(cmid, cout, 3, padding=1, bias=False).to(dev).eval()
    t = ops.sp_from_nhwc(torch.randn(2 * N, H, W, cin, generator=g).to(dev))
    t0, t1 = t[:N], t[N:]
    rng = np.random.default_rng(0)
    lines = ["# fine head, first convolution: dense form against window form, op level, 2 x 8 maps of 240 x 320 x 196 -> 196 -> 128 channels",
             "# us, median of %d (dense pair: min .. max too); fill = 2 M * 49 / (16 * 240 * 320)" % args.reps,
             "%8s %6s %6s %11s %15s %12s %11s %9s %8s" % ("per_pair", "M", "fill", "dense_pair", "dense_min..max", "window_pair",
                                                           "dense_first", "kernel_A", "winner")]
    wins, loses = [], []
    for mult in (0.5, 1, 1.5, 2):
        per = int(765 * mult)
        b = torch.from_numpy(np.repeat(np.arange(N), per)).to(dev)
        i = torch.from_numpy(np.concatenate([rng.permutation(hc * wc)[:per] for _ in range(N)])).to(dev)
        j = torch.from_numpy(np.concatenate([rng.permutation(hc * wc)[:per] for _ in range(N)])).to(dev)
        M = N * per
        geo = ((hc, wc), (hc, wc), 5, stride)

        def dense_first():
            return ops.conv_bn_act(t0, cin, conv0, bn, act=2)[0], ops.conv_bn_act(t1, cin, conv0, bn, act=2)[0]

        def dense_pair():
            h0, h1 = dense_first()
            ops.window_head(h0, h1, cmid, conv1, b, i, j, *geo)

        def window_pair():
            nb = ops.window_head_first(t0, t1, cin, conv0, bn, b, i, j, *geo)
            ops.window_head_last(nb, (H, W), cmid, conv1, b, i, j, *geo)

        t_d, d_lo, d_hi = timed(dense_pair, args.reps)
        t_w, _, _ = timed(window_pair, args.reps)
        t_f, _, _ = timed(dense_first, args.reps)
        t_a, _, _ = timed(lambda: ops.window_head_first(t0, t1, cin, conv0, bn, b, i, j, *geo), args.reps)
        fill = 2 * M * 49 / (2 * N * H * W)
        won = t_w < t_d - (d_hi - d_lo)
        lines.append("%8d %6d %6.2f %11.0f %15s %12.0f %11.0f %9.0f %8s" % (per, M, fill, t_d, "%.0f..%.0f" % (d_lo, d_hi), t_w, t_f, t_a,
                                                                           "windows" if won else "dense"))
        (wins if won else loses).append(fill)
        print(lines[-1], flush=True)
    lines.append("# window pair ahead by more than the dense pair's spread up to fill %.2f (the largest measured point at which it wins), not from fill %.2f"
                 % (max(wins, default=0.0), min(loses, default=float("inf"))))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
