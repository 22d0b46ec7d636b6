"""Op-level crossover of the two forms of the fine head's last convolution (csrc/window_head.hip, ops.WINDOW_HEAD_MAX_FILL).

    python -m tools.micro.window_head_crossover [--out profiles/window_head_crossover.txt]

On the bench's maps (2 x 8 images, 240 x 320 x 196 SP in, 128 channels out) with random distinct cells per image at 1x / 2x / 3x / 3.5x / 3.75x / 4x
the bench's 765 matches per pair (the last four bracket the crossover), it times
  dense   = conv_bn_act (fp32 fine map) + fine_preprocess (gather_windows_kernel + the merge GEMMs)
  windows = fine_preprocess_windows (window_head_kernel + the same merge GEMMs)
and the window kernel alone.  Medians of hipEvent times over --reps launches after a warm-up.
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
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    from loftr_amd import ops
    dev = "cuda:0"
    N, H, W, cin, cout, hc, wc, stride = 8, 240, 320, 196, 128, 60, 80, 4
    g = torch.Generator().manual_seed(0)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1, bias=False).to(dev).eval()
    x = torch.randn(2 * N, H, W, cin, generator=g).to(dev)
    h = ops.sp_from_nhwc(torch.where(x > 0, x, 0.01 * x))
    del x
    h0, h1 = h[:N], h[N:]
    fc0, fc1 = (torch.randn(N, hc * wc, 256, generator=g).to(dev) for _ in range(2))
    lin = dict(down_w=torch.randn(128, 256, generator=g).to(dev) * 0.06, down_b=torch.zeros(128, device=dev),
               merge_w=torch.randn(128, 256, generator=g).to(dev) * 0.06, merge_b=torch.zeros(128, device=dev))
    rng = np.random.default_rng(0)
    lines = ["# fine head, last convolution: dense form against window form, op level, 2 x 8 maps of 240 x 320 x 196 -> 128 channels",
             "# us, median of %d; fill = 2 M * 49 / (16 * 240 * 320)" % args.reps,
             "%8s %6s %6s %12s %14s %12s %8s" % ("per_pair", "M", "fill", "dense_total", "windows_total", "win_kernel", "winner")]
    wins, loses = [], []
    for mult in (1, 2, 3, 3.5, 3.75, 4):
        per = int(765 * mult)
        b = torch.from_numpy(np.repeat(np.arange(N), per)).to(dev)
        i = torch.from_numpy(np.concatenate([rng.permutation(hc * wc)[:per] for _ in range(N)])).to(dev)
        j = torch.from_numpy(np.concatenate([rng.permutation(hc * wc)[:per] for _ in range(N)])).to(dev)
        M = N * per
        geo = ((hc, wc), (hc, wc), 5, stride)

        def dense():
            f = ops.conv_bn_act(h, cin, conv, want_sp=False, want_f32=True)[1].permute(0, 3, 1, 2)
            ops.fine_preprocess(f[:N], f[N:], fc0, fc1, b, i, j, *geo, **lin)

        t_d = timed(dense, args.reps)
        t_w = timed(lambda: ops.fine_preprocess_windows(h0, h1, cin, conv, fc0, fc1, b, i, j, *geo, **lin), args.reps)
        t_k = timed(lambda: ops.window_head(h0, h1, cin, conv, b, i, j, *geo), args.reps)
        lines.append("%8d %6d %6.2f %12.0f %14.0f %12.0f %8s" % (per, M, 2 * M * 49 / (2 * N * H * W), t_d, t_w, t_k,
                                                                "windows" if t_w < t_d else "dense"))
        (wins if t_w < t_d else loses).append(2 * M * 49 / (2 * N * H * W))
        print(lines[-1], flush=True)
    lines.append("# window form ahead up to fill %.2f (the largest measured point at which it wins), behind from fill %.2f"
                 % (max(wins, default=0.0), min(loses, default=float("inf"))))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
