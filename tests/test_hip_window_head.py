"""The fine head's last convolution evaluated at the matched 5 x 5 windows only (csrc/window_head.hip) against the dense HIP path on
the same weights: exact equality.  The window kernel runs the dense kernel's arithmetic (same MFMA, k order, order of the three split
products, epilogue expression), so an output element does not depend on the tile row it sits in.

  * CPU: the kernel's index arithmetic (tile row -> window, pixel, in-image flag; patch row -> input pixel) stated in numpy and checked
    against the brute-force definition; the dispatch rule at the bench's window count and at 2x / 4x.
  * GPU, op level: the SP window tiles of ops.window_head == the SP encoding of the windows gathered from the dense convolution's fp32
    output, and ops.fine_preprocess_windows == ops.fine_preprocess on the dense maps.
  * GPU, forward level: LoFTR.forward with fine_head="windows" == fine_head="dense", every output tensor, for 1 / 3 / 8 pairs (single
    stream, side stream, two half-batch streams), first forward of a fresh model included.
"""
import os

import numpy as np
import pytest
import torch

WIN, WP = 5, 7


# ---- the kernel's index arithmetic, in numpy ------------------------------------------------------------------------------
def tile_rows(tile, nwin_tile, M, b_ids, i_ids, j_ids, w0c, w1c, stride, H, W):
    """Per tile row r of workgroup `tile` (nwin_tile windows x 25 rows): (valid, side, m, pixel, y, x, in_image) as the kernel's row table."""
    rows = []
    for r in range(nwin_tile * 25 + (32 - nwin_tile * 25 % 32) % 32):
        wl, px = divmod(r, 25)
        w = tile * nwin_tile + wl
        if wl >= nwin_tile or w >= 2 * M:
            rows.append((False, 0, 0, 0, 0, 0, False))
            continue
        side = int(w >= M)
        m = w - side * M
        cell, wc = (j_ids[m], w1c) if side else (i_ids[m], w0c)
        y = (cell // wc) * stride - WIN // 2 + px // WIN
        x = (cell % wc) * stride - WIN // 2 + px % WIN
        rows.append((True, side, m, px, y, x, 0 <= y < H and 0 <= x < W))
    return rows


def patch_rows(tile, nwin_tile, M, b_ids, i_ids, j_ids, w0c, w1c, stride, H, W):
    """Per patch row r (nwin_tile windows x 49 input pixels): (side, b, y, x) of the input pixel it stages, or None (zero page)."""
    out = []
    for r in range(nwin_tile * 49):
        wl, rem = divmod(r, 49)
        py, px = divmod(rem, WP)
        w = tile * nwin_tile + wl
        if w >= 2 * M:
            out.append(None)
            continue
        side = int(w >= M)
        m = w - side * M
        cell, wc = (j_ids[m], w1c) if side else (i_ids[m], w0c)
        y = (cell // wc) * stride - WIN // 2 - 1 + py
        x = (cell % wc) * stride - WIN // 2 - 1 + px
        out.append((side, int(b_ids[m]), y, x) if 0 <= y < H and 0 <= x < W else None)
    return out


def test_window_index_arithmetic_matches_the_definition(nwin_tile=5):
    """Every (side, match, window pixel) is produced exactly once over the tiles, with the coordinates F.unfold(kernel 5, stride, padding 2)
    gives the matched cell; and tap (ky, kx) of a tile row reads patch row arow + ky * 7 + kx, which stages exactly the input pixel
    (y + ky - 1, x + kx - 1) of the 3x3 / pad 1 convolution (None = zero padding)."""
    rng = np.random.default_rng(3)
    H, W, stride, w0c, w1c, N = 12, 20, 4, 5, 5, 2
    M = 13
    b_ids = rng.integers(0, N, M)
    i_ids = rng.permutation(3 * 5)[:M]
    j_ids = rng.permutation(3 * 5)[:M]
    seen = {}
    ntiles = -(-2 * M // nwin_tile)
    for t in range(ntiles):
        rows = tile_rows(t, nwin_tile, M, b_ids, i_ids, j_ids, w0c, w1c, stride, H, W)
        patch = patch_rows(t, nwin_tile, M, b_ids, i_ids, j_ids, w0c, w1c, stride, H, W)
        assert len(rows) % 32 == 0
        for r, (valid, side, m, px, y, x, inimg) in enumerate(rows):
            if not valid:
                continue
            assert (side, m, px) not in seen
            seen[(side, m, px)] = (y, x, inimg)
            wl = r // 25
            arow = wl * 49 + (px // WIN) * WP + px % WIN
            for ky in range(3):
                for kx in range(3):
                    yy, xx = y + ky - 1, x + kx - 1
                    want = (side, int(b_ids[m]), yy, xx) if 0 <= yy < H and 0 <= xx < W else None
                    assert patch[arow + ky * WP + kx] == want
    assert len(seen) == 2 * M * 25
    for (side, m, px), (y, x, inimg) in seen.items():                       # brute force: the unfold definition
        cell, wc = (j_ids[m], w1c) if side else (i_ids[m], w0c)
        cy, cx = (cell // wc) * stride, (cell % wc) * stride
        assert (y, x) == (cy + px // 5 - 2, cx + px % 5 - 2) and inimg == (0 <= y < H and 0 <= x < W)


def test_dispatch_rule_at_the_bench_density():
    """profiles/window_head_crossover.txt: on the bench's maps (16 images of 240 x 320) the window form wins at the bench's 6120 matches
    (765 per pair) and at twice (and three times) that many, and loses at four times; M = 0 and unsupported shapes take the dense head."""
    from loftr_amd import ops
    dense = 16 * 240 * 320
    assert ops.window_head_wins(6120, dense) and ops.window_head_wins(2 * 6120, dense) and not ops.window_head_wins(4 * 6120, dense)
    assert ops.window_head_wins(3 * 6120, dense)
    assert not ops.window_head_wins(0, dense)
    h = torch.empty(8, 24, 32, 224, dtype=torch.int32, device="meta")
    assert ops.window_head_supported(5, 196, 128, h, h)
    assert not ops.window_head_supported(5, 196, 128, h, h[:, :20])          # images of two sizes: dense
    assert not ops.window_head_supported(7, 196, 128, h, h) and not ops.window_head_supported(5, 196, 196, h, h)
    assert not ops.window_head_supported(5, 196, 112, h, h)                   # a narrower fine level: dense (window rows are 128 dwords)


def test_window_kernel_fits_two_workgroups_per_cu():
    """The occupancy the kernel is designed for, read off the compiled code object: no scratch, at most 80 KB of LDS and 256 registers."""
    import shutil
    import tempfile
    from loftr_amd import build as B
    from test_isa_audit import _asm, _kernel_resources
    if not (os.path.isfile(B._hipcc()) or shutil.which(B._hipcc())):
        pytest.skip("hipcc is not installed here")
    with tempfile.TemporaryDirectory() as d:
        res = {k: v for k, v in _kernel_resources(_asm("window_head.hip", d)[1]).items() if "window_head_kernel" in k}
    assert len(res) == 1
    for k, v in res.items():
        assert v["scratch"] == 0 and v["lds"] <= 80 * 1024 and v["vgpr"] <= 256, (k, v)


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _sp_words(v):
    """fp32 [..., C] (C % 32 == 0) -> the SP dwords [..., C] the library stores for it (csrc/gemm.h: hi = fp16(v), lo = fp16(v - hi); per
    group of 32 channels 16 dwords of hi pairs, then 16 of lo pairs)."""
    h = v.half()
    l = (v - h.float()).half()
    hb = h.view(torch.int16).to(torch.int64) & 0xFFFF
    lb = l.view(torch.int16).to(torch.int64) & 0xFFFF
    shp = v.shape[:-1] + (v.shape[-1] // 32, 16, 2)
    hb, lb = hb.reshape(shp), lb.reshape(shp)
    hi = hb[..., 0] | (hb[..., 1] << 16)
    lo = lb[..., 0] | (lb[..., 1] << 16)
    w = torch.cat((hi, lo), dim=-1).reshape(v.shape)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def _gather(dense, b_ids, ids, wc, stride):
    """dense fp32 [N, H, W, C] -> windows [M, 25, C] (zeros outside the map)."""
    N, H, W, C = dense.shape
    pad = torch.zeros(N, H + 4, W + 4, C, device=dense.device)
    pad[:, 2:-2, 2:-2] = dense
    cy, cx = (ids // wc) * stride, (ids % wc) * stride
    d = torch.arange(5, device=dense.device)
    yy = (cy[:, None, None] + d[None, :, None]).expand(-1, 5, 5)
    xx = (cx[:, None, None] + d[None, None, :]).expand(-1, 5, 5)
    return pad[b_ids[:, None, None], yy, xx].reshape(len(ids), 25, C)


def _head(dev, seed=0, cin=196, cout=128):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5)
    return conv.to(dev).eval()


def _check_op(N, H, W, b_ids, i_ids, j_ids, seed):
    from loftr_amd import ops
    dev = "cuda:0"
    stride, hc, wc = 4, H // 4, W // 4
    g = torch.Generator().manual_seed(seed)
    conv = _head(dev, seed)
    x = torch.randn(2 * N, H, W, 196, generator=g).to(dev)
    x = torch.where(x > 0, x, 0.01 * x)                                     # LeakyReLU-like, as the head's first layer leaves it
    h = ops.sp_from_nhwc(x)
    h0, h1 = h[:N], h[N:]
    _, dense = ops.conv_bn_act(h, 196, conv, want_sp=False, want_f32=True)
    b_ids, i_ids, j_ids = (torch.as_tensor(t, dtype=torch.int64, device=dev) for t in (b_ids, i_ids, j_ids))
    want0 = _sp_words(_gather(dense[:N], b_ids, i_ids, wc, stride))
    want1 = _sp_words(_gather(dense[N:], b_ids, j_ids, wc, stride))
    w0, w1 = ops.window_head(h0, h1, 196, conv, b_ids, i_ids, j_ids, (hc, wc), (hc, wc), 5, stride)
    torch.cuda.synchronize()
    assert torch.equal(w0, want0), ("side 0", int((w0 != want0).sum()))
    assert torch.equal(w1, want1), ("side 1", int((w1 != want1).sum()))
    # the whole FinePreprocess on top of either form
    fc0, fc1 = (torch.randn(N, hc * wc, 256, generator=g).to(dev) for _ in range(2))
    lin = dict(down_w=torch.randn(128, 256, generator=g).to(dev) * 0.06, down_b=torch.randn(128, generator=g).to(dev) * 0.1,
               merge_w=torch.randn(128, 256, generator=g).to(dev) * 0.06, merge_b=torch.randn(128, generator=g).to(dev) * 0.1)
    fmap = dense.permute(0, 3, 1, 2)
    a0, a1 = ops.fine_preprocess(fmap[:N], fmap[N:], fc0, fc1, b_ids, i_ids, j_ids, (hc, wc), (hc, wc), 5, stride, **lin)
    c0, c1 = ops.fine_preprocess_windows(h0, h1, 196, conv, fc0, fc1, b_ids, i_ids, j_ids, (hc, wc), (hc, wc), 5, stride, **lin)
    torch.cuda.synchronize()
    assert torch.equal(a0, c0) and torch.equal(a1, c1)


def _random_cells(N, per_pair, cells, seed):
    rng = np.random.default_rng(seed)
    b = np.repeat(np.arange(N), per_pair)
    i = np.concatenate([rng.permutation(cells)[:per_pair] for _ in range(N)])
    j = np.concatenate([rng.permutation(cells)[:per_pair] for _ in range(N)])
    return b, i, j


@pytest.mark.gpu
def test_windows_equal_a_gather_of_the_dense_map_at_the_bench_shape():
    """8 pairs of 640 x 480: fine maps 240 x 320, 765 random distinct cells per image (the bench's density)."""
    _check_op(8, 240, 320, *_random_cells(8, 765, 60 * 80, 1), seed=1)


@pytest.mark.gpu
def test_windows_on_corners_and_edges_are_zero_padded_like_the_dense_path():
    """border 0: windows (and their 7 x 7 input rings) partly outside the map, in all four corners and on every edge."""
    hc, wc = 6, 8
    cells = [0, wc - 1, (hc - 1) * wc, hc * wc - 1,            # corners
             3, (hc - 1) * wc + 4, 2 * wc, 3 * wc + wc - 1,     # top, bottom, left, right edges
             2 * wc + 3]                                        # interior
    i = np.array(cells)
    j = np.array(cells[::-1])
    _check_op(1, hc * 4, wc * 4, np.zeros(len(cells), dtype=np.int64), i, j, seed=2)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one", "seven", "all_cells"])
def test_window_counts_that_do_not_fill_a_tile(case):
    hc, wc = 5, 7
    if case == "all_cells":
        N = 2
        b = np.repeat(np.arange(N), hc * wc)
        i = np.tile(np.arange(hc * wc), N)
        j = np.tile(np.arange(hc * wc)[::-1], N)
    else:
        N, M = 2, 1 if case == "one" else 7
        b, i, j = np.array([1] * M), np.arange(M) * 3, np.arange(M) * 4 + 1
    _check_op(N, hc * 4, wc * 4, b, i, j, seed=4)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 8])
def test_forward_with_the_window_head_is_bit_identical_to_the_dense_head(n, monkeypatch):
    """LoFTR.forward, fine_head "windows" against "dense" (and the default rule), on the first n pairs of the 8-pair golden's images: the
    single-stream (serial), side-stream (n < 8) and two-halves (n = 8) schedules; the first forward of every fresh model is compared too.
    "rule_loses": the rule with its factor set to 0, i.e. the branch forward takes above the crossover -- the head's last convolution run
    densely on the main stream from the SP tensors the side streams hand over (backbone.fine_head_last), then the plain gather."""
    from loftr_amd import ops
    from test_e2e_golden import build_model, load
    rc, img0, img1, g = load("e2e_batch8")
    dev = "cuda:0"
    FILL = ops.WINDOW_HEAD_MAX_FILL
    keys = ("b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f", "conf_matrix")
    outs = {}
    for tag, kw in (("dense", dict(fine_head="dense")), ("windows", dict(fine_head="windows")), ("rule", {}), ("rule_loses", {}),
                    ("windows_serial", dict(fine_head="windows", overlap_fine_branch=False))):
        model = build_model(rc, 0.0, dev)
        for k, v in kw.items():
            setattr(model, k, v)
        monkeypatch.setattr(ops, "WINDOW_HEAD_MAX_FILL", 0.0 if tag == "rule_loses" else FILL)
        runs = []
        for _ in range(2):
            data = {"image0": torch.from_numpy(img0[:n]).to(dev), "image1": torch.from_numpy(img1[:n]).to(dev)}
            model(data)
            runs.append({k: data[k].detach().clone() for k in keys})
            assert tuple(data["hw0_f"]) == (img0.shape[2] // 2, img0.shape[3] // 2)
        torch.cuda.synchronize()
        for k, v in runs[0].items():
            assert torch.equal(v, runs[1][k]), (tag, "first vs second forward", k)
        outs[tag] = runs[1]
        head = getattr(model.fine_preprocess, "last_head", None)
        M, pixels = len(runs[1]["mconf"]), 2 * n * (img0.shape[2] // 2) * (img0.shape[3] // 2)
        # ("dense": the fine branch runs whole, as run_backbone schedules it -- FinePreprocess.forward_windows is never entered)
        want = None if tag == "dense" else "dense" if (tag == "rule_loses" or (tag == "rule" and not ops.window_head_wins(M, pixels))) else "windows"
        assert head == want, (tag, head, M)
    assert len(outs["dense"]["mconf"]) > 50 * n
    for tag in ("windows", "rule", "rule_loses", "windows_serial"):
        for k in keys:
            assert torch.equal(outs[tag][k], outs["dense"][k]), (tag, k)


@pytest.mark.gpu
def test_images_of_two_sizes_take_the_dense_head():
    from test_e2e_golden import build_model, load
    rc, img0, img1, g = load("e2e_batch8")
    dev = "cuda:0"
    model = build_model(rc, 0.0, dev)
    data = {"image0": torch.from_numpy(img0[:1]).to(dev), "image1": torch.from_numpy(np.ascontiguousarray(img1[:1, :, :416, :512])).to(dev)}
    assert not model._window_head_applies(data)
    model(data)
    assert model.fine_preprocess.last_head is None and len(data["mconf"]) > 0
