"""Both convolutions of the FPN fine head at the matched windows only (csrc/window_head_first.hip).

  * CPU: the window / neighbourhood / patch-row index arithmetic of both kernels against the unfold definition; the resources of the two
    kernels read off the compiled code object; the dispatch rule; argument checks of the entry points.
  * GPU, op level: the first kernel's neighbourhood rows == the dense layer's SP rows gathered at the 7 x 7 neighbourhoods (zeros outside
    the map); first -> last kernel == ops.window_head on the dense first-layer output; the whole FinePreprocess on either form.
  * GPU, forward level: LoFTR.forward with the dense head, both window forms, the rule, and the rule with one / both factors forced to 0:
    every output tensor identical, on the side-stream, two-halves and serial schedules.
All comparisons are torch.equal: the kernels repeat the dense kernels' arithmetic, an element's sum does not depend on its tile row."""
import ctypes
import os

import numpy as np
import pytest
import torch

WIN, NB7, P9 = 5, 7, 9             # window side, neighbourhood side (the last kernel's patch), the first kernel's patch side
NWIN = 5                           # windows of a workgroup, both kernels
BAD_ARG, UNSUPPORTED = -1, -2


# ---- the kernels' index arithmetic, in numpy ---------------------------------------------------------------------------
def _cell_origin(side, m, i_ids, j_ids, w0c, w1c, stride):
    cell, wc = (j_ids[m], w1c) if side else (i_ids[m], w0c)
    return (cell // wc) * stride, (cell % wc) * stride


def _tile_rows(tile, out, M, i_ids, j_ids, w0c, w1c, stride, H, W):
    """Per tile row r of workgroup `tile` (NWIN windows x out*out rows, padded to 32): (valid, side, m, pixel, y, x, in_image)."""
    oo = out * out
    rows = []
    for r in range(-(-NWIN * oo // 32) * 32):
        wl, px = divmod(r, oo)
        w = tile * NWIN + wl
        if wl >= NWIN or w >= 2 * M:
            rows.append((False, 0, 0, 0, 0, 0, False))
            continue
        side = int(w >= M)
        m = w - side * M
        cy, cx = _cell_origin(side, m, i_ids, j_ids, w0c, w1c, stride)
        y, x = cy - out // 2 + px // out, cx - out // 2 + px % out
        rows.append((True, side, m, px, y, x, 0 <= y < H and 0 <= x < W))
    return rows


def _patch_rows_first(tile, M, b_ids, i_ids, j_ids, w0c, w1c, stride, H, W):
    """The first kernel's patch rows (NWIN windows x 81 input pixels): (side, b, y, x) of the map pixel staged, or None (zero page)."""
    out = []
    for r in range(NWIN * P9 * P9):
        wl, rem = divmod(r, P9 * P9)
        py, px = divmod(rem, P9)
        w = tile * NWIN + wl
        if w >= 2 * M:
            out.append(None)
            continue
        side = int(w >= M)
        m = w - side * M
        cy, cx = _cell_origin(side, m, i_ids, j_ids, w0c, w1c, stride)
        y, x = cy - NB7 // 2 - 1 + py, cx - NB7 // 2 - 1 + px
        out.append((side, int(b_ids[m]), y, x) if 0 <= y < H and 0 <= x < W else None)
    return out


def test_index_arithmetic_of_both_kernels_matches_the_definition():
    """First kernel: every (side, match, neighbourhood pixel) is produced exactly once over the tiles, at scratch row
    (side * M + m) * 49 + py * 7 + px with the coordinates (cy - 3 + py, cx - 3 + px); tap (ky, kx) of a tile row reads patch row
    arow + ky * 9 + kx, which stages the input pixel (y + ky - 1, x + kx - 1) of the 3x3 / pad 1 convolution (None = zero padding).
    Last kernel: tap (ky, kx) of window pixel (wy, wx) reads scratch row (wy + ky) * 7 + wx + kx of its window, which holds the
    first layer's pixel (y + ky - 1, x + kx - 1) -- or zeros outside the map; the window pixels are F.unfold(kernel 5, padding 2)'s."""
    rng = np.random.default_rng(5)
    H, W, stride, w0c, w1c, N = 12, 20, 4, 5, 5, 2
    M = 13
    b_ids = rng.integers(0, N, M)
    i_ids = rng.permutation(3 * 5)[:M]
    j_ids = rng.permutation(3 * 5)[:M]
    ntiles = -(-2 * M // NWIN)
    scratch = {}                                             # scratch row -> (side, b, y, x, in_image) of the pixel it holds
    for t in range(ntiles):
        rows = _tile_rows(t, NB7, M, i_ids, j_ids, w0c, w1c, stride, H, W)
        patch = _patch_rows_first(t, M, b_ids, i_ids, j_ids, w0c, w1c, stride, H, W)
        assert len(rows) == 256
        for r, (valid, side, m, px, y, x, inimg) in enumerate(rows):
            if not valid:
                continue
            row = (side * M + m) * 49 + px
            assert row not in scratch
            scratch[row] = (side, int(b_ids[m]), y, x, inimg)
            wl = r // 49
            arow = wl * 81 + (px // NB7) * P9 + px % NB7
            for ky in range(3):
                for kx in range(3):
                    yy, xx = y + ky - 1, x + kx - 1
                    want = (side, int(b_ids[m]), yy, xx) if 0 <= yy < H and 0 <= xx < W else None
                    assert patch[arow + ky * P9 + kx] == want
    assert sorted(scratch) == list(range(2 * M * 49))
    for row, (side, b, y, x, inimg) in scratch.items():      # brute force: the definition of the neighbourhood rows
        w, px = divmod(row, 49)
        m = w - side * M
        cy, cx = _cell_origin(side, m, i_ids, j_ids, w0c, w1c, stride)
        assert side == int(w >= M) and (y, x) == (cy - 3 + px // 7, cx - 3 + px % 7) and inimg == (0 <= y < H and 0 <= x < W)
    seen = set()
    for t in range(ntiles):
        rows = _tile_rows(t, WIN, M, i_ids, j_ids, w0c, w1c, stride, H, W)
        assert len(rows) == 128
        for r, (valid, side, m, px, y, x, inimg) in enumerate(rows):
            if not valid:
                continue
            assert (side, m, px) not in seen
            seen.add((side, m, px))
            cy, cx = _cell_origin(side, m, i_ids, j_ids, w0c, w1c, stride)
            assert (y, x) == (cy + px // 5 - 2, cx + px % 5 - 2)                  # the unfold definition
            wl = r // 25
            arow = wl * 49 + (px // WIN) * NB7 + px % WIN                        # patch row = row of the window's scratch block
            for ky in range(3):
                for kx in range(3):
                    prow = arow + ky * NB7 + kx
                    assert prow // 49 == wl
                    s_side, s_b, s_y, s_x, s_in = scratch[(t * NWIN + wl) * 49 + prow % 49]
                    assert (s_side, s_b, s_y, s_x) == (side, int(b_ids[m]), y + ky - 1, x + kx - 1)
                    assert s_in == (0 <= s_y < H and 0 <= s_x < W)
    assert len(seen) == 2 * M * 25


def test_dispatch_rule_of_the_first_convolution():
    """profiles/window_head_first_crossover.txt: on the bench's maps (16 images of 240 x 320) both window kernels win at the bench's 6120
    matches (fill 0.49); the rule never holds without the last convolution's (window_head_wins), at M = 0, or above its own factor."""
    from loftr_amd import ops
    dense = 16 * 240 * 320
    assert ops.window_head_first_wins(6120, dense)
    assert not ops.window_head_first_wins(0, dense)
    assert not ops.window_head_first_wins(4 * 6120, dense)                   # window_head_wins does not hold there
    assert ops.WINDOW_HEAD_FIRST_MAX_FILL <= ops.WINDOW_HEAD_MAX_FILL
    m_over = int(ops.WINDOW_HEAD_FIRST_MAX_FILL * dense / 98) + 1
    assert not ops.window_head_first_wins(m_over, dense) and ops.window_head_first_wins(m_over - 1, dense)
    conv0, conv1 = torch.nn.Conv2d(196, 196, 3, padding=1, bias=False), torch.nn.Conv2d(196, 128, 3, padding=1, bias=False)
    t = torch.empty(8, 24, 32, 224, dtype=torch.int32, device="meta")
    assert ops.window_head_first_supported(5, 196, conv0, conv1, t, t, 6120)
    assert not ops.window_head_first_supported(7, 196, conv0, conv1, t, t, 6120)
    assert not ops.window_head_first_supported(5, 196, conv0, conv1, t, t[:, :20], 6120)
    assert not ops.window_head_first_supported(5, 196, conv0, conv1, t, t, 2 ** 31 // (98 * 224) + 1)      # the scratch tensor's 32-bit index
    wide = torch.nn.Conv2d(196, 224, 3, padding=1, bias=False)
    assert not ops.window_head_first_supported(5, 196, wide, torch.nn.Conv2d(224, 128, 3, padding=1, bias=False), t, t, 6120)


def test_both_kernels_fit_their_occupancy():
    """Read off the compiled code object: no scratch; the first kernel (8 waves, one workgroup per CU) at most 160 KB of LDS and 256
    registers, the last kernel (4 waves, two workgroups per CU) at most 80 KB and 256."""
    import shutil
    import tempfile
    from loftr_amd import build as B
    from test_isa_audit import _asm, _kernel_resources
    if not (os.path.isfile(B._hipcc()) or shutil.which(B._hipcc())):
        pytest.skip("hipcc is not installed here")
    with tempfile.TemporaryDirectory() as d:
        res = {k: v for k, v in _kernel_resources(_asm("window_head_first.hip", d)[1]).items() if "window_nbhd_kernel" in k}
    assert len(res) == 2
    first = [v for k, v in res.items() if "Li7ELi7E" in k]
    last = [v for k, v in res.items() if "Li5ELi4E" in k]
    assert len(first) == 1 and len(last) == 1, sorted(res)
    assert first[0]["scratch"] == 0 and first[0]["lds"] <= 160 * 1024 and first[0]["vgpr"] <= 256, first
    assert last[0]["scratch"] == 0 and last[0]["lds"] <= 80 * 1024 and last[0]["vgpr"] <= 256, last


@pytest.fixture(scope="module")
def lib():
    from loftr_amd import _lib, build as build_mod
    build_mod.build(verbose=False)
    return _lib.load()


def test_entry_points_check_their_arguments_before_any_device_work(lib):
    """Null pointers: LOFTR_ERR_BAD_ARG; M == 0: a no-op success; W != 5, channel widths other than 196 -> 196 -> 128 and a scratch
    tensor beyond 32-bit indexing: LOFTR_ERR_UNSUPPORTED -- all before anything is dereferenced or launched (host dummies, no GPU)."""
    buf = (ctypes.c_uint32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value

    def first(t0=p, prep=p, ids=p, nb=p, Cin=196, Cout=196, M=3, W=5):
        return lib.loftr_window_head_first(t0, p, 2, 24, 32, Cin, prep, 1 << 22, Cout, ids, ids, ids, M, 8, 8, 4, W, nb, None)

    assert first(t0=None) == BAD_ARG and first(prep=None) == BAD_ARG and first(ids=None) == BAD_ARG and first(nb=None) == BAD_ARG
    assert first(M=-1) == BAD_ARG
    assert first(M=0) == 0 and first(M=0, t0=None, nb=None) == 0
    assert first(W=7) == UNSUPPORTED and first(Cin=128) == UNSUPPORTED and first(Cout=128) == UNSUPPORTED
    assert first(M=2 ** 31 // (98 * 224) + 1) == UNSUPPORTED

    def last(nb=p, prep=p, ids=p, win=p, Cin=196, Cout=128, M=3, W=5):
        return lib.loftr_window_head_last(nb, 24, 32, Cin, prep, 1 << 22, Cout, ids, ids, ids, M, 8, 8, 4, W, win, win, None)

    assert last(nb=None) == BAD_ARG and last(prep=None) == BAD_ARG and last(ids=None) == BAD_ARG and last(win=None) == BAD_ARG
    assert last(M=0) == 0
    assert last(W=7) == UNSUPPORTED and last(Cin=128) == UNSUPPORTED and last(Cout=196) == UNSUPPORTED

    def both(t0=p, prep0=p, prep1=p, ids=p, out=p, nb=p, Cin=196, Cmid=196, Cf=128, M=3, W=5):
        return lib.loftr_fine_preprocess_window_head2(t0, p, 2, 24, 32, Cin, prep0, 1 << 22, Cmid, prep1, 1 << 22, p, p, 48, 48, 256,
                                                      ids, ids, ids, M, 8, 8, 4, W, Cf, p, p, p, p, out, out, p, 0, nb, None)

    assert both(t0=None) == BAD_ARG and both(prep0=None) == BAD_ARG and both(prep1=None) == BAD_ARG and both(ids=None) == BAD_ARG
    assert both(out=None) == BAD_ARG and both(nb=None) == BAD_ARG and both(M=-1) == BAD_ARG
    assert both(M=0) == 0
    assert both(W=7) == UNSUPPORTED and both(Cin=128) == UNSUPPORTED and both(Cmid=128) == UNSUPPORTED and both(Cf=196) == UNSUPPORTED
    assert both(M=2 ** 31 // (98 * 224) + 1) == UNSUPPORTED


# ---- GPU, op level -------------------------------------------------------------------------------------------------------
def _gather7(dense_sp, b_ids, ids, wc, stride):
    """dense SP int32 [N, H, W, C] -> neighbourhood rows [M, 49, C] (zero words outside the map)."""
    N, H, W, C = dense_sp.shape
    pad = torch.zeros(N, H + 6, W + 6, C, dtype=dense_sp.dtype, device=dense_sp.device)
    pad[:, 3:-3, 3:-3] = dense_sp
    cy, cx = (ids // wc) * stride, (ids % wc) * stride
    d = torch.arange(7, device=dense_sp.device)
    yy = (cy[:, None, None] + d[None, :, None]).expand(-1, 7, 7)
    xx = (cx[:, None, None] + d[None, None, :]).expand(-1, 7, 7)
    return pad[b_ids[:, None, None], yy, xx].reshape(len(ids), 49, C)


def _head(dev, seed):
    """conv 196 -> 196 + BatchNorm with random statistics (a non-trivial fold) + conv 196 -> 128."""
    g = torch.Generator().manual_seed(seed)
    conv0 = torch.nn.Conv2d(196, 196, 3, padding=1, bias=False)
    conv1 = torch.nn.Conv2d(196, 128, 3, padding=1, bias=False)
    bn = torch.nn.BatchNorm2d(196)
    with torch.no_grad():
        conv0.weight.copy_(torch.randn(196, 196, 3, 3, generator=g) * (2.0 / (9 * 196)) ** 0.5)
        conv1.weight.copy_(torch.randn(128, 196, 3, 3, generator=g) * (2.0 / (9 * 196)) ** 0.5)
        bn.weight.copy_(torch.rand(196, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(196, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(196, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(196, generator=g) + 0.5)
    return conv0.to(dev).eval(), bn.to(dev).eval(), conv1.to(dev).eval()


def _check_op(N, H, W, b_ids, i_ids, j_ids, seed):
    from loftr_amd import ops
    dev = "cuda:0"
    stride, hc, wc = 4, H // 4, W // 4
    g = torch.Generator().manual_seed(seed)
    conv0, bn, conv1 = _head(dev, seed)
    t = ops.sp_from_nhwc(torch.randn(2 * N, H, W, 196, generator=g).to(dev))
    t0, t1 = t[:N], t[N:]
    dense, _ = ops.conv_bn_act(t, 196, conv0, bn, act=2)                     # SP [2N, H, W, 224]
    b_ids, i_ids, j_ids = (torch.as_tensor(v, dtype=torch.int64, device=dev) for v in (b_ids, i_ids, j_ids))
    M = len(b_ids)
    want = torch.cat((_gather7(dense[:N], b_ids, i_ids, wc, stride), _gather7(dense[N:], b_ids, j_ids, wc, stride)))
    geo = ((hc, wc), (hc, wc), 5, stride)
    nb = ops.window_head_first(t0, t1, 196, conv0, bn, b_ids, i_ids, j_ids, *geo)
    torch.cuda.synchronize()
    assert nb.shape == (2 * M, 49, 224)
    assert torch.equal(nb, want), ("neighbourhood rows", int((nb != want).sum()), int((nb != want).any(-1).sum()))
    # pad channels 196 .. 223 (group 6: hi dwords 192 .. 207, lo dwords 208 .. 223, two channels each) are zero words
    assert not nb[..., 194:208].any() and not nb[..., 210:].any()
    # first -> last kernel against window_head on the dense first-layer output
    w0, w1 = ops.window_head(dense[:N], dense[N:], 196, conv1, b_ids, i_ids, j_ids, *geo)
    v0, v1 = ops.window_head_last(nb, (H, W), 196, conv1, b_ids, i_ids, j_ids, *geo)
    torch.cuda.synchronize()
    assert torch.equal(v0, w0), ("side 0", int((v0 != w0).sum()))
    assert torch.equal(v1, w1), ("side 1", int((v1 != w1).sum()))
    # the whole FinePreprocess on top of either form
    fc0, fc1 = (torch.randn(N, hc * wc, 256, generator=g).to(dev) for _ in range(2))
    lin = dict(down_w=torch.randn(128, 256, generator=g).to(dev) * 0.06, down_b=torch.randn(128, generator=g).to(dev) * 0.1,
               merge_w=torch.randn(128, 256, generator=g).to(dev) * 0.06, merge_b=torch.randn(128, generator=g).to(dev) * 0.1)
    a0, a1 = ops.fine_preprocess_windows(dense[:N], dense[N:], 196, conv1, fc0, fc1, b_ids, i_ids, j_ids, *geo, **lin)
    c0, c1 = ops.fine_preprocess_windows2(t0, t1, 196, conv0, bn, conv1, fc0, fc1, b_ids, i_ids, j_ids, *geo, **lin)
    torch.cuda.synchronize()
    assert torch.equal(a0, c0) and torch.equal(a1, c1)


@pytest.mark.gpu
def test_corners_and_edges_are_zero_rows_like_the_dense_padding():
    """border 0 on a 24 x 32 map: neighbourhoods (and their 9 x 9 input patches) partly outside the map, in all four corners and on every
    edge; j is the reversed list, so the two sides differ."""
    hc, wc = 6, 8
    cells = [0, wc - 1, (hc - 1) * wc, hc * wc - 1,            # corners
             3, (hc - 1) * wc + 4, 2 * wc, 3 * wc + wc - 1,     # top, bottom, left, right edges
             2 * wc + 3]                                        # interior
    _check_op(1, hc * 4, wc * 4, np.zeros(len(cells), dtype=np.int64), np.array(cells), np.array(cells[::-1]), seed=2)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one", "seven", "all_cells"])
def test_window_counts_below_across_and_off_the_five_window_tile(case):
    """N = 2 on a 20 x 28 map: 2, 14 and 140 windows (b_ids != 0)."""
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
def test_several_full_tiles_with_both_sides_in_one_tile():
    """N = 2 on a 48 x 64 map, 30 random distinct cells per image: 120 windows = 24 tiles, side 0 ends inside tile 12."""
    rng = np.random.default_rng(7)
    N, per, cells = 2, 30, 12 * 16
    b = np.repeat(np.arange(N), per)
    i = np.concatenate([rng.permutation(cells)[:per] for _ in range(N)])
    j = np.concatenate([rng.permutation(cells)[:per] for _ in range(N)])
    _check_op(N, 48, 64, b, i, j, seed=6)


# ---- GPU, forward level ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,sched", [(1, {}), (3, {}), (1, dict(backbone_halves=True)), (1, dict(overlap_fine_branch=False))],
                         ids=["1", "3", "1-halves", "1-serial"])
def test_forward_is_bit_identical_across_the_three_forms_of_the_head(n, sched, monkeypatch):
    """LoFTR.forward on the first n pairs of the 8-pair golden's images: the dense head, both window forms forced, the default rule, the
    rule with the first convolution's factor at 0 (first dense on the main stream, last at the windows) and with both factors at 0 (both
    dense on the main stream); side stream, two half streams, and no overlap.  The first forward of every fresh model equals its second;
    last_head / last_head_first report the form taken."""
    from loftr_amd import ops
    from test_e2e_golden import build_model, load
    rc, img0, img1, g = load("e2e_batch8")
    dev = "cuda:0"
    FILL, FIRST = ops.WINDOW_HEAD_MAX_FILL, ops.WINDOW_HEAD_FIRST_MAX_FILL
    keys = ("b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f", "conf_matrix")
    outs = {}
    for tag, kw, fill, first in (("dense", dict(fine_head="dense"), FILL, FIRST), ("windows", dict(fine_head="windows"), FILL, FIRST),
                                 ("rule", {}, FILL, FIRST), ("first_loses", {}, FILL, 0.0), ("both_lose", {}, 0.0, 0.0)):
        model = build_model(rc, 0.0, dev)
        for k, v in {**kw, **sched}.items():
            setattr(model, k, v)
        monkeypatch.setattr(ops, "WINDOW_HEAD_MAX_FILL", fill)
        monkeypatch.setattr(ops, "WINDOW_HEAD_FIRST_MAX_FILL", first)
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
        M, pixels = len(runs[1]["mconf"]), 2 * n * (img0.shape[2] // 2) * (img0.shape[3] // 2)
        form = lambda wins: "windows" if wins else "dense"
        want = {"dense": (None, None), "windows": ("windows", "windows"),
                "rule": (form(ops.window_head_first_wins(M, pixels)), form(ops.window_head_wins(M, pixels))),
                "first_loses": ("dense", form(ops.window_head_wins(M, pixels))), "both_lose": ("dense", "dense")}[tag]
        got = (model.fine_preprocess.last_head_first, model.fine_preprocess.last_head)
        assert got == want, (tag, got, want, M)
    assert len(outs["dense"]["mconf"]) > 50 * n
    for tag in ("windows", "rule", "first_loses", "both_lose"):
        for k in keys:
            assert torch.equal(outs[tag][k], outs["dense"][k]), (tag, k)
