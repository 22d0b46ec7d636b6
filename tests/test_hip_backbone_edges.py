"""The inference backbone's kernels -- conv_kernel<CfgD> (strided / 1x1 layers, fused FPN top-down step), conv3x3_duo_kernel (128 k / 192 /
224 columns, remainder form), conv3x3_kernel, stem_conv_kernel, upsample_add_kernel -- against PyTorch on the CPU in FLOAT64 at their tile,
stride and width edges.  Cases, restated dispatch, references, tolerances: tests/_backbone_edge_cases.py.

Five kinds of check.  (1) The whole tensor: err <= min(K noise + 1e-6 scale, cap), noise being the distance of the float32 reference to the
float64 one, the cap the bound tests/test_hip_backbone.py holds the operation to.  (2) On maps of at least 256 output pixels every channel
against its own maximum: err_c / max|ref64_c| <= K_CH noise_c + 1e-6; a BatchNorm gamma = 0 channel is act(bias) at every pixel.  (3) Integer
inputs: the result equals the integer convolution EXACTLY, whatever the summation order.  (4) Guard bands through the C ABI: inputs and
outputs are carved out of larger buffers filled with NaN words; the output guards stay bit-for-bit untouched, every word inside was written,
pad channels are zero and the values still meet (1), so no guard word was read into a result.  (5) The same image three times in a batch
gives three bit-identical outputs, equal to the single-image run.  The status codes of the argument checks are pinned too.

Each run prints its figures before it asserts and appends them to the file LOFTR_EDGES_REPORT names, if set (how
profiles/backbone_edges_accuracy.txt was written)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _backbone_edge_cases as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2


def _report(line):
    path = os.environ.get("LOFTR_EDGES_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")
    print(line)


def _ratio(err, noise):
    return err / noise if noise > 0 else (0.0 if err == 0 else float("inf"))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _sp(t):
    """float32 [B, C, H, W] (CPU) -> SP [B, H, W, ceil32(C)] on the GPU."""
    from loftr_amd import ops
    return None if t is None else ops.sp_from_nhwc(_nhwc(t).to(DEV))


def _decode(y_sp, Cc):
    """SP [B, H, W, Cp] -> float64 numpy [B, Cc, H, W]."""
    from loftr_amd import ops
    return ops.sp_to_nhwc(y_sp, Cc).permute(0, 3, 1, 2).cpu().double().numpy()


def _f32(y_nhwc):
    return y_nhwc.permute(0, 3, 1, 2).cpu().double().numpy()


def _pad_channels_are_zero(y_sp, Cc):
    from loftr_amd import ops
    Cp = y_sp.shape[-1]
    return Cp == Cc or bool((ops.sp_to_nhwc(y_sp, Cp)[..., Cc:] == 0).all())


def _check(table, name, out, got, ref, kind, family, failures, skip=()):
    """Checks 1 and 2 of one output; prints and reports the figures first."""
    assert got.shape == ref["ref64"].shape, (name, out, got.shape, ref["ref64"].shape)
    if not np.isfinite(got).all():
        failures.append((out, "not finite", int((~np.isfinite(got)).sum())))
        return
    err, tol = float(np.abs(got - ref["ref64"]).max()), E.tolerance(kind, family, ref["noise"], ref["scale"])
    _report(f"{table:5s} {name:34s} {family:8s} {out:5s} tensor  err {err:.3e} noise {ref['noise']:.3e} err/noise {_ratio(err, ref['noise']):7.3f} scale {ref['scale']:.3e} "
            f"err/scale {err / ref['scale']:.2e}")
    if err > tol:
        failures.append((out, "tensor", err, tol, ref["noise"], ref["scale"]))
    if ref.get("channels"):
        bad, ratio, worst = E.channel_failures(got, ref, family, "f32" if out.startswith("f32") else "sp", skip)
        _report(f"{table:5s} {name:34s} {family:8s} {out:5s} channel err {worst:.3e} noise {float(ref['ch_noise'].max()):.3e} err/noise {ratio:7.3f} channels {int(ref['live'].sum())}")
        if bad:
            failures.append((out, "channel", bad[:4], len(bad)))


# ---- convolutions -------------------------------------------------------------------------------------------------------------------------
def _conv_modules(c, w, bn):
    conv = nn.Conv2d(c.cin, c.cout, c.k, stride=c.stride, padding=c.k // 2, bias=False)
    conv.weight.data = w.clone()
    bnm = None
    if bn is not None:
        bnm = nn.BatchNorm2d(c.cout, eps=bn[4]).eval()
        bnm.weight.data, bnm.bias.data, bnm.running_mean.data, bnm.running_var.data = (t.clone() for t in bn[:4])
        bnm = bnm.to(DEV)
    return conv.to(DEV), bnm


def _conv_call(c, x_sp, conv, bnm, r_sp, mode, act):
    from loftr_amd import ops
    with ops.debug_switch(**dict(c.switches)):
        ops.CONV_REM = c.rem
        try:
            y_sp, y_f32 = ops.conv_bn_act(x_sp, c.cin, conv, bnm, act=act, residual=r_sp, want_sp=mode != "f32", want_f32=mode != "sp", shared_gpu=c.shared)
        finally:
            ops.CONV_REM = False
    torch.cuda.synchronize()
    return y_sp, y_f32


@pytest.mark.parametrize("name", [c.name for c in E.CONV_CASES])
def test_conv_vs_float64(name):
    """Checks 1 and 2, with the SP output alone, the fp32 output alone and both (K, K_CH: tests/_backbone_edge_cases.py)."""
    i, ref = E.conv_inputs(name), E.conv_reference(name)
    c = i["case"]
    conv, bnm = _conv_modules(c, i["w"], i["bn"])
    x_sp, r_sp = _sp(i["x"]), _sp(i["res"])
    failures = []
    skip = (E.GAMMA0_CH,) if c.weights == "bnedge" else ()
    for mode in E.conv_modes(c):
        y_sp, y_f32 = _conv_call(c, x_sp, conv, bnm, r_sp, mode, c.act)
        assert (y_sp is None) == (mode == "f32") and (y_f32 is None) == (mode == "sp")
        outs = ([("sp", _decode(y_sp, c.cout))] if y_sp is not None else []) + ([("f32", _f32(y_f32))] if y_f32 is not None else [])
        for out, got in outs:
            label = out if mode != "both" else out + "+"
            _check("conv", name, label, got, ref, "conv", c.family, failures, skip)
            if c.weights == "bnedge" and np.isfinite(got).all():         # the gamma = 0 channel: act(bias), held to the TENSOR's scale
                d = float(np.abs(got[:, E.GAMMA0_CH] - ref["gamma0_value"]).max())
                if d > 1e-6 * ref["scale"] or (out == "f32" and d != 0.0):
                    failures.append((label, "gamma = 0 channel is not act(bias)", d, ref["gamma0_value"]))
        if y_sp is not None and not _pad_channels_are_zero(y_sp, c.cout):
            failures.append((mode, "pad channels of the SP rows are not zero"))
    assert not failures, (name, failures)


@pytest.mark.parametrize("name", E.EXACT_CONV)
def test_conv_exact_on_integers(name):
    """Check 3: integer activations in [-8, 8], integer weights in [-2, 2], an integer residual where the case has one, no BatchNorm, no
    activation: every operand half is exact and every partial sum an integer, so the result is the integer convolution bit for bit."""
    c = E.CONV_BY_NAME[name]
    x, w, res, want = E.exact_conv(name)
    want = want.numpy()
    conv, _ = _conv_modules(c, w, None)
    x_sp, r_sp = _sp(x), _sp(res)
    failures = []
    for mode in E.conv_modes(c):
        y_sp, y_f32 = _conv_call(c, x_sp, conv, None, r_sp, mode, 0)
        for out, got in ([("sp", _decode(y_sp, c.cout))] if y_sp is not None else []) + ([("f32", _f32(y_f32))] if y_f32 is not None else []):
            d = E.first_difference(got, want)
            _report(f"exact {name:34s} {c.family:8s} {out + ('+' if mode == 'both' else ''):5s} differing {0 if d is None else d[0]} of {want.size} max |value| {np.abs(want).max():.0f}")
            if d is not None:
                failures.append((mode, out, "count %d, first at (image, y, x, channel) %s: got %r, want %r" % d))
        if y_sp is not None and not _pad_channels_are_zero(y_sp, c.cout):
            failures.append((mode, "pad channels of the SP rows are not zero"))
    assert not failures, (name, failures)


# ---- guard bands --------------------------------------------------------------------------------------------------------------------------
def _round64(n):
    return (n + 63) // 64 * 64


def _carve(inner, guard_words, fill=E.GUARD_WORD):
    """A copy of the int32 tensor `inner` in the middle of one larger device buffer filled with `fill`: (buffer, view of the copy)."""
    n, g = inner.numel(), _round64(guard_words)
    buf = torch.full((g + n + g,), fill, dtype=torch.int32, device=DEV)
    view = buf[g:g + n].view(inner.shape)
    view.copy_(inner)
    return buf, view


def _carve_out(shape, fill=E.GUARD_WORD):
    n = int(np.prod(shape))
    buf = torch.full((E.GUARD_OUT_WORDS + n + E.GUARD_OUT_WORDS,), fill, dtype=torch.int32, device=DEV)
    return buf, buf[E.GUARD_OUT_WORDS:E.GUARD_OUT_WORDS + n].view(shape)


def _guards_untouched(buf, inner_words, fill=E.GUARD_WORD):
    g = (buf.numel() - inner_words) // 2
    return bool((buf[:g] == fill).all()) and bool((buf[g + inner_words:] == fill).all())


def _sp_guard_checks(label, buf, view, Cc, failures):
    """Output guards untouched, every word inside written (it decodes to a finite value), pad channels zero -> decoded float64 [B, Cc, H, W]."""
    from loftr_amd import ops
    if not _guards_untouched(buf, view.numel()):
        failures.append((label, "a word of the SP output's guard band was written"))
    full = ops.sp_to_nhwc(view, view.shape[-1])
    if not bool(torch.isfinite(full).all()):
        failures.append((label, "SP words left unwritten (or not finite)", int((~torch.isfinite(full)).sum())))
    if view.shape[-1] != Cc and not bool((full[..., Cc:] == 0).all()):
        failures.append((label, "pad channels of the SP rows are not zero"))
    return full[..., :Cc].permute(0, 3, 1, 2).cpu().double().numpy()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("name", E.GUARD_CONV)
def test_conv_guard_bands(name):
    """Check 4 on the ragged and minimal convolution cases, through loftr_conv_bn_act_prepared_scratch with both outputs (the remainder
    form: SP only).  The input sits between at least four image rows of NaN words, each output between 4096."""
    from loftr_amd import ops, _lib
    i, ref = E.conv_inputs(name), E.conv_reference(name)
    c = i["case"]
    lib = _lib.load()
    conv, bnm = _conv_modules(c, i["w"], i["bn"])
    prepared = ops._prepared_conv(conv, bnm)
    Ho, Wo = E.out_hw(c.H, c.W, c.k, c.stride)
    Cp, Coutp = E.ceil32(c.cin), E.ceil32(c.cout)
    xbuf, x_in = _carve(_sp(i["x"]), max(4096, 4 * c.W * Cp))
    r_sp = _sp(i["res"])
    ybuf, y_sp = _carve_out((c.B, Ho, Wo, Coutp))
    fbuf, y_f = (None, None) if c.rem else _carve_out((c.B, Ho, Wo, c.cout))
    nscr = lib.loftr_conv_scratch_bytes(c.B, c.H, c.W, c.cout, c.k, c.k, c.stride) if c.rem else 0
    scratch = torch.empty(nscr, dtype=torch.uint8, device=DEV) if nscr else None
    assert bool(nscr) == c.rem and x_in.data_ptr() % 256 == 0 and y_sp.data_ptr() % 256 == 0
    rc = lib.loftr_conv_bn_act_prepared_scratch(_p(x_in), c.B, c.H, c.W, c.cin, _p(prepared), prepared.numel(), c.cout, c.k, c.k, c.stride, c.k // 2,
                                                c.act | (ops.CONV_SHARED_GPU if c.shared else 0), _p(r_sp), None, _p(y_sp), _p(y_f), None, _p(scratch), nscr, _stream())
    torch.cuda.synchronize()
    assert rc == OK, (name, rc)
    failures = []
    if not _guards_untouched(xbuf, x_in.numel()):
        failures.append(("x", "the input's guard band was written"))
    got = _sp_guard_checks("sp", ybuf, y_sp, c.cout, failures)
    _check("guard", name, "sp", got, ref, "conv", c.family, failures)
    if y_f is not None:
        if not _guards_untouched(fbuf, y_f.numel()):
            failures.append(("f32", "a word of the fp32 output's guard band was written"))
        if bool((y_f == E.GUARD_WORD).any()):
            failures.append(("f32", "fp32 words left unwritten", int((y_f == E.GUARD_WORD).sum())))
        _check("guard", name, "f32", y_f.view(torch.float32).permute(0, 3, 1, 2).cpu().double().numpy(), ref, "conv", c.family, failures)
    assert not failures, (name, failures)


# ---- stem -----------------------------------------------------------------------------------------------------------------------------------
def _stem_call(x, w, bn, y_sp):
    """loftr_stem_conv_bn_relu on a [B, 1, H, W] float32 GPU tensor of any strides; bn None: no BatchNorm."""
    from loftr_amd import _lib
    B, _, H, W = x.shape
    xs, ws = (C.c_long * 4)(*x.stride()), (C.c_long * 4)(*w.stride())
    bnp = [None] * 4 if bn is None else [_p(t) for t in bn[:4]]
    rc = _lib.load().loftr_stem_conv_bn_relu(_p(x), xs, B, H, W, _p(w), ws, w.shape[0], *bnp, 0.0 if bn is None else bn[4], _p(y_sp), _stream())
    torch.cuda.synchronize()
    return rc


def _stem_modules(i):
    c = i["case"]
    conv = nn.Conv2d(1, c.C0, 7, stride=2, padding=3, bias=False)
    conv.weight.data = i["w"].clone()
    bnm = nn.BatchNorm2d(c.C0, eps=i["bn"][4]).eval()
    bnm.weight.data, bnm.bias.data, bnm.running_mean.data, bnm.running_var.data = (t.clone() for t in i["bn"][:4])
    return conv.to(DEV), bnm.to(DEV)


def _stem_input(i):
    """The case's image on the GPU with the case's layout: contiguous, or the same crop of the larger image."""
    c = i["case"]
    if not c.crop:
        return i["x"].to(DEV)
    x = i["big"].to(DEV)[:, :, E.CROP_Y:E.CROP_Y + c.H, E.CROP_X:E.CROP_X + c.W]
    assert not x.is_contiguous() or c.H * c.W == 1
    return x


@pytest.mark.parametrize("name", [c.name for c in E.STEM_CASES])
def test_stem_vs_float64(name):
    """Checks 1 and 2 of stem_conv_kernel, the input contiguous or a strided view; pad channels of the SP rows are zero."""
    from loftr_amd import ops
    i, ref = E.stem_inputs(name), E.stem_reference(name)
    c = i["case"]
    conv, bnm = _stem_modules(i)
    y = ops.stem_conv_bn_relu(_stem_input(i), conv, bnm)
    torch.cuda.synchronize()
    failures = []
    assert y.shape == (c.B, (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1, E.ceil32(c.C0))
    _check("stem", name, "sp", _decode(y, c.C0), ref, "stem", "stem", failures)
    if not _pad_channels_are_zero(y, c.C0):
        failures.append(("sp", "pad channels of the SP rows are not zero"))
    assert not failures, (name, failures)


@pytest.mark.parametrize("name", [c.name for c in E.STEM_CASES])
def test_stem_exact_on_integers(name):
    """Check 3: an integer image and filter without BatchNorm (the C ABI's null BatchNorm pointers): relu(conv) exactly."""
    c = E.STEM_BY_NAME[name]
    x, w, want = E.exact_stem(name)
    y = torch.empty(c.B, want.shape[2], want.shape[3], E.ceil32(c.C0), dtype=torch.int32, device=DEV)
    assert _stem_call(x.to(DEV), w.to(DEV), None, y) == OK
    d = E.first_difference(_decode(y, c.C0), want.numpy())
    _report(f"exact {name:34s} {'stem':8s} {'sp':5s} differing {0 if d is None else d[0]} of {want.numel()} max |value| {float(want.max()):.0f}")
    assert d is None, (name, "count %d, first at (image, y, x, channel) %s: got %r, want %r" % d)
    assert _pad_channels_are_zero(y, c.C0), name


@pytest.mark.parametrize("name", E.GUARD_STEM)
def test_stem_guard_bands(name):
    """Check 4: the image (for a crop: the larger image it is a view of) between at least four rows of float NaN, the output between 4096 NaN words."""
    i, ref = E.stem_inputs(name), E.stem_reference(name)
    c = i["case"]
    src = i["big"] if c.crop else i["x"]
    nanbits = int(np.array([np.nan], np.float32).view(np.int32)[0])
    xbuf, xv = _carve(src.contiguous().view(torch.int32).to(DEV), max(4096, 4 * src.shape[-1]), fill=nanbits)
    x = xv.view(torch.float32)
    if c.crop:
        x = x[:, :, E.CROP_Y:E.CROP_Y + c.H, E.CROP_X:E.CROP_X + c.W]
    Ho, Wo = (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1
    ybuf, y = _carve_out((c.B, Ho, Wo, E.ceil32(c.C0)))
    assert _stem_call(x, i["w"].to(DEV), [t.to(DEV) for t in i["bn"][:4]] + [i["bn"][4]], y) == OK
    failures = []
    if not _guards_untouched(xbuf, xv.numel(), nanbits):
        failures.append(("x", "the input's guard band was written"))
    got = _sp_guard_checks("sp", ybuf, y, c.C0, failures)
    _check("guard", name, "sp", got, ref, "stem", "stem", failures)
    assert not failures, (name, failures)


# ---- FPN top-down step ------------------------------------------------------------------------------------------------------------------------
def _up_modules(i):
    c = i["case"]
    conv = nn.Conv2d(c.cin, c.C, 1, bias=False)
    conv.weight.data = i["w"].clone()
    return conv.to(DEV)


@pytest.mark.parametrize("name", [c.name for c in E.UP_CASES])
def test_topdown_vs_float64(name):
    """Checks 1 and 2 of upsample2x_add (upsample_add_kernel) and conv1x1_upsample_add (conv_kernel<CfgD, true>: conv_epilogue_up)."""
    from loftr_amd import ops
    i, ref = E.up_inputs(name), E.up_reference(name)
    c = i["case"]
    low = _sp(i["low"])
    y = ops.conv1x1_upsample_add(_sp(i["x"]), c.cin, _up_modules(i), low) if c.fused else ops.upsample2x_add(low, _sp(i["lat"]), c.C)
    torch.cuda.synchronize()
    assert y.shape == (c.B, 2 * c.Hl, 2 * c.Wl, E.ceil32(c.C))
    failures = []
    _check("up", name, "sp", _decode(y, c.C), ref, E.up_kind(c), E.up_kind(c), failures)
    if not _pad_channels_are_zero(y, c.C):
        failures.append(("sp", "pad channels of the SP rows are not zero"))
    assert not failures, (name, failures)


@pytest.mark.parametrize("name", E.GUARD_UP + E.GUARD_FUSED)
def test_topdown_guard_bands(name):
    """Check 4: the half-resolution map, the lateral map (or the lateral convolution's input) and the output carved out of NaN-filled buffers."""
    from loftr_amd import ops, _lib
    i, ref = E.up_inputs(name), E.up_reference(name)
    c = i["case"]
    lib = _lib.load()
    Cp = E.ceil32(c.C)
    lbuf, low = _carve(_sp(i["low"]), max(4096, 4 * c.Wl * Cp))
    ybuf, y = _carve_out((c.B, 2 * c.Hl, 2 * c.Wl, Cp))
    if c.fused:
        conv = _up_modules(i)
        prepared = ops._prepared_conv(conv, None)
        abuf, a = _carve(_sp(i["x"]), max(4096, 8 * c.Wl * E.ceil32(c.cin)))
        rc = lib.loftr_conv_bn_act_prepared_scratch(_p(a), c.B, 2 * c.Hl, 2 * c.Wl, c.cin, _p(prepared), prepared.numel(), c.C, 1, 1, 1, 0, 0, None, _p(low), _p(y), None,
                                                    None, None, 0, _stream())
    else:
        abuf, a = _carve(_sp(i["lat"]), max(4096, 8 * c.Wl * Cp))
        rc = lib.loftr_upsample2x_add(_p(low), _p(a), _p(y), c.B, c.Hl, c.Wl, c.C, _stream())
    torch.cuda.synchronize()
    assert rc == OK, (name, rc)
    failures = []
    if not (_guards_untouched(lbuf, low.numel()) and _guards_untouched(abuf, a.numel())):
        failures.append(("in", "an input's guard band was written"))
    got = _sp_guard_checks("sp", ybuf, y, c.C, failures)
    _check("guard", name, "sp", got, ref, E.up_kind(c), E.up_kind(c), failures)
    assert not failures, (name, failures)


# ---- whole network ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in E.NET_CASES])
def test_backbone_vs_float64(name):
    """forward_hip of both configurations at maps whose coarse level is 1 x 1, 1 x 33 and 3 x 5, against the module itself in float64."""
    r = E.net_reference(name)
    c = r["case"]
    m = E.net_module(c).to(DEV).to(memory_format=torch.channels_last)
    with torch.no_grad():
        hip = m.forward_hip(r["x"].to(DEV))
    torch.cuda.synchronize()
    failures = []
    for out, h, ref in zip(("coarse", "fine"), hip, r["outs"]):
        assert h.dtype == torch.float32
        _check("net", name, out[:5], h.cpu().double().numpy(), ref, "net", "net", failures)
    assert not failures, (name, failures)


# ---- position in the batch ----------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def _position_failures(name, family, outs1, outs3):
    """outs1: outputs of the single-image run, outs3: of the batch of three copies -> [(output, image, differing words)]."""
    bad = []
    for k, (o1, o3) in enumerate(zip(outs1, outs3)):
        if o1 is None:
            continue
        for b in range(3):
            if not _same(o3[b:b + 1].contiguous(), o1):
                bad.append((k, b, int((o3[b:b + 1].contiguous().view(torch.int32) != o1.view(torch.int32)).sum())))
    _report(f"batch {name:34s} {family:8s} three copies of one image, {sum(o is not None for o in outs1)} output(s): {len(bad)} copies differ from the single-image run")
    return bad


@pytest.mark.parametrize("name", E.POSITION_CONV)
def test_conv_position_in_the_batch(name):
    """Check 5: image 0 of the case three times in a batch -- its copies start at different rows of a 256-row tile / on other tiles of the
    grid -- gives three bit-identical outputs, equal to the single-image run."""
    i = E.conv_inputs(name)
    c = i["case"]
    conv, bnm = _conv_modules(c, i["w"], i["bn"])
    x1, r1 = i["x"][:1], None if i["res"] is None else i["res"][:1]
    mode = E.conv_modes(c)[-1]
    outs1 = _conv_call(c, _sp(x1), conv, bnm, _sp(r1), mode, c.act)
    outs3 = _conv_call(c, _sp(x1.repeat(3, 1, 1, 1)), conv, bnm, None if r1 is None else _sp(r1.repeat(3, 1, 1, 1)), mode, c.act)
    bad = _position_failures(name, c.family, outs1, outs3)
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", E.POSITION_STEM)
def test_stem_position_in_the_batch(name):
    from loftr_amd import ops
    i = E.stem_inputs(name)
    conv, bnm = _stem_modules(i)
    x1 = _stem_input(i)[:1]
    y1, y3 = ops.stem_conv_bn_relu(x1, conv, bnm), ops.stem_conv_bn_relu(x1.expand(3, -1, -1, -1), conv, bnm)       # (batch stride 0: the same image thrice)
    torch.cuda.synchronize()
    bad = _position_failures(name, "stem", [y1], [y3])
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", E.POSITION_UP)
def test_topdown_position_in_the_batch(name):
    from loftr_amd import ops
    i = E.up_inputs(name)
    c = i["case"]
    rep = lambda t: t[:1].repeat(3, 1, 1, 1)
    if c.fused:
        conv = _up_modules(i)
        y1 = ops.conv1x1_upsample_add(_sp(i["x"][:1]), c.cin, conv, _sp(i["low"][:1]))
        y3 = ops.conv1x1_upsample_add(_sp(rep(i["x"])), c.cin, conv, _sp(rep(i["low"])))
    else:
        y1, y3 = ops.upsample2x_add(_sp(i["low"][:1]), _sp(i["lat"][:1]), c.C), ops.upsample2x_add(_sp(rep(i["low"])), _sp(rep(i["lat"])), c.C)
    torch.cuda.synchronize()
    bad = _position_failures(name, E.up_kind(c), [y1], [y3])
    assert not bad, (name, bad)


# ---- argument checks ------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_return_their_status():
    """Null pointers, an empty output map, the fused step on an odd map, C0 > 128 and M Coutp >= 2^31 are refused by conv_run /
    loftr_stem_conv_bn_relu / loftr_upsample2x_add BEFORE any launch (csrc/conv.hip: every check stands above the first
    hipLaunchKernelGGL and above conv_prepared_layout), so the small buffers handed in here are never touched."""
    from loftr_amd import ops, _lib
    lib = _lib.load()
    conv = nn.Conv2d(32, 32, 1, bias=False).to(DEV)
    prepared = ops._prepared_conv(conv, None)
    x = torch.zeros(1, 4, 4, 32, dtype=torch.int32, device=DEV)
    low = torch.zeros(1, 2, 2, 32, dtype=torch.int32, device=DEV)
    ybuf, y = _carve_out((1, 4, 4, 32))
    fbuf, yf = _carve_out((1, 4, 4, 32))

    def run(xp=x, prep=prepared, B=1, H=4, W=4, cin=32, cout=32, k=1, stride=1, pad=0, act=0, res=None, lowp=None, ysp=y, yf32=None):
        return lib.loftr_conv_bn_act_prepared_scratch(_p(xp), B, H, W, cin, _p(prep), prepared.numel(), cout, k, k, stride, pad, act, _p(res), _p(lowp), _p(ysp), _p(yf32),
                                                      None, None, 0, _stream())
    assert run(xp=None) == BAD_ARG and run(prep=None) == BAD_ARG and run(ysp=None, yf32=None) == BAD_ARG
    assert run(H=0) == BAD_ARG and run(cin=0) == BAD_ARG and run(act=3) == BAD_ARG and run(stride=0) == BAD_ARG and run(B=-1) == BAD_ARG
    assert run(B=0) == OK                                                        # an empty batch: nothing to do
    assert run(H=2, W=2, k=3, pad=0) == UNSUPPORTED                              # Ho = 0
    assert run(H=1, W=4, k=3, pad=0) == UNSUPPORTED                              # Ho < 0
    assert run(H=3, W=4, lowp=low) == UNSUPPORTED and run(H=4, W=3, lowp=low) == UNSUPPORTED          # the fused step on an odd map
    assert run(lowp=low, yf32=yf) == UNSUPPORTED and run(lowp=low, act=1) == UNSUPPORTED and run(lowp=low, res=x) == UNSUPPORTED
    assert run(H=4096, W=4096, cout=128) == UNSUPPORTED                          # M Coutp = 2^31
    assert run(B=16, H=2048, W=2048, cout=1) == UNSUPPORTED                      # ... also where Cout itself is small (Coutp = 32)
    assert run(H=32768, W=1) == UNSUPPORTED
    assert run(cout=64) == -3                                                    # a prepared buffer of another layer: LOFTR_ERR_WORKSPACE
    # stem
    w = torch.zeros(E.STEM_UNSUPPORTED_C0, 1, 7, 7, device=DEV)
    img = torch.zeros(1, 1, 8, 8, device=DEV)
    sbuf, sy = _carve_out((1, 4, 4, E.ceil32(E.STEM_UNSUPPORTED_C0)))
    assert _stem_call(img, w, None, sy) == UNSUPPORTED
    xs, ws = (C.c_long * 4)(*img.stride()), (C.c_long * 4)(*w.stride())
    assert lib.loftr_stem_conv_bn_relu(None, xs, 1, 8, 8, _p(w), ws, 128, None, None, None, None, 0.0, _p(sy), _stream()) == BAD_ARG
    assert lib.loftr_stem_conv_bn_relu(_p(img), xs, 1, 8, 8, _p(w), ws, 128, _p(w), None, None, None, 0.0, _p(sy), _stream()) == BAD_ARG     # half a BatchNorm
    assert lib.loftr_stem_conv_bn_relu(_p(img), xs, 1, 0, 8, _p(w), ws, 128, None, None, None, None, 0.0, _p(sy), _stream()) == BAD_ARG
    # upsample2x_add
    assert lib.loftr_upsample2x_add(None, _p(x), _p(y), 1, 2, 2, 32, _stream()) == BAD_ARG and lib.loftr_upsample2x_add(_p(low), _p(x), None, 1, 2, 2, 32, _stream()) == BAD_ARG
    assert lib.loftr_upsample2x_add(_p(low), _p(x), _p(y), 1, 0, 2, 32, _stream()) == BAD_ARG and lib.loftr_upsample2x_add(_p(low), _p(x), _p(y), 1, 2, 2, 0, _stream()) == BAD_ARG
    assert lib.loftr_upsample2x_add(_p(low), _p(x), _p(y), 1, 16384, 32768, 32, _stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    for buf in (ybuf, fbuf, sbuf):                                               # nothing was launched on them
        assert bool((buf == E.GUARD_WORD).all())
    _report(f"args  {'argument checks':34s} {'all':8s} 28 refused calls returned their status, output buffers untouched")
    # the Python wrapper refuses a low map that is not half of the input
    with pytest.raises(_lib.LoftrHipError):
        ops.conv1x1_upsample_add(torch.zeros(1, 6, 4, 32, dtype=torch.int32, device=DEV), 32, conv, low)


def test_debug_switches_are_back_at_their_defaults():
    """Last in the module: every switch the cases set through ops.debug_switch is restored."""
    from loftr_amd import ops
    assert ops.debug_get("conv_patch") == (1, 1) and ops.debug_get("conv_duo") == (1, 1) and ops.debug_get("conv_rem") == (1, 1)
    assert ops.debug_get("conv_persist_cap") == (0, 0) and ops.CONV_REM is False
