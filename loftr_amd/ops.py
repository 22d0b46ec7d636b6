"""Tensor-level wrappers over the C-ABI (one function per entry point of include/loftr_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; all arithmetic of the matching
path happens in the HIP kernels.  Every wrapper requires CUDA(ROCm) float32 contiguous tensors
and raises otherwise -- there is no CPU fallback.
"""
import ctypes as C
import os
import weakref
import functools

import torch

from . import _lib
from ._lib import CoarseParams, FMap, LayerWeights, MatchOut, check

_WS = {}          # device index -> cached workspace tensor (grown on demand, never shrunk)

LAYER_FIELDS = (("q_proj", "q_proj.weight"), ("k_proj", "k_proj.weight"), ("v_proj", "v_proj.weight"),
                ("merge", "merge.weight"), ("mlp0", "mlp.0.weight"), ("mlp2", "mlp.2.weight"),
                ("norm1_w", "norm1.weight"), ("norm1_b", "norm1.bias"),
                ("norm2_w", "norm2.weight"), ("norm2_b", "norm2.bias"))


# Prepared (re-encoded) weights per module, keyed weakly by the module: kept OUT of the modules' __dict__ so that
# pickle / torch.save(model) / spawn-based launchers keep working after a forward (weak references do not pickle).
_PREPARED = weakref.WeakKeyDictionary()


def _tensors_in(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            yield from _tensors_in(o)
    elif isinstance(obj, dict):                   # the batch dict of training.spvs_* / LoFTRLoss: its tensors decide the device
        for o in obj.values():
            yield from _tensors_in(o)
    elif isinstance(obj, torch.nn.Module):
        for prm in obj.parameters():
            yield prm
            break


def _on_device(fn):
    """Run a wrapper with the GPU of its tensor arguments current: the C entry points launch on the stream handle they
    are given and never call hipSetDevice, so stream, workspace and pointers must all belong to ONE device -- the
    tensors' device, not whatever device happens to be current (a model on cuda:1 without torch.cuda.set_device).
    Tensors on different devices are rejected."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        dev = None
        for t in _tensors_in(list(args) + list(kwargs.values())):
            if t.is_cuda:
                if dev is None:
                    dev = t.device
                elif t.device != dev:
                    raise _lib.LoftrHipError(f"{fn.__name__}: tensors on different devices ({dev} and {t.device})")
        if dev is None:
            return fn(*args, **kwargs)            # no GPU tensor: the body raises its own 'expected a GPU tensor'
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapped


def _need(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.LoftrHipError(f"{name}: expected a GPU tensor (the HIP matching path has no CPU fallback)")
    if t.dtype != dtype:
        raise _lib.LoftrHipError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.LoftrHipError(f"{name}: expected a contiguous tensor")
    return t


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def debug_set(key, value):
    """loftr_hip_debug_set: a named A/B switch of the library (include/loftr_hip.h; process-global, the library reads no environment variable)."""
    check(_lib.load().loftr_hip_debug_set(key.encode(), int(value)), f"loftr_hip_debug_set({key})")


def debug_get(key):
    """(value, default) of a debug switch."""
    v, d = C.c_int(0), C.c_int(0)
    check(_lib.load().loftr_hip_debug_get(key.encode(), C.byref(v), C.byref(d)), f"loftr_hip_debug_get({key})")
    return v.value, d.value


class debug_switch:
    """``with ops.debug_switch(conv_duo=0, conv_persist_cap=8): ...`` -- switches set for the block, restored afterwards."""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = debug_get(k)[0]
            debug_set(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            debug_set(k, v)
        return False


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(nbytes, device):
    """Cached scratch buffer of at least nbytes on `device`, one per (device, that device's current stream): calls
    on one stream may share it (stream ordered), concurrent streams must not."""
    idx = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    buf = _WS.get(idx)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _WS[idx] = buf
    return buf


def _mask_u8(m, name):
    if m is None:
        return None
    if m.dtype == torch.bool:
        m = m.to(torch.uint8)
    return _need(m.contiguous(), name, torch.uint8)


# ---------------------------------------------------------------------------------------------
@_on_device
def linear(a, w):
    """a [M,K] @ w[N,K]^T on the split-fp16 GEMM core (building block, exposed for tests)."""
    _need(a, "a"); _need(w, "w")
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    lib = _lib.load()
    ws = workspace(lib.loftr_linear_workspace_bytes(M, N, K), a.device)
    check(lib.loftr_linear_fwd(_ptr(a), _ptr(w), _ptr(out), M, N, K, _ptr(ws), ws.numel(), _stream()), "loftr_linear_fwd")
    return out


@_on_device
def pos_encode_flatten(feat, pe):
    """feat [N,C,H,W] (any strides, e.g. channels-last) + pe[:, :H, :W], flattened to [N, H*W, C]."""
    if not feat.is_cuda or feat.dtype != torch.float32:
        raise _lib.LoftrHipError("feat: expected a float32 GPU tensor (the HIP matching path has no CPU fallback)")
    _need(pe, "pe")
    N, Cc, H, W = feat.shape
    out = torch.empty(N, H * W, Cc, device=feat.device, dtype=torch.float32)
    fm = _fmap(feat)
    check(_lib.load().loftr_pos_encode_flatten(C.byref(fm), _ptr(pe), pe.shape[-2], pe.shape[-1], _ptr(out),
                                               N, Cc, _stream()), "loftr_pos_encode_flatten")
    return out


def layer_weights_struct(tensors):
    """dict(field -> tensor) -> LayerWeights (keeps nothing alive: caller holds the tensors)."""
    lw = LayerWeights()
    for field, _ in LAYER_FIELDS:
        setattr(lw, field, tensors[field].data_ptr())
    return lw


@_on_device
def encoder_layer(x, source, w_struct, nhead, x_mask=None, source_mask=None, out=None):
    """One LoFTREncoderLayer.  x [nb,L,C], source [nb,S,C] -> [nb,L,C]."""
    _need(x, "x"); _need(source, "source")
    nb, L, Cc = x.shape
    S = source.shape[1]
    xm, sm = _mask_u8(x_mask, "x_mask"), _mask_u8(source_mask, "source_mask")
    if x_mask is not None and x_mask is source_mask:
        sm = xm
    out = torch.empty_like(x) if out is None else out
    lib = _lib.load()
    nbytes = lib.loftr_encoder_workspace_bytes(nb, L, S, Cc)
    ws = workspace(nbytes, x.device)
    check(lib.loftr_encoder_layer_fwd(_ptr(x), _ptr(source), _ptr(xm), _ptr(sm), C.byref(w_struct), _ptr(out),
                                      nb, L, S, Cc, nhead, _ptr(ws), ws.numel(), _stream()),
          "loftr_encoder_layer_fwd")
    return out


GRAD_FIELD_SHAPES = lambda Cc: {"q_proj": (Cc, Cc), "k_proj": (Cc, Cc), "v_proj": (Cc, Cc), "merge": (Cc, Cc), "mlp0": (2 * Cc, 2 * Cc),
                                "mlp2": (Cc, 2 * Cc), "norm1_w": (Cc,), "norm1_b": (Cc,), "norm2_w": (Cc,), "norm2_b": (Cc,)}


@_on_device
def encoder_layer_bwd(x, source, weights, grad_out, nhead, x_mask=None, source_mask=None):
    """Backward of one LoFTREncoderLayer (transformer.py:35-58 under autograd): weights = dict(field -> tensor) as for
    layer_weights_struct.  Returns (grad_x [nb,L,C], grad_source [nb,S,C], dict(field -> weight gradient))."""
    _need(x, "x"); _need(source, "source"); _need(grad_out, "grad_out")
    nb, L, Cc = x.shape
    S = source.shape[1]
    assert tuple(grad_out.shape) == (nb, L, Cc)
    xm, sm = _mask_u8(x_mask, "x_mask"), _mask_u8(source_mask, "source_mask")
    dev = x.device
    gx, gs = torch.empty_like(x), torch.empty_like(source)
    grads = {k: torch.empty(shp, device=dev, dtype=torch.float32) for k, shp in GRAD_FIELD_SHAPES(Cc).items()}
    lib = _lib.load()
    ws = workspace(lib.loftr_encoder_layer_bwd_workspace_bytes(nb, L, S, Cc, nhead), dev)
    wst, gst = layer_weights_struct(weights), layer_weights_struct(grads)
    check(lib.loftr_encoder_layer_bwd(_ptr(x), _ptr(source), _ptr(xm), _ptr(sm), C.byref(wst), _ptr(grad_out), _ptr(gx), _ptr(gs),
                                      C.byref(gst), nb, L, S, Cc, nhead, _ptr(ws), ws.numel(), _stream()), "loftr_encoder_layer_bwd")
    return gx, gs, grads


def stacked_halves(a, b):
    """The tensor [a; b] WITHOUT a copy when a and b already are the two batch halves of one buffer
    (e.g. ``x.split(n)`` of a stacked pair batch, or the outputs of pos_encode_flatten / fine_preprocess);
    None otherwise."""
    if (a.shape[1:] != b.shape[1:] or a.stride() != b.stride() or a.dtype != b.dtype or a.device != b.device
            or a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr()
            or b.storage_offset() != a.storage_offset() + a.shape[0] * a.stride(0)):
        return None
    return torch.as_strided(a, (a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), a.stride(), a.storage_offset())


@_on_device
def transformer_prepare(layer_structs, Cc, device):
    """All layer matrices re-encoded once into the library's GEMM operand format (loftr_transformer_prepare)."""
    n_layers = len(layer_structs)
    lib = _lib.load()
    buf = torch.empty(lib.loftr_transformer_prepared_bytes(n_layers, Cc), dtype=torch.uint8, device=device)
    arr = (LayerWeights * n_layers)(*layer_structs)
    with torch.cuda.device(device):
        check(lib.loftr_transformer_prepare(arr, n_layers, Cc, _ptr(buf), buf.numel(), _stream()), "loftr_transformer_prepare")
    return buf


# The coarse transformer's work queue for a shape (loftr_coarse_plan_build), per device: (device, kinds, N, L, S, order) -> uint8 tensor
_COARSE_PLANS = {}
# "persistent": one dependency-driven launch per coarse transformer call;  "persistent_call_order": the same kernel on the
# reference's call order (bit-identical results; A/B and tests);  "launches": the per-call launches of loftr_transformer_fwd;
# "auto" (default): persistent from 8 pairs on.  The dependencies are per pair, so with few pairs the 256 resident workgroups wait on each
# other -- and a resident workgroup holds its CU, which the FPN fine branch on the side stream then cannot use.  Alone the persistent form wins
# from 2 pairs on (8 pairs 3.19 vs 3.56 ms, 2 pairs of 840 x 840 2.36 vs 2.42 ms, a single 640 x 480 pair 2.06 vs 1.51 ms: tools/micro/pct_check.py,
# profiles/r06_pct_check.txt); INSIDE the forward it loses below 8 pairs (640 x 480: 1 pair 5.1-6.0 vs 4.5 ms, 2 pairs 7.5 vs 6.6, 4 pairs 11.6 vs
# 10.9, 8 pairs 20.0 vs 20.1-20.2, 16 pairs 39.3 vs 39.3; 840 x 840: 1 / 2 / 4 pairs 8.2 / 13.2 / 24.3 vs 7.3 / 12.6 / 23.9 ms;
# profiles/r06_mode_sweep.txt)
COARSE_MODE = os.environ.get("LOFTR_COARSE_MODE", "auto")
COARSE_AUTO_MIN_PAIRS = 8
COARSE_MODES = ("auto", "persistent", "persistent_call_order", "launches")

# The persistent transformer's status word (include/loftr_hip.h, loftr_transformer_fwd_planned: diag) when the caller passes no diag of
# its own: per (device, stream) a 16-byte device buffer, zeroed before the launch and copied into pinned host memory after it, both on
# the stream (no host sync).  _STATUS_PENDING holds the copy of the last such call per stream until check_transformer_status reads it.
_STATUS_BUFS = {}
_STATUS_PENDING = {}


def _status_word(device):
    """(key, (device buffer, pinned host buffer, event)) of the current stream of `device`."""
    st = torch.cuda.current_stream(device)
    key = (str(device), st.cuda_stream)
    bufs = _STATUS_BUFS.get(key)
    if bufs is None:
        bufs = _STATUS_BUFS[key] = (torch.empty(16, dtype=torch.uint8, device=device), torch.zeros(16, dtype=torch.uint8).pin_memory(),
                                    torch.cuda.Event())
    return key, bufs


def check_transformer_status(device):
    """Raise LoftrHipError when the last persistent coarse transformer call on the current stream of `device` that had no diag of
    its caller's reported a failure (2: the plan was built for another shape, nothing was computed; odd v: a workgroup gave up
    waiting for a dependency at work item (v - 1) / 2).  Meant to follow a host sync the caller makes anyway (the match count): the
    copy is complete then and waiting on its event costs nothing."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    pending = _STATUS_PENDING.pop(key, None)
    if pending is None:
        return
    host, done = pending
    done.synchronize()
    v = int(host.view(torch.int32)[0])
    if v == 0:
        return
    if v == 2:
        why = "its plan was built for another shape or order; nothing was computed"
    elif v % 2 == 1:
        why = f"a workgroup gave up waiting for a dependency at work item {(v - 1) // 2}"
    else:
        why = f"unknown status {v}"
    raise _lib.LoftrHipError(f"persistent coarse transformer (loftr_transformer_fwd_planned) failed: {why}")


def coarse_plan(kinds, N, L, S, device, order=0):
    """The persistent coarse transformer's plan for this shape, built once (None: the shape has no persistent form)."""
    key = (str(device), tuple(kinds), N, L, S, order)
    if key not in _COARSE_PLANS:
        lib = _lib.load()
        arr = (C.c_int * len(kinds))(*kinds)
        nbytes = lib.loftr_coarse_plan_bytes(arr, len(kinds), N, L, S)
        plan = None
        if nbytes:
            plan = torch.empty(nbytes, dtype=torch.uint8, device=device)
            with torch.cuda.device(device):
                check(lib.loftr_coarse_plan_build(arr, len(kinds), N, L, S, order, _ptr(plan), plan.numel(), _stream()), "loftr_coarse_plan_build")
        _COARSE_PLANS[key] = plan
    return _COARSE_PLANS[key]


@_on_device
def transformer(feat0, feat1, layer_structs, layer_names, nhead, mask0=None, mask1=None, inplace=False, prepared=None, mode=None,
                diag=None, skip_padded=False):
    """LocalFeatureTransformer.forward.  Returns new (feat0, feat1); inputs are not modified unless
    ``inplace`` (then, when feat0 / feat1 are the contiguous halves of one buffer, the layers run on
    that buffer directly instead of on a torch.cat copy of it).  ``mode``: see COARSE_MODE; ``diag``: uint8 tensor for
    loftr_transformer_fwd_planned's status word / per-item trace.  ``skip_padded`` (with masks): the caller does not read the
    features of padding tokens -- 128-token tiles without a valid token keep their input values (loftr_transformer_fwd_padded;
    per-call launches whatever ``mode`` says: the persistent form computes every tile)."""
    mode = mode or COARSE_MODE
    if mode not in COARSE_MODES:             # (a typo must not select a path: "launches" was the only value tested before)
        raise ValueError(f"coarse transformer mode {mode!r} (mode= or LOFTR_COARSE_MODE): expected one of {', '.join(COARSE_MODES)}")
    _need(feat0, "feat0"); _need(feat1, "feat1")
    N, L, Cc = feat0.shape
    S = feat1.shape[1]
    m0, m1 = _mask_u8(mask0, "mask0"), _mask_u8(mask1, "mask1")
    if L == S:          # stack -> the two self-attention calls of a layer run as one batch of 2N
        both = stacked_halves(feat0, feat1) if inplace and feat0.shape[0] == feat1.shape[0] else None
        if both is None:
            both = torch.cat([feat0, feat1], 0)
        f0, f1 = both[:N], both[N:]
        if m0 is not None:
            mb = torch.cat([m0, m1], 0)
            m0, m1 = mb[:N], mb[N:]
    else:
        f0, f1 = feat0.clone(), feat1.clone()
    n_layers = len(layer_names)
    arr = (LayerWeights * n_layers)(*layer_structs)
    kind_list = [{"self": 0, "cross": 1}[n] for n in layer_names]    # KeyError like the reference
    kinds = (C.c_int * n_layers)(*kind_list)
    lib = _lib.load()
    nbytes = lib.loftr_encoder_workspace_bytes(2 * N, L, S, Cc)
    ws = workspace(nbytes, feat0.device)
    skip_padded = bool(skip_padded) and m0 is not None
    if skip_padded:
        mode = "launches"
    if mode == "auto":
        mode = "persistent" if N >= COARSE_AUTO_MIN_PAIRS else "launches"
    plan = None
    if mode != "launches" and Cc == 256 and nhead == 8 and N > 0:
        order = 1 if mode == "persistent_call_order" else 0
        plan = coarse_plan(kind_list, N, L, S, feat0.device, order)
    if plan is not None:
        own = diag is None                   # no diag of the caller's: the status word goes to check_transformer_status
        if own:
            key, (diag, host, done) = _status_word(feat0.device)
            diag.zero_()
        check(lib.loftr_transformer_fwd_planned(_ptr(f0), _ptr(f1), _ptr(m0), _ptr(m1), arr, kinds, n_layers, N, L, S, Cc, nhead,
                                                _ptr(prepared), prepared.numel() if prepared is not None else 0,
                                                _ptr(ws), ws.numel(), _ptr(plan), plan.numel(), order,
                                                _ptr(diag), diag.numel(), _stream()),
              "loftr_transformer_fwd_planned")
        if own:
            host.copy_(diag, non_blocking=True)
            done.record()
            _STATUS_PENDING[key] = (host, done)
    elif skip_padded:
        check(lib.loftr_transformer_fwd_padded(_ptr(f0), _ptr(f1), _ptr(m0), _ptr(m1), arr, kinds, n_layers, N, L, S, Cc, nhead,
                                               _ptr(prepared), prepared.numel() if prepared is not None else 0,
                                               _ptr(ws), ws.numel(), 1, _stream()), "loftr_transformer_fwd_padded")
    else:
        check(lib.loftr_transformer_fwd(_ptr(f0), _ptr(f1), _ptr(m0), _ptr(m1), arr, kinds, n_layers, N, L, S, Cc, nhead,
                                        _ptr(prepared), prepared.numel() if prepared is not None else 0,
                                        _ptr(ws), ws.numel(), _stream()), "loftr_transformer_fwd")
    return f0, f1


@_on_device
def coarse_match(feat_c0, feat_c1, hw0_c, hw1_c, thr, border_rm, scale, match_type="dual_softmax",
                 temperature=0.1, bin_score=None, skh_iters=3, skh_prefilter=False, mask0=None, mask1=None,
                 scale0=None, scale1=None, want_conf=True, want_assign=False):
    """CoarseMatching.forward (eval).  Returns dict(conf_matrix, [conf_matrix_with_bin], b_ids, i_ids,
    j_ids, mconf, mkpts0_c, mkpts1_c, counts).  One host sync (the match count), like torch.where
    in the reference (coarse_matching.py:194)."""
    _need(feat_c0, "feat_c0"); _need(feat_c1, "feat_c1")
    N, L, Cc = feat_c0.shape
    S = feat_c1.shape[1]
    dev = feat_c0.device
    assert L == hw0_c[0] * hw0_c[1] and S == hw1_c[0] * hw1_c[1]
    m0, m1 = _mask_u8(mask0, "mask0"), _mask_u8(mask1, "mask1")
    s0 = None if scale0 is None else _need(scale0.to(torch.float32).contiguous(), "scale0")
    s1 = None if scale1 is None else _need(scale1.to(torch.float32).contiguous(), "scale1")
    cap = max(N * L, 1)
    b_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    i_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    j_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    mconf = torch.empty(cap, dtype=torch.float32, device=dev)
    mk0 = torch.empty(cap, 2, dtype=torch.float32, device=dev)
    mk1 = torch.empty(cap, 2, dtype=torch.float32, device=dev)
    counts = torch.zeros(1 + N, dtype=torch.int32, device=dev)
    p = CoarseParams(N, hw0_c[0], hw0_c[1], hw1_c[0], hw1_c[1], Cc, float(thr), int(border_rm), float(scale),
                     m0.data_ptr() if m0 is not None else None, m1.data_ptr() if m1 is not None else None,
                     s0.data_ptr() if s0 is not None else None, s1.data_ptr() if s1 is not None else None)
    mo = MatchOut(b_ids.data_ptr(), i_ids.data_ptr(), j_ids.data_ptr(), mconf.data_ptr(), mk0.data_ptr(),
                  mk1.data_ptr(), counts.data_ptr())
    lib = _lib.load()
    ws = workspace(lib.loftr_coarse_match_workspace_bytes(N, L, S, Cc), dev)
    out = {}
    if match_type == "dual_softmax":
        conf = torch.empty(N, L, S, device=dev, dtype=torch.float32) if want_conf else None
        check(lib.loftr_coarse_match_dual_softmax(_ptr(feat_c0), _ptr(feat_c1), C.byref(p), float(temperature),
                                                  _ptr(conf), C.byref(mo), _ptr(ws), ws.numel(), _stream()),
              "loftr_coarse_match_dual_softmax")
    elif match_type == "sinkhorn":
        conf = torch.empty(N, L, S, device=dev, dtype=torch.float32)
        assign = torch.empty(N, L + 1, S + 1, device=dev, dtype=torch.float32) if want_assign else None
        check(lib.loftr_coarse_match_sinkhorn(_ptr(feat_c0), _ptr(feat_c1), C.byref(p), float(bin_score),
                                              int(skh_iters), int(bool(skh_prefilter)), _ptr(conf), _ptr(assign),
                                              C.byref(mo), _ptr(ws), ws.numel(), _stream()),
              "loftr_coarse_match_sinkhorn")
        if want_assign:
            out["conf_matrix_with_bin"] = assign
    else:
        raise NotImplementedError(match_type)
    M = int(counts[0].item()) if N > 0 else 0            # the one D2H sync of the path
    out.update(conf_matrix=conf, b_ids=b_ids[:M], i_ids=i_ids[:M], j_ids=j_ids[:M], mconf=mconf[:M],
               mkpts0_c=mk0[:M], mkpts1_c=mk1[:M], counts=counts)
    return out


def _fmap(t):
    """[N,C,H,W] tensor with arbitrary (e.g. channels-last) strides -> FMap."""
    sn, sc, sh, sw = t.stride()
    return FMap(t.data_ptr(), sn, sc, sh, sw, t.shape[2], t.shape[3])


def _id_ptrs(b_ids, i_ids, j_ids):
    return [_ptr(_need(t, n, torch.int64)) for t, n in ((b_ids, "b_ids"), (i_ids, "i_ids"), (j_ids, "j_ids"))]


def _fine_preprocess_call(entry, source, dev, Cf, feat_c0, feat_c1, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride, lin, extra=()):
    """What the four forms of fine_preprocess share: the [2 M, W*W, Cf] result, the empty return, the workspace and the arguments
    from the coarse features to the stream.  `source`: the entry point's leading arguments (where the windows come from), `extra`:
    those between the workspace and the stream; `lin`: (down_w, down_b, merge_w, merge_b).  The callers have checked feat_c0 / feat_c1."""
    M = b_ids.shape[0]
    out = torch.empty(2 * M, W * W, Cf, device=dev, dtype=torch.float32)     # one buffer: the fine transformer
    out0, out1 = out[:M], out[M:]                                            # runs on it in place (no torch.cat)
    if M == 0:
        return out0, out1
    lib = _lib.load()
    ws = workspace(lib.loftr_fine_preprocess_workspace_bytes(M, W, Cf), dev)
    check(getattr(lib, entry)(*source, _ptr(feat_c0), _ptr(feat_c1), feat_c0.shape[1], feat_c1.shape[1], feat_c0.shape[2],
                              *_id_ptrs(b_ids, i_ids, j_ids), M, hw0_c[1], hw1_c[1], int(stride), int(W), Cf, *map(_ptr, lin),
                              _ptr(out0), _ptr(out1), _ptr(ws), ws.numel(), *extra, _stream()), entry)
    return out0, out1


@_on_device
def fine_preprocess(feat_f0, feat_f1, feat_c0, feat_c1, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride,
                    down_w=None, down_b=None, merge_w=None, merge_b=None):
    """FinePreprocess.forward for M > 0.  Returns (feat_f0_unfold, feat_f1_unfold) [M, W*W, Cf]."""
    for t, n in ((feat_f0, "feat_f0"), (feat_f1, "feat_f1")):
        if not t.is_cuda or t.dtype != torch.float32:
            raise _lib.LoftrHipError(f"{n}: expected a float32 GPU tensor")
    _need(feat_c0, "feat_c0"); _need(feat_c1, "feat_c1")
    f0, f1 = _fmap(feat_f0), _fmap(feat_f1)
    return _fine_preprocess_call("loftr_fine_preprocess", (C.byref(f0), C.byref(f1)), feat_f0.device, feat_f0.shape[1], feat_c0, feat_c1,
                                 b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride, (down_w, down_b, merge_w, merge_b))


# ---- the fine head at matched windows only (csrc/window_head.hip) -------------------------------------------------------
# The window form computes 2 M windows x 49 first-layer-equivalent pixels where the dense head computes every pixel of both fine
# maps; it is taken while 2 M * 49 <= WINDOW_HEAD_MAX_FILL * (dense pixels).  The factor is where the op-level timing table
# profiles/window_head_crossover.txt says the window form stops winning (tools/micro/window_head_crossover.py: ahead by 271 us at
# 1.46, behind by 90 us at 1.95 -- level at about 1.8).
WINDOW_HEAD_MAX_FILL = 1.8


def window_head_wins(M, dense_pixels):
    """The dispatch rule of LoFTR.fine_head = None: True while the window form of the fine head is the cheaper one for M matches on
    fine maps of `dense_pixels` pixels in all (both image batches)."""
    return 0 < 2 * M * 49 <= WINDOW_HEAD_MAX_FILL * dense_pixels


def window_head_supported(W, Cin, Cout, h_sp0, h_sp1):
    """What loftr_fine_preprocess_window_head covers: 5 x 5 windows, 128 output channels (its window rows are Cf dwords wide), two
    equally sized SP batches."""
    return (W == 5 and Cout == 128 and h_sp0.shape == h_sp1.shape and h_sp0.shape[3] == ceil32(Cin)
            and h_sp0.numel() < 2 ** 31)


def _window_conv_inputs(maps, Cin, conv, bn, b_ids, i_ids, j_ids):
    """The input check of every window kernel: `maps` = ((SP map of image0, its name), (of image1, its name)), or () where the input
    is no pair of maps; `conv` (with `bn` folded in) 3x3 / stride 1 / pad 1 on Cin channels; the three id vectors.
    Returns (Cout, the prepared filter, the ids' pointers)."""
    for t, n in maps:
        if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 4:
            raise _lib.LoftrHipError(f"{n}: expected a contiguous int32 (SP) GPU tensor [N, H, W, Cp]")
    if maps and (maps[0][0].shape != maps[1][0].shape or maps[0][0].shape[3] != ceil32(Cin)):
        raise _lib.LoftrHipError(f"window head: SP maps {tuple(maps[0][0].shape)} / {tuple(maps[1][0].shape)} for {Cin} channels")
    Cout, Cin_w, KH, KW = conv.weight.shape
    if (Cin_w, KH, KW) != (Cin, 3, 3) or conv.stride[0] != 1 or conv.padding[0] != 1:
        raise _lib.LoftrHipError("window head: a 3x3 / stride-1 / pad-1 convolution expected")
    return Cout, _prepared_conv(conv, bn), _id_ptrs(b_ids, i_ids, j_ids)


@_on_device
def window_head(h_sp0, h_sp1, Cin, conv, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride):
    """The W x W windows of conv(h) at the matched cells, without the map: (win0, win1) int32 SP [M, W*W, 128] -- bit for bit the
    window tiles loftr_fine_preprocess gathers from the dense convolution's fp32 output."""
    Cout, prepared, ids = _window_conv_inputs(((h_sp0, "h_sp0"), (h_sp1, "h_sp1")), Cin, conv, None, b_ids, i_ids, j_ids)
    M = b_ids.shape[0]
    win = torch.empty(2, M, W * W, ceil32(Cout), dtype=torch.int32, device=h_sp0.device)
    if M:
        N, H, Wm, _ = h_sp0.shape
        check(_lib.load().loftr_window_head(_ptr(h_sp0), _ptr(h_sp1), N, H, Wm, Cin, _ptr(prepared), prepared.numel(), Cout, *ids,
                                            M, hw0_c[1], hw1_c[1], int(stride), int(W), _ptr(win[0]), _ptr(win[1]),
                                            _stream()), "loftr_window_head")
    return win[0], win[1]


@_on_device
def fine_preprocess_windows(h_sp0, h_sp1, Cin, conv, feat_c0, feat_c1, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride,
                            down_w, down_b, merge_w, merge_b):
    """fine_preprocess with the fine head's last convolution `conv` evaluated at the matched windows only: h_sp0 / h_sp1 are that
    convolution's inputs (SP [N, H, W, ceil32(Cin)]) for the image0 / image1 batch.  Same results, bit for bit, as fine_preprocess on
    the dense maps conv_bn_act(h, Cin, conv) gives."""
    Cf, prepared, _ = _window_conv_inputs(((h_sp0, "h_sp0"), (h_sp1, "h_sp1")), Cin, conv, None, b_ids, i_ids, j_ids)
    _need(feat_c0, "feat_c0"); _need(feat_c1, "feat_c1")
    N, H, Wm, _ = h_sp0.shape
    return _fine_preprocess_call("loftr_fine_preprocess_window_head",
                                 (_ptr(h_sp0), _ptr(h_sp1), N, H, Wm, Cin, _ptr(prepared), prepared.numel()), h_sp0.device, Cf,
                                 feat_c0, feat_c1, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride, (down_w, down_b, merge_w, merge_b))


# ---- both convolutions of the fine head at matched windows only (csrc/window_head_first.hip) -----------------------------
# The head's FIRST convolution has one consumer left once the last one runs at the windows: the 7 x 7 neighbourhood of each window,
# 2 M * 49 pixels.  It is evaluated there (into a scratch tensor the last convolution's window kernel stages its patches from) while
# 2 M * 49 <= WINDOW_HEAD_FIRST_MAX_FILL * (dense pixels) AND the last convolution takes its window form (window_head_wins).  The
# factor is where profiles/window_head_first_crossover.txt (tools/micro/window_head_first_crossover.py, op level, the bench's maps)
# says the pair of window kernels stops winning against the dense first convolution + window_head (ahead by 406 us at fill 0.73,
# behind by 357 us at 0.98 -- level at about 0.85).
WINDOW_HEAD_FIRST_MAX_FILL = 0.85


def window_head_first_wins(M, dense_pixels):
    """The dispatch rule of LoFTR.fine_head = None for the head's FIRST convolution: True while evaluating it at the 7 x 7
    neighbourhoods of the M matches' windows is cheaper than on the `dense_pixels` pixels of both image batches' maps."""
    return window_head_wins(M, dense_pixels) and 2 * M * 49 <= WINDOW_HEAD_FIRST_MAX_FILL * dense_pixels


def window_head_first_supported(W, Cin, conv0, conv1, t_sp0, t_sp1, M):
    """What loftr_fine_preprocess_window_head2 covers: 5 x 5 windows, channels 196 -> 196 -> 128, two equally sized SP batches, a
    scratch tensor indexed with 32 bits."""
    return (window_head_supported(W, Cin, conv1.out_channels, t_sp0, t_sp1) and Cin == 196 and conv0.out_channels == 196
            and conv1.in_channels == 196 and 2 * M * 49 * 224 < 2 ** 31)


@_on_device
def window_head_first(t_sp0, t_sp1, Cin, conv, bn, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride):
    """act(bn(conv(t))) (LeakyReLU 0.01: the fine head's first layer) at the 7 x 7 neighbourhoods of the matched W x W windows, without
    the map: int32 SP [2 M, 49, ceil32(Cout)], window side * M + m, row py * 7 + px -- bit for bit the dense layer's SP rows
    conv_bn_act(t, Cin, conv, bn, act=2) at those pixels, zeros outside the map."""
    Cout, prepared, ids = _window_conv_inputs(((t_sp0, "t_sp0"), (t_sp1, "t_sp1")), Cin, conv, bn, b_ids, i_ids, j_ids)
    M = b_ids.shape[0]
    nb = torch.empty(2 * M, 49, ceil32(Cout), dtype=torch.int32, device=t_sp0.device)
    if M:
        N, H, Wm, _ = t_sp0.shape
        check(_lib.load().loftr_window_head_first(_ptr(t_sp0), _ptr(t_sp1), N, H, Wm, Cin, _ptr(prepared), prepared.numel(), Cout, *ids,
                                                  M, hw0_c[1], hw1_c[1], int(stride), int(W), _ptr(nb), _stream()),
              "loftr_window_head_first")
    return nb


@_on_device
def window_head_last(nb, hw_f, Cin, conv, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride):
    """window_head from window_head_first's neighbourhood rows `nb` instead of the dense map (hw_f: the map's height and width)."""
    M = b_ids.shape[0]
    if not nb.is_cuda or nb.dtype != torch.int32 or not nb.is_contiguous() or tuple(nb.shape) != (2 * M, 49, ceil32(Cin)):
        raise _lib.LoftrHipError(f"nb: expected a contiguous int32 (SP) GPU tensor [{2 * M}, 49, {ceil32(Cin)}]")
    Cout, prepared, ids = _window_conv_inputs((), Cin, conv, None, b_ids, i_ids, j_ids)
    win = torch.empty(2, M, W * W, ceil32(Cout), dtype=torch.int32, device=nb.device)
    if M:
        check(_lib.load().loftr_window_head_last(_ptr(nb), int(hw_f[0]), int(hw_f[1]), Cin, _ptr(prepared), prepared.numel(), Cout, *ids,
                                                 M, hw0_c[1], hw1_c[1], int(stride), int(W), _ptr(win[0]), _ptr(win[1]), _stream()),
              "loftr_window_head_last")
    return win[0], win[1]


@_on_device
def fine_preprocess_windows2(t_sp0, t_sp1, Cin, conv0, bn0, conv1, feat_c0, feat_c1, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride,
                             down_w, down_b, merge_w, merge_b):
    """fine_preprocess with BOTH convolutions of the fine head (conv0 + bn0 + LeakyReLU, conv1) evaluated at the matched windows only:
    t_sp0 / t_sp1 are the head's inputs (SP [N, H, W, ceil32(Cin)]) for the image0 / image1 batch.  Same results, bit for bit, as
    fine_preprocess_windows on conv_bn_act(t, Cin, conv0, bn0, act=2)."""
    Cmid, prepared0, _ = _window_conv_inputs(((t_sp0, "t_sp0"), (t_sp1, "t_sp1")), Cin, conv0, bn0, b_ids, i_ids, j_ids)
    Cf = conv1.weight.shape[0]
    if tuple(conv1.weight.shape[1:]) != (Cmid, 3, 3) or conv1.stride[0] != 1 or conv1.padding[0] != 1:
        raise _lib.LoftrHipError("window head: a 3x3 / stride-1 / pad-1 second convolution expected")
    prepared1 = _prepared_conv(conv1, None)
    _need(feat_c0, "feat_c0"); _need(feat_c1, "feat_c1")
    dev = t_sp0.device
    nb = torch.empty(2 * b_ids.shape[0], 49, ceil32(Cmid), dtype=torch.int32, device=dev)     # the first convolution's neighbourhood rows
    N, H, Wm, _ = t_sp0.shape
    return _fine_preprocess_call("loftr_fine_preprocess_window_head2",
                                 (_ptr(t_sp0), _ptr(t_sp1), N, H, Wm, Cin, _ptr(prepared0), prepared0.numel(), Cmid, _ptr(prepared1),
                                  prepared1.numel()), dev, Cf, feat_c0, feat_c1, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride,
                                 (down_w, down_b, merge_w, merge_b), extra=(_ptr(nb),))


def _slot_ids(ids, n_slots, name, device):
    """Slot ids -> int32 tensor on `device`, checked on the host against [0, n_slots) before any launch (the kernels would
    write NaN for an id outside it)."""
    host = ids.detach().cpu() if isinstance(ids, torch.Tensor) else torch.as_tensor(ids)
    if host.dim() != 1 or host.dtype.is_floating_point or host.dtype == torch.bool:
        raise _lib.LoftrHipError(f"{name}: expected a 1-D integer tensor of slot ids, got {tuple(host.shape)} {host.dtype}")
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= n_slots):
        raise _lib.LoftrHipError(f"{name}: slot id out of range [0, {n_slots}) (min {int(host.min())}, max {int(host.max())})")
    if isinstance(ids, torch.Tensor) and ids.is_cuda and ids.dtype == torch.int32 and ids.is_contiguous() and ids.device == device:
        return ids
    return host.to(torch.int32).to(device)


def _bank_map(bank, name):
    """A bank [n_slots, C, H, W] (any strides, e.g. the channels-last view of FeatureBank's [n_slots, H, W, C] storage)."""
    if not isinstance(bank, torch.Tensor) or not bank.is_cuda or bank.dtype != torch.float32 or bank.dim() != 4:
        raise _lib.LoftrHipError(f"{name}: expected a 4-D float32 GPU tensor [n_slots, C, H, W]")
    if bank.shape[0] == 0:
        raise _lib.LoftrHipError(f"{name}: empty bank")
    return bank


@_on_device
def pos_encode_flatten_gather(bank, slot_ids, pe, out=None):
    """pos_encode_flatten(bank[slot_ids]) without gathering the maps: bank [n_slots,C,H,W] (any strides), slot_ids [n] ->
    [n, H*W, C].  ``out``: a contiguous [n, H*W, C] float32 tensor to write into (e.g. one half of the coarse transformer's
    [2n, L, C] buffer)."""
    _bank_map(bank, "bank")
    _need(pe, "pe")
    n_slots, Cc, H, W = bank.shape
    ids = _slot_ids(slot_ids, n_slots, "slot_ids", bank.device)
    n = ids.shape[0]
    if out is None:
        out = torch.empty(n, H * W, Cc, device=bank.device, dtype=torch.float32)
    elif tuple(out.shape) != (n, H * W, Cc):
        raise _lib.LoftrHipError(f"out: expected shape {(n, H * W, Cc)}, got {tuple(out.shape)}")
    _need(out, "out")
    fm = _fmap(bank)
    check(_lib.load().loftr_pos_encode_flatten_gather(C.byref(fm), n_slots, _ptr(ids), n, _ptr(pe), pe.shape[-2], pe.shape[-1],
                                                      _ptr(out), Cc, _stream()), "loftr_pos_encode_flatten_gather")
    return out


@_on_device
def fine_preprocess_gather(bank_f0, slot0, bank_f1, slot1, feat_c0, feat_c1, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride,
                           down_w=None, down_b=None, merge_w=None, merge_b=None):
    """fine_preprocess with the fine maps of pair b read from bank_f0[slot0[b]] / bank_f1[slot1[b]] (banks [n_slots,Cf,h,w],
    any strides; slot0 / slot1 [N] for the N pairs of feat_c0 / feat_c1).  Returns (feat_f0_unfold, feat_f1_unfold) [M, W*W, Cf]."""
    _bank_map(bank_f0, "bank_f0"); _bank_map(bank_f1, "bank_f1")
    _need(feat_c0, "feat_c0"); _need(feat_c1, "feat_c1")
    N = feat_c0.shape[0]
    s0 = _slot_ids(slot0, bank_f0.shape[0], "slot0", bank_f0.device)
    s1 = _slot_ids(slot1, bank_f1.shape[0], "slot1", bank_f1.device)
    if s0.shape[0] != N or s1.shape[0] != N:
        raise _lib.LoftrHipError(f"slot0 / slot1: expected {N} slot ids (one per pair), got {s0.shape[0]} / {s1.shape[0]}")
    f0, f1 = _fmap(bank_f0), _fmap(bank_f1)
    return _fine_preprocess_call("loftr_fine_preprocess_gather",
                                 (C.byref(f0), bank_f0.shape[0], _ptr(s0), C.byref(f1), bank_f1.shape[0], _ptr(s1)), bank_f0.device,
                                 bank_f0.shape[1], feat_c0, feat_c1, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride,
                                 (down_w, down_b, merge_w, merge_b))


# ---- track refinement: the fine stage at points the caller names (csrc/refine_core.h, refine.hip, refine_gpu.hip) ----------
@_on_device
def refine_centres(pts0, pts1, b_ids, n_pairs, hw0_f, hw1_f, hw0_c, hw1_c, stride, s, scale0=None, scale1=None):
    """loftr_refine_centres: fine-window centres, coarse cells and snapped points of M point pairs (include/loftr_hip.h).  pts0, pts1
    [M,2] f32, b_ids [M] i64, scale0 / scale1 None or [n_pairs,2] f32, all on one device.  GPU tensors run the kernel (one launch, no
    synchronisation), CPU tensors the host routine that defines the result; both give the same bits.
    -> dict: c0, c1 [M,2] i32 (x, y), i_ids, j_ids [M] i64, pts0_s, pts1_s [M,2] f32, ok [M] u8."""
    dev = pts0.device if isinstance(pts0, torch.Tensor) else None
    for t, name, dtype, tail in ((pts0, "pts0", torch.float32, (2,)), (pts1, "pts1", torch.float32, (2,)), (b_ids, "b_ids", torch.int64, ()),
                                 (scale0, "scale0", torch.float32, (2,)), (scale1, "scale1", torch.float32, (2,))):
        if t is None and name.startswith("scale"):
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != dev or not t.is_contiguous() or tuple(t.shape[1:]) != tail:
            raise _lib.LoftrHipError(f"refine_centres: {name} must be a contiguous {dtype} tensor [*{', 2' if tail else ''}] on {dev}")
    M, n_pairs = pts0.shape[0], int(n_pairs)
    if pts1.shape[0] != M or b_ids.shape[0] != M or any(t is not None and t.shape[0] != n_pairs for t in (scale0, scale1)):
        raise _lib.LoftrHipError(f"refine_centres: expected pts0, pts1 [M,2], b_ids [M] and scales [{n_pairs},2], got "
                                 f"{[None if t is None else tuple(t.shape) for t in (pts0, pts1, b_ids, scale0, scale1)]}")
    out = {"c0": torch.zeros(M, 2, dtype=torch.int32, device=dev), "c1": torch.zeros(M, 2, dtype=torch.int32, device=dev),
           "i_ids": torch.zeros(M, dtype=torch.int64, device=dev), "j_ids": torch.zeros(M, dtype=torch.int64, device=dev),
           "pts0_s": torch.zeros(M, 2, dtype=torch.float32, device=dev), "pts1_s": torch.zeros(M, 2, dtype=torch.float32, device=dev),
           "ok": torch.zeros(M, dtype=torch.uint8, device=dev)}
    args = (_ptr(pts0), _ptr(pts1), _ptr(b_ids), M, _ptr(scale0), _ptr(scale1), n_pairs, int(hw0_f[0]), int(hw0_f[1]), int(hw1_f[0]),
            int(hw1_f[1]), int(hw0_c[0]), int(hw0_c[1]), int(hw1_c[0]), int(hw1_c[1]), int(stride), float(s), *[_ptr(t) for t in out.values()])
    if dev.type == "cuda":
        check(_lib.load().loftr_refine_centres(*args, _stream()), "loftr_refine_centres")
    else:
        check(_lib.load().loftr_refine_centres_host(*args), "loftr_refine_centres_host")
    return out


@_on_device
def fine_preprocess_gather_at(bank_f0, slot0, bank_f1, slot1, feat_c0, feat_c1, b_ids, i_ids, j_ids, c0, c1, hw0_c, hw1_c, W, stride,
                              down_w=None, down_b=None, merge_w=None, merge_b=None):
    """fine_preprocess_gather with the window of match m centred at c0[m] / c1[m] ([M,2] i32 (x, y) in fine pixels) instead of at
    stride * cell; i_ids / j_ids are still what the coarse gather reads.  Returns (feat_f0_unfold, feat_f1_unfold) [M, W*W, Cf]."""
    _bank_map(bank_f0, "bank_f0"); _bank_map(bank_f1, "bank_f1")
    _need(feat_c0, "feat_c0"); _need(feat_c1, "feat_c1")
    N, M = feat_c0.shape[0], b_ids.shape[0]
    s0 = _slot_ids(slot0, bank_f0.shape[0], "slot0", bank_f0.device)
    s1 = _slot_ids(slot1, bank_f1.shape[0], "slot1", bank_f1.device)
    if s0.shape[0] != N or s1.shape[0] != N:
        raise _lib.LoftrHipError(f"slot0 / slot1: expected {N} slot ids (one per pair), got {s0.shape[0]} / {s1.shape[0]}")
    for t, name in ((c0, "c0"), (c1, "c1")):
        if tuple(_need(t, name, torch.int32).shape) != (M, 2):
            raise _lib.LoftrHipError(f"{name}: expected [{M}, 2], got {tuple(t.shape)}")
    f0, f1 = _fmap(bank_f0), _fmap(bank_f1)
    return _fine_preprocess_call("loftr_fine_preprocess_gather_at",
                                 (C.byref(f0), bank_f0.shape[0], _ptr(s0), C.byref(f1), bank_f1.shape[0], _ptr(s1)), bank_f0.device,
                                 bank_f0.shape[1], feat_c0, feat_c1, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride,
                                 (down_w, down_b, merge_w, merge_b), extra=(_ptr(c0), _ptr(c1)))


@_on_device
def fine_preprocess_bwd(feat_f0, feat_f1, feat_c0, feat_c1, b_ids, i_ids, j_ids, hw0_c, hw1_c, W, stride, down_w, down_b, merge_w,
                        grad_out0, grad_out1):
    """Backward of fine_preprocess (fine_preprocess.py:29-59 under autograd).  Returns (grad_feat_f0, grad_feat_f1 [laid out like the
    inputs], grad_feat_c0, grad_feat_c1, grad_down_w, grad_down_b, grad_merge_w, grad_merge_b)."""
    _need(feat_c0, "feat_c0"); _need(feat_c1, "feat_c1"); _need(grad_out0, "grad_out0"); _need(grad_out1, "grad_out1")
    M = b_ids.shape[0]
    Cf, Cc = feat_f0.shape[1], feat_c0.shape[2]
    dev = feat_f0.device
    gf0, gf1 = torch.zeros_like(feat_f0), torch.zeros_like(feat_f1)             # (preserve_format: same strides as the inputs)
    gc0, gc1 = torch.zeros_like(feat_c0), torch.zeros_like(feat_c1)
    gdw, gdb = torch.zeros_like(down_w), torch.zeros_like(down_b)
    gmw, gmb = torch.zeros(Cf, 2 * Cf, device=dev), torch.zeros(Cf, device=dev)
    if M == 0:
        return gf0, gf1, gc0, gc1, gdw, gdb, gmw, gmb
    lib = _lib.load()
    ws = workspace(lib.loftr_fine_preprocess_bwd_workspace_bytes(M, int(W), Cf, Cc), dev)
    f0, f1, g0, g1 = _fmap(feat_f0), _fmap(feat_f1), _fmap(gf0), _fmap(gf1)
    check(lib.loftr_fine_preprocess_bwd(C.byref(f0), C.byref(f1), _ptr(feat_c0), _ptr(feat_c1), feat_c0.shape[1], feat_c1.shape[1], Cc,
                                        _ptr(_need(b_ids, "b_ids", torch.int64)), _ptr(_need(i_ids, "i_ids", torch.int64)),
                                        _ptr(_need(j_ids, "j_ids", torch.int64)), M, hw0_c[1], hw1_c[1], int(stride), int(W), Cf,
                                        _ptr(_need(down_w, "down_w")), _ptr(_need(down_b, "down_b")), _ptr(_need(merge_w, "merge_w")),
                                        _ptr(grad_out0), _ptr(grad_out1), C.byref(g0), C.byref(g1), _ptr(gc0), _ptr(gc1), _ptr(gdw), _ptr(gdb),
                                        _ptr(gmw), _ptr(gmb), _ptr(ws), ws.numel(), _stream()), "loftr_fine_preprocess_bwd")
    return gf0, gf1, gc0, gc1, gdw, gdb, gmw, gmb


@_on_device
def fine_match(feat_f0, feat_f1, mkpts1_c, b_ids, scale, scale1=None):
    """FineMatching for M > 0.  Returns (expec_f [M,3], mkpts1_f [M,2])."""
    _need(feat_f0, "feat_f0"); _need(feat_f1, "feat_f1")
    M, WW, Cf = feat_f0.shape
    dev = feat_f0.device
    expec = torch.empty(M, 3, device=dev, dtype=torch.float32)
    mk1f = torch.empty(M, 2, device=dev, dtype=torch.float32)
    s1 = None if scale1 is None else _need(scale1.to(torch.float32).contiguous(), "scale1")
    check(_lib.load().loftr_fine_match(_ptr(feat_f0), _ptr(feat_f1), M, WW, Cf,
                                       _ptr(_need(mkpts1_c.contiguous(), "mkpts1_c")),
                                       _ptr(_need(b_ids, "b_ids", torch.int64)), float(scale), _ptr(s1), _ptr(expec),
                                       _ptr(mk1f), _stream()), "loftr_fine_match")
    return expec, mk1f


# ---------------------------------------------------------------------------------------------
# Backward of the two matching heads (include/loftr_hip.h: "backward of the matching heads"); the autograd.Function
# wrappers that call these live in loftr_amd/autograd.py.
@_on_device
def dual_softmax_bwd(feat_c0, feat_c1, grad_conf, hw0_c, hw1_c, temperature, mask0=None, mask1=None):
    """dL/d sim_matrix [N,L,S] from dL/d conf_matrix (coarse_matching.py:110-119)."""
    _need(feat_c0, "feat_c0"); _need(feat_c1, "feat_c1"); _need(grad_conf, "grad_conf")
    N, L, Cc = feat_c0.shape
    S = feat_c1.shape[1]
    assert tuple(grad_conf.shape) == (N, L, S) and L == hw0_c[0] * hw0_c[1] and S == hw1_c[0] * hw1_c[1]
    m0, m1 = _mask_u8(mask0, "mask0"), _mask_u8(mask1, "mask1")
    p = CoarseParams(N, hw0_c[0], hw0_c[1], hw1_c[0], hw1_c[1], Cc, 0.0, 0, 1.0,
                     m0.data_ptr() if m0 is not None else None, m1.data_ptr() if m1 is not None else None, None, None)
    dsim = torch.empty(N, L, S, device=feat_c0.device, dtype=torch.float32)
    lib = _lib.load()
    ws = workspace(lib.loftr_coarse_match_workspace_bytes(N, L, S, Cc), feat_c0.device)
    check(lib.loftr_dual_softmax_bwd(_ptr(feat_c0), _ptr(feat_c1), C.byref(p), float(temperature), _ptr(grad_conf), _ptr(dsim),
                                     _ptr(ws), ws.numel(), _stream()), "loftr_dual_softmax_bwd")
    return dsim


@_on_device
def head_feat_grads(dsim, feat_c0, feat_c1, alpha, want0=True, want1=True):
    """(alpha * dsim @ feat_c1, alpha * dsim^T @ feat_c0): the einsum of coarse_matching.py:110-114 / :122-123 in reverse.
    dsim [N,L,S] fp32, possibly a strided view (last stride 1): the interior of the Sinkhorn head's [N,L+1,S+1] gradient."""
    _need(feat_c0, "feat_c0"); _need(feat_c1, "feat_c1")
    N, L, Cc = feat_c0.shape
    S = feat_c1.shape[1]
    if not (dsim.is_cuda and dsim.dtype == torch.float32 and tuple(dsim.shape) == (N, L, S) and dsim.stride(2) == 1):
        raise _lib.LoftrHipError("head_feat_grads: dsim must be a float32 GPU tensor [N,L,S] with unit last stride")
    g0 = torch.empty_like(feat_c0) if want0 else None
    g1 = torch.empty_like(feat_c1) if want1 else None
    if want0 or want1:
        check(_lib.load().loftr_head_feat_grads(_ptr(dsim), dsim.stride(1), dsim.stride(0), _ptr(feat_c0), _ptr(feat_c1), N, L, S, Cc,
                                                float(alpha), _ptr(g0), _ptr(g1), _stream()), "loftr_head_feat_grads")
    return g0, g1


@_on_device
def sinkhorn_bwd(feat_c0, feat_c1, grad_assign, hw0_c, hw1_c, bin_score, iters, mask0=None, mask1=None):
    """(dL/d couplings [N,L+1,S+1], dL/d bin_score [1]) from dL/d conf_matrix_with_bin (coarse_matching.py:121-143)."""
    _need(feat_c0, "feat_c0"); _need(feat_c1, "feat_c1"); _need(grad_assign, "grad_assign")
    N, L, Cc = feat_c0.shape
    S = feat_c1.shape[1]
    assert tuple(grad_assign.shape) == (N, L + 1, S + 1) and L == hw0_c[0] * hw0_c[1] and S == hw1_c[0] * hw1_c[1]
    m0, m1 = _mask_u8(mask0, "mask0"), _mask_u8(mask1, "mask1")
    p = CoarseParams(N, hw0_c[0], hw0_c[1], hw1_c[0], hw1_c[1], Cc, 0.0, 0, 1.0,
                     m0.data_ptr() if m0 is not None else None, m1.data_ptr() if m1 is not None else None, None, None)
    dev = feat_c0.device
    dz = torch.empty(N, L + 1, S + 1, device=dev, dtype=torch.float32)
    z = torch.empty(N, L, S, device=dev, dtype=torch.float32)
    dbin = torch.zeros(1, device=dev, dtype=torch.float32)
    lib = _lib.load()
    ws = workspace(lib.loftr_sinkhorn_bwd_workspace_bytes(N, L, S, Cc, int(iters)), dev)
    check(lib.loftr_sinkhorn_bwd(_ptr(feat_c0), _ptr(feat_c1), C.byref(p), float(bin_score), int(iters), _ptr(grad_assign), _ptr(z), _ptr(dz),
                                 _ptr(dbin), _ptr(ws), ws.numel(), _stream()), "loftr_sinkhorn_bwd")
    return dz, dbin


@_on_device
def fine_match_bwd(feat_f0, feat_f1, grad_expec):
    """(dL/d feat_f0, dL/d feat_f1) [M,WW,C] from dL/d expec_f [M,3] (fine_matching.py:43-57)."""
    _need(feat_f0, "feat_f0"); _need(feat_f1, "feat_f1"); _need(grad_expec, "grad_expec")
    M, WW, Cf = feat_f0.shape
    assert tuple(grad_expec.shape) == (M, 3)
    g0, g1 = torch.empty_like(feat_f0), torch.empty_like(feat_f1)
    check(_lib.load().loftr_fine_match_bwd(_ptr(feat_f0), _ptr(feat_f1), M, WW, Cf, _ptr(grad_expec), _ptr(g0), _ptr(g1), _stream()),
          "loftr_fine_match_bwd")
    return g0, g1


# ---------------------------------------------------------------------------------------------
# ResNet-FPN building blocks.  An SP activation is carried as (tensor int32 [B,H,W,Cp], C).
def ceil32(c):
    return (c + 31) // 32 * 32


@_on_device
def sp_from_nhwc(x_nhwc, scaled=False):
    """fp32 [B,H,W,C] contiguous -> SP int32 [B,H,W,ceil32(C)].
    scaled=True: the tensor is stored times the power of two that lifts its maximum to [2^13, 2^14) (csrc/gemm.h:
    full split-fp16 precision whatever the tensor's magnitude); returns (sp, inv_scale) with inv_scale a device float
    to hand to conv_bn_act(x_inv_scale=...)."""
    _need(x_nhwc, "x_nhwc")
    B, H, W, Cc = x_nhwc.shape
    out = torch.empty(B, H, W, ceil32(Cc), dtype=torch.int32, device=x_nhwc.device)
    if scaled:
        inv = torch.empty(1, dtype=torch.float32, device=x_nhwc.device)
        check(_lib.load().loftr_sp_from_f32_scaled(_ptr(x_nhwc), _ptr(out), B * H * W, Cc, _ptr(inv), _stream()),
              "loftr_sp_from_f32_scaled")
        return out, inv
    check(_lib.load().loftr_sp_from_f32(_ptr(x_nhwc), _ptr(out), B * H * W, Cc, _stream()), "loftr_sp_from_f32")
    return out


@_on_device
def sp_to_nhwc(x_sp, Cc):
    """SP int32 [B,H,W,Cp] -> fp32 [B,H,W,C]."""
    B, H, W, _ = x_sp.shape
    out = torch.empty(B, H, W, Cc, dtype=torch.float32, device=x_sp.device)
    check(_lib.load().loftr_sp_to_f32(_ptr(x_sp), _ptr(out), B * H * W, Cc, _stream()), "loftr_sp_to_f32")
    return out


def _prepared_conv(conv, bn):
    """Folded-BN SP filter of (conv, bn), cached on the module and rebuilt when any of the tensors it was built
    from is modified in place (tensor._version), replaced (data_ptr) or moved.  Inference weights are constant: the
    per-call weight preparation of loftr_conv_bn_act (two launches + a memset per convolution) runs once."""
    w = conv.weight
    if not w.is_cuda or w.dtype != torch.float32:
        raise _lib.LoftrHipError("conv.weight: expected a float32 GPU tensor")
    if bn is not None and bn.training:
        raise _lib.LoftrHipError("conv_bn_act folds eval-mode BatchNorm only; call .eval()")
    assert conv.bias is None and conv.dilation == (1, 1) and conv.groups == 1
    bnp = [] if bn is None else [bn.weight, bn.bias, bn.running_mean, bn.running_var]
    key = tuple((t.data_ptr(), t._version, tuple(t.stride())) for t in [w] + bnp) + (None if bn is None else float(bn.eps), str(w.device))
    cached = _PREPARED.get(conv)
    # ... or replaced by a NEW tensor object the allocator put at the same address (weak references to the originals)
    if cached is not None and cached[0] == key and all(r() is t for r, t in zip(cached[2], [w] + bnp)):
        return cached[1]
    Cout, Cin, KH, KW = w.shape
    lib = _lib.load()
    buf = torch.empty(lib.loftr_conv_workspace_bytes(Cin, Cout, KH, KW), dtype=torch.uint8, device=w.device)
    wst = (C.c_long * 4)(*w.stride())                       # contiguous or channels-last storage
    ptrs = [_ptr(t) for t in bnp] if bnp else [None] * 4
    check(lib.loftr_conv_prepare(_ptr(w), wst, Cin, Cout, KH, KW, *ptrs, float(bn.eps) if bn is not None else 0.0, _ptr(buf),
                                 buf.numel(), _stream()), "loftr_conv_prepare")
    _PREPARED[conv] = (key, buf, [weakref.ref(t) for t in [w] + bnp])
    return buf


CONV_SHARED_GPU = 0x100      # include/loftr_hip.h: LOFTR_CONV_SHARED_GPU


CONV_REM = False      # True: conv_bn_act hands 193 .. 199-channel 3x3 layers a scratch buffer (the tap-decomposed remainder form, see below)


@_on_device
def conv_bn_act(x_sp, Cin, conv, bn=None, act=0, residual=None, want_sp=True, want_f32=False, low_sp=None, shared_gpu=False,
                x_inv_scale=None):
    """nn.Conv2d(bias=False) [+ eval BatchNorm2d] [+ residual] [+ act] on an SP activation.

    x_sp int32 [B,H,W,ceil32(Cin)]; returns (y_sp or None, y_f32 [B,Ho,Wo,Cout] or None).
    low_sp (FPN top-down step): y = conv1x1(x) + bilinear_x2(low_sp), SP in / out.
    shared_gpu: the launch runs next to another stream's work (no persistent workgroups, see loftr_hip.h)."""
    w = conv.weight
    Cout, Cin_w, KH, KW = w.shape
    assert Cin_w == Cin
    stride, pad = conv.stride[0], conv.padding[0]
    B, H, W, Cp = x_sp.shape
    assert Cp == ceil32(Cin) and x_sp.dtype == torch.int32 and x_sp.is_contiguous()
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    dev = x_sp.device
    prepared = _prepared_conv(conv, bn)
    y_sp = torch.empty(B, Ho, Wo, ceil32(Cout), dtype=torch.int32, device=dev) if want_sp else None
    y_f32 = torch.empty(B, Ho, Wo, Cout, dtype=torch.float32, device=dev) if want_f32 else None
    lib = _lib.load()
    # 193 .. 199 output channels (LoFTR's 196): the channels beyond 192 as a tap-decomposed product through a scratch buffer (include/loftr_hip.h);
    # a fresh tensor per call, not the cached workspace: two streams may run convolutions at the same time
    # MEASURED AND NOT ADOPTED (CONV_REM = False): the 192-column kernel is no faster than the 224-column one -- a step of these kernels is bound by
    # its weight stream and barrier, not by its MFMA count (profiles/r06_conv_rem_ab.txt: 2586 + 217 us against 2370 us at 1/2 resolution)
    nscr = lib.loftr_conv_scratch_bytes(B, H, W, Cout, KH, KW, stride) if (CONV_REM and low_sp is None and not want_f32) else 0
    scratch = torch.empty(nscr, dtype=torch.uint8, device=dev) if nscr else None
    check(lib.loftr_conv_bn_act_prepared_scratch(_ptr(x_sp), B, H, W, Cin, _ptr(prepared), prepared.numel(), Cout, KH, KW,
                                                 stride, pad, int(act) | (CONV_SHARED_GPU if shared_gpu else 0), _ptr(residual),
                                                 _ptr(low_sp), _ptr(y_sp), _ptr(y_f32), _ptr(x_inv_scale), _ptr(scratch), nscr,
                                                 _stream()), "loftr_conv_bn_act_prepared_scratch")
    return y_sp, y_f32


@_on_device
def conv_raw(x_sp, Cin, weight, stride, pad, x_inv_scale=None):
    """Bias-free convolution of an SP activation with a filter given as a TENSOR [Cout,Cin,KH,KW] (no BatchNorm folded, no
    activation, filter encoded per call): the training forward and the input-gradient convolutions.  -> fp32 [B,Ho,Wo,Cout]."""
    _need(weight, "weight")
    Cout, Cin_w, KH, KW = weight.shape
    assert Cin_w == Cin
    B, H, W, Cp = x_sp.shape
    assert Cp == ceil32(Cin) and x_sp.dtype == torch.int32 and x_sp.is_contiguous()
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    lib = _lib.load()
    ws = workspace(lib.loftr_conv_workspace_bytes(Cin, Cout, KH, KW), x_sp.device)
    y = torch.empty(B, Ho, Wo, Cout, dtype=torch.float32, device=x_sp.device)
    wst = (C.c_long * 4)(*weight.stride())
    check(lib.loftr_conv_bn_act(_ptr(x_sp), B, H, W, Cin, _ptr(weight), wst, Cout, KH, KW, stride, pad, None, None, None, None, 0.0, 0,
                                None, None, _ptr(y), _ptr(ws), ws.numel(), _ptr(x_inv_scale), _stream()), "loftr_conv_bn_act")
    return y


@_on_device
def conv_wgrad(dy_nhwc, x_nhwc, KH, KW, stride, pad):
    """dL/dweight [Cout,Cin,KH,KW] of a bias-free convolution from dy [B,Ho,Wo,Cout] and its input x [B,H,W,Cin] (fp32, channels last)."""
    _need(dy_nhwc, "dy_nhwc"); _need(x_nhwc, "x_nhwc")
    B, H, W, Cin = x_nhwc.shape
    _, Ho, Wo, Cout = dy_nhwc.shape
    assert Ho == (H + 2 * pad - KH) // stride + 1 and Wo == (W + 2 * pad - KW) // stride + 1 and dy_nhwc.shape[0] == B
    lib = _lib.load()
    ws = workspace(lib.loftr_conv_wgrad_workspace_bytes(B, Ho, Wo, Cin, Cout, KH, KW), x_nhwc.device)
    taps = torch.empty(KH * KW, Cout, Cin, dtype=torch.float32, device=x_nhwc.device)
    check(lib.loftr_conv_wgrad(_ptr(dy_nhwc), _ptr(x_nhwc), B, H, W, Cin, Cout, KH, KW, stride, pad, _ptr(taps), _ptr(ws), ws.numel(),
                               _stream()), "loftr_conv_wgrad")
    return taps.view(KH, KW, Cout, Cin).permute(2, 3, 0, 1).contiguous()


@_on_device
def stem_conv_bn_relu(x, conv, bn):
    """conv1 (7x7, stride 2, one input channel) + eval bn1 + relu -> SP int32 [B,Ho,Wo,ceil32(C0)]."""
    if not x.is_cuda or x.dtype != torch.float32 or x.shape[1] != 1:
        raise _lib.LoftrHipError("stem: expected a float32 GPU tensor [B,1,H,W]")
    w = conv.weight
    assert tuple(w.shape[1:]) == (1, 7, 7) and conv.stride == (2, 2) and conv.padding == (3, 3) and conv.bias is None
    if bn.training:
        raise _lib.LoftrHipError("stem folds eval-mode BatchNorm only; call .eval()")
    B, _, H, W = x.shape
    C0 = w.shape[0]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, ceil32(C0), dtype=torch.int32, device=x.device)
    xs, wst = (C.c_long * 4)(*x.stride()), (C.c_long * 4)(*w.stride())
    check(_lib.load().loftr_stem_conv_bn_relu(_ptr(x), xs, B, H, W, _ptr(w), wst, C0, _ptr(bn.weight), _ptr(bn.bias),
                                              _ptr(bn.running_mean), _ptr(bn.running_var), float(bn.eps), _ptr(y),
                                              _stream()), "loftr_stem_conv_bn_relu")
    return y


def conv1x1_upsample_add(x_sp, Cin, conv, low_sp):
    """conv1x1(x) + bilinear x2 (align_corners=True) of low in one launch (one FPN top-down step); SP in / out."""
    Cout = conv.weight.shape[0]
    assert tuple(conv.weight.shape[1:]) == (Cin, 1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0)
    B, H, W, _ = x_sp.shape
    if low_sp.shape != (B, H // 2, W // 2, ceil32(Cout)) or H % 2 or W % 2 or not low_sp.is_contiguous():
        raise _lib.LoftrHipError(f"conv1x1_upsample_add: low map {tuple(low_sp.shape)} is not half of {tuple(x_sp.shape)}")
    return conv_bn_act(x_sp, Cin, conv, low_sp=low_sp)[0]


@_on_device
def upsample2x_add(low_sp, lateral_sp, Cc):
    """lateral + bilinear x2 (align_corners=True) of low; SP in, SP out."""
    B, Hl, Wl, Cp = low_sp.shape
    assert lateral_sp.shape == (B, 2 * Hl, 2 * Wl, Cp)
    out = torch.empty_like(lateral_sp)
    check(_lib.load().loftr_upsample2x_add(_ptr(low_sp), _ptr(lateral_sp), _ptr(out), B, Hl, Wl, Cc, _stream()),
          "loftr_upsample2x_add")
    return out


@_on_device
def epipolar_errors(mkpts0_f, mkpts1_f, m_bids, T_0to1, K0, K1):
    """Squared symmetric epipolar distance of every match (metrics.py:31-68) -> float32 [M], match order."""
    for name, t, dt in (("mkpts0_f", mkpts0_f, torch.float32), ("mkpts1_f", mkpts1_f, torch.float32), ("m_bids", m_bids, torch.int64),
                        ("T_0to1", T_0to1, torch.float32), ("K0", K0, torch.float32), ("K1", K1, torch.float32)):
        if not t.is_cuda or t.dtype != dt:
            raise _lib.LoftrHipError(f"{name}: expected a {dt} GPU tensor (the evaluation kernels have no CPU fallback)")
    M, N = mkpts0_f.shape[0], T_0to1.shape[0]
    assert mkpts0_f.shape == (M, 2) and mkpts1_f.shape == (M, 2) and m_bids.shape == (M,)
    assert T_0to1.shape == (N, 4, 4) and K0.shape == (N, 3, 3) and K1.shape == (N, 3, 3)
    out = torch.empty(M, dtype=torch.float32, device=mkpts0_f.device)
    args = [t.contiguous() for t in (mkpts0_f, mkpts1_f, m_bids, T_0to1, K0, K1)]
    check(_lib.load().loftr_epipolar_errors(*[_ptr(t) for t in args], M, N, _ptr(out), _stream()), "loftr_epipolar_errors")
    return out


@_on_device
def estimate_poses(mkpts0_f, mkpts1_f, m_bids, K0, K1, thresh_px, conf, seed=0):
    """Five-point RANSAC + cheirality for every pair of a batch on the GPU (csrc/pose_gpu.hip): for each pair, what the host
    estimator loftr_estimate_pose (evaluation.estimate_pose_native) returns for that pair's matches with the same seed.
    mkpts0_f / mkpts1_f [M,2] f32, m_bids [M] i64 grouped by ascending pair id (as the matcher emits them), K0 / K1 [P,3,3] f32.
    -> (R [P,3,3] f32, t [P,3] f32, inliers [M] bool in match order, n_inliers [P] i64), device tensors; n_inliers[p] == -1
    where the host estimator returns None (R, t and that pair's mask are zero there).  Synchronises the stream once."""
    for name, t, dt in (("mkpts0_f", mkpts0_f, torch.float32), ("mkpts1_f", mkpts1_f, torch.float32), ("m_bids", m_bids, torch.int64),
                        ("K0", K0, torch.float32), ("K1", K1, torch.float32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt:
            raise _lib.LoftrHipError(f"{name}: expected a {dt} GPU tensor (the pose kernels have no CPU fallback)")
    M, P = mkpts0_f.shape[0], K0.shape[0]
    if mkpts0_f.shape != (M, 2) or mkpts1_f.shape != (M, 2) or m_bids.shape != (M,):
        raise _lib.LoftrHipError(f"estimate_poses: expected mkpts0_f / mkpts1_f [M,2] and m_bids [M], got {tuple(mkpts0_f.shape)}, "
                                 f"{tuple(mkpts1_f.shape)}, {tuple(m_bids.shape)}")
    if K0.shape != (P, 3, 3) or K1.shape != (P, 3, 3):
        raise _lib.LoftrHipError(f"estimate_poses: expected K0 / K1 [P,3,3], got {tuple(K0.shape)}, {tuple(K1.shape)}")
    dev = mkpts0_f.device
    args = [t.contiguous() for t in (mkpts0_f, mkpts1_f, m_bids, K0, K1)]
    R = torch.zeros(P, 3, 3, dtype=torch.float32, device=dev)
    t = torch.zeros(P, 3, dtype=torch.float32, device=dev)
    inl = torch.zeros(M, dtype=torch.uint8, device=dev)
    n = torch.full((P,), -1, dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = torch.empty(max(1, lib.loftr_estimate_pose_batched_workspace_bytes(M, P)), dtype=torch.uint8, device=dev)
    check(lib.loftr_estimate_pose_batched(*[_ptr(a) for a in args[:3]], M, _ptr(args[3]), _ptr(args[4]), P, float(thresh_px), float(conf),
                                          int(seed), _ptr(R), _ptr(t), _ptr(inl), _ptr(n), _ptr(ws), ws.numel(), _stream()),
          "loftr_estimate_pose_batched (m_bids must lie in [0, P) and be grouped by ascending pair)")
    return R, t, inl.view(torch.bool), n


GEOMETRY_MODELS = {"homography": 0, "fundamental": 1}


def estimate_geometry(mkpts0_f, mkpts1_f, m_bids, P, model, thresh_px, conf, seed=0):
    """Homography / fundamental-matrix RANSAC + least-squares refit for every pair of a batch on the GPU
    (csrc/geometry_gpu.hip): for each pair, what the host estimator loftr_estimate_geometry (evaluation.estimate_homography_native /
    estimate_fundamental_native) returns for that pair's matches with the same seed.  No intrinsics are needed; thresh_px is in pixels.
    mkpts0_f / mkpts1_f [M,2] f32, m_bids [M] i64 grouped by ascending pair id (as the matcher emits them), P pairs,
    model "homography" (x1 ~ H x0) or "fundamental" (x1^T F x0 = 0).
    -> (mat [P,3,3] f32 with unit Frobenius norm, inliers [M] bool in match order, n_inliers [P] i64), device tensors; n_inliers[p] == -1
    where the host estimator finds no model (the matrix and that pair's mask are zero there)."""
    if model not in GEOMETRY_MODELS:
        raise _lib.LoftrHipError(f"estimate_geometry: model must be one of {sorted(GEOMETRY_MODELS)}, got {model!r}")
    for name, t, dt in (("mkpts0_f", mkpts0_f, torch.float32), ("mkpts1_f", mkpts1_f, torch.float32), ("m_bids", m_bids, torch.int64)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt:
            raise _lib.LoftrHipError(f"{name}: expected a {dt} GPU tensor (the geometry kernels have no CPU fallback)")
    M, P = mkpts0_f.shape[0], int(P)
    if mkpts0_f.shape != (M, 2) or mkpts1_f.shape != (M, 2) or m_bids.shape != (M,) or P < 0:
        raise _lib.LoftrHipError(f"estimate_geometry: expected mkpts0_f / mkpts1_f [M,2], m_bids [M] and P >= 0, got "
                                 f"{tuple(mkpts0_f.shape)}, {tuple(mkpts1_f.shape)}, {tuple(m_bids.shape)}, P = {P}")
    dev = mkpts0_f.device
    args = [t.contiguous() for t in (mkpts0_f, mkpts1_f, m_bids)]
    mat = torch.zeros(P, 3, 3, dtype=torch.float32, device=dev)
    inl = torch.zeros(M, dtype=torch.uint8, device=dev)
    n = torch.full((P,), -1, dtype=torch.int64, device=dev)
    lib, kind = _lib.load(), GEOMETRY_MODELS[model]
    ws = torch.empty(max(1, lib.loftr_estimate_geometry_batched_workspace_bytes(M, P, kind)), dtype=torch.uint8, device=dev)
    check(lib.loftr_estimate_geometry_batched(*[_ptr(a) for a in args], M, P, kind, float(thresh_px), float(conf), int(seed), _ptr(mat),
                                              _ptr(inl), _ptr(n), _ptr(ws), ws.numel(), _stream()),
          "loftr_estimate_geometry_batched (m_bids must lie in [0, P) and be grouped by ascending pair)")
    return mat, inl.view(torch.bool), n


@_on_device
def estimate_absolute_poses(pts3d, kpts, m_bids, K, thresh_px, conf, seed=0):
    """Absolute pose (P3P RANSAC + Gauss-Newton refit on the reprojection error) for every pair of a batch on the GPU
    (csrc/absolute_pose_gpu.hip): for each pair, what the host estimator loftr_estimate_absolute_pose
    (evaluation.estimate_absolute_pose_native) returns for that pair's 2D-3D matches with the same seed.
    pts3d [M,3] f32 (units of the depth), kpts [M,2] f32 pixels of the camera to resect, m_bids [M] i64 grouped by ascending pair id,
    K [P,3,3] f32 intrinsics of that camera per pair (upper triangular).
    -> (R [P,3,3] f32, t [P,3] f32 with x_cam = R X + t, inliers [M] bool in match order, n_inliers [P] i64), device tensors;
    n_inliers[p] == -1 where the host estimator finds no model (R, t and that pair's mask are zero there).  Synchronises the stream."""
    for name, t, dt in (("pts3d", pts3d, torch.float32), ("kpts", kpts, torch.float32), ("m_bids", m_bids, torch.int64), ("K", K, torch.float32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt:
            raise _lib.LoftrHipError(f"{name}: expected a {dt} GPU tensor (the absolute-pose kernels have no CPU fallback)")
    M, P = pts3d.shape[0], K.shape[0]
    if pts3d.shape != (M, 3) or kpts.shape != (M, 2) or m_bids.shape != (M,) or K.shape != (P, 3, 3):
        raise _lib.LoftrHipError(f"estimate_absolute_poses: expected pts3d [M,3], kpts [M,2], m_bids [M] and K [P,3,3], got "
                                 f"{tuple(pts3d.shape)}, {tuple(kpts.shape)}, {tuple(m_bids.shape)}, {tuple(K.shape)}")
    dev = pts3d.device
    args = [t.contiguous() for t in (pts3d, kpts, m_bids, K)]
    R = torch.zeros(P, 3, 3, dtype=torch.float32, device=dev)
    t = torch.zeros(P, 3, dtype=torch.float32, device=dev)
    inl = torch.zeros(M, dtype=torch.uint8, device=dev)
    n = torch.full((P,), -1, dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = torch.empty(max(1, lib.loftr_estimate_absolute_pose_batched_workspace_bytes(M, P)), dtype=torch.uint8, device=dev)
    check(lib.loftr_estimate_absolute_pose_batched(*[_ptr(a) for a in args[:3]], M, _ptr(args[3]), P, float(thresh_px), float(conf), int(seed),
                                                   _ptr(R), _ptr(t), _ptr(inl), _ptr(n), _ptr(ws), ws.numel(), _stream()),
          "loftr_estimate_absolute_pose_batched (m_bids must lie in [0, P) and be grouped by ascending pair)")
    return R, t, inl.view(torch.bool), n


@_on_device
def lift_keypoints(kpts, m_bids, depth, K, T=None):
    """Matched keypoints of the image that has a depth map -> 3D points on the GPU (loftr_lift_keypoints: the first half of the
    reference's warp_kpts, fp32): the depth at the keypoint rounded half to even, X = K^-1 (x d, y d, d) with the unrounded keypoint,
    then the optional camera-to-world transform.
    kpts [M,2] f32, m_bids [M] i64, depth [P,dh,dw] f32, K [P,3,3] f32, T [P,4,4] f32 or None.
    -> (pts3d [M,3] f32, valid [M] bool): invalid (zero row) where the keypoint falls outside the map or the depth there is 0."""
    for name, t, dt in (("kpts", kpts, torch.float32), ("m_bids", m_bids, torch.int64), ("depth", depth, torch.float32), ("K", K, torch.float32)) + \
            ((("T", T, torch.float32),) if T is not None else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt:
            raise _lib.LoftrHipError(f"{name}: expected a {dt} GPU tensor (the lifting kernel has no CPU fallback)")
    M, P = kpts.shape[0], K.shape[0]
    if kpts.shape != (M, 2) or m_bids.shape != (M,) or depth.dim() != 3 or depth.shape[0] != P or K.shape != (P, 3, 3) or \
            (T is not None and T.shape != (P, 4, 4)):
        raise _lib.LoftrHipError(f"lift_keypoints: expected kpts [M,2], m_bids [M], depth [P,dh,dw], K [P,3,3] and T [P,4,4] or None, got "
                                 f"{tuple(kpts.shape)}, {tuple(m_bids.shape)}, {tuple(depth.shape)}, {tuple(K.shape)}, "
                                 f"{None if T is None else tuple(T.shape)}")
    dev = kpts.device
    args = [None if t is None else t.contiguous() for t in (kpts, m_bids, depth, K, T)]
    out = torch.zeros(M, 3, dtype=torch.float32, device=dev)
    valid = torch.zeros(M, dtype=torch.uint8, device=dev)
    check(_lib.load().loftr_lift_keypoints(_ptr(args[0]), _ptr(args[1]), M, _ptr(args[2]), depth.shape[1], depth.shape[2], _ptr(args[3]),
                                           _ptr(args[4]), P, _ptr(out), _ptr(valid), _stream()), "loftr_lift_keypoints")
    return out, valid.view(torch.bool)


@_on_device
def estimate_similarities(src, dst, m_bids, P, with_scale=True, thresh=0.05, conf=0.999, seed=0):
    """3D similarity (dst ~ s R src + t; rigid, s == 1, with with_scale=False) by RANSAC over 3-point closed forms + a closed-form refit
    for every problem of a batch on the GPU (csrc/similarity_gpu.hip): for each problem, what the host estimator
    loftr_estimate_similarity (evaluation.estimate_similarity_native) returns for that problem's correspondences with the same seed,
    bit for bit.
    src [M,3], dst [M,3] f64 or f32 (widened to f64 here), m_bids [M] i64 grouped by ascending problem id, P problems; thresh in the
    units of dst.
    -> (s [P] f64, R [P,3,3] f64, t [P,3] f64, inliers [M] bool, n_inliers [P] i64), device tensors; n_inliers[p] == -1 where the
    host estimator finds no model (s, R, t and that problem's mask are zero there).  Synchronises the stream."""
    for name, t, dts in (("src", src, (torch.float64, torch.float32)), ("dst", dst, (torch.float64, torch.float32)), ("m_bids", m_bids, (torch.int64,))):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in dts:
            raise _lib.LoftrHipError(f"{name}: expected a {' or '.join(str(d) for d in dts)} GPU tensor (the similarity kernels have no CPU fallback)")
    M, P = src.shape[0], int(P)
    if src.shape != (M, 3) or dst.shape != (M, 3) or m_bids.shape != (M,) or P < 0:
        raise _lib.LoftrHipError(f"estimate_similarities: expected src [M,3], dst [M,3], m_bids [M] and P >= 0, got "
                                 f"{tuple(src.shape)}, {tuple(dst.shape)}, {tuple(m_bids.shape)}, {P}")
    dev = src.device
    args = [src.double().contiguous(), dst.double().contiguous(), m_bids.contiguous()]
    s = torch.zeros(P, dtype=torch.float64, device=dev)
    R = torch.zeros(P, 3, 3, dtype=torch.float64, device=dev)
    t = torch.zeros(P, 3, dtype=torch.float64, device=dev)
    inl = torch.zeros(M, dtype=torch.uint8, device=dev)
    n = torch.full((P,), -1, dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = torch.empty(max(1, lib.loftr_estimate_similarity_batched_workspace_bytes(M, P)), dtype=torch.uint8, device=dev)
    check(lib.loftr_estimate_similarity_batched(*[_ptr(a) for a in args], M, P, int(bool(with_scale)), float(thresh), float(conf), int(seed),
                                                _ptr(s), _ptr(R), _ptr(t), _ptr(inl), _ptr(n), _ptr(ws), ws.numel(), _stream()),
          "loftr_estimate_similarity_batched (m_bids must lie in [0, P) and be grouped by ascending problem)")
    return s, R, t, inl.view(torch.bool), n


@_on_device
def transform_model(xyz, T_cam_from_world, posed, s, R, t, out_xyz=None, out_T=None):
    """Move a model by one similarity, X' = s R X + t (loftr_transform_model_host on CPU tensors, loftr_transform_model on GPU tensors:
    one text, fp64 in a stated order, so the two sides agree bit for bit).
    xyz [N,3] f32, T_cam_from_world [n,4,4] f64, posed [n] bool or u8, s [] or [1] f64, R [3,3] f64, t [3] f64 -- all on one device.
    -> (xyz' [N,3] f32, T' [n,4,4] f64): posed images get R_c R^T and s t_c - R_c' t, the others their input bits.  out_xyz / out_T may
    be the inputs themselves (in place)."""
    named = (("xyz", xyz, torch.float32, (3,)), ("T_cam_from_world", T_cam_from_world, torch.float64, (4, 4)), ("posed", posed, None, ()),
             ("s", s, torch.float64, None), ("R", R, torch.float64, None), ("t", t, torch.float64, None))
    for name, a, dt, tail in named:
        if not isinstance(a, torch.Tensor):
            raise _lib.LoftrHipError(f"transform_model: {name} must be a tensor")
    devs = {a.device for _, a, _, _ in named} | {a.device for a in (out_xyz, out_T) if a is not None}
    if len(devs) != 1:
        raise _lib.LoftrHipError(f"transform_model: tensors on different devices ({sorted(str(d) for d in devs)})")
    if posed.dtype not in (torch.bool, torch.uint8):
        raise _lib.LoftrHipError(f"transform_model: posed must be bool or uint8, got {posed.dtype}")
    for name, a, dt, tail in named:
        if dt is not None and a.dtype != dt:
            raise _lib.LoftrHipError(f"transform_model: {name} must be {dt}, got {a.dtype}")
    N, n = xyz.shape[0], T_cam_from_world.shape[0]
    if xyz.shape != (N, 3) or T_cam_from_world.shape != (n, 4, 4) or posed.shape != (n,) or s.numel() != 1 or R.shape != (3, 3) or t.shape != (3,):
        raise _lib.LoftrHipError(f"transform_model: expected xyz [N,3], T_cam_from_world [n,4,4], posed [n], s [1], R [3,3], t [3], got "
                                 f"{tuple(xyz.shape)}, {tuple(T_cam_from_world.shape)}, {tuple(posed.shape)}, {tuple(s.shape)}, "
                                 f"{tuple(R.shape)}, {tuple(t.shape)}")
    for name, o, like in (("out_xyz", out_xyz, xyz), ("out_T", out_T, T_cam_from_world)):
        if o is not None and (o.dtype != like.dtype or o.shape != like.shape or not o.is_contiguous()):
            raise _lib.LoftrHipError(f"transform_model: {name} must be a contiguous {like.dtype} tensor of shape {tuple(like.shape)}")
    xyz_c, T_c, R_c, t_c = (a if a is out else a.contiguous() for a, out in ((xyz, out_xyz), (T_cam_from_world, out_T), (R, None), (t, None)))
    posed_c = posed.contiguous().view(torch.uint8)
    out_xyz = torch.empty_like(xyz_c) if out_xyz is None else out_xyz
    out_T = torch.empty_like(T_c) if out_T is None else out_T
    lib = _lib.load()
    args = (_ptr(xyz_c), N, _ptr(T_c), _ptr(posed_c), n, _ptr(s), _ptr(R_c), _ptr(t_c), _ptr(out_xyz), _ptr(out_T))
    if xyz.is_cuda:
        check(lib.loftr_transform_model(*args, _stream()), "loftr_transform_model")
    else:
        check(lib.loftr_transform_model_host(*args), "loftr_transform_model_host")
    return out_xyz, out_T


# ---- view overlap (csrc/overlap.hip, csrc/overlap_gpu.hip) --------------------------------------------------------------
OVERLAP_COUNTS = 8
OVERLAP_NAMES = ("n_visible", "error_bits", "n_sources", "n_targets", "n_nonzero")      # counts[0..4]; the rest are 0
OVERLAP_STAGES = ("check", "tables", "count")
OVERLAP_ERRORS = ((1, "vis_point must lie in [0, number of points)"),
                  (2, "vis_offsets must start at 0, end at the number of entries and ascend"))
_OVL_ARGS = (("vis_offsets", torch.int64, (None,)), ("vis_point", torch.int32, (None,)), ("xyz", torch.float32, (None, 3)),
             ("point_ok", torch.uint8, (None,)), ("K_src", torch.float64, (None, 9)), ("T_src", torch.float64, (None, 16)),
             ("src_ok", torch.uint8, (None,)), ("K_tgt", torch.float64, (None, 9)), ("T_tgt", torch.float64, (None, 16)),
             ("tgt_ok", torch.uint8, (None,)), ("tgt_hw", torch.float64, (None, 2)))


def view_overlap(vis_offsets, vis_point, xyz, point_ok, K_src, T_src, src_ok, K_tgt, T_tgt, tgt_ok, tgt_hw, border_px, cos_min, max_scale2,
                 timings=None):
    """loftr_view_overlap_host on CPU tensors, loftr_view_overlap (csrc/overlap_gpu.hip) on GPU tensors: the same integers; mixed devices
    are an error and there is no fallback either way.  vis_offsets [n+1] i64, vis_point [V] i32, xyz [T,3] f32, point_ok [T] u8, K_src
    [n,9] / T_src [n,16] f64, src_ok [n] u8, K_tgt [m,9] / T_tgt [m,16] f64, tgt_ok [m] u8, tgt_hw [m,2] f64 (H, W); border_px >= 0,
    cos_min in [-1, 1], max_scale2 >= 1 (inf: no scale test).
    -> dict of tensors on the inputs' device: overlap [n,m] i32, n_vis [n] i32, counts [8] i64 (OVERLAP_NAMES).  Nothing is read back
    here: a bad list leaves its bits (OVERLAP_ERRORS) in counts[1] and every other output zero, on both sides.  timings: a list that
    receives (stage, ms) pairs of the GPU stages (the call then waits for the stream)."""
    what = "view_overlap"
    arrays = (vis_offsets, vis_point, xyz, point_ok, K_src, T_src, src_ok, K_tgt, T_tgt, tgt_ok, tgt_hw)
    for (name, dt, shape), a in zip(_OVL_ARGS, arrays):
        if not isinstance(a, torch.Tensor):
            raise _lib.LoftrHipError(f"{what}: {name} must be a tensor")
    gpu = [a.is_cuda for a in arrays]
    if any(gpu) and not all(gpu):
        raise _lib.LoftrHipError(f"{what}: GPU and CPU arguments mixed (" + ", ".join(f"{s[0]}: {'GPU' if g else 'CPU'}" for s, g in zip(_OVL_ARGS, gpu))
                                 + "); there is no silent fallback: move them to one device")
    if not all(gpu) and any(a.device.type != "cpu" for a in arrays):
        raise _lib.LoftrHipError(f"{what}: tensors must live on a GPU (the kernels) or on the CPU (the host routine)")
    for (name, dt, shape), a in zip(_OVL_ARGS, arrays):
        if a.dtype != dt or a.dim() != len(shape) or any(s is not None and a.shape[d] != s for d, s in enumerate(shape)):
            raise _lib.LoftrHipError(f"{what}: {name} must be {dt} of shape {list(shape)}, got {a.dtype} {tuple(a.shape)}")
    n, m, T, V = vis_offsets.shape[0] - 1, K_tgt.shape[0], xyz.shape[0], vis_point.shape[0]
    if n < 0 or any(a.shape[0] != n for a in (K_src, T_src, src_ok)) or any(a.shape[0] != m for a in (T_tgt, tgt_ok, tgt_hw)) or \
            point_ok.shape[0] != T:
        raise _lib.LoftrHipError(f"{what}: expected vis_offsets [n+1], K_src / T_src / src_ok [n], K_tgt / T_tgt / tgt_ok / tgt_hw [m] and xyz / "
                                 f"point_ok [T], got {[tuple(a.shape) for a in arrays]}")
    border_px, cos_min, max_scale2 = float(border_px), float(cos_min), float(max_scale2)
    if not (0.0 <= border_px < float("inf")) or not (-1.0 <= cos_min <= 1.0) or not (max_scale2 >= 1.0):
        raise ValueError(f"{what}: border_px must be finite and >= 0, cos_min in [-1, 1] and max_scale2 >= 1, got {border_px}, {cos_min}, {max_scale2}")
    if n * m > 2 ** 31 or V >= 2 ** 31 or T >= 2 ** 31:
        raise ValueError(f"{what}: {n} x {m} pairs, {V} entries or {T} points are beyond the supported 2^31 (there is no sparse output)")
    if n == 0 and V != 0:
        raise ValueError(f"{what}: {V} entries without a source image")
    arrays = [a.contiguous() for a in arrays]                                            # (held until the call has returned)
    dev = arrays[0].device
    out = {"overlap": torch.zeros((n, m), dtype=torch.int32, device=dev), "n_vis": torch.zeros(n, dtype=torch.int32, device=dev),
           "counts": torch.zeros(OVERLAP_COUNTS, dtype=torch.int64, device=dev)}
    p = [_ptr(a) for a in arrays]
    args = (p[0], p[1], V, p[2], p[3], T, p[4], p[5], p[6], n, p[7], p[8], p[9], p[10], m, border_px, cos_min, max_scale2,
            _ptr(out["overlap"]), _ptr(out["n_vis"]), _ptr(out["counts"]))
    lib = _lib.load()
    if all(gpu):
        if any(a.device != dev for a in arrays):
            raise _lib.LoftrHipError(f"{what}: tensors on different devices ({sorted({str(a.device) for a in arrays})})")
        ms = _StageMs(timings, OVERLAP_STAGES)
        with torch.cuda.device(dev):                                                     # stream, workspace and pointers belong to the tensors' device
            buf = torch.empty(max(1, lib.loftr_view_overlap_workspace_bytes(n, m)), dtype=torch.uint8, device=dev)
            check(lib.loftr_view_overlap(*args, _ptr(buf), buf.numel(), ms.arg, _stream()), "loftr_view_overlap")
        ms.report()
    else:
        status = lib.loftr_view_overlap_host(*args)
        if not (status == -1 and int(out["counts"][1]) != 0):                            # a bad list is reported through counts[1], as on the GPU
            check(status, "loftr_view_overlap_host")
    return out


# ---- the two sides of a routine pair -------------------------------------------------------------------------------------------------
# The SfM routines below come in pairs: loftr_<name>_host on numpy arrays DEFINES the result, loftr_<name> reproduces it on GPU tensors.
# A pair shares one body, written against a backend that supplies what differs: how an array that belongs to the other side is refused,
# how a dtype is named, a pointer taken, an output allocated, and which of the two C entry points is called with which trailing arguments.
class _Host:
    @staticmethod
    def refuse(what, names, arrays, hint):
        import numpy as np
        if not all(isinstance(a, np.ndarray) for a in arrays):
            raise _lib.LoftrHipError(f"{what}: expected numpy arrays (GPU tensors go to {hint})")

    @staticmethod
    def dtype_of(a):
        return a.dtype.name

    @staticmethod
    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    @staticmethod
    def contiguous(a):
        import numpy as np
        return None if a is None else np.ascontiguousarray(a)

    @staticmethod
    def zeros(shape, dt, like):
        import numpy as np
        return np.zeros(shape, dt)

    empty = zeros                                                                        # (the host routines' outputs start as zeros)

    @staticmethod
    def call(name, args, why, like, ws=None, extra=(), tail=()):
        check(getattr(_lib.load(), f"loftr_{name}_host")(*args), f"loftr_{name}_host ({why})")


class _Gpu:
    @staticmethod
    def refuse(what, names, arrays, hint):
        for name, a in zip(names, arrays):
            if not isinstance(a, torch.Tensor) or not a.is_cuda:
                raise _lib.LoftrHipError(f"{name}: expected a GPU tensor ({hint})")

    @staticmethod
    def dtype_of(a):
        return str(a.dtype).replace("torch.", "")

    ptr = staticmethod(_ptr)

    @staticmethod
    def contiguous(a):
        return None if a is None else a.contiguous()

    @staticmethod
    def zeros(shape, dt, like):
        return torch.zeros(shape, dtype=getattr(torch, dt), device=like.device)

    @staticmethod
    def empty(shape, dt, like):
        return torch.empty(shape, dtype=getattr(torch, dt), device=like.device)

    @staticmethod
    def call(name, args, why, like, ws=None, extra=(), tail=()):
        """args: what both entry points take; extra: what only the kernels take before the workspace; ws: the arguments of
        loftr_<name>_workspace_bytes (None: no workspace); tail: the timing arguments before the stream."""
        lib = _lib.load()
        if ws is not None:
            buf = torch.empty(max(1, getattr(lib, f"loftr_{name}_workspace_bytes")(*ws)), dtype=torch.uint8, device=like.device)
            extra = (*extra, _ptr(buf), buf.numel())
        check(getattr(lib, f"loftr_{name}")(*args, *extra, *tail, _stream()), f"loftr_{name}")


def _check_args(B, what, hint, spec, arrays):
    """Arrays of the right side, then the (name, dtype, ndim) table `spec` against them."""
    B.refuse(what, [s[0] for s in spec], arrays, hint)
    for (name, dt, nd), a in zip(spec, arrays):
        if B.dtype_of(a) != dt or a.ndim != nd:
            raise _lib.LoftrHipError(f"{what}: {name} must be {dt} with {nd} dimension(s), got {B.dtype_of(a)} {tuple(a.shape)}")


def _outputs(B, table, size, counts, like):
    """Zeroed outputs of a (name, size key, trailing shape, dtype) table, and counts [counts] i64 last."""
    out = {k: B.zeros((size[s],) + tail, dt, like) for k, s, tail, dt in table}
    out["counts"] = B.zeros(counts, "int64", like)
    return out


class _StageMs:
    """The stage-timing buffer of one call: `arg` goes to the entry point (None without timings), report() appends (stage, ms) pairs."""

    def __init__(self, timings, stages):
        self.timings, self.stages = timings, stages
        self.buf = (C.c_float * len(stages))() if timings is not None else None
        self.arg = C.cast(self.buf, C.c_void_p) if timings is not None else None

    def report(self):
        if self.timings is not None:
            self.timings.extend(zip(self.stages, (float(v) for v in self.buf)))


_TABLE_RULES = ("offsets must start at 0, end at N and ascend; obs_image must lie in [0, n_images); cam_offsets / cam_obs "
                "must group the observations by image in ascending order")


# ---- keypoint atlas (csrc/atlas.hip, csrc/atlas_gpu.hip) -----------------------------------------------------------------
ATLAS_COUNTS = 16
ATLAS_REASONS = ("n_valid", "n_bad_row", "n_masked", "n_nonfinite", "n_negative_conf", "n_outside")     # counts[4 + reason]
ATLAS_STAGES = ("compact", "resolve", "mutual_best", "write_matches", "union_find", "labels", "number_tracks")


def _atlas_out(arrays, ptr):
    return _lib.AtlasOut(**{k: ptr(arrays[k]) for k, _ in _lib.AtlasOut._fields_})


def atlas_host(kpts0, kpts1, conf, rows, mask, row_images, n_images, gh, gw, inv, min_track_len):
    """loftr_atlas_host: the host routine that DEFINES the atlas (rules 1-4 of include/loftr_hip.h) on numpy arrays.
    kpts0 / kpts1 [M,2] f32, conf [M] f32, rows [M] i32 ascending, mask [M] u8 or None, row_images [R,2] i32.
    -> dict of numpy arrays of the bound sizes (see LoftrAtlasOut) with 'counts' [16] i64; the caller trims by counts[0..2]."""
    import numpy as np
    k0, k1 = (np.ascontiguousarray(a, np.float32).reshape(-1, 2) for a in (kpts0, kpts1))
    c = np.ascontiguousarray(conf, np.float32).reshape(-1)
    r = np.ascontiguousarray(rows, np.int32).reshape(-1)
    ri = np.ascontiguousarray(row_images, np.int32).reshape(-1, 2)
    mk = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
    M, R = k0.shape[0], ri.shape[0]
    if k1.shape[0] != M or c.shape[0] != M or r.shape[0] != M or (mk is not None and mk.shape[0] != M):
        raise ValueError(f"atlas_host: kpts0, kpts1, conf, rows and mask must agree on M, got {k0.shape}, {k1.shape}, {c.shape}, {r.shape}")
    Kb = max(1, min(2 * M, int(n_images) * int(gh) * int(gw)))
    out = {"kp_offsets": np.zeros(int(n_images) + 1, np.int64), "keypoints": np.zeros((Kb, 2), np.float32), "score": np.zeros(Kb, np.float32),
           "n_obs": np.zeros(Kb, np.int32), "row_offsets": np.zeros(R + 1, np.int64), "matches": np.zeros((max(M, 1), 2), np.int32),
           "match_conf": np.zeros(max(M, 1), np.float32), "track_id": np.full(Kb, -1, np.int32), "track_len": np.zeros(Kb, np.int32),
           "track_ok": np.zeros(Kb, np.uint8), "counts": np.zeros(ATLAS_COUNTS, np.int64)}
    ptr = _Host.ptr
    st = _atlas_out(out, ptr)
    check(_lib.load().loftr_atlas_host(ptr(k0), ptr(k1), ptr(c), ptr(r), ptr(mk), M, ptr(ri), R, int(n_images), int(gh), int(gw), float(inv),
                                       int(min_track_len), C.byref(st)),
          "loftr_atlas_host (rows must ascend within [0, R); row images must differ and lie in [0, n_images))")
    return out


@_on_device
def atlas_observe(kpts0, kpts1, conf, m_bids, mask, n_rows, match_base, row_base, row_images, n_images, gh, gw, inv, grid, obs_xy, obs_cell,
                  m_conf, m_row, m_reason, status):
    """loftr_atlas_observe: record one chunk of matches and max them into the cell grid (stream-ordered, never waits).
    kpts0 / kpts1 [n,2] f32, conf [n] f32, m_bids [n] i64, mask [n] u8 or None; the remaining tensors are the atlas's storage."""
    n = kpts0.shape[0]
    for name, t, dt in (("kpts0", kpts0, torch.float32), ("kpts1", kpts1, torch.float32), ("conf", conf, torch.float32),
                        ("m_bids", m_bids, torch.int64), ("row_images", row_images, torch.int32), ("grid", grid, torch.int64),
                        ("obs_xy", obs_xy, torch.float32), ("obs_cell", obs_cell, torch.int32), ("m_conf", m_conf, torch.float32),
                        ("m_row", m_row, torch.int32), ("m_reason", m_reason, torch.uint8), ("status", status, torch.int32)) + \
            ((("mask", mask, torch.uint8),) if mask is not None else ()):
        _need(t, name, dt)
    if kpts0.shape != (n, 2) or kpts1.shape != (n, 2) or conf.shape != (n,) or m_bids.shape != (n,) or (mask is not None and mask.shape != (n,)):
        raise _lib.LoftrHipError(f"atlas_observe: expected kpts0 / kpts1 [n,2], conf / m_bids / mask [n], got {tuple(kpts0.shape)}, "
                                 f"{tuple(kpts1.shape)}, {tuple(conf.shape)}, {tuple(m_bids.shape)}")
    end = int(match_base) + n
    if obs_xy.numel() < 4 * end or obs_cell.numel() < 2 * end or min(m_conf.numel(), m_row.numel(), m_reason.numel()) < end or \
            row_images.numel() < 2 * (int(row_base) + int(n_rows)) or grid.numel() != int(n_images) * int(gh) * int(gw):
        raise _lib.LoftrHipError("atlas_observe: the atlas storage is smaller than the matches it is asked to hold")
    check(_lib.load().loftr_atlas_observe(_ptr(kpts0), _ptr(kpts1), _ptr(conf), _ptr(m_bids), _ptr(mask), n, int(n_rows), int(match_base),
                                          int(row_base), _ptr(row_images), int(n_images), int(gh), int(gw), float(inv), _ptr(grid), _ptr(obs_xy),
                                          _ptr(obs_cell), _ptr(m_conf), _ptr(m_row), _ptr(m_reason), _ptr(status), _stream()),
          "loftr_atlas_observe")


@_on_device
def atlas_finalize(grid, obs_xy, obs_cell, m_conf, m_row, m_reason, status, M, R, n_images, gh, gw, min_track_len, timings=None):
    """loftr_atlas_finalize: keypoints, index matches and tracks from the observed matches (one finalize per grid: its words become
    keypoint indices).  -> dict of device tensors of the bound sizes (see LoftrAtlasOut) with 'counts' [16] i64; nothing is read back
    here -- the caller reads counts once and trims.  timings: a list that receives (stage, ms) pairs (the call then waits for the stream)."""
    for name, t, dt in (("grid", grid, torch.int64), ("obs_xy", obs_xy, torch.float32), ("obs_cell", obs_cell, torch.int32),
                        ("m_conf", m_conf, torch.float32), ("m_row", m_row, torch.int32), ("m_reason", m_reason, torch.uint8),
                        ("status", status, torch.int32)):
        _need(t, name, dt)
    M, R = int(M), int(R)
    G = int(n_images) * int(gh) * int(gw)
    if grid.numel() != G or obs_xy.numel() < 4 * M or obs_cell.numel() < 2 * M or min(m_conf.numel(), m_row.numel(), m_reason.numel()) < M:
        raise _lib.LoftrHipError("atlas_finalize: the atlas storage is smaller than the matches it is said to hold")
    dev = grid.device
    Kb = max(1, min(2 * M, G))
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = {"kp_offsets": e(int(n_images) + 1, torch.int64), "keypoints": e((Kb, 2), torch.float32), "score": e(Kb, torch.float32),
           "n_obs": e(Kb, torch.int32), "row_offsets": e(R + 1, torch.int64), "matches": e((max(M, 1), 2), torch.int32),
           "match_conf": e(max(M, 1), torch.float32), "track_id": e(Kb, torch.int32), "track_len": e(Kb, torch.int32),
           "track_ok": e(Kb, torch.uint8), "counts": e(ATLAS_COUNTS, torch.int64)}
    lib = _lib.load()
    ws = torch.empty(max(1, lib.loftr_atlas_finalize_workspace_bytes(M, int(n_images), int(gh), int(gw))), dtype=torch.uint8, device=dev)
    st = _atlas_out(out, _ptr)
    ms = _StageMs(timings, ATLAS_STAGES)
    check(lib.loftr_atlas_finalize(_ptr(grid), _ptr(obs_xy), _ptr(obs_cell), _ptr(m_conf), _ptr(m_row), _ptr(m_reason), M, R, int(n_images),
                                   int(gh), int(gw), int(min_track_len), _ptr(status), C.byref(st), _ptr(ws), ws.numel(),
                                   ms.arg, _stream()), "loftr_atlas_finalize")
    ms.report()
    return out


# ---- triangulation of tracks (csrc/triangulate.hip, csrc/triangulate_gpu.hip) --------------------------------------------
TRI_COUNTS = 8
TRI_STATUS = ("ok", "too_short", "no_hypothesis", "small_angle", "bad_camera")            # status codes 0..4 = counts[0..4]
TRI_STAGES = ("camera_table", "solve_8", "solve_64")
_TRI_ARGS = (("offsets", "int64", 1), ("obs_image", "int32", 1), ("obs_xy", "float32", 2), ("K", "float64", 3), ("T_cam_from_world", "float64", 3))
_TRI_OUT = (("xyz", "T", (3,), "float32"), ("n_inliers", "T", (), "int32"), ("rms_px", "T", (), "float32"), ("tri_cos", "T", (), "float32"),
            ("status", "T", (), "uint8"), ("obs_inlier", "N", (), "uint8"))


def triangulation_pairs(L):
    """loftr_triangulation_pairs: the hypothesis pairs (step 2 of the rule) of a track of L observations -> list of (i, j)."""
    buf, n = (C.c_int * 128)(), C.c_int(0)
    check(_lib.load().loftr_triangulation_pairs(int(L), C.cast(buf, C.c_void_p), C.byref(n)), "loftr_triangulation_pairs")
    return [(buf[2 * h], buf[2 * h + 1]) for h in range(n.value)]


def _triangulate_tracks(B, what, hint, arrays, thresh_px, cos_min_angle, group, timings):
    _check_args(B, what, hint, _TRI_ARGS, arrays)
    offsets, obs_image, obs_xy, K, Tc = arrays
    N, n, T = obs_image.shape[0], K.shape[0], offsets.shape[0] - 1
    if T < 0 or tuple(obs_xy.shape) != (N, 2) or tuple(K.shape) != (n, 3, 3) or tuple(Tc.shape) != (n, 4, 4):
        raise _lib.LoftrHipError(f"{what}: expected offsets [T+1], obs_image [N], obs_xy [N,2], K [n,3,3] and T_cam_from_world [n,4,4], got "
                                 f"{[tuple(a.shape) for a in arrays]}")
    if int(group) not in (0, 8, 64):
        raise _lib.LoftrHipError(f"{what}: group must be 0, 8 or 64, got {group}")
    arrays = [B.contiguous(x) for x in arrays]                                           # (held until the call has returned)
    a = [B.ptr(x) for x in arrays]
    out = _outputs(B, _TRI_OUT, {"T": T, "N": N}, TRI_COUNTS, offsets)
    ms = _StageMs(timings, TRI_STAGES)
    B.call("triangulate_tracks", (a[0], T, a[1], a[2], N, a[3], a[4], n, float(thresh_px), float(cos_min_angle), *[B.ptr(out[k]) for k in out]),
           "offsets must start at 0, end at N and ascend; obs_image must lie in [0, n_images)", offsets, ws=(T, N, n), extra=(int(group),),
           tail=(ms.arg,))
    ms.report()
    return out


def triangulate_tracks_host(offsets, obs_image, obs_xy, K, T_cam_from_world, thresh_px, cos_min_angle):
    """loftr_triangulate_tracks_host: the host routine that DEFINES the triangulation (include/loftr_hip.h) on numpy arrays:
    offsets [T+1] i64, obs_image [N] i32, obs_xy [N,2] f32, K [n,3,3] f64, T_cam_from_world [n,4,4] f64.
    -> dict of numpy arrays: xyz [T,3] f32, n_inliers [T] i32, rms_px [T] f32, tri_cos [T] f32, status [T] u8, obs_inlier [N] u8,
    counts [8] i64."""
    return _triangulate_tracks(_Host, "triangulate_tracks_host", "triangulate_tracks", (offsets, obs_image, obs_xy, K, T_cam_from_world),
                               thresh_px, cos_min_angle, 0, None)


@_on_device
def triangulate_tracks(offsets, obs_image, obs_xy, K, T_cam_from_world, thresh_px, cos_min_angle, group=0, timings=None):
    """loftr_triangulate_tracks: the triangulation kernels (csrc/triangulate_gpu.hip) on GPU tensors of the dtypes and shapes of
    triangulate_tracks_host; the same result bit for bit, whatever group (0, 8 or 64) is.  -> dict of device tensors; nothing is read
    back here: bad offsets / obs_image raise bits in counts[5], which the caller reads once.  timings: a list that receives
    (stage, ms) pairs (the call then waits for the stream)."""
    return _triangulate_tracks(_Gpu, "triangulate_tracks", "the triangulation kernels have no CPU fallback; the host routine is "
                               "triangulate_tracks_host", (offsets, obs_image, obs_xy, K, T_cam_from_world), thresh_px, cos_min_angle, group,
                               timings)


# ---- bundle adjustment of the triangulated model (csrc/bundle.hip, csrc/bundle_gpu.hip) -----------------------------------
BUNDLE_COUNTS = 16
BUNDLE_STATUS = ("converged", "max_iters", "stalled", "nothing_to_adjust")               # status codes 0..3 = counts[0]
BUNDLE_ERRORS = ((1, "obs_image outside [0, n_images)"), (2, "offsets must start at 0, end at the number of observations and ascend"),
                 (4, "cam_offsets / cam_obs are not the observations grouped by image in ascending order"))     # bits of counts[1]
BUNDLE_CLASSES = ("setup", "linearise", "factor", "track_half", "camera_half", "osum", "update", "apply", "evaluate", "accept", "write")
BUNDLE_MAX_ITERS, BUNDLE_MAX_PCG = 1000, 200
_BA_ARGS = (("offsets", "int64", 1), ("obs_image", "int32", 1), ("obs_xy", "float32", 2), ("obs_mask", "uint8", 1), ("xyz", "float32", 2),
            ("K", "float64", 3), ("T_cam_from_world", "float64", 3), ("fixed", "uint8", 1), ("cam_offsets", "int64", 1), ("cam_obs", "int32", 1))
_BA_OUT = (("T_cam_from_world", "n", (4, 4), "float64"), ("xyz", "T", (3,), "float32"), ("obs_active", "N", (), "uint8"),
           ("cam_free", "n", (), "uint8"), ("point_active", "T", (), "uint8"))


def _ba_params(what, huber_px, max_iters, pcg_iters, pcg_tol, ftol):
    import math
    ok = all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in (huber_px, pcg_tol, ftol)) and \
        all(isinstance(v, int) and not isinstance(v, bool) for v in (max_iters, pcg_iters))
    if not (ok and huber_px >= 0 and ftol >= 0 and 0 <= pcg_tol < 1 and 0 <= max_iters <= BUNDLE_MAX_ITERS and 1 <= pcg_iters <= BUNDLE_MAX_PCG):
        raise ValueError(f"{what}: huber_px and ftol must be finite and >= 0, pcg_tol in [0, 1), max_iters an integer in [0, {BUNDLE_MAX_ITERS}] and "
                         f"pcg_iters an integer in [1, {BUNDLE_MAX_PCG}], got {huber_px}, {ftol}, {pcg_tol}, {max_iters}, {pcg_iters}")
    return float(huber_px), int(max_iters), int(pcg_iters), float(pcg_tol), float(ftol)


def _ba_focal_params(what, min_focal_obs, focal_lo, focal_hi):
    import math
    ok = isinstance(min_focal_obs, int) and not isinstance(min_focal_obs, bool) and \
        all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in (focal_lo, focal_hi))
    if not (ok and min_focal_obs >= 1 and math.isfinite(focal_lo) and math.isfinite(focal_hi) and focal_lo < 1 < focal_hi):
        raise ValueError(f"{what}: min_focal_obs must be an integer >= 1 and the focal bounds finite with lo < 1 < hi, got {min_focal_obs}, "
                         f"{focal_lo}, {focal_hi}")
    return int(min_focal_obs), float(focal_lo), float(focal_hi)


# bits of counts[1] of the grouped pair: BUNDLE_ERRORS and the check of the camera groups
BUNDLE_SHARED_ERRORS = BUNDLE_ERRORS + ((8, "cam_group / group_offsets / group_cams are not the images grouped by camera in ascending order"),)
# A mode (DESIGN §18 .. §18.4) is a routine pair loftr_<call>_host / loftr_<call> and ONE row of this table: the inputs after cam_obs
# (refine_focal goes after fixed in the C call, the group arrays and G after cam_obs, radial and refine_radial after G), the outputs
# after point_active, how the shape error ends, what the rule text adds, the mode's number in the pair with position priors (§18.3;
# None: the mode takes no priors), and whether its parameters end with the radial bounds.
_BA_FOCAL_IN, _BA_FOCAL_OUT = (("refine_focal", "uint8", 1),), (("K", "n", (3, 3), "float64"), ("cam_focal", "n", (), "uint8"))
_BA_GROUP_IN = _BA_FOCAL_IN + (("cam_group", "int32", 1), ("group_offsets", "int64", 1), ("group_cams", "int32", 1))
_BA_GROUP_OUT = _BA_FOCAL_OUT + (("group_focal", "G", (), "uint8"),)
_BA_GROUP_SHAPES = "cam_offsets [n+1], cam_obs [N], refine_focal [n], cam_group [n], group_offsets [G+1] with 1 <= G <= n and group_cams [n]"
_BA_GROUP_RULE = "; cam_group / group_offsets / group_cams must group the images by camera in ascending order"
_BA_MODES = {
    "bundle_adjust": ((), (), "cam_offsets [n+1] and cam_obs [N]", "", 0, False),
    "bundle_adjust_focal": (_BA_FOCAL_IN, _BA_FOCAL_OUT, "cam_offsets [n+1], cam_obs [N] and refine_focal [n]", "", 1, False),
    "bundle_adjust_shared": (_BA_GROUP_IN, _BA_GROUP_OUT, _BA_GROUP_SHAPES, _BA_GROUP_RULE, 2, False),
    "bundle_adjust_radial": (_BA_GROUP_IN + (("radial", "float64", 1), ("refine_radial", "uint8", 1)),
                             _BA_GROUP_OUT + (("radial", "n", (), "float64"), ("cam_radial", "n", (), "uint8"), ("group_radial", "G", (), "uint8")),
                             _BA_GROUP_SHAPES + ", radial [n] and refine_radial [n]", _BA_GROUP_RULE, None, True)}


def _ba_radial_params(what, radial_lo, radial_hi):
    import math
    ok = all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in (radial_lo, radial_hi))
    if not (ok and math.isfinite(radial_lo) and math.isfinite(radial_hi) and radial_lo <= radial_hi):
        raise ValueError(f"{what}: the radial bounds must be finite with lo <= hi, got {radial_lo}, {radial_hi}")
    return float(radial_lo), float(radial_hi)


# Position priors on the camera centres are one more trait of a mode: three inputs, one output, 24 counts, and ONE routine
# pair, loftr_bundle_adjust_prior(_host), that takes the arguments of the grouped pair (NULL below the mode) and the mode's number.
BUNDLE_PRIOR_COUNTS = 24
_BA_PRIOR_IN = (("prior_xyz", "float64", 2), ("prior_sigma", "float64", 2), ("prior_mask", "uint8", 1))
_BA_PRIOR_OUT = (("cam_prior", "n", (), "uint8"),)


def _bundle_adjust(B, call, arrays, params, focal, timings, prior=None, radial=None):
    """The body of all ten: the table check, the shapes, the parameters, zeroed outputs, the timing buffers (per kernel class, not per
    stage: the median launch and the total, and the launches issued), the call.  prior: None, or (prior_xyz, prior_sigma, prior_mask);
    radial: (radial_lo, radial_hi) of the mode with a radial coefficient."""
    extra_in, extra_out, shapes, rule, prior_mode, radial_bounds = _BA_MODES[call]
    name = call if prior is None else "bundle_adjust_prior"
    what, hint = (name + "_host", name) if B is _Host else \
        (name, f"the bundle-adjustment kernels have no CPU fallback; the host routine is {name}_host")
    _check_args(B, what, hint, _BA_ARGS + extra_in, arrays)
    if prior is not None:
        _check_args(B, what, hint, _BA_PRIOR_IN, prior)
    offsets, obs_image, obs_xy, obs_mask, xyz, K, Tc, fixed, cam_offsets, cam_obs = arrays[:10]
    N, n, T = obs_image.shape[0], K.shape[0], offsets.shape[0] - 1
    refine, groups, rad = arrays[10:11], arrays[11:14], arrays[14:]     # (refine_focal,), (cam_group, group_offsets, group_cams), (radial, refine_radial), or empty
    size = {"T": T, "N": N, "n": n}
    if groups:
        size["G"] = G = groups[1].shape[0] - 1
    if T < 0 or tuple(obs_xy.shape) != (N, 2) or obs_mask.shape[0] != N or tuple(xyz.shape) != (T, 3) or tuple(K.shape) != (n, 3, 3) or \
            tuple(Tc.shape) != (n, 4, 4) or fixed.shape[0] != n or cam_offsets.shape[0] != n + 1 or cam_obs.shape[0] != N or \
            any(x.shape[0] != n for x in (*refine, *groups[::2], *rad)) or (groups and (G < 0 or G > n or (n > 0 and G == 0))):
        raise _lib.LoftrHipError(f"{what}: expected offsets [T+1], obs_image [N], obs_xy [N,2], obs_mask [N], xyz [T,3], K [n,3,3], "
                                 f"T_cam_from_world [n,4,4], fixed [n], {shapes}, got {[tuple(a.shape) for a in arrays]}")
    if prior is not None and (tuple(prior[0].shape) != (n, 3) or tuple(prior[1].shape) != (n, 3) or prior[2].shape[0] != n):
        raise _lib.LoftrHipError(f"{what}: expected prior_xyz [n,3], prior_sigma [n,3] and prior_mask [n] with n = {n}, got "
                                 f"{[tuple(x.shape) for x in prior]}")
    params = _ba_params(what, *params)
    if focal is not None:
        params += _ba_focal_params(what, *focal)
    if radial_bounds:
        params += _ba_radial_params(what, *radial)
    arrays = [B.contiguous(x) for x in arrays]                                           # (held until the call has returned)
    a = [B.ptr(x) for x in arrays]
    head = (a[0], T, a[1], a[2], a[3], N, a[4], a[5], a[6], a[7])
    if prior is None:
        out = _outputs(B, _BA_OUT + extra_out, size, BUNDLE_COUNTS, offsets)
        args = (*head, *a[10:11], n, a[8], a[9], *a[11:14], *([G] if groups else []), *a[14:], *params, *[B.ptr(out[k]) for k in out])
        ws = (T, N, n)
    else:               # the pointers laid out as the grouped pair's, NULL for what the mode lacks (its parameters are ignored below mode 1)
        prior = [B.contiguous(x) for x in prior]
        a += [None] * (14 - len(a))
        out = _outputs(B, _BA_OUT + extra_out + _BA_PRIOR_OUT, size, BUNDLE_PRIOR_COUNTS, offsets)
        named = dict(out, **{k: None for k in ("K", "cam_focal", "group_focal") if k not in out})
        order = [k for k, *_ in _BA_OUT] + ["K", "cam_focal", "group_focal", "cam_prior", "counts"]
        args = (*head, a[10], n, a[8], a[9], a[11], a[12], a[13], size.get("G", 0), *[B.ptr(x) for x in prior], prior_mode,
                *(params if len(params) > 5 else params + (1, 0.5, 2.0)), *[B.ptr(named[k]) for k in order])
        ws = (T, N, n, prior_mode)
    ms = (C.c_float * (2 * len(BUNDLE_CLASSES)))() if timings is not None else None
    launches = (C.c_long * len(BUNDLE_CLASSES))() if timings is not None else None
    cast = lambda x: C.cast(x, C.c_void_p) if x is not None else None
    B.call(name, args, _TABLE_RULES + rule, offsets, ws=ws, tail=(cast(ms), cast(launches)))
    if timings is not None:
        timings.update({name: (float(ms[2 * k]), float(ms[2 * k + 1]), int(launches[k])) for k, name in enumerate(BUNDLE_CLASSES)})
    return out


def _ba_prior_call(B, mode, base, refine_focal, groups, prior, params, focal, timings):
    """The row of _BA_MODES whose number in the prior pair is `mode`: 0 pose, 1 focal, 2 shared."""
    if mode not in (0, 1, 2):
        raise ValueError(f"bundle_adjust_prior: mode must be 0 (pose), 1 (focal) or 2 (shared), got {mode!r}")
    call = {row[4]: call for call, row in _BA_MODES.items()}[mode]
    arrays = tuple(base) + ((refine_focal,) if mode >= 1 else ()) + (tuple(groups) if mode == 2 else ())
    return _bundle_adjust(B, call, arrays, params, focal if mode >= 1 else None, timings, prior=tuple(prior))


def bundle_adjust_prior_host(mode, offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal,
                             cam_group, group_offsets, group_cams, prior_xyz, prior_sigma, prior_mask, huber_px, max_iters, pcg_iters,
                             pcg_tol, ftol, min_focal_obs=20, focal_lo=0.5, focal_hi=2.0):
    """loftr_bundle_adjust_prior_host: the host routine that DEFINES the bundle adjustment with position priors on the camera centres
    (include/loftr_hip.h) on numpy arrays.  mode 0, 1, 2: the rule of bundle_adjust_host, _focal_host, _shared_host with
    the prior term; refine_focal (mode 0) and the group arrays (mode < 2) are ignored and may be None.  prior_xyz [n,3] f64,
    prior_sigma [n,3] f64, prior_mask [n] u8.  -> the mode's dict plus cam_prior [n] u8; counts [24] i64."""
    return _ba_prior_call(_Host, mode, (offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs), refine_focal,
                          (cam_group, group_offsets, group_cams), (prior_xyz, prior_sigma, prior_mask),
                          (huber_px, max_iters, pcg_iters, pcg_tol, ftol), (min_focal_obs, focal_lo, focal_hi), None)


@_on_device
def bundle_adjust_prior(mode, offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal,
                        cam_group, group_offsets, group_cams, prior_xyz, prior_sigma, prior_mask, huber_px, max_iters, pcg_iters, pcg_tol,
                        ftol, min_focal_obs=20, focal_lo=0.5, focal_hi=2.0, timings=None):
    """loftr_bundle_adjust_prior: the kernels (csrc/bundle_gpu.hip) on GPU tensors; the same result as bundle_adjust_prior_host bit for
    bit, the same launch schedule, timing classes and single readback as bundle_adjust."""
    return _ba_prior_call(_Gpu, mode, (offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs), refine_focal,
                          (cam_group, group_offsets, group_cams), (prior_xyz, prior_sigma, prior_mask),
                          (huber_px, max_iters, pcg_iters, pcg_tol, ftol), (min_focal_obs, focal_lo, focal_hi), timings)


def bundle_adjust_host(offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, huber_px, max_iters,
                       pcg_iters, pcg_tol, ftol):
    """loftr_bundle_adjust_host: the host routine that DEFINES the bundle adjustment (include/loftr_hip.h) on numpy arrays: offsets [T+1]
    i64, obs_image [N] i32, obs_xy [N,2] f32, obs_mask [N] u8, xyz [T,3] f32, K [n,3,3] f64, T_cam_from_world [n,4,4] f64, fixed [n] u8,
    cam_offsets [n+1] i64, cam_obs [N] i32.  -> dict of numpy arrays: T_cam_from_world [n,4,4] f64, xyz [T,3] f32, obs_active [N] u8,
    cam_free [n] u8, point_active [T] u8, counts [16] i64."""
    return _bundle_adjust(_Host, "bundle_adjust", (offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs),
                          (huber_px, max_iters, pcg_iters, pcg_tol, ftol), None, None)


@_on_device
def bundle_adjust(offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, huber_px, max_iters, pcg_iters,
                  pcg_tol, ftol, timings=None):
    """loftr_bundle_adjust: the bundle-adjustment kernels (csrc/bundle_gpu.hip) on GPU tensors of the dtypes and shapes of
    bundle_adjust_host; the same result bit for bit.  -> dict of device tensors; nothing is read back here: the error bits are in
    counts[1], which the caller reads once.  timings: a dict that receives per kernel class (BUNDLE_CLASSES) the tuple
    (median ms of a launch, total ms, launches issued); the call then waits for the stream."""
    return _bundle_adjust(_Gpu, "bundle_adjust", (offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs),
                          (huber_px, max_iters, pcg_iters, pcg_tol, ftol), None, timings)


def bundle_adjust_focal_host(offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal,
                             huber_px, max_iters, pcg_iters, pcg_tol, ftol, min_focal_obs, focal_lo, focal_hi):
    """loftr_bundle_adjust_focal_host: the host routine that DEFINES the bundle adjustment with focal refinement (include/loftr_hip.h;
    DESIGN §18.1) on numpy arrays: those of bundle_adjust_host plus refine_focal [n] u8.  -> its dict plus K [n,3,3] f64 and
    cam_focal [n] u8; counts[13] is the number of cameras that refine their focal."""
    return _bundle_adjust(_Host, "bundle_adjust_focal",
                          (offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal),
                          (huber_px, max_iters, pcg_iters, pcg_tol, ftol), (min_focal_obs, focal_lo, focal_hi), None)


@_on_device
def bundle_adjust_focal(offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal, huber_px,
                        max_iters, pcg_iters, pcg_tol, ftol, min_focal_obs, focal_lo, focal_hi, timings=None):
    """loftr_bundle_adjust_focal: the kernels of the 7-wide camera block (csrc/bundle_gpu.hip) on GPU tensors; the same result as
    bundle_adjust_focal_host bit for bit, the same launch schedule, timing classes and single readback as bundle_adjust."""
    return _bundle_adjust(_Gpu, "bundle_adjust_focal",
                          (offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal),
                          (huber_px, max_iters, pcg_iters, pcg_tol, ftol), (min_focal_obs, focal_lo, focal_hi), timings)


def bundle_adjust_shared_host(offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal,
                              cam_group, group_offsets, group_cams, huber_px, max_iters, pcg_iters, pcg_tol, ftol, min_focal_obs, focal_lo,
                              focal_hi):
    """loftr_bundle_adjust_shared_host: the host routine that DEFINES the bundle adjustment with one focal step per group of images
    (include/loftr_hip.h) on numpy arrays: those of bundle_adjust_focal_host plus cam_group [n] i32, group_offsets [G+1] i64,
    group_cams [n] i32.  -> its dict plus group_focal [G] u8; counts[14] is the number of groups that refine."""
    return _bundle_adjust(_Host, "bundle_adjust_shared",
                          (offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal, cam_group,
                           group_offsets, group_cams),
                          (huber_px, max_iters, pcg_iters, pcg_tol, ftol), (min_focal_obs, focal_lo, focal_hi), None)


@_on_device
def bundle_adjust_shared(offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal, cam_group,
                         group_offsets, group_cams, huber_px, max_iters, pcg_iters, pcg_tol, ftol, min_focal_obs, focal_lo, focal_hi,
                         timings=None):
    """loftr_bundle_adjust_shared: the kernels of the grouped focal step (csrc/bundle_gpu.hip) on GPU tensors; the same result as
    bundle_adjust_shared_host bit for bit, the same timing classes and single readback as bundle_adjust."""
    return _bundle_adjust(_Gpu, "bundle_adjust_shared",
                          (offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal, cam_group,
                           group_offsets, group_cams),
                          (huber_px, max_iters, pcg_iters, pcg_tol, ftol), (min_focal_obs, focal_lo, focal_hi), timings)


def bundle_adjust_radial_host(offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal,
                              cam_group, group_offsets, group_cams, radial, refine_radial, huber_px, max_iters, pcg_iters, pcg_tol, ftol,
                              min_focal_obs, focal_lo, focal_hi, radial_lo, radial_hi):
    """loftr_bundle_adjust_radial_host: the host routine that DEFINES the bundle adjustment with one focal step and one radial coefficient
    per group of images (include/loftr_hip.h) on numpy arrays: those of bundle_adjust_shared_host plus radial [n] f64 (the
    start values) and refine_radial [n] u8.  -> its dict plus radial [n] f64, cam_radial [n] u8 and group_radial [G] u8; counts[15] is the
    number of images that refine their radial coefficient."""
    return _bundle_adjust(_Host, "bundle_adjust_radial",
                          (offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal, cam_group,
                           group_offsets, group_cams, radial, refine_radial),
                          (huber_px, max_iters, pcg_iters, pcg_tol, ftol), (min_focal_obs, focal_lo, focal_hi), None, radial=(radial_lo, radial_hi))


@_on_device
def bundle_adjust_radial(offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal, cam_group,
                         group_offsets, group_cams, radial, refine_radial, huber_px, max_iters, pcg_iters, pcg_tol, ftol, min_focal_obs,
                         focal_lo, focal_hi, radial_lo, radial_hi, timings=None):
    """loftr_bundle_adjust_radial: the kernels of the grouped focal and radial steps (csrc/bundle_gpu.hip) on GPU tensors; the same result
    as bundle_adjust_radial_host bit for bit, the same timing classes and single readback as bundle_adjust."""
    return _bundle_adjust(_Gpu, "bundle_adjust_radial",
                          (offsets, obs_image, obs_xy, obs_mask, xyz, K, T_cam_from_world, fixed, cam_offsets, cam_obs, refine_focal, cam_group,
                           group_offsets, group_cams, radial, refine_radial),
                          (huber_px, max_iters, pcg_iters, pcg_tol, ftol), (min_focal_obs, focal_lo, focal_hi), timings, radial=(radial_lo, radial_hi))


# ---- pixels without the radial coefficient of their camera (csrc/radial_core.h, csrc/undistort.hip, csrc/undistort_gpu.hip) ----
UNDISTORT_COUNTS = 8
UNDISTORT_ERRORS = ((1, "image outside [0, n_images)"),)                                  # bits of counts[1]
_UND_ARGS = (("xy", "float32", 2), ("image", "int32", 1), ("K", "float64", 3), ("radial", "float64", 1))


def _undistort(B, name, arrays):
    what, hint = (name + "_host", name) if B is _Host else (name, f"the kernel has no CPU fallback; the host routine is {name}_host")
    _check_args(B, what, hint, _UND_ARGS, arrays)
    xy, image, K, radial = arrays
    M, n = xy.shape[0], K.shape[0]
    if tuple(xy.shape) != (M, 2) or image.shape[0] != M or tuple(K.shape) != (n, 3, 3) or radial.shape[0] != n:
        raise _lib.LoftrHipError(f"{what}: expected xy [M,2], image [M], K [n,3,3] and radial [n], got {[tuple(a.shape) for a in arrays]}")
    arrays = [B.contiguous(x) for x in arrays]                                           # (held until the call has returned)
    a = [B.ptr(x) for x in arrays]
    out = {"xy": B.zeros((M, 2), "float32", xy), "ok": B.zeros((M,), "uint8", xy), "counts": B.zeros(UNDISTORT_COUNTS, "int64", xy)}
    args = (a[0], a[1], M, a[2], a[3], n, *[B.ptr(out[k]) for k in out])
    if B is _Host:
        status = getattr(_lib.load(), f"loftr_{name}_host")(*args)
        if not (status == -1 and int(out["counts"][1]) != 0):                            # a bad image is reported through counts[1], as on the GPU
            check(status, f"loftr_{name}_host")
    else:
        B.call(name, args, "", xy)
    return out


def undistort_points_host(xy, image, K, radial):
    """loftr_undistort_points_host: the host routine that DEFINES the pinhole pixels of distorted ones (include/loftr_hip.h)
    on numpy arrays: xy [M,2] f32, image [M] i32, K [n,3,3] f64, radial [n] f64.  -> dict of numpy arrays: xy [M,2] f32 (NaN where not
    ok), ok [M] u8, counts [8] i64 (points ok, error bits, points not ok)."""
    return _undistort(_Host, "undistort_points", (xy, image, K, radial))


def distort_points_host(xy, image, K, radial):
    """loftr_distort_points_host: the other direction from the same text (pinhole pixels -> distorted ones); arguments and result as
    undistort_points_host."""
    return _undistort(_Host, "distort_points", (xy, image, K, radial))


@_on_device
def undistort_points(xy, image, K, radial):
    """loftr_undistort_points: the kernel (csrc/undistort_gpu.hip, a thread per point) on GPU tensors; the same result as
    undistort_points_host bit for bit.  Nothing is read back here: the error bit is in counts[1], which the caller reads once."""
    return _undistort(_Gpu, "undistort_points", (xy, image, K, radial))


# ---- correspondence table of the images without a pose (csrc/register.hip, csrc/register_gpu.hip) --------------------------
REGISTER_COUNTS = 8
REGISTER_STAGES = ("track", "count", "rank", "write")
REGISTER_RANK_BLOCK = 256
REGISTER_MIN_CORR = 4
REGISTER_ERRORS = BUNDLE_ERRORS                                                          # bits of counts[2]
_REG_ARGS = (("offsets", "int64", 1), ("obs_image", "int32", 1), ("obs_xy", "float32", 2), ("xyz", "float32", 2), ("status", "uint8", 1),
             ("posed", "uint8", 1), ("cam_offsets", "int64", 1), ("cam_obs", "int32", 1))
_REG_OUT = (("n_corr", "n", (), "int32"), ("cand_rank", "n", (), "int32"), ("cand_image", "n", (), "int32"), ("cand_offsets", "n1", (), "int64"),
            ("corr_xyz", "N", (3,), "float32"), ("corr_xy", "N", (2,), "float32"), ("corr_bid", "N", (), "int64"), ("corr_obs", "N", (), "int32"))


def _register_corr(B, what, hint, arrays, min_corr, timings):
    _check_args(B, what, hint, _REG_ARGS, arrays)
    offsets, obs_image, obs_xy, xyz, status, posed, cam_offsets, cam_obs = arrays
    N, n, T = obs_image.shape[0], posed.shape[0], offsets.shape[0] - 1
    if T < 0 or tuple(obs_xy.shape) != (N, 2) or tuple(xyz.shape) != (T, 3) or status.shape[0] != T or cam_offsets.shape[0] != n + 1 or \
            cam_obs.shape[0] != N:
        raise _lib.LoftrHipError(f"{what}: expected offsets [T+1], obs_image [N], obs_xy [N,2], xyz [T,3], status [T], posed [n], "
                                 f"cam_offsets [n+1] and cam_obs [N], got {[tuple(a.shape) for a in arrays]}")
    if not isinstance(min_corr, int) or isinstance(min_corr, bool) or min_corr < REGISTER_MIN_CORR:
        raise ValueError(f"{what}: min_corr must be an integer >= {REGISTER_MIN_CORR}, got {min_corr}")
    arrays = [B.contiguous(x) for x in arrays]                                           # (held until the call has returned)
    a = [B.ptr(x) for x in arrays]
    out = _outputs(B, _REG_OUT, {"n": n, "n1": n + 1, "N": N}, REGISTER_COUNTS, offsets)
    ms = _StageMs(timings, REGISTER_STAGES)
    B.call("register_corr", (a[0], T, a[1], a[2], N, a[3], a[4], a[5], n, a[6], a[7], int(min_corr), *[B.ptr(out[k]) for k in out]),
           _TABLE_RULES, offsets, ws=(T, N, n), tail=(ms.arg,))
    ms.report()
    return out


def register_corr_host(offsets, obs_image, obs_xy, xyz, status, posed, cam_offsets, cam_obs, min_corr):
    """loftr_register_corr_host: the host routine that DEFINES the correspondence table of the unposed images (include/loftr_hip.h) on
    numpy arrays: offsets [T+1] i64, obs_image [N] i32, obs_xy [N,2] f32, xyz [T,3] f32, status [T] u8, posed [n] u8, cam_offsets [n+1]
    i64, cam_obs [N] i32.  -> dict of numpy arrays sized by the bounds (n_corr, cand_rank, cand_image [n] i32, cand_offsets [n+1] i64,
    corr_xyz [N,3] f32, corr_xy [N,2] f32, corr_bid [N] i64, corr_obs [N] i32; rows past counts[1] / counts[0] are zero) and counts [8]
    i64."""
    return _register_corr(_Host, "register_corr_host", "register_corr", (offsets, obs_image, obs_xy, xyz, status, posed, cam_offsets, cam_obs),
                          min_corr, None)


@_on_device
def register_corr(offsets, obs_image, obs_xy, xyz, status, posed, cam_offsets, cam_obs, min_corr, timings=None):
    """loftr_register_corr: the kernels of the correspondence table (csrc/register_gpu.hip) on GPU tensors of the dtypes and shapes of
    register_corr_host; the same result bit for bit.  -> dict of device tensors; nothing is read back here: the error bits are in
    counts[2], C and P in counts[0] and counts[1], which the caller reads once.  timings: a list that receives (stage, ms) pairs (the
    call then waits for the stream)."""
    return _register_corr(_Gpu, "register_corr", "the correspondence-table kernels have no CPU fallback; the host routine is register_corr_host",
                          (offsets, obs_image, obs_xy, xyz, status, posed, cam_offsets, cam_obs), min_corr, timings)


# ---- track completion (csrc/complete.hip, csrc/complete_gpu.hip) -----------------------------------------------------------
COMPLETE_COUNTS = 8
COMPLETE_NAMES = ("n_links", "error_bits", "n_sources", "n_pairs", "n_inside", "n_proposals", "n_lost", "n_blocked")      # counts[0..7]
COMPLETE_MAX_REACH = 8
COMPLETE_STAGES = ("camera_table", "check", "link", "resolve")
COMPLETE_ERRORS = BUNDLE_ERRORS[:2] + ((4, "obs_image must not descend within a row"), (8, "kp_row outside [-1, T)"))    # bits of counts[1]
_CPL_ARGS = (("offsets", "int64", 1), ("obs_image", "int32", 1), ("xyz", "float32", 2), ("status", "uint8", 1), ("kp_offsets", "int64", 1),
             ("keypoints", "float32", 2), ("kp_cell", "int32", 1), ("kp_row", "int32", 1), ("K", "float64", 3), ("T_cam_from_world", "float64", 3),
             ("posed", "uint8", 1))
_CPL_OUT = (("kp_row_new", "K", (), "int32"), ("link_r2", "K", (), "float32"))


def _complete_tracks(B, what, hint, arrays, gh, gw, inv, thresh_px, reach, timings):
    _check_args(B, what, hint, _CPL_ARGS, arrays)
    offsets, obs_image, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, Tc, posed = arrays
    N, n, T, Kp = obs_image.shape[0], posed.shape[0], offsets.shape[0] - 1, keypoints.shape[0]
    if T < 0 or tuple(xyz.shape) != (T, 3) or status.shape[0] != T or kp_offsets.shape[0] != n + 1 or tuple(keypoints.shape) != (Kp, 2) or \
            kp_cell.shape[0] != Kp or kp_row.shape[0] != Kp or tuple(K.shape) != (n, 3, 3) or tuple(Tc.shape) != (n, 4, 4):
        raise _lib.LoftrHipError(f"{what}: expected offsets [T+1], obs_image [N], xyz [T,3], status [T], kp_offsets [n+1], keypoints [K,2], kp_cell "
                                 f"/ kp_row [K], K [n,3,3], T_cam_from_world [n,4,4] and posed [n], got {[tuple(a.shape) for a in arrays]}")
    if not isinstance(reach, int) or isinstance(reach, bool) or not 0 <= reach <= COMPLETE_MAX_REACH:
        raise ValueError(f"{what}: reach must be an integer in [0, {COMPLETE_MAX_REACH}], got {reach}")
    if not (float(thresh_px) >= 0 and float(thresh_px) < float("inf")) or min(int(gh), int(gw)) < 0:
        raise ValueError(f"{what}: thresh_px must be finite and >= 0 and the grid gh x gw >= 0, got {thresh_px}, {gh} x {gw}")
    arrays = [B.contiguous(x) for x in arrays]                                           # (held until the call has returned)
    a = [B.ptr(x) for x in arrays]
    out = _outputs(B, _CPL_OUT, {"K": Kp}, COMPLETE_COUNTS, offsets)
    ms = _StageMs(timings, COMPLETE_STAGES)
    B.call("complete_tracks", (a[0], T, a[1], N, a[2], a[3], a[4], a[5], a[6], a[7], Kp, a[8], a[9], a[10], n, float(inv), int(gh), int(gw),
                               float(thresh_px), reach, *[B.ptr(out[k]) for k in out]),
           "offsets / kp_offsets must start at 0, end at N / K and ascend; obs_image must lie in [0, n_images) and not descend within a row; "
           "kp_row must lie in [-1, T)", offsets, ws=(T, N, Kp, n), tail=(ms.arg,))
    ms.report()
    return out


def complete_tracks_host(offsets, obs_image, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, T_cam_from_world, posed, gh, gw, inv,
                         thresh_px, reach):
    """loftr_complete_tracks_host: the host routine that DEFINES track completion (include/loftr_hip.h) on numpy arrays: offsets [T+1] i64,
    obs_image [N] i32, xyz [T,3] f32, status [T] u8, kp_offsets [n+1] i64, keypoints [K,2] f32, kp_cell / kp_row [K] i32, K [n,3,3] f64,
    T_cam_from_world [n,4,4] f64, posed [n] u8; the atlas grid (gh, gw, inv), thresh_px and reach (0 .. COMPLETE_MAX_REACH cells).
    -> dict of numpy arrays: kp_row_new [K] i32, link_r2 [K] f32 (NaN where there is no link), counts [8] i64 (COMPLETE_NAMES)."""
    return _complete_tracks(_Host, "complete_tracks_host", "complete_tracks",
                            (offsets, obs_image, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, T_cam_from_world, posed), gh, gw, inv,
                            thresh_px, reach, None)


@_on_device
def complete_tracks(offsets, obs_image, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, T_cam_from_world, posed, gh, gw, inv, thresh_px,
                    reach, timings=None):
    """loftr_complete_tracks: the completion kernels (csrc/complete_gpu.hip) on GPU tensors of the dtypes and shapes of
    complete_tracks_host; the same result bit for bit.  -> dict of device tensors; nothing is read back here: the error bits are in
    counts[1], which the caller reads once (kp_row_new is then kp_row).  timings: a list that receives (stage, ms) pairs (the call then
    waits for the stream)."""
    return _complete_tracks(_Gpu, "complete_tracks", "the completion kernels have no CPU fallback; the host routine is complete_tracks_host",
                            (offsets, obs_image, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, T_cam_from_world, posed), gh, gw, inv,
                            thresh_px, reach, timings)


# ---- track merging (csrc/merge.hip, csrc/merge_gpu.hip) ------------------------------------------------------------------------
MERGE_COUNTS = 8
MERGE_NAMES = ("n_merges", "error_bits", "n_sources", "n_pairs", "n_meetings", "n_disjoint", "n_accepted", "n_relabelled")   # counts[0..7]
MERGE_STAGES = ("camera_table", "check", "meet", "pair", "relabel")
_MRG_ARGS = (("offsets", "int64", 1), ("obs_image", "int32", 1), ("obs_xy", "float32", 2), ("obs_mask", "uint8", 1)) + _CPL_ARGS[2:]
_MRG_OUT = (("row_into", "T", (), "int32"), ("merge_r2", "T", (), "float32"), ("kp_row_new", "K", (), "int32"))


def _merge_tracks(B, what, hint, arrays, gh, gw, inv, thresh_px, reach, timings):
    _check_args(B, what, hint, _MRG_ARGS, arrays)
    offsets, obs_image, obs_xy, obs_mask, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, Tc, posed = arrays
    N, n, T, Kp = obs_image.shape[0], posed.shape[0], offsets.shape[0] - 1, keypoints.shape[0]
    if T < 0 or tuple(obs_xy.shape) != (N, 2) or obs_mask.shape[0] != N or tuple(xyz.shape) != (T, 3) or status.shape[0] != T or \
            kp_offsets.shape[0] != n + 1 or tuple(keypoints.shape) != (Kp, 2) or kp_cell.shape[0] != Kp or kp_row.shape[0] != Kp or \
            tuple(K.shape) != (n, 3, 3) or tuple(Tc.shape) != (n, 4, 4):
        raise _lib.LoftrHipError(f"{what}: expected offsets [T+1], obs_image [N], obs_xy [N,2], obs_mask [N], xyz [T,3], status [T], kp_offsets "
                                 f"[n+1], keypoints [K,2], kp_cell / kp_row [K], K [n,3,3], T_cam_from_world [n,4,4] and posed [n], got "
                                 f"{[tuple(a.shape) for a in arrays]}")
    if not isinstance(reach, int) or isinstance(reach, bool) or not 0 <= reach <= COMPLETE_MAX_REACH:
        raise ValueError(f"{what}: reach must be an integer in [0, {COMPLETE_MAX_REACH}], got {reach}")
    if not (float(thresh_px) >= 0 and float(thresh_px) < float("inf")) or min(int(gh), int(gw)) < 0:
        raise ValueError(f"{what}: thresh_px must be finite and >= 0 and the grid gh x gw >= 0, got {thresh_px}, {gh} x {gw}")
    arrays = [B.contiguous(x) for x in arrays]                                           # (held until the call has returned)
    a = [B.ptr(x) for x in arrays]
    out = _outputs(B, _MRG_OUT, {"T": max(T, 0), "K": Kp}, MERGE_COUNTS, offsets)
    ms = _StageMs(timings, MERGE_STAGES)
    B.call("merge_tracks", (a[0], T, a[1], a[2], a[3], N, a[4], a[5], a[6], a[7], a[8], a[9], Kp, a[10], a[11], a[12], n, float(inv), int(gh),
                            int(gw), float(thresh_px), reach, *[B.ptr(out[k]) for k in out]),
           "offsets / kp_offsets must start at 0, end at N / K and ascend; obs_image must lie in [0, n_images) and not descend within a row; "
           "kp_row must lie in [-1, T)", offsets, ws=(T, N, Kp, n), tail=(ms.arg,))
    ms.report()
    return out


def merge_tracks_host(offsets, obs_image, obs_xy, obs_mask, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, T_cam_from_world, posed,
                      gh, gw, inv, thresh_px, reach):
    """loftr_merge_tracks_host: the host routine that DEFINES track merging (include/loftr_hip.h) on numpy arrays: those of
    complete_tracks_host plus obs_xy [N,2] f32 and obs_mask [N] u8 after obs_image.
    -> dict of numpy arrays: row_into [T] i32, merge_r2 [T] f32 (NaN where the row does not merge), kp_row_new [K] i32, counts [8] i64
    (MERGE_NAMES)."""
    return _merge_tracks(_Host, "merge_tracks_host", "merge_tracks",
                         (offsets, obs_image, obs_xy, obs_mask, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, T_cam_from_world, posed),
                         gh, gw, inv, thresh_px, reach, None)


@_on_device
def merge_tracks(offsets, obs_image, obs_xy, obs_mask, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, T_cam_from_world, posed, gh, gw,
                 inv, thresh_px, reach, timings=None):
    """loftr_merge_tracks: the merging kernels (csrc/merge_gpu.hip) on GPU tensors of the dtypes and shapes of merge_tracks_host; the same
    result bit for bit.  -> dict of device tensors; nothing is read back here: the error bits are in counts[1], which the caller reads
    once (row_into is then the identity, kp_row_new is kp_row).  timings: a list that receives (stage, ms) pairs (the call then waits for
    the stream)."""
    return _merge_tracks(_Gpu, "merge_tracks", "the merging kernels have no CPU fallback; the host routine is merge_tracks_host",
                         (offsets, obs_image, obs_xy, obs_mask, xyz, status, kp_offsets, keypoints, kp_cell, kp_row, K, T_cam_from_world, posed),
                         gh, gw, inv, thresh_px, reach, timings)


# ---- track splitting (csrc/split.hip, csrc/split_gpu.hip) ------------------------------------------------------------------
SPLIT_COUNTS = 16
SPLIT_NAMES = ("n_tracks", "error_bits", "n_ignored", "n_internal", "n_conflict", "n_open", "n_inconsistent_tracks", "n_inconsistent_keypoints",
               "n_rescued", "n_rounds", "largest_component")                                # counts[0..10]
SPLIT_STATES = ("ignored", "internal", "conflict", "open")                               # edge_state codes 0..3
SPLIT_STAGES = ("check", "clear", "propose", "accept", "merge", "number", "write")       # the launch classes; a round's four are summed
SPLIT_ERRORS = ((1, "edge_kp outside [0, K)"), (2, "track_id outside [-1, T) or kp_image outside [0, n_images)"),
                (4, "kp_image must not descend (keypoints are ordered by image)"), (8, "edge_conf must be finite and >= 0"),
                (16, "a member list longer than n_images"))                              # bits of counts[1]
_SPL_ARGS = (("edge_kp", "int32", 2), ("edge_conf", "float32", 1), ("kp_image", "int32", 1), ("track_id", "int32", 1), ("track_ok", "uint8", 1))
_SPL_OUT = (("track_id_new", "K", (), "int32"), ("track_len_new", "K", (), "int32"), ("edge_state", "E", (), "uint8"),
            ("round_accepted", "R", (), "int32"))


def _split_tracks(B, what, hint, arrays, n_images, min_track_len, max_rounds, timings):
    _check_args(B, what, hint, _SPL_ARGS, arrays)
    edge_kp, edge_conf, kp_image, track_id, track_ok = arrays
    E, K, T = edge_kp.shape[0], kp_image.shape[0], track_ok.shape[0]
    if tuple(edge_kp.shape) != (E, 2) or edge_conf.shape[0] != E or track_id.shape[0] != K:
        raise _lib.LoftrHipError(f"{what}: expected edge_kp [E,2], edge_conf [E], kp_image [K], track_id [K] and track_ok [T], got "
                                 f"{[tuple(a.shape) for a in arrays]}")
    for name, v, lo in (("n_images", n_images, 0), ("min_track_len", min_track_len, 1), ("max_rounds", max_rounds, 0)):
        if not isinstance(v, int) or isinstance(v, bool) or v < lo:
            raise ValueError(f"{what}: {name} must be an integer >= {lo}, got {v}")
    arrays = [B.contiguous(x) for x in arrays]                                           # (held until the call has returned)
    a = [B.ptr(x) for x in arrays]
    out = _outputs(B, _SPL_OUT, {"K": K, "E": E, "R": max_rounds}, SPLIT_COUNTS, edge_kp)
    args = (a[0], a[1], E, a[2], a[3], K, a[4], T, n_images, min_track_len, max_rounds, *[B.ptr(out[k]) for k in out])
    if B is _Host:
        status = _lib.load().loftr_split_tracks_host(*args)
        if not (status == -1 and int(out["counts"][1]) != 0):                            # a bad table is reported through counts[1], as on the GPU
            check(status, "loftr_split_tracks_host")
        return out
    stages = ("check",) + ("clear", "propose", "accept", "merge") * max_rounds + ("number", "write")
    ms = _StageMs(None if timings is None else [], stages)
    B.call("split_tracks", args, "", edge_kp, ws=(E, K, T, max_rounds), tail=(ms.arg,))
    if timings is not None:
        ms.report()
        timings.extend((name, sum(v for n, v in ms.timings if n == name)) for name in SPLIT_STAGES)
    return out


def split_tracks_host(edge_kp, edge_conf, kp_image, track_id, track_ok, n_images, min_track_len=2, max_rounds=32):
    """loftr_split_tracks_host: the host routine that DEFINES track splitting (include/loftr_hip.h) on numpy arrays: edge_kp
    [E,2] i32 (global keypoint indices), edge_conf [E] f32, kp_image [K] i32 (not descending), track_id [K] i32, track_ok [T] u8.
    -> dict of numpy arrays: track_id_new [K] i32, track_len_new [K] i32 (the first counts[0] entries), edge_state [E] u8 (SPLIT_STATES),
    round_accepted [max_rounds] i32, counts [16] i64 (SPLIT_NAMES).  A bad table leaves its bits in counts[1] and every other output
    zero."""
    return _split_tracks(_Host, "split_tracks_host", "split_tracks", (edge_kp, edge_conf, kp_image, track_id, track_ok), n_images,
                         min_track_len, max_rounds, None)


@_on_device
def split_tracks(edge_kp, edge_conf, kp_image, track_id, track_ok, n_images, min_track_len=2, max_rounds=32, timings=None):
    """loftr_split_tracks: the splitting kernels (csrc/split_gpu.hip) on GPU tensors of the dtypes and shapes of split_tracks_host; the
    same result bit for bit.  -> dict of device tensors; nothing is read back here: the error bits are in counts[1], which the caller
    reads once (every other output is then zero).  timings: a list that receives (launch class, ms) pairs, the rounds summed (the call
    then waits for the stream)."""
    return _split_tracks(_Gpu, "split_tracks", "the splitting kernels have no CPU fallback; the host routine is split_tracks_host",
                         (edge_kp, edge_conf, kp_image, track_id, track_ok), n_images, min_track_len, max_rounds, timings)


# ---- rotation averaging over the view graph (csrc/rotation.hip, csrc/rotation_gpu.hip) ------------------------------------
ROTATION_COUNTS = 16
ROTATION_NAMES = ("n_in_graph", "error_bits", "n_invalid", "n_duplicate", "n_used", "support_sum", "n_tree", "n_tree_unsupported", "tree_depth",
                  "n_components", "n_iters", "n_pcg_iters", "n_ok", "n_outlier", "status", "root")          # counts[0..15]
ROTATION_INFO = ("cost_start", "cost_end", "last_step", "max_ok_chord")                  # info[0..3]
ROTATION_STATES = ("invalid", "outside", "ok", "outlier")                                # edge_state codes 0..3
ROTATION_STATUS = ("converged", "max_iters", "stalled", "nothing")                       # counts[14]
ROTATION_STAGES = ("check", "support", "tree", "start", "refine", "write")
ROTATION_ERRORS = ((1, "edge_image outside [0, n_images)"), (2, "an edge that joins an image to itself"),
                   (4, "adj_offsets / adj_edge must group the edges by image with neighbours ascending, one used edge per pair"),
                   (8, "root outside [-1, n_images)"))                                   # bits of counts[1]
_ROT_ARGS = (("edge_image", "int32", 2), ("edge_R", "float64", 3), ("edge_weight", "int32", 1), ("adj_offsets", "int64", 1),
             ("adj_edge", "int32", 1), ("edge_use", "uint8", 1))
_ROT_OUT = (("R", "n", (3, 3), "float64"), ("in_graph", "n", (), "uint8"), ("edge_state", "E", (), "uint8"), ("edge_chord", "E", (), "float64"),
            ("support", "E", (), "int32"), ("tree", "E", (), "uint8"), ("edge_use", "E", (), "uint8"))


def _rotation_averaging(B, what, hint, arrays, n_images, root, cycle_cos_half, loss_chord, max_chord, step_tol, max_iters, pcg_iters, pcg_tol,
                        timings):
    _check_args(B, what, hint, _ROT_ARGS, arrays)
    edge_image, edge_R, edge_weight, adj_offsets, adj_edge, edge_use = arrays
    E = edge_image.shape[0]
    for name, v, lo in (("n_images", n_images, 0), ("root", root, -(1 << 31)), ("max_iters", max_iters, 0), ("pcg_iters", pcg_iters, 0)):
        if not isinstance(v, int) or isinstance(v, bool) or v < lo:
            raise ValueError(f"{what}: {name} must be an integer >= {lo}, got {v}")
    if (tuple(edge_image.shape) != (E, 2) or tuple(edge_R.shape) != (E, 3, 3) or edge_weight.shape[0] != E or adj_edge.shape[0] != 2 * E
            or adj_offsets.shape[0] != n_images + 1 or edge_use.shape[0] != E):
        raise _lib.LoftrHipError(f"{what}: expected edge_image [E,2], edge_R [E,3,3], edge_weight [E], adj_offsets [n_images + 1], adj_edge "
                                 f"[2E] and edge_use [E], got {[tuple(a.shape) for a in arrays]}")
    arrays = [B.contiguous(x) for x in arrays]                                           # (held until the call has returned)
    a = [B.ptr(x) for x in arrays]
    out = _outputs(B, _ROT_OUT, {"n": n_images, "E": E}, ROTATION_COUNTS, edge_image)
    out["info"] = B.zeros(len(ROTATION_INFO), "float64", edge_image)
    args = (a[0], a[1], a[2], E, n_images, root, a[3], a[4], a[5], float(cycle_cos_half), float(loss_chord), float(max_chord), float(step_tol),
            max_iters, pcg_iters, float(pcg_tol), *[B.ptr(out[k]) for k in out])
    if B is _Host:
        status = _lib.load().loftr_rotation_averaging_host(*args)
        if not (status == -1 and int(out["counts"][1]) != 0):                            # a bad graph is reported through counts[1], as on the GPU
            check(status, "loftr_rotation_averaging_host")
        return out
    ms = _StageMs(timings, ROTATION_STAGES)
    B.call("rotation_averaging", args, "", edge_image, ws=(E, n_images), tail=(ms.arg,))
    ms.report()
    return out


def rotation_averaging_host(edge_image, edge_R, edge_weight, adj_offsets, adj_edge, edge_use, n_images, root, cycle_cos_half, loss_chord,
                            max_chord, step_tol, max_iters=20, pcg_iters=30, pcg_tol=1e-4):
    """loftr_rotation_averaging_host: the host routine that DEFINES rotation averaging (include/loftr_hip.h) on numpy arrays:
    edge_image [E,2] i32, edge_R [E,3,3] f64, edge_weight [E] i32, adj_offsets [n_images + 1] i64, adj_edge [2E] i32, edge_use [E] u8; the
    angles already converted (rotations.average_rotations does that, and builds the adjacency).
    -> dict of numpy arrays: R [n,3,3] f64, in_graph [n] u8, edge_state [E] u8 (ROTATION_STATES), edge_chord [E] f64, support [E] i32,
    tree [E] u8, edge_use [E] u8, counts [16] i64 (ROTATION_NAMES), info [4] f64 (ROTATION_INFO).  A bad graph leaves its bits in
    counts[1] and every other output zero."""
    return _rotation_averaging(_Host, "rotation_averaging_host", "rotation_averaging",
                               (edge_image, edge_R, edge_weight, adj_offsets, adj_edge, edge_use), n_images, root, cycle_cos_half,
                               loss_chord, max_chord, step_tol, max_iters, pcg_iters, pcg_tol, None)


@_on_device
def rotation_averaging(edge_image, edge_R, edge_weight, adj_offsets, adj_edge, edge_use, n_images, root, cycle_cos_half, loss_chord,
                       max_chord, step_tol, max_iters=20, pcg_iters=30, pcg_tol=1e-4, timings=None):
    """loftr_rotation_averaging: the kernels (csrc/rotation_gpu.hip) on GPU tensors of the dtypes and shapes of rotation_averaging_host;
    the same result bit for bit.  -> dict of device tensors; nothing is read back here: the error bits are in counts[1], which the caller
    reads once (every other output is then zero).  timings: a list that receives (stage, ms) pairs (the call then waits for the
    stream)."""
    return _rotation_averaging(_Gpu, "rotation_averaging",
                               "the rotation-averaging kernels have no CPU fallback; the host routine is rotation_averaging_host",
                               (edge_image, edge_R, edge_weight, adj_offsets, adj_edge, edge_use), n_images, root, cycle_cos_half,
                               loss_chord, max_chord, step_tol, max_iters, pcg_iters, pcg_tol, timings)


# ---- localisation against a triangulated model (csrc/model_lookup.hip,csrc/model_lookup_gpu.hip) ------------------------
MODEL_COUNTS = 16
MODEL_REASONS = ("n_kept", "n_bad_row", "n_masked", "n_nonfinite", "n_negative_conf", "n_outside", "n_no_keypoint", "n_no_point",
                 "n_fused")                                                                  # match_reason codes 0..8 = counts[4 + reason]
MODEL_STATUS = ((1, "rows outside [0, R)"), (2, "rows that do not ascend"), (4, "row_query outside [0, Q) or descending"),
                (8, "row_db outside [0, n_images)"), (16, "keypoints outside the grid, or cells that do not ascend strictly within an image"),
                (32, "kp_point outside [-1, P)"))
MODEL_STAGES = ("lookup", "keep", "write")
_CELLS_ARGS = (("kp_offsets", "int64", 1), ("keypoints", "float32", 2), ("kp_point", "int32", 1))
_MODEL_ARGS = (("kp_offsets", "int64", 1), ("kp_cell", "int32", 1), ("kp_point", "int32", 1), ("xyz", "float32", 2))
_QUERY_ARGS = (("kpts_db", "float32", 2), ("kpts_q", "float32", 2), ("conf", "float32", 1), ("rows", "int32", 1), ("mask", "uint8", 1),
               ("row_db", "int32", 1), ("row_query", "int32", 1))
_MODEL_OUT = (("pts3d", 3, "float32"), ("kpts", 2, "float32"), ("q_ids", 0, "int64"), ("match", 0, "int32"), ("point", 0, "int32"),
              ("conf", 0, "float32"))


def _model_cells(B, what, hint, arrays, P, gh, gw, inv):
    """-> (kp_cell [K] i32, status [1] i32) of the backend's kind"""
    _check_args(B, what, hint, _CELLS_ARGS, arrays)
    kp_offsets, keypoints, kp_point = arrays
    K = keypoints.shape[0]
    if kp_offsets.shape[0] < 1 or min(int(gh), int(gw)) < 0:
        raise _lib.LoftrHipError(f"{what}: expected kp_offsets [n_images+1] and a grid of gh x gw >= 0 cells, got {tuple(kp_offsets.shape)}, {gh} x {gw}")
    if tuple(keypoints.shape) != (K, 2) or kp_point.shape[0] != K:
        raise _lib.LoftrHipError(f"{what}: expected keypoints [K,2] and kp_point [K], got {tuple(keypoints.shape)}, {tuple(kp_point.shape)}")
    arrays = [B.contiguous(x) for x in arrays]                                           # (held until the call has returned)
    a = [B.ptr(x) for x in arrays]
    cell, status = B.empty(K, "int32", keypoints), B.empty(1, "int32", keypoints)
    B.call("model_cells", (a[0], kp_offsets.shape[0] - 1, a[1], a[2], K, int(P), int(gh), int(gw), float(inv), B.ptr(cell), B.ptr(status)),
           "kp_offsets must start at 0, end at K and ascend", keypoints)
    return cell, status


def model_cells_host(kp_offsets, keypoints, kp_point, P, gh, gw, inv):
    """loftr_model_cells_host on numpy arrays: kp_offsets [n_images+1] i64, keypoints [K,2] f32, kp_point [K] i32 -> (kp_cell [K] i32,
    status bits: 16 cells not strictly ascending within an image or outside the grid, 32 kp_point outside [-1, P))."""
    cell, status = _model_cells(_Host, "model_cells_host", "model_cells", (kp_offsets, keypoints, kp_point), P, gh, gw, inv)
    return cell, int(status[0])


@_on_device
def model_cells(kp_offsets, keypoints, kp_point, P, gh, gw, inv):
    """loftr_model_cells on GPU tensors of the dtypes of model_cells_host -> (kp_cell [K] i32, status [1] i32), device tensors; nothing
    is read back here."""
    return _model_cells(_Gpu, "model_cells", "the host form is model_cells_host", (kp_offsets, keypoints, kp_point), P, gh, gw, inv)


def _model_lookup(B, what, hint, model, gh, gw, inv, queries, Q, timings):
    given = [(s, a) for s, a in zip(_MODEL_ARGS + _QUERY_ARGS, model + queries) if a is not None]          # (mask may be None)
    _check_args(B, what, hint, [s for s, _ in given], [a for _, a in given])
    kp_offsets, kp_cell, kp_point, xyz = model
    kd, kq, c, rows, mask, row_db, row_query = queries
    K, P, M, R = kp_cell.shape[0], xyz.shape[0], kd.shape[0], row_db.shape[0]
    if kp_offsets.shape[0] < 1 or kp_point.shape[0] != K or tuple(xyz.shape) != (P, 3):
        raise _lib.LoftrHipError(f"{what}: expected kp_offsets [n_images+1], kp_cell / kp_point [K] and xyz [P,3], got "
                                 f"{[tuple(a.shape) for a in model]}")
    if tuple(kd.shape) != (M, 2) or tuple(kq.shape) != (M, 2) or c.shape[0] != M or rows.shape[0] != M or \
            (mask is not None and mask.shape[0] != M) or row_query.shape[0] != R:
        raise _lib.LoftrHipError(f"{what}: expected kpts_db / kpts_q [M,2], conf / rows / mask [M] and row_db / row_query [R], got "
                                 f"{[None if a is None else tuple(a.shape) for a in queries]}")
    Q = int(Q)
    if Q < 0:
        raise _lib.LoftrHipError(f"{what}: Q must be >= 0, got {Q}")
    model, queries = [B.contiguous(a) for a in model], [B.contiguous(a) for a in queries]  # (held until the call has returned)
    m, q = [B.ptr(a) for a in model], [B.ptr(a) for a in queries]
    out = {k: B.empty((max(M, 1), w) if w else max(M, 1), dt, kp_offsets) for k, w, dt in _MODEL_OUT}
    out.update(q_offsets=B.empty(Q + 1, "int64", kp_offsets), match_reason=B.empty(M, "uint8", kp_offsets),
               counts=B.empty(MODEL_COUNTS, "int64", kp_offsets))
    md = _lib.Model(kp_offsets=m[0], kp_cell=m[1], kp_point=m[2], xyz=m[3], K=K, P=P, n_images=kp_offsets.shape[0] - 1, gh=int(gh), gw=int(gw),
                    inv=float(inv))
    st = _lib.ModelLookupOut(**{k: B.ptr(out[k]) for k, _ in _lib.ModelLookupOut._fields_})
    ms = _StageMs(timings, MODEL_STAGES)
    B.call("model_lookup", (C.byref(md), *q[:5], M, q[5], q[6], R, Q, C.byref(st)),
           "rows must ascend within [0, R), row_query within [0, Q) without descending, row_db within [0, n_images); "
           "kp_offsets must start at 0, end at K and ascend", kp_offsets, ws=(M, Q), tail=(ms.arg,))
    ms.report()
    return out


def model_lookup_host(kp_offsets, kp_cell, kp_point, xyz, gh, gw, inv, kpts_db, kpts_q, conf, rows, mask, row_db, row_query, Q):
    """loftr_model_lookup_host: the host routine that DEFINES the fused 2D-3D correspondences (include/loftr_hip.h) on numpy arrays:
    the model (kp_offsets [n_images+1] i64, kp_cell / kp_point [K] i32, xyz [P,3] f32, grid), the matches (kpts_db / kpts_q [M,2] f32,
    conf [M] f32, rows [M] i32 ascending, mask [M] u8 or None) and the rows (row_db / row_query [R] i32).
    -> dict of numpy arrays of the bound size M (pts3d, kpts, q_ids, match, point, conf), q_offsets [Q+1] i64, match_reason [M] u8 and
    counts [16] i64; the caller trims by counts[0]."""
    return _model_lookup(_Host, "model_lookup_host", "model_lookup", (kp_offsets, kp_cell, kp_point, xyz), gh, gw, inv,
                         (kpts_db, kpts_q, conf, rows, mask, row_db, row_query), Q, None)


@_on_device
def model_lookup(kp_offsets, kp_cell, kp_point, xyz, gh, gw, inv, kpts_db, kpts_q, conf, rows, mask, row_db, row_query, Q, timings=None):
    """loftr_model_lookup: the lookup / fusion kernels (csrc/model_lookup_gpu.hip) on GPU tensors of the dtypes and shapes of
    model_lookup_host; the same result bit for bit.  -> dict of device tensors; nothing is read back here: bad rows raise bits in
    counts[3], which the caller reads once, with counts[0] = C to trim by.  timings: a list that receives (stage, ms) pairs (the call
    then waits for the stream)."""
    return _model_lookup(_Gpu, "model_lookup", "the lookup kernels have no CPU fallback; the host routine is model_lookup_host",
                         (kp_offsets, kp_cell, kp_point, xyz), gh, gw, inv, (kpts_db, kpts_q, conf, rows, mask, row_db, row_query), Q, timings)


# ---- training-mode glue of the backbone (csrc/train_glue.hip; resnet_fpn.py:22-40,66-77,110-116) ------------------------------------------
def _dense4(t, name):
    """A 4-D fp32 GPU tensor [N,C,H,W] stored densely either NCHW or NHWC (channels_last: what the convolution nodes produce); returns
    (tensor as given or made contiguous, channels_last flag)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
        raise _lib.LoftrHipError(f"{name}: expected a 4-D float32 GPU tensor")
    if t.data_ptr() % 16:                                        # (a view into the middle of a buffer: the kernels use 16-byte accesses)
        t = t.clone(memory_format=torch.preserve_format)
    if t.is_contiguous():
        return t, 0
    if t.is_contiguous(memory_format=torch.channels_last) and t.shape[1] % 4 == 0 and t.shape[1] <= 1024:
        return t, 1
    return t.contiguous(), 0


def _like_layout(t, cl):
    """t in the layout `cl` names (a copy only when it is not already there, or not 16-byte aligned)."""
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.preserve_format)
    if cl:
        return t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)
    return t.contiguous()


@_on_device
def bn_train_fwd(x, gamma, beta, eps):
    """nn.BatchNorm2d in .train() mode on an [N,C,H,W] fp32 tensor (NCHW or channels-last storage, kept): (y, mean [C], invstd [C], unbiased
    variance [C])."""
    x, cl = _dense4(x, "x")
    N, Cc, H, W = x.shape
    lib = _lib.load()
    y = torch.empty_like(x)                                      # preserves the memory format
    mean, invstd, varu = (torch.empty(Cc, dtype=torch.float32, device=x.device) for _ in range(3))
    ws = workspace(lib.loftr_bn_train_workspace_bytes(N, Cc, H * W), x.device)
    check(lib.loftr_bn_train_fwd(_ptr(x), N, Cc, H * W, cl, _ptr(gamma), _ptr(beta), float(eps), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(varu),
                                 _ptr(ws), ws.numel(), _stream()), "loftr_bn_train_fwd")
    return y, mean, invstd, varu


@_on_device
def bn_train_bwd(dy, x, mean, invstd, gamma):
    """(dx, dgamma, dbeta) of bn_train_fwd; dx in x's layout."""
    x, cl = _dense4(x, "x")
    dy = _like_layout(dy, cl)
    N, Cc, H, W = x.shape
    lib = _lib.load()
    dx = torch.empty_like(x)
    dgamma, dbeta = (torch.empty(Cc, dtype=torch.float32, device=x.device) for _ in range(2))
    ws = workspace(lib.loftr_bn_train_workspace_bytes(N, Cc, H * W), x.device)
    check(lib.loftr_bn_train_bwd(_ptr(dy), _ptr(x), N, Cc, H * W, cl, _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(dx), _ptr(dgamma), _ptr(dbeta),
                                 _ptr(ws), ws.numel(), _stream()), "loftr_bn_train_bwd")
    return dx, dgamma, dbeta


ACT_CODES = {"none": 0, "relu": 1, "leaky_relu": 2}


@_on_device
def act_fwd(a, b, act, slope=0.01):
    """act(a + b) (b may be None), act in ACT_CODES; elementwise: any dense layout, the result takes a's."""
    a, cl = _dense4(a, "a") if a.dim() == 4 else (_need(a, "a"), 0)
    if b is not None:
        assert b.shape == a.shape
        b = _like_layout(b, cl) if a.dim() == 4 else _need(b, "b")
    y = torch.empty_like(a)
    check(_lib.load().loftr_act_fwd(_ptr(a), _ptr(b), a.numel(), ACT_CODES[act], float(slope), _ptr(y), _stream()), "loftr_act_fwd")
    return y


@_on_device
def act_bwd(dy, y, act, slope=0.01):
    y, cl = _dense4(y, "y") if y.dim() == 4 else (_need(y, "y"), 0)
    dy = _like_layout(dy, cl) if y.dim() == 4 else _need(dy, "dy")
    dx = torch.empty_like(y)
    check(_lib.load().loftr_act_bwd(_ptr(dy), _ptr(y), dy.numel(), ACT_CODES[act], float(slope), _ptr(dx), _stream()), "loftr_act_bwd")
    return dx


@_on_device
def upsample2x_bilinear(x):
    """F.interpolate(x, scale_factor=2., mode='bilinear', align_corners=True) of an [N,C,H,W] fp32 tensor, in x's memory format."""
    x, cl = _dense4(x, "x")
    N, Cc, H, W = x.shape
    y = torch.empty(N, Cc, 2 * H, 2 * W, dtype=torch.float32, device=x.device, memory_format=torch.channels_last if cl else torch.contiguous_format)
    check(_lib.load().loftr_upsample2x_bilinear_fwd(_ptr(x), N, Cc, H, W, cl, _ptr(y), _stream()), "loftr_upsample2x_bilinear_fwd")
    return y


@_on_device
def upsample2x_bilinear_bwd(dy):
    dy, cl = _dense4(dy, "dy")
    N, Cc, Ho, Wo = dy.shape
    dx = torch.empty(N, Cc, Ho // 2, Wo // 2, dtype=torch.float32, device=dy.device, memory_format=torch.channels_last if cl else torch.contiguous_format)
    check(_lib.load().loftr_upsample2x_bilinear_bwd(_ptr(dy), N, Cc, Ho // 2, Wo // 2, cl, _ptr(dx), _stream()), "loftr_upsample2x_bilinear_bwd")
    return dx
