"""Case table, float64 reference and tolerance of the coarse encoder's edge tests.

tests/test_hip_encoder_edges.py (GPU) compares `ops.encoder_layer` / `ops.transformer` with the numpy oracle evaluated in float64 at the
sizes where the hand-written work distribution of csrc/encoder_fused.hip, proj_kv_kernel / kv_finalize_kernel and the persistent kernel
changes path: 32 tokens per wave, 128 per workgroup, one K / V partial per 128 source rows, the xsplit / gpc mapping below 8 sequences.
tests/test_encoder_edges_oracle.py (CPU) shows that this comparison can fail: the float64 oracle with one small mistake built in must
sit at least 20 tolerances away from the unmodified one on every case.

Reference: `oracle.loftr_oracle.encoder_layer` / `local_feature_transformer` on float64 inputs (ref64) and on the float32 inputs (ref32);
noise = max|ref32 - ref64| is float32's own distance to exact arithmetic on the case, scale = max|ref64|.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import loftr_oracle as O
from loftr_amd.synth import _encoder_layer, make_weights

C, H = 256, 8

# ---- tolerance ------------------------------------------------------------------------------------------------------------------------
# err <= k * noise + 1e-6 * scale (the form of test_conv2d_node_vs_float64), never above the project's own bounds: 2e-5 * max(1, scale) for
# one layer (test_single_encoder_layer_vs_oracle), 2e-4 for the transformer (test_hip_vs_oracle_stages).  k = twice the largest err / noise
# measured on an MI355X (profiles/encoder_edges_accuracy.txt: 1.99 over the layer cases, 1.22 over the transformer cases and modes), rounded
# up to an integer; the factor 2 covers the summation-order differences between machines and between the persistent and the launch form.
K_LAYER = 4
K_TRANSFORMER = 3


def layer_tolerance(noise, scale):
    return min(K_LAYER * noise + 1e-6 * scale, 2e-5 * max(1.0, scale))


def transformer_tolerance(noise, scale):
    return min(K_TRANSFORMER * noise + 1e-6 * scale, 2e-4)


# ---- layer cases ----------------------------------------------------------------------------------------------------------------------
LayerCase = namedtuple("LayerCase", "name nb L S self_attn masked log2_scale seed")


def _lc(name, nb, L, S, self_attn=False, masked=False, log2_scale=0, seed=0):
    return LayerCase(name, nb, L, S, self_attn, masked, log2_scale, seed)


# The magnitude case: layer-0 inputs are backbone output plus position encoding, not LayerNorm bounded.  x and source are multiplied by the
# largest power of two for which every fp16-pair operand of the layer, evaluated by the float64 oracle, stays inside the range DESIGN.md
# (section 3, csrc/gemm.h) states (an unscaled operand below 65504, P * 2^5 below 2^14).  layer_float64(want_operands=True) computes them; with (3, 129, 129), seed as below:
#   2^5:  x 137   source 148   Q' 0.032   32 P 4.28e3   message 4.09   hidden 98    -> inside
#   2^6:  x 274   source 297   Q' 0.017   32 P 1.69e4   message 4.11   hidden 196   -> 32 P is beyond 2^14 = 16384
# (P = KV Wm grows with the square of the source: K = elu + 1 and V are both linear in it).  tests/test_encoder_edges_oracle.py re-checks
# both lines.
MAGNITUDE_LOG2 = 5

LAYER_CASES = (
    # x-side token edges: 32 tokens per wave, 128 per workgroup
    [_lc(f"x_L{L}", 3, L, 129) for L in (1, 31, 32, 33, 127, 128, 129, 257)]
    # source edges: 128-row K / V tiles, splits = ceil(S / 128), 1 / S
    + [_lc(f"src_S{S}", 3, 129, S, seed=3 if S == 127 else 0) for S in (1, 127, 128, 385)]      # (seed: phantom_source_rows, one row, reaches 20 tolerances)
    # sequence-count edges: xsplit = 8 / nseq clamped to the group count, gpc
    + [_lc(f"nseq_{nb}", nb, 257, 129) for nb in (1, 2, 4, 5, 8, 9)]
    + [_lc("nseq_1_two_groups", 1, 129, 129), _lc("nseq_2_one_group", 2, 33, 129)]
    # self form: the source is x, one mask object for both
    + [_lc("self_3x129", 3, 129, 129, self_attn=True), _lc("self_8x257", 8, 257, 257, self_attn=True)]
    # masks (layer_masks below)
    + [_lc("mask_3x129x385", 3, 129, 385, masked=True), _lc("mask_9x257x127", 9, 257, 127, masked=True),
       _lc("mask_2x33x129", 2, 33, 129, masked=True), _lc("mask_self_4x257", 4, 257, 257, self_attn=True, masked=True)]
    # magnitude
    + [_lc("magnitude_up", 3, 129, 129, log2_scale=MAGNITUDE_LOG2), _lc("magnitude_down", 3, 129, 129, log2_scale=-6)]
)
LAYER_CASE_BY_NAME = {c.name: c for c in LAYER_CASES}
assert len(LAYER_CASE_BY_NAME) == len(LAYER_CASES)


def _inside(b, period):
    """b, moved down a little when it sits on a multiple of `period`: a boundary INSIDE a wave / a tile."""
    return b - 5 if b % period == 0 and b > 5 else b


def layer_masks(c):
    """(x_mask, source_mask) of a masked case, bool [nb, L] / [nb, S]; the self form has ONE mask.
    sequence 0: x valid up to a token inside a wave, the source up to a token inside a 128-row tile (and inside a wave);
    sequence 1, S >= 384: source rows 128..255 masked (a wholly masked middle tile) plus ten scattered rows of the next, valid tile;
    sequence 2 of more than three: x mask all zero (with three sequences none is free: 0, 1 and the last carry the patterns above);
    last sequence: source mask all zero."""
    xm = np.ones((c.nb, c.L), bool)
    xm[0, _inside(c.L - c.L // 3, 32):] = False
    if c.self_attn:
        xm[-1] = False
        return xm, xm
    sm = np.ones((c.nb, c.S), bool)
    sm[0, _inside(_inside(c.S - c.S // 4, 128), 32):] = False
    if c.S >= 384:
        sm[1, 128:256] = False
        sm[1, 258:378:12] = False
        assert (~sm[1, 256:384]).sum() == 10
    if c.nb > 3:
        xm[2] = False
    sm[-1] = False
    return xm, sm


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False


@functools.lru_cache(maxsize=None)
def layer_inputs(name):
    """Weights (synth._encoder_layer), seeded standard-normal float32 x / source, masks.  Shared by every test: read-only."""
    c = LAYER_CASE_BY_NAME[name]
    rng = np.random.default_rng([c.nb, c.L, c.S, int(c.self_attn), int(c.masked)] + ([c.seed] if c.seed else []))
    w = {}
    _encoder_layer(rng, "l.", C, w)
    f = np.float32(2.0 ** c.log2_scale)
    x = rng.standard_normal((c.nb, c.L, C)).astype(np.float32) * f
    src = x if c.self_attn else rng.standard_normal((c.nb, c.S, C)).astype(np.float32) * f
    xm, sm = layer_masks(c) if c.masked else (None, None)
    _freeze(x, src, xm, sm, *w.values())
    return dict(case=c, w=w, x=x, src=src, xm=xm, sm=sm)


@functools.lru_cache(maxsize=None)
def layer_reference(name):
    """ref64, ref32, noise, scale of a layer case (computed once per process)."""
    i = layer_inputs(name)
    ref64 = O.encoder_layer(i["x"].astype(np.float64), i["src"].astype(np.float64), i["w"], "l.", H, i["xm"], i["sm"])
    ref32 = O.encoder_layer(i["x"], i["src"], i["w"], "l.", H, i["xm"], i["sm"])
    assert ref64.dtype == np.float64 and ref32.dtype == np.float32
    _freeze(ref64, ref32)
    return dict(ref64=ref64, ref32=ref32, noise=float(np.abs(ref32 - ref64).max()), scale=float(np.abs(ref64).max()))


# ---- the float64 layer once more, with one mistake built in -----------------------------------------------------------------------------
MUTATIONS = ("x_mask_boundary", "source_mask_boundary", "last_source_row_dropped", "phantom_source_rows", "v_length_from_x_side",
             "neighbour_sequence_source", "token_blocks_exchanged")


# v_length taken from the x side TOGETHER with 1 / S cancels exactly (values / v_length ... * v_length, linear_attention.py:41-45): no comparison
# of outputs can see that, and it is no error.  The mistake that can happen is one-sided: the x kernel multiplies by v_length = L while the
# K / V kernel divided by S.  That scales a token's whole message by L / S, which LayerNorm1 removes except through ln_eps: the output moves
# by about (1 - (S / L)^2) * ln_eps / var(message).
BOTH_LENGTHS_FROM_X_SIDE = "both_lengths_from_x_side"


def mutation_applies(c, m):
    if m == "phantom_source_rows":
        # no row between S and the next multiple of 128 otherwise; a phantom row weighs K = 1 whatever the inputs: beside real rows of
        # K ~ 2^5 (magnitude_up) the 127 of them count as four
        return c.S % 128 != 0 and c.log2_scale <= 0
    if m == "v_length_from_x_side":
        # visible through ln_eps only (above): the lengths have to differ by more than rounding (127 / 128 against 129 move the output by
        # 3e-5 .. 5e-5), and with S = 1 the message is one token's V, not an average, its variance 100 times ln_eps' reach
        return c.S > 1 and max(c.L, c.S) >= 1.5 * min(c.L, c.S)
    if m == "neighbour_sequence_source":
        return c.nb > 1
    if m == "token_blocks_exchanged":
        return c.L > 32
    return True


def _clear_last_valid(mask, shape):
    """The mask with sequence 0's last valid token cleared (a boundary moved by one token)."""
    m = np.ones(shape, bool) if mask is None else mask.copy()
    m[0, np.flatnonzero(m[0])[-1]] = False
    return m


def layer_float64(name, mutation=None, want_operands=False):
    """LoFTREncoderLayer.forward (transformer.py:35-58, linear_attention.py:20-47) in float64 from the oracle's pieces, with hooks on
    the intermediates.  mutation None reproduces oracle.encoder_layer (tested).  Mutations model kernel mistakes:
      x_mask_boundary / source_mask_boundary   the mask of sequence 0 ends one token early
      last_source_row_dropped                  every sequence's last valid source row is missing from KV and Ksum (`row < S - 1`)
      phantom_source_rows                      rows S .. next multiple of 128 enter as K = elu(0) + 1 = 1, V = 0 (no `row < S` guard)
      v_length_from_x_side                     the x side multiplies by v_length = L, the K / V side divided by S
      neighbour_sequence_source                sequence n reads KV / Ksum of sequence (n + 1) % nb
      token_blocks_exchanged                   the outputs of the first two 32-token blocks change places"""
    i = layer_inputs(name)
    c, w = i["case"], i["w"]
    g = lambda n: w["l." + n].astype(np.float64)
    x, src = i["x"].astype(np.float64), i["src"].astype(np.float64)
    xm, sm = i["xm"], i["sm"]
    if mutation == "x_mask_boundary":
        xm = _clear_last_valid(xm, (c.nb, c.L))
    if mutation == "source_mask_boundary":
        sm = _clear_last_valid(sm, (c.nb, c.S))
    nb, L, S, D = c.nb, c.L, c.S, C // H
    Q = O.elu_feature_map((x @ g("q_proj.weight").T).reshape(nb, L, H, D))
    K = O.elu_feature_map((src @ g("k_proj.weight").T).reshape(nb, S, H, D))
    V = (src @ g("v_proj.weight").T).reshape(nb, S, H, D)
    if xm is not None:
        Q = Q * xm[:, :, None, None]
    if sm is not None:
        K, V = K * sm[:, :, None, None], V * sm[:, :, None, None]
    if mutation == "last_source_row_dropped":
        keep = np.ones((nb, S), bool)
        for n in range(nb):
            valid = np.flatnonzero(sm[n]) if sm is not None else np.arange(S)
            if len(valid):
                keep[n, valid[-1]] = False
        K, V = K * keep[:, :, None, None], V * keep[:, :, None, None]
    v_length = float(L if mutation in ("v_length_from_x_side", BOTH_LENGTHS_FROM_X_SIDE) else S)
    V = V / float(L if mutation == BOTH_LENGTHS_FROM_X_SIDE else S)
    KV = np.einsum("nshd,nshv->nhdv", K, V)
    Ksum = K.sum(axis=1)
    if mutation == "phantom_source_rows":
        Ksum = Ksum + float(-S % 128)
    if mutation == "neighbour_sequence_source":
        KV, Ksum = np.roll(KV, -1, axis=0), np.roll(Ksum, -1, axis=0)
    Z = 1.0 / (np.einsum("nlhd,nhd->nlh", Q, Ksum) + 1e-6)
    msg = np.einsum("nlhd,nhdv,nlh->nlhv", Q, KV, Z) * v_length
    merged = msg.reshape(nb, L, C) @ g("merge.weight").T
    msgn = O.layer_norm(merged, g("norm1.weight"), g("norm1.bias"))
    hid = np.maximum(np.concatenate([x, msgn], axis=2) @ g("mlp.0.weight").T, 0)
    out = x + O.layer_norm(hid @ g("mlp.2.weight").T, g("norm2.weight"), g("norm2.bias"))
    if mutation == "token_blocks_exchanged":
        n = min(32, L - 32)
        out[:, :n], out[:, 32:32 + n] = out[:, 32:32 + n].copy(), out[:, :n].copy()
    if want_operands:
        # what the kernels hold as fp16 (hi, lo) pairs: the inputs, Q' = z (.) Q, P = KV folded into the merge weight (stored times 2^5),
        # the normalised message, the hidden layer
        P = np.einsum("nhdv,jhv->njhd", KV, g("merge.weight").reshape(C, H, D))
        return out, {"x": np.abs(x).max(), "source": np.abs(src).max(), "Q'": np.abs(Q * (Z * v_length)[..., None]).max(),
                     "32 P": 32.0 * np.abs(P).max(), "message": np.abs(msgn).max(), "hidden": hid.max()}
    return out


def operands_in_range(ops_max):
    return all(v < (2.0 ** 14 if k == "32 P" else 65504.0) for k, v in ops_max.items())


# ---- transformer cases -----------------------------------------------------------------------------------------------------------------
TransformerCase = namedtuple("TransformerCase", "name N L S masked")
TRANSFORMER_CASES = [TransformerCase(f"{N}x{L}x{S}" + ("_masked" if m else ""), N, L, S, m) for N, L, S, m in
                     ((1, 33, 129, False), (2, 129, 127, True), (3, 160, 96, True),
                      (1, 128, 128, False),        # stacked self calls, nseq = 2
                      (4, 129, 129, True),         # nseq 8 in the self calls, 4 in the cross calls
                      (8, 130, 75, True),          # mode "auto" selects the persistent form
                      (9, 64, 64, False))]         # 18 stacked sequences
TRANSFORMER_CASE_BY_NAME = {c.name: c for c in TRANSFORMER_CASES}


def prefix_masks(N, T, shift):
    """Valid prefixes that end inside a wave, another one per sequence; sequence 0's (about two thirds of T) leaves every 128-token tile
    behind it without a valid token when T > 128."""
    m = np.ones((N, T), bool)
    for n in range(N):
        b = max(1, T - T // 3 - (7 * n + shift) % max(1, T // 2))
        b = b - 3 if b % 32 == 0 and b > 3 else b
        m[n, b:] = False
    return m


@functools.lru_cache(maxsize=None)
def transformer_setup():
    from loftr_amd import get_cfg
    cfg = get_cfg(thr=0.0)
    w = make_weights(0, cfg)
    _freeze(*[v for v in w.values() if isinstance(v, np.ndarray) and v.ndim])
    return cfg, w


@functools.lru_cache(maxsize=None)
def transformer_inputs(name):
    c = TRANSFORMER_CASE_BY_NAME[name]
    rng = np.random.default_rng([c.N, c.L, c.S, int(c.masked)])
    f0 = rng.standard_normal((c.N, c.L, C)).astype(np.float32)
    f1 = rng.standard_normal((c.N, c.S, C)).astype(np.float32)
    m0 = prefix_masks(c.N, c.L, 0) if c.masked else None
    m1 = prefix_masks(c.N, c.S, 3) if c.masked else None
    _freeze(f0, f1, m0, m1)
    return dict(case=c, f0=f0, f1=f1, m0=m0, m1=m1)


@functools.lru_cache(maxsize=None)
def transformer_reference(name):
    cfg, w = transformer_setup()
    i = transformer_inputs(name)
    run = lambda a, b: O.local_feature_transformer(a, b, w, "loftr_coarse.", cfg["coarse"]["layer_names"], cfg["coarse"]["nhead"], i["m0"], i["m1"])
    ref64 = run(i["f0"].astype(np.float64), i["f1"].astype(np.float64))
    ref32 = run(i["f0"], i["f1"])
    assert ref64[0].dtype == np.float64 and ref32[0].dtype == np.float32
    _freeze(*ref64, *ref32)
    return dict(ref64=ref64, ref32=ref32, noise=float(max(np.abs(a - b).max() for a, b in zip(ref32, ref64))),
                scale=float(max(np.abs(a).max() for a in ref64)))
