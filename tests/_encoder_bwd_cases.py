"""Case table, float64 reference and tolerances of the encoder-layer backward's edge tests.

tests/test_hip_encoder_bwd_edges.py (GPU) compares `ops.encoder_layer_bwd` (loftr_encoder_layer_bwd, csrc/encoder_bwd.hip, with the
split-K weight gradient launch_wgrad / launch_reduce_partials of csrc/head_grads.hip) and `ops.encoder_layer` with torch.autograd of the
layer in FLOAT64 at the sizes where the hand-written work distribution changes path:
  * launch_outer_accum (KV / Ksum over the S source tokens, dKV / dKsum over the L tokens of x): one block per (pair, head) up to 1024
    tokens; above, ceil(Tn / 512) chunks, at most 16, each rounded up to 64 tokens, the last one ragged, then outer_reduce_kernel --
    under padding masks too: a mask boundary inside a chunk, a chunk masked entirely, a pair with one valid token;
  * attn_q_kernel / attn_kv_bwd_kernel: 256 tokens per block (a last block of one token; L != S with the short side below a block);
  * ln_bwd_kernel: LN_ROWS_PB = 64 rows per partial, ragged last block; reduce_partials_kernel below 16 partials,
    reduce_partials_tall_kernel from 16 (T = 960 / 961 for the LayerNorm gradients, T = 1920 / 1921 for the weight gradients);
  * launch_wgrad: one partial shorter than the chunk, a second partial of ONE token, a chunk other than 128 (mlp0, O = 512: 160 tokens
    at T = 8257), the fine shape (C = 128, D = 16) beyond one partial;
  * the debug switches `wgrad_chunk` and `reduce_tall` (FORCED).
tests/test_encoder_bwd_oracle.py (CPU) holds every condition stated here and shows that the comparison can fail.

Reference: `layer` below, LoFTREncoderLayer + LinearAttention (transformer.py:35-58, linear_attention.py:20-47) restated in torch, under
torch.autograd on the CPU: on the float64 casts of the float32 inputs (ref64) and on the inputs themselves (ref32).  Outputs: `out`,
`grad_x`, `grad_source` and the ten weight gradients.  It is pinned to the committed glayer_* fixtures by the CPU test.

The ReLU condition.  The layer has one non-smooth point, relu(hcat W0^T).  With plain random inputs some pre-activations lie within
float32 rounding of zero and change sign between float32 and float64 (profiles/r05_relu_flip_probe.txt): ref32 is then 1e-2 of the
maximum away from ref64 in grad_x, and a comparison measures nothing.  So in ref64 every pre-activation of mlp.0 is at least
RELU_MARGIN = 1e-4 of the largest |pre-activation| away from zero; the case builder redraws, from the case's generator, the rows of x
that own an offending entry (x and source are independent, so only that row's pre-activations change), at most RELU_ROUNDS times.  The
kernels take their ReLU mask from their own float32 h1, whose distance to float64 is of the order 1e-6 of the ROW's scale (DESIGN.md
section 5: loftr_linear_fwd scales its operands per row); the margin is 100 times that.  The case with a tenth of its rows of x times 30
("rows") measures the margin against the largest |pre-activation| of the entry's own ROW: against the global maximum (30 times larger) an
ordinary row of 512 pre-activations of unit scale has an entry inside the margin 24 times out of 25 and no redraw ends, while the
kernel's error is per row -- the row-wise margin is still 100 times it, and test_reference_noise holds ref32 to ref64 there as
everywhere.  ELU's derivative is continuous and needs no condition.

Tolerance, per output tensor: err = max|got - ref64|, noise = max|ref32 - ref64|, scale = max|ref64|; err <= K[group] noise + 1e-6 scale.
"""
import functools
import importlib.util
import os
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_layer_grad", os.path.join(HERE, "golden", "make_golden_layer_grad.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

FIELDS = tuple(f for f, _ in MG.FIELDS)
MATRICES = ("q_proj", "k_proj", "v_proj", "merge", "mlp0", "mlp2")
VECTORS = ("norm1_w", "norm1_b", "norm2_w", "norm2_b")
DATA = ("out", "grad_x", "grad_source")
OUTPUTS = DATA + tuple("grad_" + f for f in FIELDS)
GROUP = {**{k: "data" for k in DATA}, **{"grad_" + f: "matrix" for f in MATRICES}, **{"grad_" + f: "vector" for f in VECTORS}}

# ---- tolerance ------------------------------------------------------------------------------------------------------------------------
# err <= K[group] * noise + 1e-6 * scale.  K = twice the largest err / noise measured on an MI355X over all cases, forced paths and
# tensors of the group, rounded up to an integer (the factor 2 covers summation-order differences between machines, as in
# tests/_sinkhorn_cases.py).  The lines of profiles/encoder_bwd_accuracy.txt the constants were taken from:
#   K["data"]   =  5 <- 2.24   1x8257x257x256  default  grad_source   data   err 1.586e-05 noise 7.096e-06 err/noise   2.24 scale 1.007e+01
#   K["matrix"] =  7 <- 3.27   1x8257x257x256  default  grad_v_proj   matrix err 7.913e-04 noise 2.417e-04 err/noise   3.27 scale 5.583e+02
#   K["vector"] = 12 <- 5.92   1x8257x257x256  default  grad_norm1_w  vector err 7.309e-04 noise 1.235e-04 err/noise   5.92 scale 2.200e+02
# All three are sums over the 8257 tokens of the largest case, where ref32's own error happens to be small for its length (1.2e-4 / 220 =
# 5.6e-7 of the scale for grad_norm1_w; the kernel's 7.3e-4 is 3.3e-6 of the scale).  The smallest distance of a modelled mistake under
# these constants is about 1000 tolerances (tests/test_encoder_bwd_oracle.py asks for DETECTION_FACTOR).
K = {"data": 5, "matrix": 7, "vector": 12}
RELU_MARGIN = 1e-4
RELU_ROUNDS = 20
DETECTION_FACTOR = 10.0     # a modelled mistake sits this many tolerances from ref64 in at least one tensor, on every case it applies to


def tolerance(key, noise, scale):
    return K[GROUP[key]] * noise + 1e-6 * scale


# ---- the kernels' work distribution, restated -------------------------------------------------------------------------------------------
LN_ROWS_PB, ATTN_TOKENS, TALL_FROM, OUTER_ONE_BLOCK, OUTER_MAX_SPLITS = 64, 256, 16, 1024, 16


def _cdiv(a, b):
    return -(-a // b)


def wgrad_chunk(T, O, forced=0):
    """wgrad_chunk of csrc/head_grads.hip: tokens per split-K partial."""
    if forced > 0:
        return forced
    tiles = _cdiv(O, 128)
    target = 1 if tiles >= 256 else 256 // tiles
    c = _cdiv(_cdiv(T, target), 32) * 32
    return min(max(c, 128), 512)


def wgrad_partials(T, O, forced=0):
    """(partials, tokens in the last one) of launch_wgrad."""
    ch = wgrad_chunk(T, O, forced)
    ns = _cdiv(T, ch)
    return ns, T - (ns - 1) * ch


def wgrad_part_floats(T, O, I, forced=0):
    return max(_cdiv(T, wgrad_chunk(T, min(o, O), forced)) * min(o, O) * I for o in range(128, O + 128, 128))


def outer_splits(Tn, scratch_floats=None, per_split=0):
    """(chunks, tokens per chunk) of launch_outer_accum over Tn tokens; one chunk when the scratch cannot hold the partials."""
    splits = min(_cdiv(Tn, 512), OUTER_MAX_SPLITS) if Tn > OUTER_ONE_BLOCK else 1
    if scratch_floats is not None and splits * per_split > scratch_floats:
        splits = 1
    if splits == 1:
        return 1, Tn
    chunk = _cdiv(_cdiv(Tn, splits), 64) * 64
    return _cdiv(Tn, chunk), chunk


def outer_chunks(Tn):
    n, ch = outer_splits(Tn)
    return [(k * ch, min(Tn, (k + 1) * ch)) for k in range(n)]


Plan = namedtuple("Plan", "T Ts nlb ln_tall q_blocks kv_blocks outer_x outer_src wg wg_src wg_mlp0 chunk_mlp0")


def plan(nb, L, S, C, H, forced_chunk=0):
    """What loftr_encoder_layer_bwd launches for a shape.  wg / wg_src: (partials, tokens in the last) of the C-row weight gradients over
    the nb L tokens of x (q_proj, merge, mlp2) and over the nb S source tokens (k_proj, v_proj); wg_mlp0: of mlp.0 (2C rows)."""
    T, Ts, D = nb * L, nb * S, C // H
    scratch = max(wgrad_part_floats(T, 2 * C, 2 * C, forced_chunk), wgrad_part_floats(Ts, 2 * C, 2 * C, forced_chunk))      # wpart_need
    per = nb * H * (D * D + D)
    nlb = _cdiv(T, LN_ROWS_PB)
    return Plan(T, Ts, nlb, nlb >= TALL_FROM, _cdiv(L, ATTN_TOKENS), _cdiv(S, ATTN_TOKENS), outer_splits(L, scratch, per), outer_splits(S, scratch, per),
                wgrad_partials(T, C, forced_chunk), wgrad_partials(Ts, C, forced_chunk), wgrad_partials(T, 2 * C, forced_chunk),
                wgrad_chunk(T, 2 * C, forced_chunk))


# ---- edges: what a case is in the table for, as a predicate of the case and its plan ----------------------------------------------------
def _mask_chunks(c, side):
    """Per pair, the number of valid tokens in each outer_accum chunk of x (side 0) / source (side 1)."""
    m = masks(c)[side]
    return [[int(m[n, a:b].sum()) for a, b in outer_chunks(m.shape[1])] for n in range(c.nb)]


EDGES = {
    "single_short_partial": lambda c, p: p.wg == (1, p.T) and p.wg_src == (1, p.Ts) and p.wg_mlp0 == (1, p.T) and max(p.T, p.Ts) < 128
        and p.outer_x == (1, c.L) and p.outer_src == (1, c.S) and (p.q_blocks, p.kv_blocks) == (1, 1) and not p.ln_tall,
    "wgrad_x_one_full_partial": lambda c, p: p.wg == (1, 128) and p.wg_mlp0 == (1, 128),
    "wgrad_src_one_full_partial": lambda c, p: p.wg_src == (1, 128),
    "wgrad_x_second_partial_one_token": lambda c, p: p.wg == (2, 1) and p.wg_mlp0 == (2, 1),
    "wgrad_src_second_partial_one_token": lambda c, p: p.wg_src == (2, 1),
    "attn_q_last_block_one_token": lambda c, p: p.q_blocks >= 2 and c.L % ATTN_TOKENS == 1,
    "attn_kv_last_block_one_token": lambda c, p: p.kv_blocks >= 2 and c.S % ATTN_TOKENS == 1,
    "attn_kv_one_token_short_of_a_block": lambda c, p: c.S == ATTN_TOKENS - 1,
    "attn_q_full_block": lambda c, p: c.L == ATTN_TOKENS and c.nb > 1,
    "attn_short_side_below_a_block": lambda c, p: c.L != c.S and min(c.L, c.S) < ATTN_TOKENS <= max(c.L, c.S),
    "outer_x_1024_one_block": lambda c, p: c.L == 1024 and p.outer_x == (1, 1024),
    "outer_src_1024_one_block": lambda c, p: c.S == 1024 and p.outer_src == (1, 1024),
    "outer_x_1025_three_chunks": lambda c, p: c.L == 1025 and p.outer_x == (3, 384) and outer_chunks(c.L)[-1] == (768, 1025),
    "outer_src_1025_three_chunks": lambda c, p: c.S == 1025 and p.outer_src == (3, 384) and outer_chunks(c.S)[-1] == (768, 1025),
    "outer_16_chunk_cap": lambda c, p: _cdiv(c.L, 512) > OUTER_MAX_SPLITS and p.outer_x == (15, 576) and c.L - 14 * 576 == 193,
    "ln_15_partials_flat": lambda c, p: p.nlb == 15 and not p.ln_tall and p.T % LN_ROWS_PB == 0,
    "ln_16_partials_tall_one_row_block": lambda c, p: p.nlb == 16 and p.ln_tall and p.T % LN_ROWS_PB == 1,
    "wgrad_15_partials_flat": lambda c, p: p.wg == (15, 128) and p.wg_mlp0 == (15, 128),
    "wgrad_16_partials_tall": lambda c, p: p.wg == (16, 1) and p.wg_mlp0 == (16, 1),
    "mlp0_chunk_160": lambda c, p: p.chunk_mlp0 == 160 and p.wg_mlp0 == (52, 97) and p.wg == (65, 65),
    "short_x_long_split_source": lambda c, p: c.L < 64 and p.outer_src[0] >= 3 and p.outer_x[0] == 1 and c.nb == 2 and p.wg == (1, p.T),
    "long_split_x_short_source": lambda c, p: c.S < 64 and p.outer_x[0] >= 3 and p.outer_src[0] == 1 and c.nb == 2 and p.wg_src == (1, p.Ts),
    "fine_beyond_one_partial": lambda c, p: (c.C, c.C // c.H) == (128, 16) and p.wg[0] >= 2 and p.wg_mlp0[0] >= 2 and p.wg_mlp0 == p.wg,
    "fine_tall": lambda c, p: (c.C, c.C // c.H) == (128, 16) and (p.ln_tall or p.wg[0] >= TALL_FROM),
    "fine_tall_wgrad": lambda c, p: (c.C, c.C // c.H) == (128, 16) and p.wg[0] >= TALL_FROM and p.ln_tall,
    "masked_small": lambda c, p: c.masks == "golden" and p.outer_src == (1, c.S),
    "mask_src_boundary_inside_chunk": lambda c, p: p.outer_src[0] == 3 and any(0 < v[1] < p.outer_src[1] and v[0] == p.outer_src[1] for v in _mask_chunks(c, 1)),
    "mask_src_chunk_fully_masked": lambda c, p: p.outer_src[0] == 3 and any(v[2] == 0 and v[0] > 0 for v in _mask_chunks(c, 1)),
    "mask_src_single_valid_token": lambda c, p: p.outer_src[0] == 3 and any(sum(v) == 1 for v in _mask_chunks(c, 1)),
    "mask_x_boundary_inside_chunk": lambda c, p: p.outer_x[0] == 3 and any(0 < v[1] < p.outer_x[1] and v[0] == p.outer_x[1] for v in _mask_chunks(c, 0)),
    "mask_x_chunk_fully_masked": lambda c, p: p.outer_x[0] == 3 and any(v[2] == 0 and v[0] > 0 for v in _mask_chunks(c, 0)),
    "mask_x_single_valid_token": lambda c, p: p.outer_x[0] == 3 and any(sum(v) == 1 for v in _mask_chunks(c, 0)),
    "mask_pair_without_padding": lambda c, p: c.masks in ("split", "split_t") and all(m[2].all() for m in masks(c)),
    "tiny_gradient": lambda c, p: c.gmode == "tiny",
    "row_magnitudes": lambda c, p: c.gmode == "rows" and p.wg[0] >= 2 and p.outer_x[0] >= 2 and p.T % LN_ROWS_PB > 16,
}

# ---- cases -----------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name nb L S C H masks gmode seed edges")
SEEDS = {}                   # name -> seed other than 0 (chosen where a condition on the inputs missed with seed 0)
G_TINY = 1e-6


def _build_cases():
    cases = []

    def add(nb, L, S, C, *edges, masks=None, gmode="normal", tag=""):
        name = f"{tag}{nb}x{L}x{S}x{C}"
        cases.append(Case(name, nb, L, S, C, 8, masks, gmode, SEEDS.get(name, 0), edges))
    add(2, 48, 35, 256, "single_short_partial")
    add(5, 25, 25, 128, "single_short_partial")
    add(1, 128, 129, 256, "wgrad_x_one_full_partial", "wgrad_src_second_partial_one_token")
    add(1, 129, 128, 256, "wgrad_src_one_full_partial", "wgrad_x_second_partial_one_token")
    add(1, 257, 255, 256, "attn_q_last_block_one_token", "attn_kv_one_token_short_of_a_block", "attn_short_side_below_a_block")
    add(3, 256, 40, 256, "attn_q_full_block", "attn_short_side_below_a_block")
    add(1, 1024, 1025, 256, "outer_x_1024_one_block", "outer_src_1025_three_chunks", "attn_kv_last_block_one_token")
    add(1, 1025, 1024, 256, "outer_src_1024_one_block", "outer_x_1025_three_chunks", "attn_q_last_block_one_token")
    add(1, 960, 64, 256, "ln_15_partials_flat")
    add(1, 961, 64, 256, "ln_16_partials_tall_one_row_block")
    add(1, 1920, 48, 256, "wgrad_15_partials_flat")
    add(1, 1921, 48, 256, "wgrad_16_partials_tall")
    add(1, 8257, 257, 256, "outer_16_chunk_cap", "mlp0_chunk_160", "attn_kv_last_block_one_token")
    add(2, 40, 1300, 256, "short_x_long_split_source")
    add(2, 1300, 40, 256, "long_split_x_short_source")
    add(11, 25, 25, 128, "fine_beyond_one_partial")
    add(41, 25, 25, 128, "fine_beyond_one_partial", "fine_tall")
    add(77, 25, 25, 128, "fine_beyond_one_partial", "fine_tall", "fine_tall_wgrad")
    add(3, 1025, 1089, 256, "mask_src_boundary_inside_chunk", "mask_src_chunk_fully_masked", "mask_src_single_valid_token", "mask_x_boundary_inside_chunk",
        "mask_pair_without_padding", masks="split", tag="mask_")
    add(3, 1089, 1025, 256, "mask_x_boundary_inside_chunk", "mask_x_chunk_fully_masked", "mask_x_single_valid_token", "mask_src_boundary_inside_chunk",
        "mask_pair_without_padding", masks="split_t", tag="mask_")
    add(2, 40, 56, 256, "masked_small", masks="golden", tag="mask_")
    add(3, 256, 40, 256, "tiny_gradient", gmode="tiny", tag="gtiny_")
    add(1, 1300, 300, 256, "row_magnitudes", gmode="rows", tag="grows_")
    return cases


CASES = _build_cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
# (case, switches): the paths the debug switches select, on the same cases, reference and tolerances
FORCED = [(name, sw) for name in ("1x1025x1024x256", "41x25x25x128") for sw in (dict(wgrad_chunk=512), dict(wgrad_chunk=128, reduce_tall=0))]
FORCED.append(("1x1921x48x256", dict(reduce_tall=0)))
SWITCH_DEFAULTS = {"wgrad_chunk": 0, "reduce_tall": 1}
MAX_ELEMENTS = 8257 * 256


def masks(c):
    """(x_mask [nb, L], source_mask [nb, S]) bool, True = valid; (None, None) without masks.
    split:   pair 0 -- source valid below 700 (S = 1089, chunks [0, 384) [384, 768) [768, 1089): the second is cut, the third fully masked),
             x valid below 725;  pair 1 -- ONE valid source token;  pair 2 -- no padding.      split_t: the two sides exchanged.
    golden:  the masks of glayer_cross_mask."""
    if c.masks is None:
        return None, None
    xm, sm = np.ones((c.nb, c.L), bool), np.ones((c.nb, c.S), bool)
    if c.masks == "golden":
        xm[0, c.L - 7:], sm[0, c.S - 11:], sm[1, c.S - 3:] = False, False, False
    elif c.masks == "split":
        sm[0, 700:], xm[0, 725:], sm[1, 1:] = False, False, False
    elif c.masks == "split_t":
        xm[0, 700:], sm[0, 725:], xm[1, 1:] = False, False, False
    else:
        raise KeyError(c.masks)
    return xm, sm


def edge_failures():
    """[(case, edge)] where a case is not at the edge it is in the table for."""
    return [(c.name, e) for c in CASES for e in c.edges if not EDGES[e](c, plan(c.nb, c.L, c.S, c.C, c.H))]


assert not edge_failures(), edge_failures()
assert all(c.edges for c in CASES) and {e for c in CASES for e in c.edges} == set(EDGES), set(EDGES) - {e for c in CASES for e in c.edges}
assert max(c.nb * max(c.L, c.S) * c.C for c in CASES) <= MAX_ELEMENTS


# ---- the layer, restated ---------------------------------------------------------------------------------------------------------------
def layer(x, source, w, H, x_mask=None, source_mask=None, keep=None):
    """out [nb, L, C] of one encoder layer with linear attention; w: field -> tensor.  keep: a dict that receives the intermediates
    `k` (the key projection), `pre` (mlp.0's pre-activations) and `hcat` (its input), with their gradients retained."""
    nb, L, C = x.shape
    S, D = source.shape[1], C // H
    q = (x @ w["q_proj"].t()).view(nb, L, H, D)
    k = source @ w["k_proj"].t()
    v = (source @ w["v_proj"].t()).view(nb, S, H, D)
    Q, Kf = F.elu(q) + 1, F.elu(k.view(nb, S, H, D)) + 1
    if x_mask is not None:
        Q = Q * x_mask[:, :, None, None]
    if source_mask is not None:
        Kf, v = Kf * source_mask[:, :, None, None], v * source_mask[:, :, None, None]
    v = v / S
    KV = torch.einsum("nshd,nshv->nhdv", Kf, v)
    Z = 1 / (torch.einsum("nlhd,nhd->nlh", Q, Kf.sum(dim=1)) + 1e-6)
    msg = (torch.einsum("nlhd,nhdv,nlh->nlhv", Q, KV, Z) * S).reshape(nb, L, C)
    msg = F.layer_norm(msg @ w["merge"].t(), (C,), w["norm1_w"], w["norm1_b"])
    hcat = torch.cat([x, msg], dim=2)
    pre = hcat @ w["mlp0"].t()
    if keep is not None:
        for t in (k, pre, hcat):
            if t.requires_grad:
                t.retain_grad()
        keep.update(k=k, pre=pre, hcat=hcat)
    msg = F.layer_norm(torch.relu(pre) @ w["mlp2"].t(), (C,), w["norm2_w"], w["norm2_b"])
    return x + msg


def run_layer(inp, dtype, G=None, x_mask=None, source_mask=None, keep=None):
    """{out, grad_x, grad_source, grad_<field>} (numpy, of `dtype`) of the restated layer under torch.autograd on the CPU.  G, x_mask and
    source_mask default to the case's own."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)                       # (a copy: the shared inputs are read-only)
    x, s = t(inp["x"]).requires_grad_(True), t(inp["source"]).requires_grad_(True)
    w = {f: t(inp["w"][n]).requires_grad_(True) for f, n in MG.FIELDS}
    xm = inp["x_mask"] if x_mask is None else x_mask
    sm = inp["source_mask"] if source_mask is None else source_mask
    out = layer(x, s, w, inp["H"], None if xm is None else t(xm), None if sm is None else t(sm), keep)
    out.backward(t(inp["G"] if G is None else G))
    r = dict(out=out.detach().numpy(), grad_x=x.grad.numpy(), grad_source=s.grad.numpy(), **{"grad_" + f: w[f].grad.numpy() for f in FIELDS})
    if keep is not None:
        keep.update({key: (v.detach().numpy(), None if v.grad is None else v.grad.numpy()) for key, v in list(keep.items())})
    return r


def pre_activations(inp, rows=None):
    """mlp.0's pre-activations in float64, [nb L, 2C] (of all rows: the attention of a row depends on no other row of x)."""
    t = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=torch.float64)
    keep = {}
    with torch.no_grad():
        layer(t(inp["x"]), t(inp["source"]), {f: t(inp["w"][n]) for f, n in MG.FIELDS}, inp["H"], t(inp["x_mask"]), t(inp["source_mask"]), keep)
    return keep["pre"].numpy().reshape(-1, keep["pre"].shape[-1])


def relu_margin(c, pre):
    """The smallest |pre-activation| in units of its yardstick: the largest |pre-activation| of the tensor, or of the entry's row where
    rows of x carry magnitudes of their own (gmode "rows"; see the module docstring)."""
    a = np.abs(pre)
    ref = a.max(axis=1, keepdims=True) if c.gmode == "rows" else a.max()
    return a / ref


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Seeded float32 x, source, G (drawn independently, in the order of make_golden_layer_grad.build), weights of
    make_golden_layer_grad.layer_weights, masks; the ReLU condition enforced by redrawing rows of x.  Shared by every test: read-only."""
    c = CASE_BY_NAME[name]
    rng = np.random.default_rng([c.nb, c.L, c.S, c.C, c.seed])
    x = rng.standard_normal((c.nb, c.L, c.C)).astype(np.float32)
    source = rng.standard_normal((c.nb, c.S, c.C)).astype(np.float32)
    G = rng.standard_normal((c.nb, c.L, c.C)).astype(np.float32)
    w = MG.layer_weights(rng, c.C)
    rowscale = np.ones((c.nb, c.L, 1), np.float32)
    if c.gmode == "tiny":
        G *= np.float32(G_TINY)
    elif c.gmode == "rows":                       # the running tile scale of head_grad_kernel, the per-row operand scale of loftr_linear_fwd
        G *= (np.exp(-14.0 * rng.random((c.nb, c.L, 1))) * 1e-2).astype(np.float32)
        rowscale[rng.random((c.nb, c.L, 1)) < 0.1] = 30.0
        x *= rowscale
    xm, sm = masks(c)
    inp = dict(case=c, x=x, source=source, G=G, w=w, x_mask=xm, source_mask=sm, H=c.H)
    rounds = 0
    while True:
        bad = np.flatnonzero((relu_margin(c, pre_activations(inp)) < RELU_MARGIN).any(axis=1))
        if bad.size == 0 or rounds == RELU_ROUNDS:
            break
        rounds += 1
        flat = x.reshape(-1, c.C)
        flat[bad] = rng.standard_normal((bad.size, c.C)).astype(np.float32) * rowscale.reshape(-1, 1)[bad]
    assert bad.size == 0, (name, "the redraw loop did not end", rounds, bad.size)
    inp["relu_rounds"] = rounds
    _freeze(x, source, G, xm, sm, *w.values())
    return inp


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref64 / ref32 (key -> array), and per key noise = max|ref32 - ref64| and scale = max|ref64|; the retained intermediates of the
    float64 run (k, pre, hcat: (value, gradient))."""
    inp = inputs(name)
    keep = {}
    ref64, ref32 = run_layer(inp, torch.float64, keep=keep), run_layer(inp, torch.float32)
    assert all(v.dtype == np.float64 for v in ref64.values()) and all(v.dtype == np.float32 for v in ref32.values())
    _freeze(*ref64.values(), *ref32.values())
    return dict(ref64=ref64, ref32=ref32, keep=keep, noise={k: float(np.abs(ref32[k] - ref64[k]).max()) for k in OUTPUTS},
                scale={k: float(np.abs(ref64[k]).max()) for k in OUTPUTS})


def distance_in_tolerances(got, r):
    """The largest max|got - ref64| over the tensors of `got`, each in units of its tolerance."""
    return max(float(np.abs(np.asarray(v, np.float64) - r["ref64"][k]).max()) / tolerance(k, r["noise"][k], r["scale"][k]) for k, v in got.items())


# ---- modelled mistakes, on ref64 ---------------------------------------------------------------------------------------------------------
MUTATIONS = ("lost_token", "lost_chunk", "mask_ignored", "layernorm_partial", "residual_dropped")


def mutation_applies(c, m):
    if m == "lost_chunk":
        return outer_splits(c.S)[0] >= 2
    if m == "mask_ignored":
        return c.masks is not None
    return True


def mutated(name, m):
    """The tensors a kernel with the mistake `m` would return where they differ from ref64 (key -> float64 array)."""
    inp, r = inputs(name), reference(name)
    c, ref = inp["case"], r["ref64"]
    if m == "lost_token":                         # the last token of the last split-K partial, missing from d k_proj and from d mlp.0
        (_, dk), (_, dpre), (hcat, _) = r["keep"]["k"], r["keep"]["pre"], r["keep"]["hcat"]
        src = inp["source"].astype(np.float64)
        return {"grad_k_proj": ref["grad_k_proj"] - np.outer(dk[-1, -1], src[-1, -1]), "grad_mlp0": ref["grad_mlp0"] - np.outer(dpre[-1, -1], hcat[-1, -1])}
    if m == "lost_chunk":                         # the last outer_accum chunk of the source missing from KV and Ksum: those tokens masked
        sm = np.ones((c.nb, c.S), bool) if inp["source_mask"] is None else inp["source_mask"].copy()
        sm[:, outer_chunks(c.S)[-1][0]:] = False
        xm = np.ones((c.nb, c.L), bool) if inp["x_mask"] is None else inp["x_mask"]
        return run_layer(inp, torch.float64, x_mask=xm, source_mask=sm)
    if m == "mask_ignored":                       # one masked source token counted
        sm = inp["source_mask"].copy()
        n, s = np.argwhere(~sm)[0]
        sm[n, s] = True
        return run_layer(inp, torch.float64, source_mask=sm)
    if m == "layernorm_partial":                  # the last, ragged, 64-row block missing from d norm2.weight / d norm2.bias
        G = inp["G"].copy().reshape(-1, c.C)
        G[(plan(c.nb, c.L, c.S, c.C, c.H).nlb - 1) * LN_ROWS_PB:] = 0
        got = run_layer(inp, torch.float64, G=G.reshape(c.nb, c.L, c.C))
        return {k: got[k] for k in ("grad_norm2_w", "grad_norm2_b")}
    if m == "residual_dropped":                   # grad_x of the last token without + G
        gx = ref["grad_x"].copy()
        gx[-1, -1] -= inp["G"][-1, -1].astype(np.float64)
        return {"grad_x": gx}
    raise KeyError(m)


# ---- the conditions on the inputs, as figures --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def facts(name):
    """What tests/test_encoder_bwd_oracle.py asserts, computed in one pass over the case's reference."""
    inp, r = inputs(name), reference(name)
    c = inp["case"]
    pre64 = r["keep"]["pre"][0].reshape(-1, 2 * c.C)
    sm = inp["source_mask"]
    return dict(relu_rounds=inp["relu_rounds"], relu_margin=float(relu_margin(c, pre64).min()),
                finite=all(bool(np.isfinite(r[k][o]).all()) for k in ("ref64", "ref32") for o in OUTPUTS), noise=r["noise"], scale=r["scale"],
                min_valid_source=c.S if sm is None else int(sm.sum(1).min()),
                elements=max(int(np.prod(r["ref64"][k].shape)) for k in OUTPUTS),
                mutation_distance={m: distance_in_tolerances(mutated(name, m), r) for m in MUTATIONS if mutation_applies(c, m)})
