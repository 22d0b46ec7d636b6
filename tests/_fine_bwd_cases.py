"""Case table, float64 reference and tolerances of the FinePreprocess backward's edge tests.

tests/test_hip_fine_bwd_edges.py (GPU) runs `FinePreprocess(...).train()` of loftr_amd.loftr under autograd (forward: ops.fine_preprocess;
backward: loftr_fine_preprocess_bwd, csrc/fine_bwd.hip, with launch_wgrad / launch_colsum / launch_reduce_partials of
csrc/head_grads.hip) against torch.autograd of the module in FLOAT64 at the match counts where the work distribution changes path.  With
M matches and W x W windows the merge_feat gradients reduce over T = 2 M W^2 rows, the down_proj gradients over R = 2 M rows:
  * launch_wgrad at O = Cf = 128 (one row tile, chunk 128): one short partial (M = 1), a second partial of 22 rows (M = 3), 25 full
    partials (M = 64), 17 partials through the tall reduction (M = 41); the down-projection gradient at R = 128 (one full partial) and
    R = 130 (a second partial of two rows);
  * colsum_part_kernel (COLSUM_ROWS = 256 rows per block): T = 250 in one block, T = 300 with 44 rows in a second;
  * scatter_windows_kernel / scatter_cc_kernel: atomic adds of windows clipped at the four corners of the maps, of neighbouring windows
    (5 x 5 at stride 4 overlap by one pixel), of two matches on one cell, and of 48 matches on ONE cell of image 0 spread over three
    cells of image 1;
  * another geometry: Cf = 64, Cc = 128, W = 3.
tests/test_fine_bwd_oracle.py (CPU) holds every condition stated here and shows that the comparison can fail.

Reference: `fine_preprocess` below, fine_preprocess.py:29-59 restated in torch (F.unfold with kernel W, stride, padding W // 2), under
torch.autograd on the CPU, on the float64 casts of the float32 inputs (ref64) and on the inputs themselves (ref32).  The CPU test pins it
to the committed gfpre fixture.  The graph is smooth: no condition on the inputs beyond the geometry.

Matches: N = 2 pairs, maps of 6 x 8 and 5 x 9 coarse cells.  The first four matches sit on the four corner cells of both maps (windows
clipped on two sides), as many of them as the case has matches (M = 1 and M = 3 have fewer than four); matches 4 and 5 share their cell
of image 0.  The case `one_cell` puts every match on corner cell 0 of image 0, pair 0.

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

LEAVES = ("feat_f0", "feat_f1", "feat_c0", "feat_c1")
PARAMS = ("down_proj.weight", "down_proj.bias", "merge_feat.weight", "merge_feat.bias")
PARAM_KEY = {n: "grad_" + n.replace(".", "_") for n in PARAMS}
MAPS = ("out0", "out1") + tuple("grad_" + k for k in LEAVES)
OUTPUTS = MAPS + tuple(PARAM_KEY.values())
GROUP = {**{k: "maps" for k in MAPS}, "grad_down_proj_weight": "matrix", "grad_merge_feat_weight": "matrix", "grad_down_proj_bias": "vector",
         "grad_merge_feat_bias": "vector"}

# ---- tolerance ------------------------------------------------------------------------------------------------------------------------
# err <= K[group] * noise + 1e-6 * scale.  K = twice the largest err / noise measured on an MI355X over all cases, both memory formats
# and the tensors of the group, rounded up to an integer (the rule of tests/_sinkhorn_cases.py).  The lines of
# profiles/fine_bwd_accuracy.txt the constants were taken from:
#   K["maps"]   = 4 <- 1.61   one_cell_m48  channels_last grad_feat_c0           maps   err 1.003e-04 noise 6.238e-05 err/noise   1.61 scale 1.809e+02
#   K["matrix"] = 3 <- 1.01   m3            contiguous    grad_down_proj_weight  matrix err 2.191e-05 noise 2.165e-05 err/noise   1.01 scale 1.166e+02
#   K["vector"] = 9 <- 4.25   m5            contiguous    grad_merge_feat_bias   vector err 2.023e-05 noise 4.763e-06 err/noise   4.25 scale 4.792e+01
# (the atomic adds of the two scatter kernels arrive in another order on every run: the `maps` figure of the 48-deep cell moved between
# 1.55 and 1.61 in two runs; every other kernel of this pass sums in a fixed order.)
K = {"maps": 4, "matrix": 3, "vector": 9}
DETECTION_FACTOR = 10.0     # a modelled mistake sits this many tolerances from ref64 in at least one tensor, on every case it applies to


def tolerance(key, noise, scale):
    return K[GROUP[key]] * noise + 1e-6 * scale


# ---- the kernels' work distribution, restated -------------------------------------------------------------------------------------------
COLSUM_ROWS, TALL_FROM = 256, 16


def _cdiv(a, b):
    return -(-a // b)


def wgrad_chunk(T, O):
    """wgrad_chunk of csrc/head_grads.hip."""
    tiles = _cdiv(O, 128)
    target = 1 if tiles >= 256 else 256 // tiles
    return min(max(_cdiv(_cdiv(T, target), 32) * 32, 128), 512)


def wgrad_partials(T, O):
    ns = _cdiv(T, wgrad_chunk(T, O))
    return ns, T - (ns - 1) * wgrad_chunk(T, O)


Plan = namedtuple("Plan", "T R merge down colsum_T colsum_R")


def plan(M, W, Cf):
    """(partials, rows in the last) of the merge_feat and down_proj weight gradients and of the two column sums."""
    T, R = 2 * M * W * W, 2 * M
    blocks = lambda rows: (_cdiv(rows, COLSUM_ROWS), rows - (_cdiv(rows, COLSUM_ROWS) - 1) * COLSUM_ROWS)
    return Plan(T, R, wgrad_partials(T, Cf), wgrad_partials(R, Cf), blocks(T), blocks(R))


EDGES = {
    "single_short_partial": lambda c, p: (p.T, p.R) == (50, 2) and p.merge == (1, 50) and p.down == (1, 2) and p.colsum_T == (1, 50),
    "merge_second_partial_22_rows": lambda c, p: p.T == 150 and p.merge == (2, 22),
    "colsum_below_one_block": lambda c, p: p.T == 250 and p.colsum_T == (1, 250),
    "colsum_second_block": lambda c, p: p.T == 300 and p.colsum_T == (2, 44),
    "down_one_full_partial": lambda c, p: p.R == 128 and p.down == (1, 128),
    "merge_25_full_partials": lambda c, p: p.T == 3200 and p.merge == (25, 128),
    "down_second_partial_two_rows": lambda c, p: p.R == 130 and p.down == (2, 2) and p.T == 3250 and p.merge == (26, 50),
    "merge_17_partials_tall": lambda c, p: p.T == 2050 and p.merge == (17, 2) and p.merge[0] >= TALL_FROM,
    "atomic_depth": lambda c, p: c.layout == "one_cell" and c.M == 48,
    "small_channels_w3": lambda c, p: (c.Cf, c.Cc, c.W, c.M) == (64, 128, 3, 20),
}

Case = namedtuple("Case", "name M Cf Cc W layout seed edges")
N, HC0, HC1, STRIDE = 2, (6, 8), (5, 9), 4
SEEDS = {}
ONE_CELL_J = (0, 22, 44)                       # the three cells of image 1 in `one_cell`: a corner, an interior cell, the last corner


def _build_cases():
    cases = []

    def add(M, *edges, Cf=128, Cc=256, W=5, layout="spread", tag="m"):
        name = f"{tag}{M}"
        cases.append(Case(name, M, Cf, Cc, W, layout, SEEDS.get(name, 0), edges))
    add(1, "single_short_partial")
    add(3, "merge_second_partial_22_rows")
    add(5, "colsum_below_one_block")
    add(6, "colsum_second_block")
    add(64, "down_one_full_partial", "merge_25_full_partials")
    add(65, "down_second_partial_two_rows")
    add(41, "merge_17_partials_tall")
    add(48, "atomic_depth", layout="one_cell", tag="one_cell_m")
    add(20, "small_channels_w3", Cf=64, Cc=128, W=3, tag="w3_m")
    return cases


CASES = _build_cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def edge_failures():
    return [(c.name, e) for c in CASES for e in c.edges if not EDGES[e](c, plan(c.M, c.W, c.Cf))]


assert not edge_failures(), edge_failures()
assert all(c.edges for c in CASES) and {e for c in CASES for e in c.edges} == set(EDGES)


def corners(hw):
    h, w = hw
    return [0, w - 1, (h - 1) * w, h * w - 1]


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Seeded float32 maps, coarse features, match ids, upstream gradients and weights (the recipe of make_golden_layer_grad.build with
    the corner cells on both maps).  Shared by every test: read-only."""
    c = CASE_BY_NAME[name]
    rng = np.random.default_rng([c.M, c.Cf, c.Cc, c.W, c.seed])
    (h0, w0), (h1, w1), M = HC0, HC1, c.M
    b = np.sort(rng.integers(0, N, M)).astype(np.int64)
    i = rng.integers(0, h0 * w0, M).astype(np.int64)
    j = rng.integers(0, h1 * w1, M).astype(np.int64)
    if c.layout == "one_cell":
        b[:], i[:] = 0, 0
        j[:] = np.asarray(ONE_CELL_J)[np.arange(M) % 3]
    else:
        k = min(M, 4)
        i[:k], j[:k], b[:k] = corners(HC0)[:k], corners(HC1)[::-1][:k], 0
        if M >= 6:
            i[5], b[5], j[5] = i[4], b[4], (j[4] + 1) % (h1 * w1)               # cell (b, i) carries two matches
    kai = lambda o, ii: (rng.standard_normal((o, ii)) * np.sqrt(2.0 / o)).astype(np.float32)
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    inp = dict(case=c, feat_f0=f32(N, c.Cf, h0 * STRIDE, w0 * STRIDE), feat_f1=f32(N, c.Cf, h1 * STRIDE, w1 * STRIDE), feat_c0=f32(N, h0 * w0, c.Cc),
               feat_c1=f32(N, h1 * w1, c.Cc), b_ids=b, i_ids=i, j_ids=j, G0=f32(M, c.W ** 2, c.Cf), G1=f32(M, c.W ** 2, c.Cf),
               w={"down_proj.weight": kai(c.Cf, c.Cc), "down_proj.bias": (0.1 * rng.standard_normal(c.Cf)).astype(np.float32),
                  "merge_feat.weight": kai(c.Cf, 2 * c.Cf), "merge_feat.bias": (0.1 * rng.standard_normal(c.Cf)).astype(np.float32)},
               W=c.W, stride=STRIDE, hc0=HC0, hc1=HC1)
    _freeze(*(v for v in inp.values() if isinstance(v, np.ndarray)), *inp["w"].values())
    return inp


# ---- the module, restated --------------------------------------------------------------------------------------------------------------
def windows(feat, W, stride):
    """[N, cells, W W, C]: the W x W window around every stride-th pixel of feat [N, C, H, W'], zero outside the map."""
    n, ch = feat.shape[:2]
    u = F.unfold(feat, kernel_size=(W, W), stride=stride, padding=W // 2)
    return u.view(n, ch, W * W, -1).permute(0, 3, 2, 1)


def fine_preprocess(ff0, ff1, fc0, fc1, w, b, i, j, W, stride, keep=None):
    """(out0, out1) [M, W W, Cf].  keep: a dict that receives `win` [2M, W W, Cf] (the gathered windows of both sides) and `cc` [2M, Cc] (the
    gathered coarse rows), their gradients retained."""
    win = torch.cat([windows(ff0, W, stride)[b, i], windows(ff1, W, stride)[b, j]], 0)
    cc = torch.cat([fc0[b, i], fc1[b, j]], 0)
    if keep is not None:
        win.retain_grad(); cc.retain_grad()
        keep.update(win=win, cc=cc)
    cwin = F.linear(cc, w["down_proj.weight"], w["down_proj.bias"])
    out = F.linear(torch.cat([win, cwin[:, None, :].expand(-1, W * W, -1)], -1), w["merge_feat.weight"], w["merge_feat.bias"])
    return out[:len(b)], out[len(b):]


def run(inp, dtype, keep=None):
    """{out0, out1, grad_feat_*, grad_<parameter>} (numpy, of `dtype`) under torch.autograd on the CPU."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)                       # (a copy: the shared inputs are read-only)
    leaf = {k: t(inp[k]).requires_grad_(True) for k in LEAVES}
    w = {k: t(v).requires_grad_(True) for k, v in inp["w"].items()}
    ids = [torch.tensor(np.asarray(inp[k])) for k in ("b_ids", "i_ids", "j_ids")]
    o0, o1 = fine_preprocess(*(leaf[k] for k in LEAVES), w, *ids, inp["W"], inp["stride"], keep)
    ((o0 * t(inp["G0"])).sum() + (o1 * t(inp["G1"])).sum()).backward()
    if keep is not None:
        keep.update({k: v.grad.numpy() for k, v in list(keep.items())})           # (only the gradients are used)
    return dict(out0=o0.detach().numpy(), out1=o1.detach().numpy(), **{"grad_" + k: v.grad.numpy() for k, v in leaf.items()},
                **{PARAM_KEY[k]: v.grad.numpy() for k, v in w.items()})


@functools.lru_cache(maxsize=None)
def reference(name):
    inp = inputs(name)
    keep = {}
    ref64, ref32 = run(inp, torch.float64, keep), run(inp, torch.float32)
    assert all(v.dtype == np.float64 for v in ref64.values()) and all(v.dtype == np.float32 for v in ref32.values())
    _freeze(*ref64.values(), *ref32.values())
    return dict(ref64=ref64, ref32=ref32, keep=keep, noise={k: float(np.abs(ref32[k] - ref64[k]).max()) for k in OUTPUTS},
                scale={k: float(np.abs(ref64[k]).max()) for k in OUTPUTS})


def distance_in_tolerances(got, r):
    return max(float(np.abs(np.asarray(v, np.float64) - r["ref64"][k]).max()) / tolerance(k, r["noise"][k], r["scale"][k]) for k, v in got.items())


# ---- modelled mistakes, on ref64 ---------------------------------------------------------------------------------------------------------
MUTATIONS = ("clipped_pixel_clamped", "shared_cell_overwritten", "colsum_last_block")


def shared_cells(inp):
    """[(first match, second match)] of the cells (b, i) of image 0 that carry more than one match."""
    seen, pairs = {}, []
    for m, key in enumerate(zip(inp["b_ids"].tolist(), inp["i_ids"].tolist())):
        if key in seen and all(a != seen[key] for a, _ in pairs):
            pairs.append((seen[key], m))
        seen.setdefault(key, m)
    return pairs


def clipped_matches(inp):
    """Matches whose window on image 0 leaves the map."""
    (h, w), r, st = inp["hc0"], inp["W"] // 2, inp["stride"]
    cy, cx = inp["i_ids"] // w * st, inp["i_ids"] % w * st
    return np.flatnonzero((cy - r < 0) | (cx - r < 0) | (cy + r >= h * st) | (cx + r >= w * st))


def mutation_applies(c, m):
    if m == "shared_cell_overwritten":
        return bool(shared_cells(inputs(c.name)))
    return True


def _window_pixels(inp, m):
    """(ww, y, x) of match m's window on image 0, y and x possibly outside the map."""
    (h, w), W, st = inp["hc0"], inp["W"], inp["stride"]
    cell = int(inp["i_ids"][m])
    ww = np.arange(W * W)
    return ww, cell // w * st + ww // W - W // 2, cell % w * st + ww % W - W // 2


def mutated(name, m):
    inp, r = inputs(name), reference(name)
    c, ref, dwin, dcc = inp["case"], r["ref64"], r["keep"]["win"], r["keep"]["cc"]
    Hf, Wf = inp["hc0"][0] * inp["stride"], inp["hc0"][1] * inp["stride"]
    if m == "clipped_pixel_clamped":              # a clipped window's out-of-map pixel scattered to the clamped in-map pixel
        g = ref["grad_feat_f0"].copy()
        for mm in clipped_matches(inp):
            ww, y, x = _window_pixels(inp, mm)
            out = (y < 0) | (y >= Hf) | (x < 0) | (x >= Wf)
            np.add.at(g[inp["b_ids"][mm]], (slice(None), np.clip(y[out], 0, Hf - 1), np.clip(x[out], 0, Wf - 1)), dwin[mm, ww[out]].T)
        return {"grad_feat_f0": g}
    if m == "shared_cell_overwritten":            # the second match of a shared cell overwrites the first instead of adding to it
        gc, gf = ref["grad_feat_c0"].copy(), ref["grad_feat_f0"].copy()
        for first, _ in shared_cells(inp):
            b, i = inp["b_ids"][first], inp["i_ids"][first]
            gc[b, i] -= dcc[first]
            ww, y, x = _window_pixels(inp, first)
            ok = (y >= 0) & (y < Hf) & (x >= 0) & (x < Wf)
            np.add.at(gf[b], (slice(None), y[ok], x[ok]), -dwin[first, ww[ok]].T)
        return {"grad_feat_c0": gc, "grad_feat_f0": gf}
    if m == "colsum_last_block":                  # the ragged last 256-row block missing from d merge_feat.bias
        dy = np.concatenate([inp["G0"], inp["G1"]], 0).astype(np.float64).reshape(-1, c.Cf)
        first = (plan(c.M, c.W, c.Cf).colsum_T[0] - 1) * COLSUM_ROWS
        return {"grad_merge_feat_bias": ref["grad_merge_feat_bias"] - dy[first:].sum(0)}
    raise KeyError(m)


@functools.lru_cache(maxsize=None)
def facts(name):
    inp, r = inputs(name), reference(name)
    c = inp["case"]
    cells0 = set(zip(inp["b_ids"].tolist(), inp["i_ids"].tolist()))
    cells1 = set(zip(inp["b_ids"].tolist(), inp["j_ids"].tolist()))
    depth0 = max(np.bincount(inp["b_ids"] * (HC0[0] * HC0[1]) + inp["i_ids"]))
    return dict(finite=all(bool(np.isfinite(r[k][o]).all()) for k in ("ref64", "ref32") for o in OUTPUTS), noise=r["noise"], scale=r["scale"],
                corners0=sum((0, k) in cells0 for k in corners(HC0)), corners1=sum((0, k) in cells1 for k in corners(HC1)),
                cells0=len(cells0), cells1=len(cells1), depth0=int(depth0), shared=len(shared_cells(inp)), clipped=len(clipped_matches(inp)),
                mutation_distance={m: distance_in_tolerances(mutated(name, m), r) for m in MUTATIONS if mutation_applies(c, m)})
