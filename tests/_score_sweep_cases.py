"""Case table, float64 reference and tolerances of the dual-softmax score sweep's edge tests.

tests/test_hip_score_sweep_edges.py (GPU) compares `ops.coarse_match` at C = 256 with the numpy oracle evaluated in float64 at the sizes
where the hand-written work distribution of csrc/score_sweep.h (sweep::score_sweep_kernel), sweep_plan, merge_stats_kernel,
merge_colmax_kernel and select_kernel changes path: 32 rows per wave and 256 per workgroup (rows beyond L re-read row L - 1), 32-column
panels in a four-stage ring filled two panels ahead (a ragged last panel has a clamped DMA and element-wise stores), chunks of at most 30
panels, (pair, chunk) groups dealt over 8 XCDs, and the numerical regimes of pass A (one shared exp reference per 32 x 32 tile while the
tile's spread stays below FAST_SPREAD = 64 and the unit has no ragged panel; per-row / per-column references otherwise) and pass B
(log-sum-exp form, masked form with dead units skipped, per-element or per-panel arg-max tracking).
tests/test_score_sweep_oracle.py (CPU) holds every condition on the inputs that is stated here and shows that the comparison can fail.

Reference: `oracle.loftr_oracle.dual_softmax_conf` (Sinkhorn cases: `sinkhorn_conf`) on the float64 casts of the float32 inputs (ref64)
and on the float32 inputs themselves (ref32).  noise_abs = max|ref32 - ref64| and noise_rel = max|ref32 - ref64| / ref64 are float32's
own distance to exact arithmetic on the case, scale = max ref64.  All three are taken over the entries the respective check uses.

Two checks.  The ABSOLUTE one is the project's (TOL_CONF is its cap); where conf is of the order 1 / (L S) it cannot see a row or column
sum that lost or doubled a term.  The RELATIVE one can: on `flat` inputs every valid entry is >= REL_FLOOR and all are compared; on the
other regimes the entries >= REL_FLOOR are, and they include every row's and every column's maximum.  Its bound stays below
1 / (2 max(L, S)) on every case: half of what one dropped or doubled term changes in a sum of equal terms.

Inputs: seeded standard-normal float32 descriptors with planted correspondences (f1[c] += weight * f0[r]).  Among a pair's valid tokens, every
token of the longer side has a partner (tokens of the shorter side have several, one at full weight), so that every row and every column maximum is a planted entry that leads its
runner-up clearly: the match ids are then those of `coarse_match_select(ref64)` exactly, without a flip allowance.

Masks are MegaDepth-style valid rectangles at the top left.  A pair whose mask is all zero on one side is left out: the data loader pads
images, it cannot produce an image without pixels.  Where border_rm = 0 (a grid side below 4 cells) only ONE image of a pair is padded:
without border removal the reference reports the tied 1 / (L S) entries of padding rows x padding columns as matches, which is no
property of the sweep.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import loftr_oracle as O
from _cases import TOL_CONF

C = 256
TEMPERATURE = 0.1
BIN_SCORE, SKH_ITERS = 1.0, 3                  # the settings of test_sinkhorn_paths_vs_oracle
REL_FLOOR = 1e-12

# ---- tolerance ------------------------------------------------------------------------------------------------------------------------
# err_abs <= min(K_ABS * noise_abs + 1e-6 * scale, TOL_CONF),   err_rel <= K_REL * noise_rel + 1e-6.
# K = twice the largest err / noise measured on an MI355X over all cases and paths, rounded up to an integer (the factor 2 covers
# summation-order differences between machines, as in tests/_encoder_edge_cases.py).  The lines of profiles/score_sweep_accuracy.txt the
# constants were taken from:
#   K_ABS    = 6 <- 2.94   col_S1               conf   abs err 7.224e-07 noise 2.456e-07
#   K_REL    = 7 <- 3.09   row_L1               conf   rel err 1.773e-06 noise 5.732e-07
#   K_ABS_OT = 2 <- 0.82   ot_3x257x961_masked  conf   abs err 5.980e-07 noise 7.330e-07
#   K_REL_OT = 3 <- 1.06   ot_2x33x1921_masked  conf   rel err 4.717e-06 noise 4.455e-06
# The two dual-softmax maxima come from the one-row and the one-column case, where conf is ONE softmax and float32's own noise is at
# its smallest; at full-size units the ratios are 0.3 ... 1.1 relative and up to 2.4 absolute (mag_all_exact, scores of about 100).
K_ABS = 6
K_REL = 7
K_ABS_OT = 2
K_REL_OT = 3
MARGIN_FACTOR = 10.0       # every row / column maximum of ref64 leads its runner-up by this many relative tolerances
DETECTION_FACTOR = 10.0    # a modelled mistake sits this many relative tolerances from ref64 (tests/test_score_sweep_oracle.py)


def abs_tolerance(c, noise_abs, scale):
    return min((K_ABS_OT if c.kind == "ot" else K_ABS) * noise_abs + 1e-6 * scale, TOL_CONF)


def rel_tolerance(c, noise_rel):
    return (K_REL_OT if c.kind == "ot" else K_REL) * noise_rel + 1e-6


# ---- the kernel's work distribution, restated ------------------------------------------------------------------------------------------
BR, WAVE, PC, MAX_PPC, NUM_XCD = 256, 32, 32, 30, 8
FAST_SPREAD = 64.0
Plan = namedtuple("Plan", "RB NP NCH PPC")


def _cdiv(a, b):
    return -(-a // b)


def sweep_plan(L, S):
    """sweep_plan of csrc/coarse_match.hip: a function of (L, S) only."""
    NP = _cdiv(S, PC)
    PPC = _cdiv(NP, _cdiv(NP, MAX_PPC))
    return Plan(_cdiv(L, BR), NP, _cdiv(NP, PPC), PPC)


def chunk_panels(S):
    p = sweep_plan(1, S)
    return [min(p.PPC, p.NP - c * p.PPC) for c in range(p.NCH)]


assert [chunk_panels(S) for S in (1, 160, 957, 960, 961, 992, 1921)] == [[1], [5], [30], [30], [16, 15], [16, 15], [21, 21, 19]]
assert [957 % 32, 957 % 4, 961 % 32, 1921 % 32] == [29, 1, 1, 1]


def grid(n):
    """n tokens as the most nearly square h x w grid; a prime as 1 x n."""
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


assert [grid(n) for n in (255, 256, 513, 957, 960, 961, 992, 1921, 257)] == [(15, 17), (16, 16), (19, 27), (29, 33), (30, 32), (31, 31),
                                                                              (31, 32), (17, 113), (1, 257)]


def border_rm(L, S):
    """1 where both grids have an interior worth the name (every side >= 4 cells), else 0 (primes are 1 x n grids)."""
    return 1 if min(grid(L) + grid(S)) >= 4 else 0


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
# kind: "ds" dual softmax, "ot" Sinkhorn (the sweep's pass 2 stores the scores).  regime: see REGIMES.  masked: None or a pattern of masks().
Case = namedtuple("Case", "name kind N L S regime masked seed")
# planted weight, descriptor amplitude, weight of a token's further partners relative to its first.  flat: tile spreads of about 10, every conf >= REL_FLOOR; peaked: as the existing tests, spreads of
# about 24, conf reaches 1; the other three are `peaked` with a few rows / columns multiplied (regime_scaling); ot: the existing Sinkhorn
# test's inputs (no temperature: scores are dot / 256).
REGIMES = {"flat": (0.5, 1.0, 0.6), "peaked": (1.5, 1.0, 0.8), "near_limit": (1.5, 1.0, 0.8), "mixed": (1.5, 1.0, 0.8), "all_exact": (1.5, 1.0, 0.8),
           "ot": (1.5, 2.0, 0.6)}
# f1 = BACKGROUND * noise + sum over its partners of weight_k * f0[partner]: a planted score is weight_k |f0|^2 / (C * temperature), about
# 10 weight_k, and two partners of one token differ by 2.0 (flat) or 3.0 (peaked) against a noise of 0.22.  (peaked: 0.8, because the further
# partner of a row multiplied by alpha has conf exp(-(1 - 0.8) 15 alpha) in its column, which has to stay above REL_FLOOR.)
BACKGROUND = 0.25
ROW_EDGES = (1, 31, 32, 33, 255, 256, 257, 513)                                     # S = 160, N = 3
COL_EDGES = (1, 3, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 957, 960, 961, 992, 1921)      # L = 257, N = 3
XCD_SHAPES, XCD_N = ((257, 160), (257, 992), (33, 1921)), (1, 3, 8, 9)
MAGNITUDE_SHAPE = (3, 513, 992)
SEEDS = {}                                     # name -> seed other than 0 (chosen where the margin condition missed with seed 0)


def _build_cases():
    cases, seen = [], set()

    def add(name, kind, N, L, S, regime="flat", masked=None):
        key = (kind, N, L, S, regime, masked)
        if key not in seen:                    # (3, 257, 160) and (3, 257, 992) are a row, a column and an XCD case: listed once
            seen.add(key)
            cases.append(Case(name, kind, N, L, S, regime, masked, SEEDS.get(name, 0)))
    for L in ROW_EDGES:
        add(f"row_L{L}", "ds", 3, L, 160)
    for S in COL_EDGES:
        add(f"col_S{S}", "ds", 3, 257, S)
    for L, S in XCD_SHAPES:
        for N in XCD_N:
            add(f"xcd_N{N}_{L}x{S}", "ds", N, L, S)
    for regime in ("flat", "peaked", "near_limit", "mixed", "all_exact"):
        add(f"mag_{regime}", "ds", *MAGNITUDE_SHAPE, regime=regime)
    add("mask_3x513x992", "ds", 3, 513, 992, masked="units")
    add("mask_2x257x961", "ds", 2, 257, 961, masked="one_side")
    add("mask_9x33x160", "ds", 9, 33, 160, masked="one_side")
    for N, L, S in ((3, 257, 961), (2, 33, 1921), (3, 257, 957)):
        add(f"ot_{N}x{L}x{S}", "ot", N, L, S, regime="ot")
        add(f"ot_{N}x{L}x{S}_masked", "ot", N, L, S, regime="ot", masked="one_side")
    return cases


CASES = _build_cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
DS_CASES = [c for c in CASES if c.kind == "ds"]
OT_CASES = [c for c in CASES if c.kind == "ot"]
assert max(c.N * c.L * c.S for c in CASES) == max(9 * 257 * 992, 3 * 513 * 992)


def is_flat(c):
    return c.regime == "flat"


def is_degenerate(c):
    """Too few tokens for the 'more than 10 matches' condition (L = 1, S = 1, S = 3 at N = 3)."""
    return c.N * min(c.L, c.S) <= 10


def masks(c):
    """(m0 [N, h0, w0], m1 [N, h1, w1]) bool valid rectangles at the top left, or (None, None)."""
    if c.masked is None:
        return None, None
    (h0, w0), (h1, w1) = grid(c.L), grid(c.S)
    m0, m1 = np.ones((c.N, h0, w0), bool), np.ones((c.N, h1, w1), bool)

    def crop(m, n, vh, vw):
        m[n, vh:] = False
        m[n, :, vw:] = False
    if c.masked == "units":
        assert (c.N, c.L, c.S) == (3, 513, 992) and sweep_plan(c.L, c.S) == Plan(3, 31, 2, 16)
        crop(m0, 0, 17, 25); crop(m1, 0, 29, 30)       # the valid extent ends inside a wave (row 16 * 27 + 24 = 456) and inside a panel (column 28 * 32 + 29 = 925)
        crop(m0, 1, 9, 27)                             # 9 * 27 = 243 valid rows: row blocks 1 and 2 are all padding -> dead units (image 1 whole)
        crop(m1, 2, 15, 29)                            # 15 * 32 = 480 columns: chunk 1 (columns 512 ...) is all padding -> dead units
        assert m0[1].reshape(-1)[BR:].sum() == 0 and m1[2].reshape(-1)[16 * PC:].sum() == 0
        assert (np.flatnonzero(m0[0].reshape(-1))[-1] + 1) % WAVE != 0 and (np.flatnonzero(m1[0].reshape(-1))[-1] + 1) % PC != 0
    elif c.masked == "one_side":
        # even pairs pad image 0, odd pairs image 1 (the module docstring says why not both); the last pair that keeps image 1 whole
        # keeps the ragged last panel's columns valid
        for n in range(c.N):
            m, h, w = (m0, h0, w0) if n % 2 == 0 else (m1, h1, w1)
            crop(m, n, h if h < 3 else h - 1 - n % max(1, h // 3), w - 2 - (3 * n) % max(1, w // 4))
    else:
        raise KeyError(c.masked)
    assert m0.reshape(c.N, -1).any(1).all() and m1.reshape(c.N, -1).any(1).all()
    return m0, m1


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False


def correspondences(v0, v1, rng):
    """(rows, cols, first): the planted pairs of one image pair among its valid tokens v0 / v1 (index arrays).  Every token of the longer
    side has one partner, tokens of the shorter side several; `first` marks the one partner of each that gets the full weight (the others
    get a fraction of it, so that no two partners of a token tie).  The last valid row and the first valid column are full-weight partners."""
    nr, nc = len(v0), len(v1)
    if nc >= nr:
        t = np.arange(nc)
        return v0[rng.permutation(nr)[t % nr]], v1, t < nr
    t = np.arange(nr)
    return v0, v1[rng.permutation(nc)[(nr - 1 - t) % nc]], t >= nr - nc


def scores64(f0, f1, kind="ds"):
    """The float64 score volume as the oracle forms it (coarse_matching.py:108-114; Sinkhorn: no temperature)."""
    s = (f0.astype(np.float64) / C ** .5) @ (f1.astype(np.float64) / C ** .5).transpose(0, 2, 1)
    return s / TEMPERATURE if kind == "ds" else s


def unit_spreads(scores, L, S):
    """[N, RB, NCH]: the largest max - min over the kernel's 32 x 32 tiles of each work unit (pair, 256-row block, chunk).  The kernel's
    tiles: wave rows clamped to L - 1, 32-column panels (a ragged panel's columns clamped to S - 1)."""
    p = sweep_plan(L, S)
    N = scores.shape[0]
    pad = np.pad(scores, ((0, 0), (0, _cdiv(L, WAVE) * WAVE - L), (0, p.NP * PC - S)), mode="edge")
    t = pad.reshape(N, -1, WAVE, p.NP, PC)
    sp = t.max(axis=(2, 4)) - t.min(axis=(2, 4))
    out = np.zeros((N, p.RB, p.NCH))
    for rb in range(p.RB):
        for cc in range(p.NCH):
            out[:, rb, cc] = sp[:, rb * (BR // WAVE):(rb + 1) * (BR // WAVE), cc * p.PPC:(cc + 1) * p.PPC].max(axis=(1, 2))
    return out


SPREAD_LOW, SPREAD_HIGH = 56.0, 72.0           # a margin of 8 on either side of FAST_SPREAD: float32 rounding of scores below 100 is 1e-5
NEAR_LIMIT = (48.0, 56.0)


def regime_scaling(c, corr):
    """(scaled rows [(pair, row)], scaled columns [(pair, column)], intended units as a bool [N, RB, NCH] or None)."""
    if c.regime not in ("near_limit", "mixed", "all_exact"):
        return [], [], None
    p = sweep_plan(c.L, c.S)
    assert c.S >= c.L and p.RB >= 2 and p.NCH >= 2
    chunk_of = lambda j: j // (p.PPC * PC)

    def row_with_partners_in_every_chunk(n, rb):
        rows, cols, _ = corr[n]
        for i in range(rb * BR, min(c.L, (rb + 1) * BR)):
            if set(chunk_of(cols[rows == i])) == set(range(p.NCH)):
                return i
        raise AssertionError(("no row with a partner in every chunk", c.name, rb))

    def column_with_partner_in(n, rb, cc):
        rows, cols, _ = corr[n]
        for j in range(cc * p.PPC * PC, min(c.S, (cc + 1) * p.PPC * PC)):
            if rows[j] // BR == rb:
                return j
        raise AssertionError(("no column with its partner in the row block", c.name, rb, cc))
    intended = np.zeros((c.N, p.RB, p.NCH), bool)
    if c.regime == "all_exact":
        intended[:] = True
        return [(n, row_with_partners_in_every_chunk(n, rb)) for n in range(c.N) for rb in range(p.RB)], [], intended
    # rows of row block 1 of pair 0, columns of chunk 1 of pair 1
    intended[0, 1, :] = True
    intended[1, :, 1] = True
    return [(0, row_with_partners_in_every_chunk(0, 1))], [(1, column_with_partner_in(1, rb, 1)) for rb in range(p.RB)], intended


def _scaled(f0, f1, srows, scols, alpha):
    f0, f1 = f0.copy(), f1.copy()
    for n, i in srows:
        f0[n, i] *= np.float32(alpha)
    for n, j in scols:
        f1[n, j] *= np.float32(alpha)
    return f0, f1


def _regime_measure(c, spreads, intended):
    return float(spreads.max()) if c.regime == "near_limit" else float(spreads[intended].min())


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Seeded float32 descriptors, masks, grids.  Shared by every test: read-only."""
    c = CASE_BY_NAME[name]
    weight, amp, more = REGIMES[c.regime]
    rng = np.random.default_rng([c.N, c.L, c.S, c.seed])
    f0 = rng.standard_normal((c.N, c.L, C)).astype(np.float32) * np.float32(amp)
    f1 = rng.standard_normal((c.N, c.S, C)).astype(np.float32) * np.float32(amp)
    f1 *= np.float32(BACKGROUND)
    m0, m1 = masks(c)
    corr = []
    for n in range(c.N):
        v0 = np.arange(c.L) if m0 is None else np.flatnonzero(m0[n].reshape(-1))
        v1 = np.arange(c.S) if m1 is None else np.flatnonzero(m1[n].reshape(-1))
        rows, cols, first = correspondences(v0, v1, rng)
        np.add.at(f1[n], cols, np.where(first, weight, more * weight).astype(np.float32)[:, None] * f0[n, rows])
        corr.append((rows, cols, first))
    srows, scols, intended = regime_scaling(c, corr)
    alpha = 1.0
    if intended is not None:
        # the factor that brings the largest tile spread (near_limit) / the smallest of the intended units' spreads (mixed, all_exact)
        # to the target, rounded to 1 / 64 so that it does not depend on the last bits of a matrix product
        target = 52.0 if c.regime == "near_limit" else 80.0
        alpha = 3.0
        for _ in range(12):
            m = _regime_measure(c, unit_spreads(scores64(*_scaled(f0, f1, srows, scols, alpha)), c.L, c.S), intended)
            if abs(m - target) <= 1.0:
                break
            alpha = round(alpha * target / m * 64) / 64
        f0, f1 = _scaled(f0, f1, srows, scols, alpha)
    _freeze(f0, f1, m0, m1, intended)
    return dict(case=c, f0=f0, f1=f1, m0=m0, m1=m1, hw0=grid(c.L), hw1=grid(c.S), border_rm=border_rm(c.L, c.S), corr=corr,
                scaled_rows=srows, scaled_cols=scols, alpha=alpha, intended=intended)


def flat_masks(i):
    c = i["case"]
    return (None, None) if i["m0"] is None else (i["m0"].reshape(c.N, -1), i["m1"].reshape(c.N, -1))


def valid_entries(i):
    c = i["case"]
    m0, m1 = flat_masks(i)
    return np.ones((c.N, c.L, c.S), bool) if m0 is None else (m0[:, :, None] & m1[:, None, :])


def _oracle_conf(i, dt):
    c = i["case"]
    m0, m1 = flat_masks(i)
    if c.kind == "ds":
        return O.dual_softmax_conf(i["f0"].astype(dt), i["f1"].astype(dt), TEMPERATURE, m0, m1)
    return O.sinkhorn_conf(i["f0"].astype(dt), i["f1"].astype(dt), dt(BIN_SCORE), SKH_ITERS, m0, m1)[0]


@functools.lru_cache(maxsize=2)               # (volumes of up to 2.3 M float64 entries: the figures below are what stays cached)
def reference(name):
    """ref64, ref32, the valid entries, the entries of the relative check, the reference selection, noise and scale."""
    i = inputs(name)
    c = i["case"]
    ref64, ref32 = _oracle_conf(i, np.float64), _oracle_conf(i, np.float32)
    assert ref64.dtype == np.float64 and ref32.dtype == np.float32
    valid = valid_entries(i)
    relset = valid & (ref64 >= REL_FLOOR)
    d = np.abs(ref32 - ref64)
    sel = O.coarse_match_select(ref64, 0.0, i["border_rm"], i["hw0"], i["hw1"], (i["hw0"][0] * 8, i["hw0"][1] * 8), i["m0"], i["m1"])
    _freeze(ref64, ref32, valid, relset)
    return dict(ref64=ref64, ref32=ref32, valid=valid, relset=relset, sel=sel, noise_abs=float(d[valid].max()),
                scale=float(ref64[valid].max()), noise_rel=float((d[relset] / ref64[relset]).max()))


def rel_error(got, r):
    """max |got - ref64| / ref64 over the entries of the relative check."""
    return float((np.abs(got - r["ref64"])[r["relset"]] / r["ref64"][r["relset"]]).max())


# ---- the float64 dual softmax once more, with one mistake built in ----------------------------------------------------------------------
MUTATIONS = ("row_sum_omits_last_column", "col_sum_counts_last_row_twice", "row_sum_omits_first_column_of_chunk_1",
             "col_stats_shifted_in_last_panel")


def mutation_applies(c, m, i=None):
    """By shape; with masks the entries the mistake touches also have to be valid in some pair."""
    p = sweep_plan(c.L, c.S)
    m0, m1 = flat_masks(i if i is not None else inputs(c.name))
    v0 = np.ones((c.N, c.L), bool) if m0 is None else m0
    v1 = np.ones((c.N, c.S), bool) if m1 is None else m1
    if c.kind != "ds":
        return False
    if m == "row_sum_omits_last_column":                       # the ragged panel
        return c.S % PC != 0 and c.S > 1 and bool((v1[:, c.S - 1] & (v1.sum(1) > 1)).any())
    if m == "col_sum_counts_last_row_twice":                   # the clamped phantom row of a partial row block
        return c.L % BR != 0 and bool(v0[:, c.L - 1].any())
    if m == "row_sum_omits_first_column_of_chunk_1":
        return p.NCH >= 2 and bool(v1[:, p.PPC * PC].any())
    if m == "col_stats_shifted_in_last_panel":
        return bool((v1[:, (p.NP - 1) * PC:].sum(1) >= 2).any())
    raise KeyError(m)


def dual_softmax_float64(name, mutation=None):
    """coarse_matching.py:105-119 in float64 from its pieces.  mutation None reproduces oracle.dual_softmax_conf (tested)."""
    i = inputs(name)
    c = i["case"]
    p = sweep_plan(c.L, c.S)
    sim = scores64(i["f0"], i["f1"])
    if i["m0"] is not None:
        sim = np.where(valid_entries(i), sim, -O.INF)
    er = np.exp(sim - sim.max(axis=2, keepdims=True))          # softmax over the columns (dim 2): row statistics
    ec = np.exp(sim - sim.max(axis=1, keepdims=True))          # softmax over the rows (dim 1): column statistics
    rs, cs = er.sum(axis=2, keepdims=True), ec.sum(axis=1, keepdims=True)
    if mutation == "row_sum_omits_last_column":
        rs = rs - er[:, :, c.S - 1:]
    elif mutation == "col_sum_counts_last_row_twice":
        cs = cs + ec[:, c.L - 1:, :]
    elif mutation == "row_sum_omits_first_column_of_chunk_1":
        j = p.PPC * PC
        rs = rs - er[:, :, j:j + 1]
    elif mutation == "col_stats_shifted_in_last_panel":
        # column j of the last panel is normalised with the (max, sum) of its right-hand neighbour (cyclic inside the panel)
        j0 = (p.NP - 1) * PC
        sh = np.concatenate([np.arange(j0), j0 + (np.arange(c.S - j0) + 1) % (c.S - j0)])
        cmax = sim.max(axis=1, keepdims=True)
        with np.errstate(over="ignore"):                                   # (a padding column's -1e9 beside a valid one)
            ec = np.exp(sim - cmax[:, :, sh])
        cs = cs[:, :, sh]
    elif mutation is not None:
        raise KeyError(mutation)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (ec / cs) * (er / rs)


# ---- the conditions on the inputs, as figures (cached per case; the volumes are not) ----------------------------------------------------
def _top2_margin(x, axis):
    """(top - runner-up) / top along an axis of a non-negative array (1 where there is no second entry)."""
    if x.shape[axis] < 2:
        return np.ones(tuple(np.delete(x.shape, axis)))
    t = np.partition(x, -2, axis=axis)
    top, second = np.take(t, -1, axis=axis), np.take(t, -2, axis=axis)
    with np.errstate(divide="ignore", invalid="ignore"):                # (rows / columns without a valid entry: not looked at)
        return (top - second) / top


@functools.lru_cache(maxsize=None)
def facts(name):
    """What tests/test_score_sweep_oracle.py asserts, computed in one pass over the case's reference."""
    i, r = inputs(name), reference(name)
    c = i["case"]
    m0, m1 = flat_masks(i)
    v0 = np.ones((c.N, c.L), bool) if m0 is None else m0
    v1 = np.ones((c.N, c.S), bool) if m1 is None else m1
    x = np.where(r["valid"], r["ref64"], 0.0)
    rowmax, colmax = x.max(axis=2), x.max(axis=1)
    f = dict(noise_abs=r["noise_abs"], noise_rel=r["noise_rel"], scale=r["scale"], finite=bool(np.isfinite(r["ref64"]).all() and np.isfinite(r["ref32"]).all()),
             min_valid=float(r["ref64"][r["valid"]].min()), all_valid_in_relset=bool((r["relset"] == r["valid"]).all()),
             maxima_in_relset=bool((rowmax[v0] >= REL_FLOOR).all() and (colmax[v1] >= REL_FLOOR).all()),
             row_margin=float(_top2_margin(x, 2)[v0].min()), col_margin=float(_top2_margin(x, 1)[v1].min()),
             matches=len(r["sel"]["b_ids"]), matches_per_pair=np.bincount(r["sel"]["b_ids"], minlength=c.N).tolist())
    if c.kind == "ds":
        f["hooked_distance"] = float(np.abs(np.where(r["valid"], dual_softmax_float64(name) - r["ref64"], 0.0)).max())
        if is_flat(c):
            f["mutation_distance"] = {m: rel_error(dual_softmax_float64(name, m), r) for m in MUTATIONS if mutation_applies(c, m, i)}
        if i["m0"] is None:
            f["unit_spreads"] = unit_spreads(scores64(i["f0"], i["f1"]), c.L, c.S)
    return f
