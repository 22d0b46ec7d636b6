"""Case table, exact reference and modelled mistakes of the coarse selection's edge tests.

tests/test_hip_select_edges.py (GPU) runs `ops.coarse_match` and compares what callers read -- b_ids / i_ids / j_ids / mconf / mkpts*_c
and counts -- with `oracle.loftr_oracle.coarse_match_select` applied to the conf_matrix THE KERNEL ITSELF RETURNED.  Selection
(merge_colmax_kernel, valid_hw_kernel, select_kernel, scan_blocks_kernel, scatter_kernel of csrc/coarse_match.hip) is integer logic on
that matrix, so the comparison is exact: ids in the reference's order (ascending (b, i), not sorted by the test), mconf bitwise
conf[b, i, j], coarse keypoints bitwise the reference's float32 values, counts[0] = M and counts[1:] = bincount(b_ids).  No tolerance,
no flip allowance, no margin condition on the inputs.  tests/test_select_oracle.py (CPU) holds every condition stated here on the
oracle's own float32 confidence and shows, with one modelled mistake per edge, that the comparison can fail.

Paths (who writes the row / column partials the selection reads):
  P1     sweep + conf_matrix, C = 256, no masks (panel arg-max, select_kernel reads the panel back)
  P2     sweep with masks (per-element arg-max)
  P3     sweep, conf_matrix elided (want_conf=False): no tie walk, see expected_elided
  P4     tiled kernels, C = 64 / 128, with and without masks
  P5     Sinkhorn row-streaming (bin_score 1.0, 3 iterations), with / without masks, with / without prefilter
  P6     Sinkhorn separate kernels (S + 1 > 12 288)

Cases (the smallest shapes that reach each edge; descriptors are seeded standard normals with planted correspondences):
  threshold   N 3, 9x11 / 10x9, border 1: thr = 0, thr = the median mconf of that run (strict >: matches AT thr vanish), nextafter(thr, 0)
  borders     7x9 / 9x7 at border 0..3; 5x5 at border 2 (one interior cell); 4x5 at border 2 (no interior row: M = 0)
  padding     N 4, 8x10 / 9x8, border 2: full masks; rectangles (5,6)/(6,5); a valid extent == border (limit 0, nothing survives);
              valid extents BELOW the border on both images (python's negative slice wraps the limit to hc - 1: rows and columns of the
              padding survive the border test and the reference reports tied padding x padding entries)
  ties        N 2, 5x7 / 31x32 (S = 992: sweep chunks of 16 + 15 panels, boundary at column 512), border 1: duplicated columns of
              feat_c1, the first a border cell, the second interior; same panel, two panels of one chunk, two chunks (TIE_PLACEMENTS)
  scan        N 24, 105x105 / 4x4, C 64: 264 600 rows = 1 034 select blocks, the second round of scan_blocks_kernel and its carry
  many_pairs  N 70 at 2x3 / 3x3, N 130 at 1x1 / 3x3 (a wave spans 64 pairs), border 0
  straddle    N 3, 7x13 / 9x11: 273 rows, block 0 holds three pairs, block 1 holds 17 rows; P6 at N 2, 4x5 / 100x123
  scales      the straddle grids with per-pair scale0 / scale1, non-dyadic and different in x and y
  empty       thr = 0.999 on flat inputs, every path.  N = 0: ops.coarse_match hands the library the data pointer of an empty
              tensor, which is null, and the library refuses null descriptors before it looks at N -- the shape is not accepted
              and is left out.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import loftr_oracle as O

TEMPERATURE = 0.1
BIN_SCORE, SKH_ITERS = 1.0, 3
SCALE = 8.0
BACKGROUND = 0.25

Path = namedtuple("Path", "kind C masked want_conf prefilter")
PATHS = {
    "P1": Path("ds", 256, False, True, False),
    "P2": Path("ds", 256, True, True, False),
    "P3": Path("ds", 256, False, False, False),
    "P4_64": Path("ds", 64, False, True, False),
    "P4_128": Path("ds", 128, False, True, False),
    "P4_64m": Path("ds", 64, True, True, False),
    "P4_128m": Path("ds", 128, True, True, False),
    "P5": Path("ot", 256, False, True, False),
    "P5m": Path("ot", 256, True, True, False),
    "P5p": Path("ot", 256, False, True, True),
    "P5mp": Path("ot", 256, True, True, True),
    "P6": Path("ot", 256, False, True, False),
    "P6m": Path("ot", 256, True, True, False),
}

# Duplicated columns of feat_c1 (first occurrence j1: a border cell of the 31 x 32 grid, second occurrence j2: interior), by where the two
# lie in the sweep's work distribution.  A 32-column panel is one row of the 31 x 32 grid.
#   same_panel         both in one panel
#   same_chunk         panel 0 (the top border row) is a copy of panel 10 AS A WHOLE: pass A's shared-reference variant forms a column's
#                      (reference, sum) per 32 x 32 tile relative to the TILE's maximum, so two equal columns get bitwise equal
#                      statistics only if their tiles are equal -- which a whole-panel copy guarantees
#   same_chunk_single  ONE duplicated column in another panel of the same chunk          } exact ties only where the columns' statistics do
#   two_chunks         single duplicated columns on either side of the chunk boundary 512 } not depend on the tile they sit in; elsewhere
#                      the run's report line says so and the placement is not required (TIE_OPTIONAL)
TIE_PLACEMENTS = {"same_panel": ((160, 167), (352, 360)), "same_chunk": tuple((x, 320 + x) for x in range(32)),
                  "same_chunk_single": ((95, 420),), "two_chunks": ((64, 900), (127, 600))}
TIE_OPTIONAL = ("same_chunk_single", "two_chunks")
TIE_BOTH_INTERIOR, TIE_BOTH_ROW = (200, 700), 17   # both occurrences interior: the FIRST one is the match
# (second occurrence, the interior row of the 5 x 7 grid planted on it; x0 in 1 .. 4: interior under the small pad too)
TIE_PLANTS = ((167, 8), (360, 9), (325, 10), (330, 11), (420, 15), (900, 16), (600, 18), (700, TIE_BOTH_ROW))
SCALES0 = np.array([[1.9, 1.37], [0.83, 1.21], [1.13, 0.77]], np.float32)
SCALES1 = np.array([[0.83, 1.21], [1.57, 0.91], [1.9, 1.37]], np.float32)

# masks: None (whatever the path asks for: a small pad if it is a masked path), "padding" (the padding case's rectangles)
Config = namedtuple("Config", "name N hw0 hw1 border plant masks scales thr paths")


def _configs():
    c = []
    c.append(Config("threshold", 3, (9, 11), (10, 9), 1, "perm", None, False, "median", ("P1", "P2", "P4_64", "P4_128m", "P5", "P5m")))
    for b in (0, 1, 2, 3):
        c.append(Config(f"borders_b{b}", 2, (7, 9), (9, 7), b, "interior", None, False, 0.0, ("P1", "P4_64", "P5")))
    c.append(Config("borders_one_cell", 2, (5, 5), (5, 5), 2, "interior", None, False, 0.0, ("P1", "P4_64", "P5")))
    c.append(Config("borders_no_interior", 2, (4, 5), (4, 5), 2, "interior", None, False, 0.0, ("P1", "P4_64", "P5")))
    c.append(Config("padding", 4, (8, 10), (9, 8), 2, "padding", "padding", False, 0.0, ("P2", "P4_64m", "P4_128m", "P5m", "P5mp")))
    c.append(Config("ties", 2, (5, 7), (31, 32), 1, "ties", None, False, 0.0, ("P1", "P2", "P3", "P4_128", "P5")))
    c.append(Config("scan", 24, (105, 105), (4, 4), 0, "scan", None, False, 0.0, ("P4_64",)))
    c.append(Config("many_pairs_70", 70, (2, 3), (3, 3), 0, "perm", None, False, 0.0, ("P1", "P4_64")))
    c.append(Config("many_pairs_130", 130, (1, 1), (3, 3), 0, "perm", None, False, 0.0, ("P1", "P4_64")))
    c.append(Config("straddle", 3, (7, 13), (9, 11), 1, "perm", None, False, 0.0, ("P1", "P4_64", "P4_128", "P5", "P5p")))
    c.append(Config("straddle_wide", 2, (4, 5), (100, 123), 1, "perm", None, False, 0.0, ("P6", "P6m")))
    c.append(Config("scales", 3, (7, 13), (9, 11), 1, "perm", None, True, 0.0, ("P1", "P2")))
    c.append(Config("empty", 3, (7, 13), (9, 11), 1, "flat", None, False, 0.999,
                    ("P1", "P2", "P3", "P4_64", "P4_128m", "P5", "P5m", "P5p", "P5mp")))
    c.append(Config("empty_wide", 2, (4, 5), (100, 123), 1, "flat", None, False, 0.999, ("P6",)))
    return c


CONFIGS = _configs()
CONFIG_BY_NAME = {c.name: c for c in CONFIGS}
assert len(CONFIG_BY_NAME) == len(CONFIGS)
RUNS = [(c.name, p) for c in CONFIGS for p in c.paths]
assert 24 * 105 * 105 == 264600 > 1024 * 256 and -(-264600 // 256) == 1034 and 3 * 7 * 13 == 273
assert all((100 * 123 + 1 > 12288) == p.startswith("P6") for n, p in RUNS for c in [CONFIG_BY_NAME[n]] if c.hw1 == (100, 123))


def _L(c):
    return c.hw0[0] * c.hw0[1]


def _S(c):
    return c.hw1[0] * c.hw1[1]


def _rect(N, hw, valid):
    m = np.zeros((N,) + hw, bool)
    for n, (vh, vw) in enumerate(valid):
        m[n, :vh, :vw] = True
    return m


def masks(c, path):
    """(m0 [N, h0, w0], m1 [N, h1, w1]) bool valid rectangles at the top left, or (None, None)."""
    if not PATHS[path].masked:
        assert c.masks is None
        return None, None
    (h0, w0), (h1, w1) = c.hw0, c.hw1
    if c.masks == "padding":
        assert (c.N, c.hw0, c.hw1, c.border) == (4, (8, 10), (9, 8), 2)
        #           pair 0: full     1: rectangles   2: valid height of image 0 == border   3: both below the border on one axis (wrap)
        return _rect(4, c.hw0, [(8, 10), (5, 6), (2, 10), (1, 7)]), _rect(4, c.hw1, [(9, 8), (6, 5), (9, 8), (6, 1)])
    # the small pad: even pairs lose the last column of image 0, odd pairs the last row of image 1 (1-wide grids stay whole)
    v0 = [(h0, w0 - 1) if n % 2 == 0 and w0 > 1 else (h0, w0) for n in range(c.N)]
    v1 = [(h1 - 1, w1) if n % 2 == 1 and h1 > 1 else (h1, w1) for n in range(c.N)]
    return _rect(c.N, c.hw0, v0), _rect(c.N, c.hw1, v1)


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False


@functools.lru_cache(maxsize=4)
def _inputs(name, kind, C):
    c = CONFIG_BY_NAME[name]
    L, S = _L(c), _S(c)
    rng = np.random.default_rng([c.N, L, S, C, kind == "ot"])
    # Sinkhorn scores carry no temperature: a planted score is weight * amp^2.  2.4: the prefilter removes some rows and keeps others
    amp = np.float32(2.4 if kind == "ot" else 1.0)
    f0 = rng.standard_normal((c.N, L, C)).astype(np.float32) * amp
    f1 = rng.standard_normal((c.N, S, C)).astype(np.float32) * amp
    if c.plant == "flat":
        f0 *= np.float32(0.3); f1 *= np.float32(0.3)
        _freeze(f0, f1)
        return f0, f1
    f1 *= np.float32(BACKGROUND)
    for n in range(c.N):
        if c.plant == "scan":                             # the 16 columns on rows spread over the pair, the last row included
            rows, cols, wt = (np.arange(S) * (L - 1)) // (S - 1), np.arange(S), np.ones(S, np.float32)
        else:
            K = max(L, S)
            rows, cols = rng.permutation(K) % L, np.arange(K) % S
            wt = np.where(np.arange(K) < min(L, S), 1.0, 0.6).astype(np.float32)
        np.add.at(f1[n], cols, wt[:, None] * f0[n, rows])
        if c.plant == "interior" and c.border > 0:        # up to four cells interior to both grids matched to each other, whatever the border
            b, (h0, w0), (h1, w1) = c.border, c.hw0, c.hw1
            ri = [y * w0 + x for y in range(b, h0 - b) for x in range(b, w0 - b)]
            ci = [y * w1 + x for y in range(b, h1 - b) for x in range(b, w1 - b)]
            for i, j in list(zip(ri, ci))[:4]:
                f1[n, j] = np.float32(BACKGROUND) * rng.standard_normal(C).astype(np.float32) * amp + np.float32(1.5) * f0[n, i]
        if c.plant == "padding" and n == 1:               # the 2 x 2 interior of pair 1's valid rectangles: cells (2, 2), (2, 3) <-> (2, 2), (3, 2)
            for i, j in ((22, 18), (23, 26)):
                f1[n, j] = np.float32(BACKGROUND) * rng.standard_normal(C).astype(np.float32) * amp + np.float32(1.5) * f0[n, i]
        if c.plant == "ties":
            for j2, i in TIE_PLANTS:
                f1[n, j2] = np.float32(BACKGROUND) * rng.standard_normal(C).astype(np.float32) * amp + np.float32(1.5) * f0[n, i]
            for j1, j2 in [p for pl in TIE_PLACEMENTS.values() for p in pl] + [TIE_BOTH_INTERIOR]:
                f1[n, j1] = f1[n, j2]
    _freeze(f0, f1)
    return f0, f1


def inputs(name, path):
    """Seeded float32 descriptors, masks, scales of one run.  Shared between tests: read-only."""
    c, p = CONFIG_BY_NAME[name], PATHS[path]
    f0, f1 = _inputs(name, p.kind, p.C)
    m0, m1 = masks(c, path)
    _freeze(m0, m1)
    s0, s1 = (SCALES0[:c.N], SCALES1[:c.N]) if c.scales else (None, None)
    return dict(config=c, path=p, f0=f0, f1=f1, m0=m0, m1=m1, scale0=s0, scale1=s1)


def oracle_conf(i):
    """The oracle's own float32 confidence of a run (the CPU test's stand-in for the kernel's matrix)."""
    c, p = i["config"], i["path"]
    m0 = None if i["m0"] is None else i["m0"].reshape(c.N, -1)
    m1 = None if i["m1"] is None else i["m1"].reshape(c.N, -1)
    if p.kind == "ds":
        return O.dual_softmax_conf(i["f0"], i["f1"], TEMPERATURE, m0, m1)
    return O.sinkhorn_conf(i["f0"], i["f1"], np.float32(BIN_SCORE), SKH_ITERS, m0, m1, prefilter=p.prefilter)[0]


def expected(conf, i, thr):
    """The reference selection on `conf` (float32) plus the counts the kernels report beside it."""
    c = i["config"]
    assert conf.dtype == np.float32
    sel = O.coarse_match_select(conf, thr, c.border, c.hw0, c.hw1, (c.hw0[0] * 8, c.hw0[1] * 8), i["m0"], i["m1"], i["scale0"], i["scale1"])
    assert len(sel["mconf"]) == len(sel["b_ids"])         # thr >= 0: the reference's `mconf != 0` filter keeps every match
    out = {k: sel[k] for k in ("b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c")}
    out["counts"] = np.concatenate([[len(sel["b_ids"])], np.bincount(sel["b_ids"], minlength=c.N)]).astype(np.int32)
    return out


DTYPES = dict(b_ids=np.int64, i_ids=np.int64, j_ids=np.int64, mconf=np.float32, mkpts0_c=np.float32, mkpts1_c=np.float32, counts=np.int32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(out, want, conf, N):
    """Every assertion of the issue on one run, as a list of failures (empty: the run agrees exactly)."""
    bad = []
    for k, dt in DTYPES.items():
        if np.asarray(out[k]).dtype != dt:
            bad.append((k, "dtype", str(np.asarray(out[k]).dtype)))
    b, ii, jj = (np.asarray(out[k]) for k in ("b_ids", "i_ids", "j_ids"))
    counts = np.asarray(out["counts"])
    if counts.shape != (1 + N,) or counts[0] != len(b) or counts[0] != len(want["b_ids"]):
        bad.append(("counts[0]", int(counts[0]) if counts.size else None, len(b), len(want["b_ids"])))
    got_ids, want_ids = np.stack([b, ii, jj], 1), np.stack([want["b_ids"], want["i_ids"], want["j_ids"]], 1)
    if got_ids.shape != want_ids.shape or not np.array_equal(got_ids, want_ids):
        diff = sorted(set(map(tuple, got_ids.tolist())) ^ set(map(tuple, want_ids.tolist())))
        bad.append(("ids", len(got_ids), len(want_ids), diff[:8] if diff else "same set, another order"))
        return bad
    if not np.array_equal(counts[1:], np.bincount(b, minlength=N)):
        bad.append(("counts[1:]", counts[1:].tolist()[:16]))
    if not np.array_equal(_bits(out["mconf"]), _bits(conf[b, ii, jj])):
        bad.append(("mconf", "not bitwise conf[b, i, j]"))
    for k in ("mkpts0_c", "mkpts1_c"):
        if np.asarray(out[k]).shape != want[k].shape or not np.array_equal(_bits(out[k]), _bits(want[k])):
            bad.append((k, "not bitwise the reference's"))
    return bad


# ---- the selection once more, the way the kernels do it, with one mistake built in -------------------------------------------------------
MISTAKES = ("ge_threshold", "limit_off_by_one", "limit_clamped", "last_tied_column", "no_tie_walk", "scan_carry_dropped",
            "wave_counts_to_first_pair", "xy_scale_swapped", "bj_order")
# the case each mistake has to change (tests/test_select_oracle.py asserts it)
MISTAKE_CASE = {"ge_threshold": ("threshold", "P1"), "limit_off_by_one": ("borders_b2", "P1"), "limit_clamped": ("padding", "P2"),
                "last_tied_column": ("ties", "P1"), "no_tie_walk": ("ties", "P1"), "scan_carry_dropped": ("scan", "P4_64"),
                "wave_counts_to_first_pair": ("many_pairs_130", "P1"), "xy_scale_swapped": ("scales", "P1"), "bj_order": ("straddle", "P1")}


def _limits(i, mistake):
    """[N, 4] upper limits (h0, w0, h1, w1) of the border test: upper_limit of csrc/coarse_match.hip."""
    c = i["config"]
    hc = np.array([c.hw0[0], c.hw0[1], c.hw1[0], c.hw1[1]])
    if i["m0"] is None:
        lim = np.tile(hc - c.border, (c.N, 1))
    else:
        hv = np.stack([i["m0"].sum(1).max(-1), i["m0"].sum(2).max(-1), i["m1"].sum(1).max(-1), i["m1"].sum(2).max(-1)], 1).astype(int)
        lim = hv - c.border
        lim = np.maximum(lim, 0) if mistake == "limit_clamped" else np.where(lim < 0, np.maximum(lim + hc, 0), lim)
    return lim + 1 if mistake == "limit_off_by_one" else lim


def model_select(conf, i, thr, mistake=None):
    """select_kernel / scan_blocks_kernel / scatter_kernel restated in numpy.  mistake None: equals `expected` (tested on every run);
    "no_tie_walk" is ALSO what the kernels document for an elided conf_matrix (expected_elided)."""
    c = i["config"]
    N, L, S = conf.shape
    (h0, w0), (h1, w1), b = c.hw0, c.hw1, c.border
    thr = np.float32(thr)
    rowmax, colmax = conf.max(2, keepdims=True), conf.max(1, keepdims=True)
    ok = (conf >= thr) if mistake == "ge_threshold" else (conf > thr)
    if b > 0:
        lim = _limits(i, mistake)
        y0, x0, y1, x1 = np.arange(L) // w0, np.arange(L) % w0, np.arange(S) // w1, np.arange(S) % w1
        r_ok = (y0 >= b) & (x0 >= b) & (y0[None] < lim[:, 0:1]) & (x0[None] < lim[:, 1:2])
        c_ok = (y1 >= b) & (x1 >= b) & (y1[None] < lim[:, 2:3]) & (x1[None] < lim[:, 3:4])
        ok = ok & r_ok[:, :, None] & c_ok[:, None, :]
    ok = ok & (conf == rowmax) & (conf == colmax)
    if mistake == "no_tie_walk":
        j = (conf == rowmax).argmax(2)
        flag = np.take_along_axis(ok, j[:, :, None], 2)[:, :, 0]
    elif mistake == "last_tied_column":
        j, flag = S - 1 - ok[:, :, ::-1].argmax(2), ok.any(2)
    else:
        j, flag = ok.argmax(2), ok.any(2)
    flag, j = flag.reshape(-1), j.reshape(-1)
    rows = np.flatnonzero(flag)                            # flat rows n * L + i, ascending
    blk = rows // 256
    nblk = -(-N * L // 256)
    block_count = np.bincount(blk, minlength=nblk)
    off = np.cumsum(block_count) - block_count
    total = int(block_count.sum())
    if mistake == "scan_carry_dropped":                    # each round of 1024 blocks starts at 0 again
        for base in range(0, nblk, 1024):
            seg = block_count[base:base + 1024]
            off[base:base + 1024] = np.cumsum(seg) - seg
            total = int(seg.sum())
    rank = np.arange(len(rows)) - (np.cumsum(block_count) - block_count)[blk]
    dst = off[blk] + rank
    n, ii, jj = rows // L, rows % L, j[rows]
    if mistake == "bj_order":
        o = np.lexsort((jj, n))
        n, ii, jj = n[o], ii[o], jj[o]
    cap = max(N * L, 1)
    out = dict(b_ids=np.zeros(cap, np.int64), i_ids=np.zeros(cap, np.int64), j_ids=np.zeros(cap, np.int64), mconf=np.zeros(cap, np.float32),
               mkpts0_c=np.zeros((cap, 2), np.float32), mkpts1_c=np.zeros((cap, 2), np.float32))
    s0 = np.full((N, 2), SCALE, np.float32) if i["scale0"] is None else np.float32(SCALE) * i["scale0"]
    s1 = np.full((N, 2), SCALE, np.float32) if i["scale1"] is None else np.float32(SCALE) * i["scale1"]
    if mistake == "xy_scale_swapped":
        s0, s1 = s0[:, ::-1], s1[:, ::-1]
    out["b_ids"][dst], out["i_ids"][dst], out["j_ids"][dst] = n, ii, jj
    out["mconf"][dst] = conf[n, ii, jj]
    out["mkpts0_c"][dst] = np.stack([ii % w0, ii // w0], 1).astype(np.float32) * s0[n]
    out["mkpts1_c"][dst] = np.stack([jj % w1, jj // w1], 1).astype(np.float32) * s1[n]
    out = {k: v[:total] for k, v in out.items()}
    if mistake == "wave_counts_to_first_pair":             # a wave's 64 consecutive rows all counted to the pair of its first match
        first = {}
        for r in rows:
            first.setdefault(r // 64, r // L)
        per = np.bincount([first[r // 64] for r in rows], minlength=N)
    else:
        per = np.bincount(rows // L, minlength=N)
    out["counts"] = np.concatenate([[total], per]).astype(np.int32)
    return out


def expected_elided(conf_materialised, i, thr):
    """want_conf=False: the reference selection on the materialised run's conf_matrix without the rows whose FIRST column attaining
    the row maximum fails a test (the documented deviation in select_kernel's comment: no matrix, no tie walk)."""
    return model_select(conf_materialised, i, thr, "no_tie_walk")


def later_tie_rows(want, conf, j1, j2):
    """Matches of `want` at column j2 whose row attains the same confidence at the earlier column j1."""
    b, ii, jj = want["b_ids"], want["i_ids"], want["j_ids"]
    k = jj == j2
    return int((_bits(conf[b[k], ii[k], j1]) == _bits(conf[b[k], ii[k], j2])).sum())


def tie_report(conf, want):
    """{placement: (columns bitwise equal in conf, later-tie rows)}."""
    out = {}
    for name, pairs in TIE_PLACEMENTS.items():
        exact = all(np.array_equal(_bits(conf[:, :, j1]), _bits(conf[:, :, j2])) for j1, j2 in pairs)
        out[name] = (exact, sum(later_tie_rows(want, conf, j1, j2) for j1, j2 in pairs))
    return out


def median_threshold(mconf):
    """The exact float32 value of the median match confidence (an element of mconf)."""
    return np.sort(np.asarray(mconf, np.float32))[len(mconf) // 2]


def border_sides_hit(conf, i):
    """For each of the eight border sides: the number of matches of the border-free selection that lie in its strip."""
    c = i["config"]
    free = O.coarse_match_select(conf, 0.0, 0, c.hw0, c.hw1, (c.hw0[0] * 8, c.hw0[1] * 8))
    (h0, w0), (h1, w1), b = c.hw0, c.hw1, c.border
    y0, x0, y1, x1 = free["i_ids"] // w0, free["i_ids"] % w0, free["j_ids"] // w1, free["j_ids"] % w1
    return [int(s.sum()) for s in (y0 < b, x0 < b, y1 < b, x1 < b, y0 >= h0 - b, x0 >= w0 - b, y1 >= h1 - b, x1 >= w1 - b)]
