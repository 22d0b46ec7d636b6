"""Case table, float64 reference and tolerances of the fine matching's edge tests.

tests/test_hip_fine_match_edges.py (GPU) compares `ops.fine_match` (fine_match_kernel of csrc/fine.hip: one wave per match, lane r owns
window position r, channels in strides of 64 lanes, four matches per workgroup) with `oracle.loftr_oracle.fine_matching` in FLOAT64 at
every window size the operator accepts (W = 2 .. 8: WW = 4 .. 64, the last with no inactive lane), at channel counts that are and are
not multiples of 64, at match counts that leave 1 .. 3 matches in the last workgroup, in every regime of its softmax and with
per-pair scales gathered through unsorted b_ids.  tests/test_fine_match_oracle.py (CPU) holds the conditions stated here and shows
that the comparison can fail.

Reference: ref64 = the oracle on the float64 casts of the float32 inputs, ref32 = the oracle on the float32 inputs; noise =
max|ref32 - ref64| per output group over the case.  Groups and bounds (every output must be finite):
  xy   expec_f[:, :2]    err <= K_XY * noise + 1e-6
  px   mkpts1_f          err <= min(K_PX * noise + one float32 ulp of the largest coordinate, TOL_PX)
  std  expec_f[:, 2]     conditioned cases (both variances >= 1e-4 in float64 on every match): err <= K_STD * noise + 1e-6;
                         elsewhere std is a square root of a cancelled difference clamped at 1e-10: err <= 5e-3 (the bound the
                         goldens use) and std >= 2e-5 (1 - 1e-6), twice the square root of the clamp
No case's own px noise exceeds a quarter of TOL_PX (tested), so the cap does not hide a failure.

Regimes, by the amplitude a of the standard-normal windows (scores are about a^2 N(0, 1)):
  flat a = 0.7, moderate a = 1, peaked a = 3, onehot a = 12 (all but one exponential underflow, the variance clamps),
  corner   a = 3 with feat_f0's centre feature planted on a CORNER of window 1: the expectation is +-1, the offset the full W // 2
  shifted  moderate plus 50 in every channel: scores of about 2500 sqrt(C), whose float32 spacing is the softmax's input noise
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import loftr_oracle as O
from _cases import TOL_PX

SCALE = 2.0                                    # hw0_i / hw0_f; RESCALED names the cases that use a smaller one
STD_LOOSE, STD_FLOOR = 5e-3, 2e-5 * (1 - 1e-6)
VAR_CONDITIONED = 1e-4
N_PAIRS = 3
SCALE1 = np.array([[1.9, 1.37], [0.83, 1.21], [1.13, 0.77]], np.float32)       # per pair, x != y, non-dyadic

# ---- tolerance ------------------------------------------------------------------------------------------------------------------------
# K = twice the largest err / noise of its group measured on an MI355X over all cases, rounded up to an integer (the rule of
# tests/_encoder_edge_cases.py).  The lines of profiles/select_fine_match_accuracy.txt the constants were taken from:
#   K_XY  = 3 <- 1.49   fine   w3_c64_m257_shifted            xy  err 1.237e-03 noise 8.283e-04
#   K_PX  = 4 <- 2.00   fine   w5_c128_m257_moderate_scaled   px  err 3.052e-05 noise 1.526e-05
#   K_STD = 2 <- 1.00   fine   w3_c96_m3_flat_scaled          std err 1.192e-07 noise 1.192e-07   (conditioned cases: where K_STD applies)
# Where a group's noise is 0 (both oracle runs round to the same float32, e.g. coordinates of 2 000 px with a spacing of 1.2e-4) there
# is no ratio to take; such a case is held by the additive term alone: 1e-6, or one ulp of its largest coordinate.
K_XY = 3
K_PX = 4
K_STD = 2

Case = namedtuple("Case", "name W C M regime scaled coords scale")
# A case whose own px noise exceeds TOL_PX / 4 at SCALE gets a smaller image-to-fine-map scale, so that TOL_PX's cap does not hide a
# failure: 257 shifted matches at C = 64 include near-tied scores of about 20 000, where float32's spacing of 0.002 moves xy by 8e-4.
RESCALED = {"w3_c64_m257_shifted": 0.125}
REGIMES = {"flat": 0.7, "moderate": 1.0, "peaked": 3.0, "onehot": 12.0, "corner": 3.0, "shifted": 1.0}


def _cases():
    rows = [(5, 128, 257, "flat", False, 2000), (5, 128, 257, "moderate", True, 500), (5, 128, 5, "peaked", False, 2000),
            (5, 128, 5, "onehot", False, 2000), (5, 128, 4, "corner", True, 500), (5, 128, 5, "shifted", False, 2000),
            (2, 32, 1, "moderate", False, 2000), (2, 64, 3, "peaked", False, 500), (2, 128, 3, "corner", False, 2000),
            (3, 96, 3, "flat", True, 500), (3, 256, 4, "onehot", False, 2000), (3, 64, 257, "shifted", False, 500),
            (7, 32, 5, "moderate", False, 2000), (7, 96, 3, "corner", False, 500), (7, 256, 3, "peaked", True, 500),
            (8, 64, 257, "flat", True, 500), (8, 256, 5, "moderate", False, 2000), (8, 128, 1, "peaked", False, 2000),
            (8, 96, 4, "corner", True, 500), (8, 32, 3, "onehot", False, 500), (5, 32, 1, "flat", True, 500)]
    names = [f"w{W}_c{C}_m{M}_{reg}{'_scaled' if sc else ''}" for W, C, M, reg, sc, co in rows]
    return [Case(n, *row, RESCALED.get(n, SCALE)) for n, row in zip(names, rows)]


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
assert {c.W for c in CASES} == {2, 3, 5, 7, 8} and {c.C for c in CASES} == {32, 64, 96, 128, 256} and {c.M for c in CASES} == {1, 3, 4, 5, 257}
assert {c.regime for c in CASES} == set(REGIMES) and {c.M % 4 for c in CASES} == {0, 1, 3}


def corner_of(m, W):
    """Window position (row-major) of the corner match m's peak sits on: the four corners in turn."""
    return ((0, 0), (0, W - 1), (W - 1, 0), (W - 1, W - 1))[m % 4]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Seeded float32 windows, coarse key points, unsorted b_ids, per-pair scales.  Shared between tests: read-only."""
    c = CASE_BY_NAME[name]
    WW = c.W * c.W
    rng = np.random.default_rng([c.W, c.C, c.M, sorted(REGIMES).index(c.regime)])
    a = np.float32(REGIMES[c.regime])
    f0 = rng.standard_normal((c.M, WW, c.C)).astype(np.float32) * a
    f1 = rng.standard_normal((c.M, WW, c.C)).astype(np.float32) * a
    if c.regime == "corner":
        for m in range(c.M):
            y, x = corner_of(m, c.W)
            f1[m, y * c.W + x] = f0[m, WW // 2]
    if c.regime == "shifted":
        f0 += np.float32(50); f1 += np.float32(50)
    mk1c = rng.uniform(0, c.coords, (c.M, 2)).astype(np.float32)
    mk1c[0] = c.coords                                                   # the largest coordinate is in the case
    b_ids = rng.integers(0, N_PAIRS, c.M).astype(np.int64)
    b_ids[0] = N_PAIRS - 1                                               # not sorted, and not pair 0 first
    if c.M > 1:
        b_ids[-1] = 0
    scale1 = SCALE1.copy() if c.scaled else None
    for arr in (f0, f1, mk1c, b_ids, scale1):
        if arr is not None:
            arr.flags.writeable = False
    return dict(case=c, f0=f0, f1=f1, mkpts1_c=mk1c, b_ids=b_ids, scale1=scale1)


def _oracle(i, dt):
    c = i["case"]
    s1 = None if i["scale1"] is None else i["scale1"].astype(dt)
    expec, _, mk1 = O.fine_matching(i["f0"].astype(dt), i["f1"].astype(dt), None, i["mkpts1_c"].astype(dt), i["b_ids"], (c.scale, c.scale), (1, 1),
                                    scale1=s1, has_scale0=s1 is not None)
    return np.asarray(expec, np.float64), np.asarray(mk1, np.float64)


MISTAKES = ("centre_index_minus_one", "grid_step_2_over_W", "xy_swapped", "half_window_as_float", "scale1_of_pair_0", "no_variance_clamp",
            "temperature_1_over_C")


def fine_match_float64(name, mistake=None):
    """fine_matching.py:43-69 in float64 from its pieces -> (expec [M, 3], mkpts1_f [M, 2], var [M, 2]).  mistake None reproduces
    oracle.fine_matching (tested); the others are the modelled mistakes of tests/test_fine_match_oracle.py."""
    i = inputs(name)
    c = i["case"]
    W, WW = c.W, c.W * c.W
    f0, f1 = i["f0"].astype(np.float64), i["f1"].astype(np.float64)
    picked = f0[:, WW // 2 - (1 if mistake == "centre_index_minus_one" else 0)]
    sim = np.einsum("mc,mrc->mr", picked, f1) * ((1.0 / c.C) if mistake == "temperature_1_over_C" else (1.0 / c.C ** .5))
    e = np.exp(sim - sim.max(1, keepdims=True))
    heat = e / e.sum(1, keepdims=True)
    lin = np.arange(W) * (2.0 / (W if mistake == "grid_step_2_over_W" else W - 1)) - 1.0
    gx, gy = np.tile(lin, W), np.repeat(lin, W)
    if mistake == "xy_swapped":
        gx, gy = gy, gx
    grid = np.stack([gx, gy], -1)
    coords = heat @ grid
    var = (heat[:, :, None] * grid[None] ** 2).sum(1) - coords ** 2
    with np.errstate(invalid="ignore"):
        std = np.sqrt(var if mistake == "no_variance_clamp" else np.maximum(var, 1e-10)).sum(-1)
    s1 = c.scale if i["scale1"] is None else c.scale * i["scale1"].astype(np.float64)[0 if mistake == "scale1_of_pair_0" else i["b_ids"]]
    half = W / 2 if mistake == "half_window_as_float" else W // 2
    mk1 = i["mkpts1_c"].astype(np.float64) + coords * half * s1
    return np.concatenate([coords, std[:, None]], -1), mk1, var


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref64 / ref32 of the oracle, the noise of each group, whether the case is conditioned, one ulp of the largest coordinate."""
    i = inputs(name)
    e64, p64 = _oracle(i, np.float64)
    e32, p32 = _oracle(i, np.float32)
    var = fine_match_float64(name)[2]
    return dict(expec=e64, px=p64, expec32=e32, px32=p32, noise_xy=float(np.abs(e32[:, :2] - e64[:, :2]).max()),
                noise_std=float(np.abs(e32[:, 2] - e64[:, 2]).max()), noise_px=float(np.abs(p32 - p64).max()),
                conditioned=bool((var >= VAR_CONDITIONED).all()), min_var=float(var.min()),
                ulp_px=float(np.spacing(np.float32(np.abs(p64).max()))))


def bounds(name):
    r = reference(name)
    return dict(xy=K_XY * r["noise_xy"] + 1e-6, px=min(K_PX * r["noise_px"] + r["ulp_px"], TOL_PX),
                std=(K_STD * r["noise_std"] + 1e-6) if r["conditioned"] else STD_LOOSE)


def check(name, expec, mk1):
    """(figures {group: (err, noise, bound)}, failures) of one result against ref64."""
    r, b = reference(name), bounds(name)
    expec, mk1 = np.asarray(expec, np.float64), np.asarray(mk1, np.float64)
    bad = []
    if expec.shape != r["expec"].shape or mk1.shape != r["px"].shape:
        return {}, [("shape", expec.shape, mk1.shape)]
    if not (np.isfinite(expec).all() and np.isfinite(mk1).all()):
        bad.append(("not finite", int((~np.isfinite(expec)).sum()), int((~np.isfinite(mk1)).sum())))
    with np.errstate(invalid="ignore"):
        fig = dict(xy=(float(np.nanmax(np.abs(expec[:, :2] - r["expec"][:, :2]))), r["noise_xy"], b["xy"]),
                   px=(float(np.nanmax(np.abs(mk1 - r["px"]))), r["noise_px"], b["px"]),
                   std=(float(np.nanmax(np.abs(expec[:, 2] - r["expec"][:, 2]))), r["noise_std"], b["std"]))
    for g, (err, _, bound) in fig.items():
        if not err <= bound:
            bad.append((g, err, bound))
    if not r["conditioned"] and not (expec[:, 2] >= STD_FLOOR).all():
        bad.append(("std below twice the square root of the clamp", float(np.nanmin(expec[:, 2]))))
    return fig, bad
