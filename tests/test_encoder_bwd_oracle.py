"""CPU: the conditions tests/_encoder_bwd_cases.py states about its cases hold, and the float64 comparison of
tests/test_hip_encoder_bwd_edges.py can fail.  The restated layer reproduces the committed glayer_* fixtures (gradients of the reference's
own LoFTREncoderLayer); the restated dispatch arithmetic gives the constants the kernels' comments quote and puts every case at the edge
it is in the table for; the ReLU condition holds on every case and its redraw loop ended before its cap; no pair is without a valid
source token; ref32 stays inside half of every tolerance; and each modelled kernel mistake sits at least DETECTION_FACTOR tolerances from
ref64 in at least one output tensor on every case it applies to.  These are conditions on the choice of the inputs: a case that misses
one gets another seed (SEEDS), never another factor."""
import json
import os

import numpy as np
import pytest
import torch

import _encoder_bwd_cases as E

ALL = [c.name for c in E.CASES]


@pytest.mark.parametrize("name", ["glayer_self", "glayer_cross_mask", "glayer_fine"])
def test_restated_layer_reproduces_the_reference_goldens(name):
    """float32, as the fixtures were written: out, grad_x, grad_source and every weight-gradient digest within 1e-6 of the maximum.

    The bound is at float32's own noise (ref32 is up to 9e-7 of the maximum from ref64 in grad_source), so it holds only where torch's
    float32 matrix products sum in the order the fixtures were written with.  On an Intel host (AVX-512, MKL) every tensor and digest is
    reproduced with difference 0.0, at 1, 2, 4, 8 and 16 threads.  On an AMD EPYC 9575F host (AVX-512, 16 threads) the same code MISSES
    the bound: glayer_self grad_source 3.34e-6 of a maximum of 3.19 (1.05e-6), glayer_cross_mask grad_source 2.86e-6, glayer_fine
    grad_q_proj/colsum 2.68e-5 of a scale of 8.67 (3.1e-6).  The float64 run of the restatement is 7.1e-7 / 9.2e-7 / 5.6e-7 of the
    maximum from the three fixtures in grad_source and up to 3.7e-6 in the column-sum digests: the fixtures' own float32 noise, which no
    evaluation other than a bitwise repetition gets below.  The bound is the one the issue set and is left as it is."""
    g = np.load(os.path.join(E.HERE, "golden", f"{name}.npz"))
    rc = json.loads(str(g["recipe"]))
    got = E.run_layer(dict(E.MG.build(rc), H=rc["H"]), torch.float32)
    for k in E.DATA:
        assert np.abs(got[k] - g[k]).max() <= 1e-6 * np.abs(g[k]).max(), (name, k, float(np.abs(got[k] - g[k]).max()))
    for f in E.FIELDS:
        key = "grad_" + f
        for part, v in E.MG.digest(key, got[key]).items():
            ref = g[part]
            scale = max(float(np.abs(ref).max()), float(g[f"{key}/absmax"]) if f in E.MATRICES else 0.0)
            assert np.abs(v - ref).max() <= 1e-6 * scale, (name, part, float(np.abs(v - ref).max()), scale)


def test_dispatch_arithmetic():
    assert (E.LN_ROWS_PB, E.ATTN_TOKENS, E.TALL_FROM, E.OUTER_ONE_BLOCK, E.OUTER_MAX_SPLITS) == (64, 256, 16, 1024, 16)
    assert E.outer_splits(1024) == (1, 1024) and E.outer_splits(1025) == (3, 384) and E.outer_chunks(1025) == [(0, 384), (384, 768), (768, 1025)]
    assert E.outer_chunks(1089) == [(0, 384), (384, 768), (768, 1089)] and E.outer_splits(1300) == (3, 448)
    assert E.outer_splits(8257) == (15, 576) and E.outer_chunks(8257)[-1] == (8064, 8257) and E.outer_splits(4800) == (10, 512)
    assert E.outer_splits(8257, scratch_floats=10, per_split=1) == (1, 8257)
    assert E.wgrad_chunk(8257, 512) == 160 and E.wgrad_partials(8257, 512) == (52, 97) and E.wgrad_chunk(8192, 512) == 128
    assert E.wgrad_chunk(8257, 256) == 128 and E.wgrad_chunk(9600, 256) == 128 and E.wgrad_chunk(10 ** 6, 256) == 512
    assert E.wgrad_partials(127, 256) == (1, 127) and E.wgrad_partials(128, 256) == (1, 128) and E.wgrad_partials(129, 256) == (2, 1)
    assert [E.wgrad_partials(T, 256)[0] for T in (1920, 1921)] == [15, 16] and [E.wgrad_partials(T, 512)[0] for T in (1920, 1921)] == [15, 16]
    assert E.wgrad_partials(1025, 256, 512) == (3, 1) and E.wgrad_chunk(5, 256, forced=512) == 512
    assert [E.plan(1, T, 64, 256, 8).nlb for T in (960, 961)] == [15, 16] and [E.plan(1, T, 64, 256, 8).ln_tall for T in (960, 961)] == [False, True]
    # the scratch holds the outer_accum partials of every case: no case falls back to one block for want of room
    for c in E.CASES:
        p = E.plan(c.nb, c.L, c.S, c.C, c.H)
        assert p.outer_x == E.outer_splits(c.L) and p.outer_src == E.outer_splits(c.S), c.name
        for Tn in (c.L, c.S):
            ch = E.outer_chunks(Tn)
            assert ch[0][0] == 0 and ch[-1][1] == Tn and all(a < b for a, b in ch) and all(ch[k][1] == ch[k + 1][0] for k in range(len(ch) - 1))


def test_every_case_is_at_the_edge_it_is_listed_for():
    assert not E.edge_failures()
    assert {e for c in E.CASES for e in c.edges} == set(E.EDGES)
    shapes = {(c.nb, c.L, c.S, c.C, c.H) for c in E.CASES if c.masks is None and c.gmode == "normal"}
    assert shapes >= {(2, 48, 35, 256, 8), (5, 25, 25, 128, 8), (1, 128, 129, 256, 8), (1, 129, 128, 256, 8), (1, 257, 255, 256, 8), (3, 256, 40, 256, 8),
                      (1, 1024, 1025, 256, 8), (1, 1025, 1024, 256, 8), (1, 960, 64, 256, 8), (1, 961, 64, 256, 8), (1, 1920, 48, 256, 8),
                      (1, 1921, 48, 256, 8), (1, 8257, 257, 256, 8), (2, 40, 1300, 256, 8), (2, 1300, 40, 256, 8), (11, 25, 25, 128, 8),
                      (41, 25, 25, 128, 8), (77, 25, 25, 128, 8)}
    assert {(c.nb, c.L, c.S, c.C, c.H, c.masks) for c in E.CASES if c.masks} == {(3, 1025, 1089, 256, 8, "split"), (3, 1089, 1025, 256, 8, "split_t"),
                                                                                 (2, 40, 56, 256, 8, "golden")}
    assert sorted(c.gmode for c in E.CASES if c.gmode != "normal") == ["rows", "tiny"]
    assert all(n in E.CASE_BY_NAME for n, _ in E.FORCED)
    assert [(n, sw) for n, sw in E.FORCED] == [("1x1025x1024x256", {"wgrad_chunk": 512}), ("1x1025x1024x256", {"wgrad_chunk": 128, "reduce_tall": 0}),
                                               ("41x25x25x128", {"wgrad_chunk": 512}), ("41x25x25x128", {"wgrad_chunk": 128, "reduce_tall": 0}),
                                               ("1x1921x48x256", {"reduce_tall": 0})]
    # what the forced switches change on their cases: another partial count, or the generic reduction where the tall one would run
    assert E.plan(1, 1025, 1024, 256, 8, 512).wg == (3, 1) != E.plan(1, 1025, 1024, 256, 8).wg == (9, 1)
    assert E.plan(41, 25, 25, 128, 8, 512).wg == (3, 1) and E.plan(41, 25, 25, 128, 8).ln_tall and E.plan(1, 1921, 48, 256, 8).wg[0] >= E.TALL_FROM


def test_mask_patterns():
    i = E.inputs("mask_3x1025x1089x256")
    xm, sm = i["x_mask"], i["source_mask"]
    assert sm[0].sum() == 700 and sm[0, :700].all() and xm[0].sum() == 725 and sm[1].sum() == 1 and sm[1, 0] and xm[1].all() and xm[2].all() and sm[2].all()
    assert E._mask_chunks(i["case"], 1) == [[384, 316, 0], [1, 0, 0], [384, 384, 321]] and E._mask_chunks(i["case"], 0)[0] == [384, 341, 0]
    t = E.inputs("mask_3x1089x1025x256")
    assert np.array_equal(t["x_mask"], sm) and np.array_equal(t["source_mask"], xm)
    g = E.inputs("mask_2x40x56x256")
    ref = E.MG.build(E.MG.CASES["glayer_cross_mask"])
    assert np.array_equal(g["x_mask"], ref["x_mask"]) and np.array_equal(g["source_mask"], ref["source_mask"])


@pytest.mark.parametrize("name", ALL)
def test_relu_condition_and_reference_noise(name):
    """The ReLU condition holds and its redraw loop ended; no pair without a valid source token; the case is small; ref32 is inside half
    of every tolerance and within 1e-5 of the tensor's scale (one pre-activation changing sign between float32 and float64 moves
    grad_x by 1e-2 of its scale; float32 rounding in sums of up to 8257 terms is of the order 1e-6)."""
    c, f = E.CASE_BY_NAME[name], E.facts(name)
    assert f["finite"]
    assert f["relu_margin"] >= E.RELU_MARGIN and f["relu_rounds"] < E.RELU_ROUNDS, (name, f["relu_margin"], f["relu_rounds"])
    assert f["min_valid_source"] >= 1 and f["elements"] <= E.MAX_ELEMENTS
    for k in E.OUTPUTS:
        noise, scale = f["noise"][k], f["scale"][k]
        assert scale > 0 and noise <= E.tolerance(k, noise, scale) / 2 and noise <= 1e-5 * scale, (name, k, noise, scale)
    inp = E.inputs(name)
    if c.gmode == "tiny":
        assert np.abs(inp["G"]).max() < 1e-5
    if c.gmode == "rows":
        rows_g, rows_x = np.abs(inp["G"]).max(-1).ravel(), np.abs(inp["x"]).max(-1).ravel()
        assert rows_g.max() / rows_g.min() > 1e4 and 0.05 < (rows_x > 30).mean() < 0.2


@pytest.mark.parametrize("name,mutation", [(c.name, m) for c in E.CASES for m in E.MUTATIONS if E.mutation_applies(c, m)])
def test_mutation_is_far_outside_the_tolerance(name, mutation):
    d = E.facts(name)["mutation_distance"][mutation]
    assert d >= E.DETECTION_FACTOR, (name, mutation, d)


def test_every_mutation_meets_its_edge():
    applies = {m: {c.name for c in E.CASES if E.mutation_applies(c, m)} for m in E.MUTATIONS}
    assert len(E.MUTATIONS) == 5 and all(applies.values())
    assert applies["lost_token"] == applies["layernorm_partial"] == applies["residual_dropped"] == set(ALL)
    assert applies["lost_chunk"] == {c.name for c in E.CASES if c.S > 1024} and len(applies["lost_chunk"]) >= 4
    assert applies["mask_ignored"] == {c.name for c in E.CASES if c.masks}
