"""CPU: the conditions tests/_head_bwd_cases.py states about its cases hold, and the float64 comparison of
tests/test_hip_head_bwd_edges.py can fail.  The two heads restated in torch reproduce the committed grad_* fixtures (gradients of the
reference's own modules) in float32 and oracle.grad_oracle's hand-derived backward in float64; the restated dispatch arithmetic puts every
case at the edge it is in the table for; ref32 stays inside half of every tolerance and within 1e-5 of the scale on every compared tensor
(d bin_score is not compared with ref64 on the six DBIN_UNCLAIMED cases; its self check is, on every case); the row-wise check leaves out no row with a gradient; and each modelled kernel mistake sits at least
DETECTION_FACTOR tolerances from ref64 in at least one compared tensor on every case it applies to."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _head_bwd_cases as E

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_grad", os.path.join(HERE, "golden", "make_golden_grad.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

HEADS = [c.name for c in E.CASES]


@pytest.mark.parametrize("name", ["grad_ds", "grad_ds_mask", "grad_dense_mask", "grad_ce", "grad_ot", "grad_ot_mask"])
def test_restated_heads_reproduce_the_reference_goldens(name):
    """float32, as the fixtures were written: the confidences at the ground truth and, from the fixture's own d loss / d conf, both
    descriptor gradients (and d bin_score) within 1e-5 of the tensor's maximum."""
    g = np.load(os.path.join(HERE, "golden", f"{name}.npz"))
    rc = json.loads(str(g["recipe"]))
    inp = MG.build_inputs(rc)
    head = "ot" if rc.get("match_type") == "sinkhorn" else "ds"
    v0 = v1 = None
    if rc["masks"]:
        v0, v1 = inp["mask0"].reshape(rc["N"], -1), inp["mask1"].reshape(rc["N"], -1)
    got = E.run_head(head, inp["feat_c0"], inp["feat_c1"], g["grad_conf"], torch.float32, MG.TEMPERATURE, MG.BIN_SCORE, MG.SKH_ITERS, v0, v1)
    b, i, j = np.nonzero(inp["conf_gt"])
    assert np.abs(got["conf"][b, i, j] - g["conf_at_gt"]).max() <= 1e-5 * np.abs(g["conf_at_gt"]).max()
    pairs = [("feat0", g["grad_feat_c0"]), ("feat1", g["grad_feat_c1"])] + ([("dbin", np.atleast_1d(g["grad_bin_score"]))] if head == "ot" else [])
    for k, ref in pairs:
        assert np.abs(ref).max() > 0 and np.abs(got[k] - ref).max() <= 1e-5 * np.abs(ref).max(), (k, float(np.abs(got[k] - ref).max()), float(np.abs(ref).max()))


def test_dispatch_arithmetic_and_edges():
    assert (E.RCH, E.WAVES, E.LANES, E.COLS, E.TILE, E.WARPS, E.DBIN_THREADS, E.LOSS_BLOCKS) == (32, 4, 64, 256, 128, 2, 1024, 1024)
    assert E.col_chunks(31) == (1, 31, 1) and E.col_chunks(33) == (2, 17, 1) and E.col_chunks(65) == (3, 22, 2) and E.col_chunks(257) == (9, 29, 5)
    assert E.col_chunks(258) == (9, 29, 6) and E.col_chunks(64) == (2, 32, 2) and E.generic_partials(129, 127) == (4, 2, 1, 127)
    assert not E.edge_failures() and {e for c in E.CASES for e in c.edges} == set(E.EDGES)
    ds = {(c.N, c.L, c.S, c.C, c.G, c.mask) for c in E.DS_CASES}
    assert ds == ({(3, L, 160, 256, "dense", None) for L in (1, 31, 32, 33, 65, 257)} | {(2, 33, 160, 256, "dense", None)}
                  | {(3, 33, S, 256, "dense", None) for S in (1, 63, 64, 65, 255, 256, 257, 961)}
                  | {(3, L, S, 256, "dense", m) for L, S in ((257, 160), (33, 257)) for m in "ab"}
                  | {(3, 65, 257, 256, G, None) for G in ("dense", "sparse", "loss", "rows")}
                  | {(2, 129, 127, C, "dense", m) for C in (32, 128) for m in (None, "c")} | {(2, 33, 257, 128, "dense", None)})
    ot = {(c.N, c.L, c.S, c.C, c.G, c.mask, c.iters, c.bin_score, c.want1) for c in E.OT_CASES}
    std = lambda N, L, S, C=256, G="dense", m=None, it=3, b=1.0, w=True: (N, L, S, C, G, m, it, b, w)
    assert ot == ({std(3, L, 160) for L in (1, 30, 31, 32, 63, 257)} | {std(3, 33, S) for S in (1, 62, 63, 64, 254, 255, 256, 960, 961)}
                  | {std(2, 3, S, G="norow") for S in (5119, 5120, 12287, 12288)} | {std(1, 129, 12288, G="norow")} | {std(2, 33, 65, it=it) for it in (0, 1, 2)}
                  | {std(3, L, S, m=m) for L, S in ((257, 160), (33, 257)) for m in "ab"} | {std(2, 129, 127, C=128, m="c")}
                  | {std(3, 63, 257, G=G) for G in ("dense", "loss", "bins")} | {std(2, 33, 65, b=-3.0), std(2, 33, 65, w=False)})
    # N rows mod 4 takes every value; the d bin_score sum runs below and above its 1024 threads; both pass alignments occur
    for head in ("ds", "ot"):
        assert {c.N * (c.L + (head == "ot")) % 4 for c in E.CASES if c.head == head} == {0, 1, 2, 3}
    assert {c.N * (c.L + c.S + 1) < 1024 for c in E.OT_CASES} == {True, False} and {c.S % 4 == 0 for c in E.OT_CASES} == {True, False}
    assert {(c.M, c.W, c.C, c.peaked, c.plain) for c in E.FINE_CASES} == (
        {(M, 5, 128, False, False) for M in (1, 3, 4, 5, 1025)} | {(37, W, 128, False, False) for W in (2, 3, 7, 8)}
        | {(37, 5, C, False, False) for C in (32, 64, 96, 160)} | {(37, 5, 128, True, False), (1, 5, 128, False, True)}) and not E.FINE_SEEDS
    assert {(c.kind, c.M, c.masked) for c in E.LOSS_CASES} == {(k, M, m) for k in range(4) for M in (0, 1, 256, 257) for m in (False, True)}
    assert {(c.M, c.fine_type, c.correct) for c in E.FINE_LOSS_CASES} == {(M, t, ok) for M in (1, 256, 257) for t in ("l2", "l2_with_std") for ok in (True, False)}


@pytest.mark.parametrize("name", HEADS)
def test_head_reference(name):
    c, f, i = E.CASE_BY_NAME[name], E.facts(name), E.inputs(name)
    assert f["finite"] and not f["exact"], f["exact"]
    # two independent derivations of the backward (torch.autograd of the restated head; the hand-derived oracle) and the step-by-step
    # restatement the mistakes are built into agree in float64 to 1e-10 of the scale
    for d in (f["oracle_distance"], f["formula_distance"]):
        for k, v in d.items():
            assert v <= 1e-10, (name, k, v)
    assert set(E.outputs_of(c)) == set(E.HEAD_OUTPUTS[c.head]) - ({"dbin"} if name in E.DBIN_UNCLAIMED else set()) - (set() if c.want1 else {"feat1"})
    for k in E.outputs_of(c):
        noise, scale = f["noise"][k], f["scale"][k]
        assert scale > 0 and noise <= E.abs_tolerance(k, noise, scale) / 2 and noise <= 1e-5 * scale, (name, k, noise, scale)
    if c.head == "ot":
        # d bin_score: where it is compared with ref64 the tolerance is a small share of the value (the check cannot become empty); where
        # it is not, a side has 1 or 3 tokens; and ref64 itself passes the self check the GPU run is held to
        if name in E.DBIN_UNCLAIMED:
            assert min(c.L, c.S) <= 3
        else:
            assert E.abs_tolerance("dbin", f["noise"]["dbin"], f["scale"]["dbin"]) <= E.DBIN_TOLERANCE_SHARE * f["scale"]["dbin"]
        assert f["self_check"][0] <= f["self_check"][1] and f["self_check"][1] <= 2e-7 * max(f["scale"]["dbin"], 1e-3 * f["scale"]["dZ"])
    for k, left in f["left_out"].items():
        # the row-wise check leaves out the rows that are identically zero in ref64 -- those of masked tokens, and of a pair with ONE valid
        # token on each side (conf = 1 there whatever the descriptors: d sim = 2 t - t - t) -- and no other
        assert left == 0 and f["noise_row"][k] <= E.row_tolerance(k, f["noise_row"][k]) / 2, (name, k, left)
        if c.mask is None:
            assert f["zero_rows"][k] == 0, (name, k)
    if c.mask is not None:
        v0, v1 = i["v0"], i["v1"]
        one = [n for n in range(c.N) if v0[n].sum() == 1 and v1[n].sum() == 1]
        # (Sinkhorn: a masked row's only live entry is its dustbin -- its mass is fixed, d Z is exactly 0 there; a lone token has its dustbin too)
        rows0 = int((~v0).sum()) + (len(one) if c.head == "ds" else 0)
        assert f["zero_rows"]["feat0"] == rows0 == f["zero_rows"]["dsim" if c.head == "ds" else "dZ"] and len(one) == (c.mask == "b")
    if c.G == "sparse":                               # every row carries a planted entry: nothing may be left out either
        assert i["planted"].any(2).all() and f["left_out"]["dsim"] == 0


@pytest.mark.parametrize("name,mutation", [(c.name, m) for c in E.CASES for m in (E.DS_MUTATIONS if c.head == "ds" else E.OT_MUTATIONS)
                                           if E.mutation_applies(c, m)])
def test_head_mutation_is_far_outside_the_tolerance(name, mutation):
    d = E.facts(name)["mutation_distance"][mutation]
    assert d >= E.DETECTION_FACTOR, (name, mutation, d)


def test_every_mutation_meets_its_edge():
    ap = lambda cases, muts, fn: {m: {c.name for c in cases if fn(c, m)} for m in muts}
    ds, ot = ap(E.DS_CASES, E.DS_MUTATIONS, E.mutation_applies), ap(E.OT_CASES, E.OT_MUTATIONS, E.mutation_applies)
    every_ds, every_ot = {c.name for c in E.DS_CASES}, {c.name for c in E.OT_CASES}
    assert len(E.DS_MUTATIONS) == 5 and ds["col_sum_omits_last_chunk"] == ds["row_sum_omits_last_stride"] == ds["factor_2_dropped"] == every_ds
    assert ds["mask_fill_not_zeroed"] == {c.name for c in E.DS_CASES if c.mask} and len(ds["mask_fill_not_zeroed"]) == 6
    assert ds["r_and_c_exchanged"] == every_ds and all(c.L != c.S for c in E.DS_CASES)
    assert len(E.OT_MUTATIONS) == 7
    iterated = every_ot - {"ot_iters0"}
    assert ot["du_overwritten_at_T"] == iterated and ot["log_mu_of_dustbin_for_all_rows"] == iterated - {"ot_col_S1"}
    variants = {"ot_var_S5119", "ot_var_S5120", "ot_var_S12287", "ot_var_S12288", "ot_var_129x12288"}
    assert set(E.DBIN_UNCLAIMED) == (variants - {"ot_var_129x12288"}) | {"ot_row_L1", "ot_col_S1"} and {c.name for c in E.OT_CASES if c.G == "norow"} == variants
    assert ot["col_sums_omit_dustbin_row"] == iterated - variants
    assert ot["one_reverse_iteration_fewer"] == iterated - variants - {"ot_row_L1", "ot_col_S1"}
    assert ot["corner_twice_in_dbin"] == ot["corner_left_out_of_dbin"] == every_ot
    assert ot["second_pair_dustbins_at_first_offset"] == every_ot - {"ot_var_129x12288"}
    fine = ap(E.FINE_CASES, E.FINE_MUTATIONS, E.fine_mutation_applies)
    assert fine["std_term_dropped"] == {c.name for c in E.FINE_CASES} and len(E.FINE_CASES) == 15 and fine["centre_index_rounded_down"] == {"fine_W2", "fine_W8"}
    assert fine["last_channel_stride_not_written"] == {"fine_C32", "fine_C96", "fine_C160"}
    loss = ap(E.LOSS_CASES, E.LOSS_MUTATIONS, E.loss_mutation_applies)
    dense = {c.name for c in E.LOSS_CASES if c.kind >= 2}
    assert loss["rows_beyond_1024_not_written"] == loss["columns_beyond_256_not_written"] == dense and len(dense) == 16
    assert loss["clamp_open_everywhere"] == dense | {c.name for c in E.LOSS_CASES if c.kind == 1 or c.M >= 256}


# ---- fine_match_bwd ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in E.FINE_CASES])
def test_fine_reference_and_mutations(name):
    from oracle import grad_oracle as GO
    c, i, r = E.FINE_BY_NAME[name], E.fine_inputs(name), E.fine_reference(name)
    WW = c.W * c.W
    assert (i["g"][:, 2] != 0).all() and i["f1"][0].any() == c.plain
    for k in ("d0", "d1"):
        noise, scale = r["noise"][k], r["scale"][k]
        assert np.isfinite(r["ref64"][k]).all() and noise <= E.abs_tolerance(k, noise, scale) / 2 and noise <= 1e-5 * scale, (name, k, noise, scale)
        assert (scale > 0) == (c.M > 1 or c.plain or k == "d1")                                        # (fine_M1: the uniform match alone, d0 = 0)
    off = np.arange(WW) != WW // 2
    assert not r["ref64"]["d0"][:, off].any() and not r["ref32"]["d0"][:, off].any()
    # match 0: a uniform heat map (its std gradient is the full one);  the last match: one-hot, the variance clamp closed -- d expec_f's
    # std column moves nothing there
    std_only = np.zeros_like(i["g"]); std_only[:, 2] = 1
    d0, d1 = GO.fine_matching_grad(i["f0"], i["f1"], std_only)
    # (f1 = 0: d0 = sum_r dsim_r f1_r = 0, d1 = dsim_r f0;  W = 2: x^2 = 1 at every position, the variance 1 - E[x]^2 is flat at E[x] = 0)
    assert (np.abs(d1[0]).max() > 0) == (c.W > 2) and (np.abs(d0[0]).max() == 0) == (not c.plain)
    if c.M > 1:
        assert not d0[-1].any() and not d1[-1].any() and np.abs(d1[1:-1]).max() > 0
    for m in E.FINE_MUTATIONS:
        if E.fine_mutation_applies(c, m):
            d = E.distance_in_tolerances(E.fine_mutated(name, m), r)
            assert d >= E.DETECTION_FACTOR, (name, m, d)


# ---- the loss gradients ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in E.LOSS_CASES])
def test_loss_reference_and_mutations(name):
    c, i, r = E.LOSS_BY_NAME[name], E.loss_inputs(name), E.loss_reference(name)
    conf, g = i["conf"], r["ref64"]["grad_conf"]
    assert conf.min() > 0 and conf.max() < 1 and (conf < 1e-6).any() and (conf > np.float32(1 - 1e-6)).any() and g.shape == conf.shape
    assert len(set(zip(i["b"].tolist(), i["i"].tolist(), i["j"].tolist()))) == c.M and (i["i"] > 0).all()
    if c.masked:
        assert not i["m1"][3].any() and i["m0"][3].all() and i["m0"].reshape(5, -1).any(1).all()
    noise, scale = r["noise"]["grad_conf"], r["scale"]["grad_conf"]
    assert np.isfinite(g).all() and noise <= E.abs_tolerance("grad_conf", noise, scale) / 2 and noise <= 1e-5 * scale, (name, noise, scale)
    assert (scale > 0) == (c.kind >= 1 or c.M > 0)    # (sparse focal without ground truth: no gradient at all)
    if c.kind <= 1 and c.M >= 256:                    # supervised entries on both closed sides of the clamp
        at = conf[i["b"], i["i"], i["j"]]
        assert (at < 1e-6).any() and (at > np.float32(1 - 1e-6)).any() and (g[i["b"], i["i"], i["j"]] == 0).sum() >= 2 * (c.M // 5)
    for m in E.LOSS_MUTATIONS:
        if E.loss_mutation_applies(c, m):
            d = E.distance_in_tolerances(E.loss_mutated(name, m), r)
            assert d >= E.DETECTION_FACTOR, (name, m, d)


@pytest.mark.parametrize("name", [c.name for c in E.FINE_LOSS_CASES])
def test_fine_loss_reference(name):
    c, i, r = E.FINE_LOSS_BY_NAME[name], E.fine_loss_inputs(name), E.fine_loss_reference(name)
    g, noise, scale = r["ref64"]["grad_expec"], r["noise"]["grad_expec"], r["scale"]["grad_expec"]
    correct = np.abs(i["gt"]).max(1) < 1.0
    assert correct.any() == c.correct and correct[0] == c.correct and not g[:, 2].any()
    assert noise <= E.abs_tolerance("grad_expec", noise, scale) / 2 and noise <= 1e-5 * scale
    # without a correct match, in training mode: plain l2 supervises entry 0 falsely; l2_with_std gives it weight 0 -- no gradient at all
    assert (scale > 0) == (c.correct or c.fine_type == "l2")
    if not c.correct and c.fine_type == "l2":
        assert g[0, :2].all() and not g[1:].any()
