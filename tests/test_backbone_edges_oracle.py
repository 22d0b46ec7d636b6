"""CPU: the conditions tests/_backbone_edge_cases.py states about its cases hold, and the float64 comparison of
tests/test_hip_backbone_edges.py can fail.  The restated dispatch of conv_run puts every case on the kernel and at the edge it is in the
table for; ref32 stays inside the caps of both checks; the integer cases are exact in float32; the GPU module skips nothing.  The float64
reference with one modelled kernel mistake built in sits at least DETECTION_FACTOR tolerances from the unmodified one on every case the
mistake applies to (the dropped low half of one channel group: PRECISION_FLOOR at more than 128 input channels)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _backbone_edge_cases as E

CONV = [c.name for c in E.CONV_CASES]


def test_dispatch_arithmetic_and_constants():
    assert (E.BM, E.BN, E.NS, E.BK, E.TY, E.TX, E.NUM_XCD) == (256, 128, 3, 32, 8, 32, 8)
    # the backbone's own layers at 480 x 640, B = 2: where conv_run sends them
    assert E.conv_path(128, 3, 1) == "duo128" and E.conv_path(256, 3, 1) == "duo128" and E.conv_path(196, 3, 1) == "wide224"
    assert E.conv_path(196, 3, 1, rem=True) == "rem" and E.conv_path(196, 3, 1, rem=True, want_f32=True) == "wide224" and E.conv_path(200, 3, 1, rem=True) == "wide224"
    assert E.conv_path(192, 3, 1) == "duo192" and E.conv_path(40, 3, 1) == "generic" and E.conv_path(128, 3, 1, conv_duo=0) == "generic"
    assert E.conv_path(196, 3, 2) == "gemm" and E.conv_path(256, 1, 1) == "gemm" and E.conv_path(196, 3, 1, conv_patch=0) == "gemm" and E.conv_path(128, 1, 1, up=True) == "gemm"
    p = E.gemm_plan(2, 128, 196, 3, 2, 22, 30)                   # the one map tests/test_hip_backbone.py runs the strided layers at
    assert (p.M, p.tiles_m, p.tiles_n, p.nk, p.chunk, p.grid, p.last_rows) == (330, 2, 2, 36, 1, 16, 74)
    p = E.gemm_plan(2, 128, 196, 3, 2, 240, 320)
    assert (p.M, p.tiles_m, p.chunk, p.idle) == (38400, 150, 19, 4)
    assert E.patch_plan(2, 128, 240, 320, "duo128")[:4] == (10, 30, 600, 1) and E.patch_plan(2, 196, 120, 160, "wide224")[:4] == (5, 15, 150, 1)
    assert E.patch_plan(2, 200, 60, 100, "generic", persist_cap=8).grid == 8 and E.patch_plan(2, 200, 60, 100, "generic").grid == 128 and E.patch_plan(8, 200, 60, 100, "generic").grid == 256
    assert E.stem_grid(2, 480, 640) == (10, 30, 2) and E.stem_grid(1, 1, 1) == (1, 1, 1) and E.stem_grid(3, 17, 65) == (2, 2, 3)
    for tiles_m in range(1, 40):                                 # xcd_tile visits every tile exactly once
        for tiles_n in (1, 2, 4):
            seen = [E.xcd_tile(w, tiles_m, tiles_n) for w in range(E.NUM_XCD * E._cdiv(tiles_m, E.NUM_XCD) * tiles_n)]
            assert sorted(t for t in seen if t is not None) == [(m, n) for m in range(tiles_m) for n in range(tiles_n)]


def test_every_case_is_at_the_edge_it_is_listed_for():
    assert not E.conv_edge_failures()
    assert {e for c in E.CONV_CASES for e in c.edges} == set(E.CONV_EDGES)
    shapes = {(c.B, c.cin, c.cout, c.k, c.stride, c.H, c.W) for c in E.CONV_CASES if c.family == "gemm"}
    assert shapes >= {(1, 32, 32, 1, 1, 1, 1), (1, 128, 128, 1, 1, 15, 17), (1, 32, 128, 1, 1, 16, 16), (1, 64, 196, 1, 2, 1, 513), (5, 128, 196, 3, 2, 13, 17),
                      (1, 128, 196, 3, 2, 31, 31), (3, 256, 512, 3, 2, 48, 64), (3, 96, 256, 1, 1, 25, 31), (3, 512, 512, 1, 1, 24, 32), (3, 256, 512, 1, 2, 31, 33),
                      (2, 128, 129, 1, 1, 9, 13), (2, 40, 40, 3, 2, 9, 13), (2, 196, 196, 3, 1, 9, 33)}
    three = [c for c in E.CONV_CASES if c.family != "gemm"]
    assert {(c.H, c.W) for c in three} == {(1, 1), (1, 33), (2, 2), (7, 31), (8, 32), (9, 33), (9, 65)}
    assert {E.plan_of(c).tiles for c in three} >= {1, 7, 8, 9}
    widths = {(c.family, c.cin, c.cout) for c in three if not c.switches}
    assert widths >= {("duo128", 16, 128), ("duo128", 128, 256), ("duo128", 512, 512), ("duo128", 256, 384), ("duo192", 196, 192), ("wide224", 196, 196),
                      ("wide224", 128, 224), ("wide224", 64, 193), ("generic", 64, 40), ("generic", 96, 160), ("rem", 196, 196)}
    for fam, cov in E.conv_coverage().items():
        assert cov["acts"] == {0, 1, 2} and cov["bn"] == {True, False} and cov["res"] == {True, False}, fam
    assert not [(c.name, e) for c in E.STEM_CASES for e in c.edges if not E.STEM_EDGES[e](c, E.stem_grid(c.B, c.H, c.W))]
    assert {(c.H, c.W) for c in E.STEM_CASES} == {(1, 1), (15, 63), (16, 64), (17, 65), (50, 71)} and {c.C0 for c in E.STEM_CASES} == {128, 96, 40, 8}
    assert {c.B for c in E.STEM_CASES} == {1, 3} and {c.crop for c in E.STEM_CASES} == {True, False} and E.STEM_UNSUPPORTED_C0 == 160
    assert not [(c.name, e) for c in E.UP_CASES for e in c.edges if not E.UP_EDGES[e](c)]
    assert {c.B for c in E.UP_CASES} == {1, 3, 5} and {c.C for c in E.UP_CASES} == {40, 128, 196, 256, 512}
    assert {(c.resolution, c.H, c.W, c.B) for c in E.NET_CASES} == {(r, h, w, b) for r, hw in (((8, 2), ((8, 8), (8, 264), (24, 40))), ((16, 4), ((16, 16), (48, 80))))
                                                                      for h, w in hw for b in (1, 3)}


def test_the_gpu_module_skips_nothing():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_hip_backbone_edges.py")).read()
    assert not [w for w in ("pytest.skip", "mark.skip", "skipif", "importorskip", "xfail") if w in src]


def _check_noise(kind, family, ref, name):
    assert np.isfinite(ref["ref64"]).all() and np.isfinite(ref["ref32"]).all() and ref["scale"] > 0, name
    assert ref["noise"] <= E.CAP[kind] * ref["scale"] / 2, (name, ref["noise"], ref["scale"])      # (float32 bilinear weights: up to 0.45 of the 2e-6 cap)
    assert ref["noise"] <= E.tolerance(kind, family, ref["noise"], ref["scale"]), name
    if ref.get("channels"):
        assert ref["ch_noise"].max() <= 4e-6, (name, float(ref["ch_noise"].max()))
        assert ref["live"].sum() >= len(ref["live"]) // 2 and all((ref["ch_noise"] <= E.channel_tolerance(family, out, ref["ch_noise"]) / 2).all() for out in E.K_CH[family]), name


@pytest.mark.parametrize("name", CONV)
def test_conv_reference_noise(name):
    c, r = E.CONV_BY_NAME[name], E.conv_reference(name)
    _check_noise("conv", c.family, r, name)
    Ho, Wo = E.out_hw(c.H, c.W, c.k, c.stride)
    assert r["ref64"].shape == (c.B, c.cout, Ho, Wo) and r["channels"] == (c.B * Ho * Wo >= 256)
    if c.weights == "bnedge":                                    # the gamma = 0 channel is act(beta) everywhere, the tiny variance lifts its channel
        assert r["channels"] and np.abs(r["ref64"][:, E.GAMMA0_CH] - r["gamma0_value"]).max() <= 1e-7 * max(1.0, abs(r["gamma0_value"])) and r["gamma0_value"] != 0
        assert r["ch_scale"][E.TINY_VAR_CH] >= 20 * np.median(r["ch_scale"])
    if c.weights == "rows":
        assert r["channels"] and r["ch_scale"][E.SMALL_ROW] <= 2e-2 * np.median(r["ch_scale"]) and r["ch_scale"][E.LARGE_ROW] >= 20 * np.median(r["ch_scale"])
        assert r["live"][E.SMALL_ROW]


@pytest.mark.parametrize("name", [c.name for c in E.STEM_CASES])
def test_stem_reference_noise(name):
    _check_noise("stem", "stem", E.stem_reference(name), name)
    i = E.stem_inputs(name)
    assert i["x"].is_contiguous() != i["case"].crop or i["x"].numel() == 1 * i["case"].B


@pytest.mark.parametrize("name", [c.name for c in E.UP_CASES])
def test_up_reference_noise(name):
    c = E.UP_BY_NAME[name]
    _check_noise(E.up_kind(c), E.up_kind(c), E.up_reference(name), name)


@pytest.mark.parametrize("name", [c.name for c in E.NET_CASES])
def test_net_reference_noise(name):
    r = E.net_reference(name)
    c = r["case"]
    assert r["outs"][0]["ref64"].shape[2:] == (c.H // c.resolution[0], c.W // c.resolution[0]) and r["outs"][1]["ref64"].shape[2:] == (c.H // c.resolution[1], c.W // c.resolution[1])
    for o in r["outs"]:
        assert o["scale"] > 0 and o["noise"] <= E.CAP["net"] * o["scale"] / 4, (name, o["noise"], o["scale"])


@pytest.mark.parametrize("name", E.EXACT_CONV)
def test_exact_conv_cases_are_exact_in_float32(name):
    c = E.CONV_BY_NAME[name]
    x, w, res, want = E.exact_conv(name)
    assert c.cin * c.k * c.k <= 4608 and float(want.abs().max()) < 32768 and float(want.abs().max()) > 0
    assert all(torch.equal(t, t.round()) for t in (x, w, want)) and x.abs().max() <= 8 and w.abs().max() <= 2
    got = F.conv2d(x, w, stride=c.stride, padding=c.k // 2)
    got = got + res if res is not None else got
    assert E.first_difference(got.double().numpy(), want.numpy()) is None
    assert torch.equal(x.half().float(), x) and torch.equal((w * 4096).half().float(), w * 4096)       # hi parts exact, lo parts zero


@pytest.mark.parametrize("name", [c.name for c in E.STEM_CASES])
def test_exact_stem_cases_are_exact_in_float32(name):
    x, w, want = E.exact_stem(name)
    assert E.first_difference(F.relu(F.conv2d(x, w, stride=2, padding=3)).double().numpy(), want.numpy()) is None and float(want.max()) > 0


def test_first_difference_reports_position_and_count():
    a = np.zeros((2, 3, 4, 5)); b = a.copy(); b[1, 2, 0, 3] = 1; b[1, 0, 3, 4] = 2
    assert E.first_difference(a, a) is None and E.first_difference(b, a) == (2, (1, 0, 3, 2), 1.0, 0.0)


@pytest.mark.parametrize("name,mutation", [(c.name, m) for c in E.CONV_CASES for m in E.CONV_MUTATIONS if E.conv_mutation_applies(c, m)])
def test_conv_mutation_is_far_outside_the_tolerance(name, mutation):
    c, i, r = E.CONV_BY_NAME[name], E.conv_inputs(name), E.conv_reference(name)
    with torch.no_grad():
        mut = E.conv_forward(i, torch.float64, mutation).numpy()
    d = E.distance_in_tolerances(mut, r, "conv", c.family, skip=(E.GAMMA0_CH,) if c.weights == "bnedge" else ())
    need = E.PRECISION_FLOOR if mutation == "lo_part_of_one_channel_group_dropped" and c.cin > 128 else E.DETECTION_FACTOR
    assert d >= need, (name, mutation, d)


def test_unmutated_forward_is_the_reference():
    for name in ("g_five_images_res", "c_196to196_9x33_bnedge", "g_cin40"):
        with torch.no_grad():
            assert np.array_equal(E.conv_forward(E.conv_inputs(name), torch.float64).numpy(), E.conv_reference(name)["ref64"])


@pytest.mark.parametrize("name", [c.name for c in E.STEM_CASES if c.C0 == 40])
def test_stem_mutation_is_far_outside_the_tolerance(name):
    r = E.stem_reference(name)
    with torch.no_grad():
        mut = E.stem_forward(E.stem_inputs(name), torch.float64, "last_channel_group_unwritten").numpy()
    assert E.distance_in_tolerances(mut, r, "stem", "stem") >= E.DETECTION_FACTOR


@pytest.mark.parametrize("name", [c.name for c in E.UP_CASES if c.Hl > 1 or c.Wl > 1])
def test_up_mutation_is_far_outside_the_tolerance(name):
    c, r = E.UP_BY_NAME[name], E.up_reference(name)
    with torch.no_grad():
        mut = E.up_forward(E.up_inputs(name), torch.float64, E.UP_MUTATIONS[0]).numpy()
    assert E.distance_in_tolerances(mut, r, E.up_kind(c), E.up_kind(c)) >= E.DETECTION_FACTOR


def test_every_mutation_meets_its_edge():
    applies = {m: {c.name for c in E.CONV_CASES if E.conv_mutation_applies(c, m)} for m in E.CONV_MUTATIONS}
    assert len(E.CONV_MUTATIONS) == 8 and all(applies.values())
    assert applies["tile_takes_image_of_its_first_row"] >= {"g_five_images", "g_ten_tiles", "g_cout129", "g_cin40", "g_512_s2"}
    assert applies["odd_H_stride_2_last_row_outside"] >= {"g_odd_s2", "g_m257_h1", "g_512_s2", "g_five_images"}
    assert applies["one_tap_of_last_pixel_of_ragged_tile_reads_zero"] >= {"g_m1", "g_m255", "g_m257_h1", "c_16to128_9x33", "c_64to40_1x1", "c_196to196_9x33_rem"}
    assert {E.CONV_BY_NAME[n].family for n in applies["bn_eps_left_out"]} == set(E.FAMILIES)
    assert {E.CONV_BY_NAME[n].family for n in applies["residual_added_after_activation"]} >= {"gemm"}
    assert {E.CONV_BY_NAME[n].family for n in applies["left_tap_reads_previous_rows_last_pixel"]} == set(E.FAMILIES)
    assert {E.CONV_BY_NAME[n].cin for n in applies["lo_part_of_one_channel_group_dropped"]} >= {16, 32, 128, 512}
