"""CPU: the float64 comparison of tests/test_hip_encoder_edges.py can fail.  For every layer case of tests/_encoder_edge_cases.py and
every modelled kernel mistake that applies to it, the float64 oracle with the mistake built in differs from the unmodified one by at
least 20 times the case's tolerance; the oracle's own float32 run stays inside half of it.  The factor 20 is a condition on the choice of
the inputs, not a measurement: a case that misses it gets other inputs, never another factor."""
import numpy as np
import pytest

import _encoder_edge_cases as E

DETECTION_FACTOR = 20.0


def _tol(name):
    r = E.layer_reference(name)
    return E.layer_tolerance(r["noise"], r["scale"])


@pytest.mark.parametrize("name", [c.name for c in E.LAYER_CASES])
def test_layer_reference_noise_is_well_inside_the_tolerance(name):
    r = E.layer_reference(name)
    assert np.isfinite(r["ref64"]).all() and np.isfinite(r["ref32"]).all()
    assert r["noise"] <= _tol(name) / 2, (name, r["noise"], _tol(name))


@pytest.mark.parametrize("name", [c.name for c in E.TRANSFORMER_CASES])
def test_transformer_reference_noise_is_well_inside_the_tolerance(name):
    r = E.transformer_reference(name)
    assert all(np.isfinite(a).all() for a in r["ref64"] + r["ref32"])
    assert r["noise"] <= E.transformer_tolerance(r["noise"], r["scale"]) / 2, (name, r["noise"], r["scale"])


@pytest.mark.parametrize("name", [c.name for c in E.LAYER_CASES])
def test_hooked_layer_is_the_oracle(name):
    """layer_float64 without a mutation is oracle.encoder_layer in float64 (float64 rounding apart)."""
    r = E.layer_reference(name)
    assert np.abs(E.layer_float64(name) - r["ref64"]).max() <= 1e-12 * r["scale"]


@pytest.mark.parametrize("name,mutation", [(c.name, m) for c in E.LAYER_CASES for m in E.MUTATIONS if E.mutation_applies(c, m)])
def test_mutation_is_far_outside_the_tolerance(name, mutation):
    r = E.layer_reference(name)
    d = float(np.abs(E.layer_float64(name, mutation) - r["ref64"]).max())
    assert d >= DETECTION_FACTOR * _tol(name), (name, mutation, d, _tol(name), d / _tol(name))


def test_every_mutation_and_every_edge_is_exercised():
    used = {m for c in E.LAYER_CASES for m in E.MUTATIONS if E.mutation_applies(c, m)}
    assert used == set(E.MUTATIONS) and len(E.MUTATIONS) == 7
    shapes = {(c.nb, c.L, c.S) for c in E.LAYER_CASES}
    assert {L for nb, L, S in shapes if (nb, S) == (3, 129)} >= {1, 31, 32, 33, 127, 128, 129, 257}
    assert {S for nb, L, S in shapes if (nb, L) == (3, 129)} >= {1, 127, 128, 385}
    assert {nb for nb, L, S in shapes if (L, S) == (257, 129)} >= {1, 2, 4, 5, 8, 9}
    for c in E.LAYER_CASES:
        if c.masked:
            xm, sm = E.layer_masks(c)
            assert xm[0].sum() % 32 != 0 and sm[0].sum() % 128 != 0 and 0 < xm[0].sum() < c.L and 0 < sm[0].sum() < c.S
            assert not sm[-1].any() and (c.self_attn or xm[-1].all())


def test_mask_edge_patterns():
    xm, sm = E.layer_masks(E.LAYER_CASE_BY_NAME["mask_3x129x385"])
    assert not sm[1, 128:256].any() and sm[1, :128].all() and (~sm[1, 256:384]).sum() == 10 and sm[1, 384]
    xm, sm = E.layer_masks(E.LAYER_CASE_BY_NAME["mask_9x257x127"])
    assert not xm[2].any() and sm[2].all()
    for c in E.TRANSFORMER_CASES:
        if c.masked:
            for m in (E.transformer_inputs(c.name)["m0"], E.transformer_inputs(c.name)["m1"]):
                n_valid = m.sum(1)
                assert (n_valid > 0).all() and (n_valid % 32 != 0).all() and (n_valid < m.shape[1]).all()
                assert all(m[n, :k].all() for n, k in enumerate(n_valid))                    # prefixes
                assert m.shape[1] <= 128 or not m[0, 128:].any()                              # a tile without a valid token


def test_magnitude_factor_is_the_largest_inside_the_operand_range():
    """magnitude_up multiplies x and source by the largest power of two that keeps the float64 oracle's intermediates inside the range
    the kernels' fp16 (hi, lo) operands have: an unscaled operand below 65504, P * 2^5 below 2^14."""
    _, inside = E.layer_float64("magnitude_up", want_operands=True)
    assert E.operands_in_range(inside), inside
    up = E.LAYER_CASE_BY_NAME["magnitude_up"]
    E.LAYER_CASE_BY_NAME["_magnitude_next"] = up._replace(name="_magnitude_next", log2_scale=up.log2_scale + 1)
    try:
        _, beyond = E.layer_float64("_magnitude_next", want_operands=True)
    finally:
        del E.LAYER_CASE_BY_NAME["_magnitude_next"]
    assert not E.operands_in_range(beyond), beyond
    assert E.LAYER_CASE_BY_NAME["magnitude_down"].log2_scale == -6


@pytest.mark.parametrize("name", [c.name for c in E.LAYER_CASES if c.L != c.S])
def test_both_lengths_from_the_wrong_side_cancel(name):
    """`v_length and 1 / S taken as L instead of S`, both at once, is no error and cannot be seen: values / v_length ... * v_length
    cancels (linear_attention.py:41-45).  The mutation of the table is therefore the one-sided form (v_length_from_x_side)."""
    r = E.layer_reference(name)
    d = float(np.abs(E.layer_float64(name, E.BOTH_LENGTHS_FROM_X_SIDE) - r["ref64"]).max())
    assert d <= 1e-12 * r["scale"], (name, d)


def test_cases_left_out_beyond_the_structural_conditions_are_these_six():
    """By shape alone phantom rows apply where S is no multiple of 128 and v_length_from_x_side where L != S.  mutation_applies leaves
    out six of those pairs, for the reasons written there (the mistake's size is set by the shape, not by the inputs): pinned here so that
    the list cannot grow unnoticed."""
    by_shape = {"phantom_source_rows": lambda c: c.S % 128 != 0, "v_length_from_x_side": lambda c: c.L != c.S}
    left_out = {(c.name, m) for c in E.LAYER_CASES for m, f in by_shape.items() if f(c) and not E.mutation_applies(c, m)}
    assert left_out == {("magnitude_up", "phantom_source_rows"), ("x_L127", "v_length_from_x_side"), ("x_L128", "v_length_from_x_side"),
                        ("src_S1", "v_length_from_x_side"), ("src_S127", "v_length_from_x_side"), ("src_S128", "v_length_from_x_side")}
