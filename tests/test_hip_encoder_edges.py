"""The coarse encoder against the numpy oracle in FLOAT64 at its wave, tile and XCD-split edges (cases, reference and tolerance:
tests/_encoder_edge_cases.py).  Every other coarse-transformer test compares the kernels with themselves (scheduled against call order,
persistent against launches, padded against unpadded, run against run): a mistake all forms share passes them.

Tolerance: err <= k * noise + 1e-6 * scale, capped by the project's own bounds (2e-5 * max(1, scale) for a layer, 2e-4 for the
transformer), where noise is the distance of the oracle's own float32 run to its float64 run on the same case.  k is twice the largest
err / noise measured on an MI355X, rounded up: 1.99 (magnitude_down) -> k = 4 for the layer cases, 1.22 (8x130x75_masked) -> k = 3 for the
transformer cases (profiles/encoder_edges_accuracy.txt holds the lines they were taken from; the factor 2 covers summation-order
differences between machines and between the persistent and the launch form).  Each run prints its own figures before it asserts, and appends them to the
file LOFTR_EDGES_REPORT names, if set (how profiles/encoder_edges_accuracy.txt was written).
"""
import os

import numpy as np
import pytest

import _encoder_edge_cases as E

pytestmark = pytest.mark.gpu


def _report(line):
    path = os.environ.get("LOFTR_EDGES_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")
    print(line)


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared inputs are read-only)


@pytest.mark.parametrize("name", [c.name for c in E.LAYER_CASES])
def test_encoder_layer_vs_float64(name):
    """ops.encoder_layer (loftr_encoder_layer_fwd: proj_kv_kernel, kv_finalize_kernel, efx::encoder_x_kernel) against ref64 over ALL
    tokens -- the unpadded entry point computes padding tokens too, and so does the reference.  Finite everywhere first: a sequence whose
    source mask is all zero has Ksum = 0, and the reference's message there is exactly 0 (linear_attention.py:37-45; before the den == 0
    guard of encoder_x_body such a sequence came back finite but 4-5 off: NaN from the merge, turned into 0 by the ReLU of mlp.0).
    k = K_LAYER = 4, see the module docstring."""
    import torch
    from loftr_amd import ops
    from loftr_amd.loftr import LoFTREncoderLayer
    i, r = E.layer_inputs(name), E.layer_reference(name)
    c = i["case"]
    layer = LoFTREncoderLayer(E.C, E.H).eval()
    layer.load_state_dict({k[2:]: torch.from_numpy(v.copy()) for k, v in i["w"].items()})
    layer = layer.cuda()
    x, xm = _t(i["x"]), _t(i["xm"])
    if c.self_attn:
        src, sm = x, xm                                  # the self form: one tensor, one mask object
    else:
        src, sm = _t(i["src"]), _t(i["sm"])
    with torch.no_grad():
        got = ops.encoder_layer(x, src, layer.weight_struct(), E.H, xm, sm)
    torch.cuda.synchronize()
    got = got.cpu().numpy().astype(np.float64)
    bad = ~np.isfinite(got)
    assert not bad.any(), (name, "not finite: sequences", sorted(set(np.nonzero(bad)[0].tolist())), "values", int(bad.sum()))
    err = float(np.abs(got - r["ref64"]).max())
    tol = E.layer_tolerance(r["noise"], r["scale"])
    _report(f"layer       {name:20s} {'':22s} err {err:.3e} noise {r['noise']:.3e} err/noise {err / r['noise']:6.2f} scale {r['scale']:8.3f}")
    assert err <= tol, (name, err, tol, r["noise"], r["scale"])


@pytest.fixture(scope="module")
def coarse():
    """The model's coarse transformer (8 layers) with synth.make_weights(0, cfg), as in test_hip_parity._coarse_transformer_case."""
    import torch
    from loftr_amd import LoFTR
    cfg, w = E.transformer_setup()
    model = LoFTR(cfg).eval()
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in w.items()}, strict=False)
    tr = model.cuda().loftr_coarse
    structs = [layer.weight_struct() for layer in tr.layers]
    return tr, structs, tr._prepared(structs, torch.device("cuda", 0))


@pytest.mark.parametrize("name", [c.name for c in E.TRANSFORMER_CASES])
def test_coarse_transformer_vs_float64(name, coarse):
    """ops.transformer (inplace=False) against ref64 as per-call launches (coarse_transformer_scheduled), as the persistent kernel
    (coarse_persistent_kernel with its K fold) and as the persistent kernel in call order; the status word stays 0.  Masked cases also
    with skip_padded=True (128-token tiles without a valid token keep their input), compared on the valid tokens.
    k = K_TRANSFORMER = 3, see the module docstring."""
    import torch
    from loftr_amd import ops
    tr, structs, prepared = coarse
    i, r = E.transformer_inputs(name), E.transformer_reference(name)
    c = i["case"]
    f0, f1, m0, m1 = _t(i["f0"]), _t(i["f1"]), _t(i["m0"]), _t(i["m1"])
    tol = E.transformer_tolerance(r["noise"], r["scale"])
    runs = [("launches", False), ("persistent", False), ("persistent_call_order", False)] + ([("launches", True)] if c.masked else [])
    failures = []
    for mode, skip in runs:
        diag = torch.zeros(16, dtype=torch.uint8, device="cuda")
        with torch.no_grad():
            out = ops.transformer(f0, f1, structs, tr.layer_names, tr.nhead, m0, m1, inplace=False, prepared=prepared, mode=mode, diag=diag,
                                  skip_padded=skip)
        torch.cuda.synchronize()
        assert int(diag.view(torch.int32)[0].item()) == 0, (name, mode)
        err = 0.0
        for got, ref, m in zip(out, r["ref64"], (i["m0"], i["m1"])):
            got = got.cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all(), (name, mode, skip)
            d = np.abs(got - ref)
            err = max(err, float((d[m] if skip else d).max()))
        label = mode + ("+skip_padded" if skip else "")
        _report(f"transformer {name:20s} {label:22s} err {err:.3e} noise {r['noise']:.3e} err/noise {err / r['noise']:6.2f} scale {r['scale']:8.3f}")
        if err > tol:
            failures.append((label, err))
    assert not failures, (name, failures, tol, r["noise"], r["scale"])
