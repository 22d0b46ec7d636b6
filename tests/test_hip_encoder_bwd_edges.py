"""loftr_encoder_layer_bwd (csrc/encoder_bwd.hip: outer_accum_kernel / outer_reduce_kernel, attn_q_kernel, attn_kv_bwd_kernel,
ln_bwd_kernel; csrc/head_grads.hip: launch_wgrad, reduce_partials_kernel, reduce_partials_tall_kernel) and loftr_encoder_layer_fwd
against torch.autograd of the layer in FLOAT64 at the chunk, block, partial-count and dispatch edges of their work distribution, under
padding masks that cut, empty and nearly empty a chunk, with gradients of very small and of row-wise different magnitude, and on the
paths the debug switches `wgrad_chunk` and `reduce_tall` select.  Cases, reference, tolerances and the conditions the inputs meet:
tests/_encoder_bwd_cases.py.

Per tensor (out, grad_x, grad_source, the six weight matrices entry by entry, the four LayerNorm gradients):
err = max|got - ref64| <= K[group] * noise + 1e-6 * scale, where noise is the distance of the reference's own float32 run to its float64
run on the same case.  Each run prints its figures before it asserts, and appends them to the file LOFTR_EDGES_REPORT names, if set (how
profiles/encoder_bwd_accuracy.txt was written)."""
import os

import numpy as np
import pytest

import _encoder_bwd_cases as E

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


def _run(inp):
    import torch
    from loftr_amd import ops
    w = {f: _t(inp["w"][n]) for f, n in E.MG.FIELDS}
    x, s, xm, sm = _t(inp["x"]), _t(inp["source"]), _t(inp["x_mask"]), _t(inp["source_mask"])
    gx, gs, gw = ops.encoder_layer_bwd(x, s, w, _t(inp["G"]), inp["H"], xm, sm)
    out = ops.encoder_layer(x, s, ops.layer_weights_struct(w), inp["H"], xm, sm)
    torch.cuda.synchronize()
    return dict(out=out.cpu().numpy(), grad_x=gx.cpu().numpy(), grad_source=gs.cpu().numpy(), **{"grad_" + f: gw[f].cpu().numpy() for f in E.FIELDS})


def _check(name, path, got, r):
    failures = []
    for k in E.OUTPUTS:
        assert got[k].shape == r["ref64"][k].shape and np.isfinite(got[k]).all(), (name, path, k, "shape or not finite")
        err, noise, scale = float(np.abs(got[k].astype(np.float64) - r["ref64"][k]).max()), r["noise"][k], r["scale"][k]
        tol = E.tolerance(k, noise, scale)
        _report(f"{name:24s} {path:24s} {k:13s} {E.GROUP[k]:6s} err {err:.3e} noise {noise:.3e} err/noise {err / noise if noise > 0 else float('inf'):6.2f} "
                f"scale {scale:.3e} err/tol {err / tol:5.2f}")
        if err > tol:
            failures.append((k, err, tol, noise, scale))
    assert not failures, (name, path, failures)


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_encoder_layer_bwd_vs_float64(name):
    """All twelve gradients and the forward's `out` against ref64.  K: see tests/_encoder_bwd_cases.py."""
    _check(name, "default", _run(E.inputs(name)), E.reference(name))


@pytest.mark.parametrize("name,switches", E.FORCED, ids=[f"{n}-{'-'.join(f'{k}={v}' for k, v in sw.items())}" for n, sw in E.FORCED])
def test_encoder_layer_bwd_forced_paths_vs_float64(name, switches):
    """The same cases, reference and tolerances on the paths the debug switches select: a forced split-K chunk, the generic reduction in
    place of the tall one.  The switches are back at their defaults afterwards."""
    from loftr_amd import ops
    with ops.debug_switch(**switches):
        assert all(ops.debug_get(k)[0] == v for k, v in switches.items())
        got = _run(E.inputs(name))
    assert {k: ops.debug_get(k) for k in E.SWITCH_DEFAULTS} == {k: (v, v) for k, v in E.SWITCH_DEFAULTS.items()}
    _check(name, ",".join(f"{k}={v}" for k, v in switches.items()), got, E.reference(name))
