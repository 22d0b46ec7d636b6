"""FinePreprocess of loftr_amd.loftr in training mode under autograd (forward: ops.fine_preprocess; backward: loftr_fine_preprocess_bwd,
csrc/fine_bwd.hip, with launch_wgrad, colsum_part_kernel and the partial reductions of csrc/head_grads.hip) against torch.autograd of the
module in FLOAT64 at the match counts where the split-K partials, the column-sum blocks and the reductions change path, with windows
clipped at the corners of both maps, cells that carry several matches (up to all 48 on one), and fine maps in both memory formats.
Cases, reference and tolerances: tests/_fine_bwd_cases.py.

Per tensor (out0, out1, the four feature gradients, the two weight matrices entry by entry, the two biases):
err = max|got - ref64| <= K[group] * noise + 1e-6 * scale, noise being the distance of the reference's own float32 run to its float64 run.
Each run prints its figures before it asserts, and appends them to the file LOFTR_EDGES_REPORT names, if set (how
profiles/fine_bwd_accuracy.txt was written)."""
import os

import numpy as np
import pytest

import _fine_bwd_cases as E

pytestmark = pytest.mark.gpu


def _report(line):
    path = os.environ.get("LOFTR_EDGES_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")
    print(line)


def _run(inp, memory_format):
    import torch
    from loftr_amd.loftr import FinePreprocess
    c = inp["case"]
    t = lambda a: torch.from_numpy(np.array(a)).cuda()                           # (a copy: the shared inputs are read-only)
    cfg = {"fine_concat_coarse_feat": True, "fine_window_size": c.W, "coarse": {"d_model": c.Cc}, "fine": {"d_model": c.Cf}}
    fp = FinePreprocess(cfg).cuda().train()
    fp.load_state_dict({k: t(v) for k, v in inp["w"].items()}, strict=True)
    leaf = {k: t(inp[k]).requires_grad_(True) for k in ("feat_c0", "feat_c1")}
    leaf.update({k: t(inp[k]).contiguous(memory_format=memory_format).requires_grad_(True) for k in ("feat_f0", "feat_f1")})
    (h0, w0), (h1, w1), st = inp["hc0"], inp["hc1"], inp["stride"]
    data = {"hw0_f": (h0 * st, w0 * st), "hw0_c": (h0, w0), "hw1_c": (h1, w1), "b_ids": t(inp["b_ids"]), "i_ids": t(inp["i_ids"]), "j_ids": t(inp["j_ids"])}
    o0, o1 = fp(*(leaf[k] for k in E.LEAVES), data)
    assert o0.requires_grad and o1.requires_grad
    ((o0 * t(inp["G0"])).sum() + (o1 * t(inp["G1"])).sum()).backward()
    torch.cuda.synchronize()
    params = dict(fp.named_parameters())
    return dict(out0=o0.detach().cpu().numpy(), out1=o1.detach().cpu().numpy(), **{"grad_" + k: v.grad.cpu().numpy() for k, v in leaf.items()},
                **{E.PARAM_KEY[n]: params[n].grad.cpu().numpy() for n in E.PARAMS})


@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_fine_preprocess_bwd_vs_float64(name, layout):
    """Both outputs, the four feature gradients and the four parameter gradients against ref64.  K: see tests/_fine_bwd_cases.py."""
    import torch
    got = _run(E.inputs(name), torch.channels_last if layout == "channels_last" else torch.contiguous_format)
    r = E.reference(name)
    failures = []
    for k in E.OUTPUTS:
        assert got[k].shape == r["ref64"][k].shape and np.isfinite(got[k]).all(), (name, layout, k, "shape or not finite")
        err, noise, scale = float(np.abs(got[k].astype(np.float64) - r["ref64"][k]).max()), r["noise"][k], r["scale"][k]
        tol = E.tolerance(k, noise, scale)
        _report(f"{name:14s} {layout:13s} {k:22s} {E.GROUP[k]:6s} err {err:.3e} noise {noise:.3e} err/noise {err / noise if noise > 0 else float('inf'):6.2f} "
                f"scale {scale:.3e} err/tol {err / tol:5.2f}")
        if err > tol:
            failures.append((k, err, tol, noise, scale))
    assert not failures, (name, layout, failures)
