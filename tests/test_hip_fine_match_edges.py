"""Fine matching (fine_match_kernel of csrc/fine.hip through ops.fine_match) against the numpy oracle in FLOAT64 at every window size
it accepts, at channel counts that leave its 64-lane channel loop uneven, with 1 .. 3 matches in the last workgroup, in every regime
of its softmax (flat, moderate, peaked, saturated, peak in a window corner, large equal scores) and with per-pair scales gathered
through unsorted b_ids.  Cases, reference, bounds and the conditions the inputs meet: tests/_fine_match_cases.py.  Its backward is held
to float64 by tests/test_hip_head_bwd_edges.py; the goldens reach the forward at W = 5, C = 128 only.
Each case prints its figures before it asserts and appends them to the file LOFTR_EDGES_REPORT names, if set (how
profiles/select_fine_match_accuracy.txt was written)."""
import os

import numpy as np
import pytest

import _fine_match_cases as F

pytestmark = pytest.mark.gpu


def _report(line):
    path = os.environ.get("LOFTR_EDGES_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")
    print(line)


def _ratio(err, noise):
    return err / noise if noise > 0 else (0.0 if err == 0 else float("inf"))


@pytest.mark.parametrize("name", [c.name for c in F.CASES])
def test_fine_match_vs_float64(name):
    import torch
    from loftr_amd import ops
    i, r = F.inputs(name), F.reference(name)
    c = i["case"]
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared inputs are read-only)
    args = dict(f0=t(i["f0"]), f1=t(i["f1"]), mk=t(i["mkpts1_c"]), b=t(i["b_ids"]), s1=t(i["scale1"]))
    before = {k: v.clone() for k, v in args.items() if v is not None}
    expec, mk1 = ops.fine_match(args["f0"], args["f1"], args["mk"], args["b"], c.scale, scale1=args["s1"])
    torch.cuda.synchronize()
    assert expec.dtype == torch.float32 and mk1.dtype == torch.float32 and tuple(expec.shape) == (c.M, 3) and tuple(mk1.shape) == (c.M, 2)
    fig, bad = F.check(name, expec.cpu().numpy(), mk1.cpu().numpy())
    for g, (err, noise, bound) in fig.items():
        kind = "" if g != "std" else (" conditioned" if r["conditioned"] else " loose")
        _report(f"fine   {name:30s} {g:3s} err {err:.3e} noise {noise:.3e} err/noise {_ratio(err, noise):6.2f} bound {bound:.3e}{kind}")
    for k, v in before.items():
        assert torch.equal(args[k], v), (name, k, "an input was written to")
    assert not bad, (name, bad)
