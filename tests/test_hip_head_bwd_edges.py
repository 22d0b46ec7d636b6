"""The backward of the two matching heads and of their losses -- loftr_dual_softmax_bwd (csrc/dual_softmax_bwd.h), loftr_sinkhorn_bwd
(csrc/sinkhorn_bwd.h), loftr_fine_match_bwd, loftr_coarse_loss_grad and loftr_fine_loss_grad (csrc/train_bwd.hip), through loftr_amd.ops,
loftr_amd.autograd and loftr_amd.training.LoFTRLoss -- against references in FLOAT64 at the sizes where their work distribution changes
path: row chunks that are empty, hold one row or end ragged, rows that are no multiple of the four waves of a block, columns on each side
of the 64-lane stride and the 256-column block, masks that end inside a chunk, leave whole units dead or leave ONE token, upstream
gradients that are dense, sparse, a loss's own or spread over six magnitudes, C != 256 (the generic score path), every variant of the
Sinkhorn iteration the backward re-runs, 0 to 3 iterations, windows of 2 x 2 to 8 x 8, channel counts that are no multiple of 64, and the
second round of the loss kernels' strided loops.  Cases, references and tolerances: tests/_head_bwd_cases.py.

Per tensor: err = max|got - ref64| <= K_ABS[group] * noise + 1e-6 * scale, and row by row (d sim, d Z, the descriptor gradients, d1)
max_j|got - ref64| / max_j|ref64| <= K_ROW[group] * (the same of the reference's float32 run) + 1e-6.  Each run prints its figures before
it asserts, and appends them to the file LOFTR_EDGES_REPORT names, if set (how profiles/head_bwd_accuracy.txt was written)."""
import os

import numpy as np
import pytest

import _head_bwd_cases as E

pytestmark = pytest.mark.gpu


def _report(line):
    path = os.environ.get("LOFTR_EDGES_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")
    print(line)


def _compare(name, got, r, exact=()):
    """Report every (tensor, check) of `got` against the reference record, then assert them all, with the exact conditions missed."""
    failures = list(exact)
    for k, v in got.items():
        assert v.shape == r["ref64"][k].shape, (name, k, v.shape)
        if not np.isfinite(v).all():
            failures.append((k, "not finite"))
    for k, check, err, noise, scale, tol in E.measure(got, r):
        ratio = err / noise if noise > 0 else (0.0 if err == 0 else float("inf"))
        _report(f"{name:22s} {k:10s} {E.GROUP[k]:5s} {check} err {err:.3e} noise {noise:.3e} err/noise {ratio:6.2f} scale {scale:.3e} "
                f"err/tol {err / tol if tol > 0 else (0.0 if err == 0 else float('inf')):5.2f}")
        if not err <= tol:
            failures.append((k, check, err, tol, noise, scale))
    assert not failures, (name, failures)


def _t(a, dev="cuda"):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)                                 # (a copy: the shared inputs are read-only)


def _masks(i):
    return (None, None) if i["v0"] is None else (_t(i["v0"]), _t(i["v1"]))


@pytest.mark.parametrize("name", [c.name for c in E.DS_CASES])
def test_dual_softmax_bwd_vs_float64(name):
    """d sim from ops.dual_softmax_bwd, the descriptor gradients through autograd.dual_softmax_match(...)["conf_matrix"].backward(G)."""
    import torch
    from loftr_amd import autograd, ops
    i = E.inputs(name)
    c, (hw0, hw1) = i["case"], i["hw"]
    m0, m1 = _masks(i)
    f0, f1, G = _t(i["f0"]), _t(i["f1"]), _t(i["G"])
    dsim = ops.dual_softmax_bwd(f0, f1, G, hw0, hw1, E.TEMPERATURE, m0, m1)
    a, b = f0.clone().requires_grad_(True), f1.clone().requires_grad_(True)
    kw = dict(thr=0.2, border_rm=0, scale=8.0, match_type="dual_softmax", temperature=E.TEMPERATURE, want_conf=True)
    if m0 is not None:
        kw.update(mask0=m0, mask1=m1)
    autograd.dual_softmax_match(a, b, hw0, hw1, **kw)["conf_matrix"].backward(G)
    torch.cuda.synchronize()
    got = dict(dsim=dsim.cpu().numpy(), feat0=a.grad.cpu().numpy(), feat1=b.grad.cpu().numpy())
    _compare(name, got, E.reference(name), E.exact_violations(c, i, got))


@pytest.mark.parametrize("name", [c.name for c in E.OT_CASES])
def test_sinkhorn_bwd_vs_float64(name):
    """d Z [N, L + 1, S + 1] and d bin_score from ops.sinkhorn_bwd, the descriptor gradients and d bin_score through
    autograd.sinkhorn_match(...)["conf_matrix_with_bin"].backward(G) (one case: feat_c0 alone requires a gradient)."""
    import torch
    from loftr_amd import autograd, ops
    i = E.inputs(name)
    c, (hw0, hw1) = i["case"], i["hw"]
    m0, m1 = _masks(i)
    f0, f1, G = _t(i["f0"]), _t(i["f1"]), _t(i["G"])
    dz, dbin = ops.sinkhorn_bwd(f0, f1, G, hw0, hw1, c.bin_score, c.iters, m0, m1)
    a, b = f0.clone().requires_grad_(True), f1.clone().requires_grad_(c.want1)
    bin_score = torch.tensor(c.bin_score, device="cuda", requires_grad=True)
    kw = dict(thr=0.2, border_rm=0, scale=8.0, match_type="sinkhorn", skh_iters=c.iters, skh_prefilter=False, want_assign=True)
    if m0 is not None:
        kw.update(mask0=m0, mask1=m1)
    autograd.sinkhorn_match(a, b, bin_score, hw0, hw1, **kw)["conf_matrix_with_bin"].backward(G)
    torch.cuda.synchronize()
    assert (b.grad is None) == (not c.want1)
    r = E.reference(name)
    got = dict(dZ=dz.cpu().numpy(), dbin=dbin.cpu().numpy().reshape(1), feat0=a.grad.cpu().numpy())
    if c.want1:
        got["feat1"] = b.grad.cpu().numpy()
    node = bin_score.grad.cpu().numpy().reshape(1)    # d bin_score once more, as the autograd node hands it to the parameter
    # d bin_score against the float64 sum of this run's own dustbin entries of d Z (every case), then everything against ref64
    exact = E.exact_violations(c, i, got)
    for tag, value in (("", got["dbin"]), (":node", node)):
        err, tol = E.dbin_self_check(got["dZ"], value)
        _report(f"{name + tag:22s} {'dbin':10s} self  abs err {err:.3e} tol {tol:.3e} err/tol {err / tol:5.2f}")
        if not err <= tol:
            exact.append(("dbin", "self" + tag, err, tol))
    _compare(name, {k: v for k, v in got.items() if k in E.outputs_of(c)}, r, exact)
    if "dbin" in E.outputs_of(c):
        _compare(name + ":node", dict(dbin=node), r)


@pytest.mark.parametrize("name", [c.name for c in E.FINE_CASES])
def test_fine_match_bwd_vs_float64(name):
    import torch
    from loftr_amd import ops
    i = E.fine_inputs(name)
    c = i["case"]
    d0, d1 = ops.fine_match_bwd(_t(i["f0"]), _t(i["f1"]), _t(i["g"]))
    torch.cuda.synchronize()
    got = dict(d0=d0.cpu().numpy(), d1=d1.cpu().numpy())
    off = np.arange(c.W * c.W) != c.W * c.W // 2
    _compare(name, got, E.fine_reference(name), ["d0 off the centre row"] if got["d0"][:, off].any() else [])


def _loss_data(i):
    c = i["case"]
    M = c.M
    ids = [np.zeros(1, np.int64)] * 3 if M == 0 else [i["b"], i["i"], i["j"]]     # (the reference's placeholder (0, 0, 0) without ground truth)
    data = dict(spv_b_ids=_t(ids[0]), spv_i_ids=_t(ids[1]), spv_j_ids=_t(ids[2]), _spv_count=M)
    if c.masked:
        data.update(mask0=_t(i["m0"]), mask1=_t(i["m1"]))
    return data


@pytest.mark.parametrize("name", [c.name for c in E.LOSS_CASES])
def test_coarse_loss_grad_vs_float64(name):
    """d loss_c / d conf of LoFTRLoss on a synthetic leaf (no head in front), all four kinds."""
    import torch
    from loftr_amd.training import LoFTRLoss
    i = E.loss_inputs(name)
    c = i["case"]
    conf = _t(i["conf"]).requires_grad_(True)
    loss = LoFTRLoss(E.loss_cfg(c.kind)).train()
    value = loss.compute_coarse_loss(conf, _loss_data(i))
    value.backward()
    torch.cuda.synchronize()
    r = E.loss_reference(name)
    # the value the gradient belongs to: float64 sums rounded once to float32 (the (0, 0, 0) placeholder's term is 2.6e-6 of the dense loss)
    got_value, want = float(value.detach()), E.loss_value(i)
    _report(f"{name:22s} loss_c     value got {got_value:.9e} ref64 {want:.9e} rel {abs(got_value - want) / max(abs(want), 1e-30):.2e}")
    assert abs(got_value - want) <= 1e-6 * abs(want), (name, got_value, want)
    got = dict(grad_conf=conf.grad.cpu().numpy())
    _compare(name, got, r, ["non-zero where ref64 is exactly 0"] if got["grad_conf"][r["ref64"]["grad_conf"] == 0].any() else [])


@pytest.mark.parametrize("name", [c.name for c in E.FINE_LOSS_CASES])
def test_fine_loss_grad_vs_float64(name):
    import torch
    from loftr_amd.training import LoFTRLoss
    i = E.fine_loss_inputs(name)
    c = i["case"]
    e = _t(i["expec_f"]).requires_grad_(True)
    loss = LoFTRLoss(E.loss_cfg(0, c.fine_type)).train()
    value = loss.compute_fine_loss(e, _t(i["gt"]))
    assert value is not None                          # (training mode: a loss even without a correct match)
    value.backward()
    torch.cuda.synchronize()
    r = E.fine_loss_reference(name)
    got = dict(grad_expec=(e.grad if e.grad is not None else torch.zeros_like(e)).cpu().numpy())
    _compare(name, got, r, ["non-zero where ref64 is exactly 0"] if got["grad_expec"][r["ref64"]["grad_expec"] == 0].any() else [])
