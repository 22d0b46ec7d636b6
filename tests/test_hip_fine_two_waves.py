"""fine_pair_kernel with eight waves per workgroup (two matches per SIMD on one weight stream, csrc/fine_fused.hip) against its
four-wave form and against the float64 restatement of tests/test_hip_fine_fused.py.  A match is computed by one wave from the
same inputs in the same order in both forms, so the outputs must agree to the bit: at match counts where the 8-match workgroup
holds a single wave with a match of its own, is one short of full, full, overflows by one, and twice that; wherever a match sits in
the batch (a wave reading its neighbour's Ksum / KV scratch would show here); and through LoFTR.forward."""
import pytest
import torch

from loftr_amd import ops
from test_hip_fine_fused import _enc64, fine  # noqa: F401  (the module's model fixture and its float64 layers)

pytestmark = pytest.mark.gpu

T, MMAX = 25, 17                                   # W = 5 windows, Cf = 128
COUNTS = [1, 7, 8, 9, 16, 17]


@pytest.fixture(scope="module")
def batch(fine):  # noqa: F811
    """17 matches, their float64 result (matches do not interact: the first M of them are the case M) and both kernels' outputs per M."""
    tf, w = fine
    g = torch.Generator(device="cpu").manual_seed(MMAX * 131 + T)
    f0 = torch.randn(MMAX, T, 128, generator=g).cuda()
    f1 = (0.6 * f0 + 0.8 * torch.randn(MMAX, T, 128, generator=g).cuda()).contiguous()
    with torch.no_grad():
        x0, x1 = f0.double(), f1.double()
        x0, x1 = _enc64(x0, x0, w, "loftr_fine.layers.0."), _enc64(x1, x1, w, "loftr_fine.layers.0.")
        x0 = _enc64(x0, x1, w, "loftr_fine.layers.1.")
        x1 = _enc64(x1, x0, w, "loftr_fine.layers.1.")
    return tf, f0, f1, x0, x1


def _run(tf, f0, f1, waves):
    with torch.no_grad(), ops.debug_switch(fine_waves=waves):
        o0, o1 = tf(f0.contiguous(), f1.contiguous())
    torch.cuda.synchronize()
    return o0, o1


def test_the_switch_exists_and_defaults_to_the_rule():
    assert ops.debug_get("fine_waves") == (0, 0)


@pytest.mark.parametrize("M", COUNTS)
def test_eight_waves_equal_four_waves_and_fp64(batch, M):
    tf, f0, f1, x0, x1 = batch
    a0, a1 = _run(tf, f0[:M], f1[:M], 4)
    b0, b1 = _run(tf, f0[:M], f1[:M], 8)
    assert torch.equal(a0, b0) and torch.equal(a1, b1)
    assert torch.isfinite(b0).all() and torch.isfinite(b1).all()
    # the bound of test_fused_fine_transformer_vs_fp64
    tol = 2e-6 * max(1.0, float(x0[:M].abs().max())) + 1e-5
    for o0, o1 in ((a0, a1), (b0, b1)):
        e0, e1 = float((o0.double() - x0[:M]).abs().max()), float((o1.double() - x1[:M]).abs().max())
        assert e0 <= tol and e1 <= tol, (M, e0, e1, tol)


@pytest.mark.parametrize("waves", [4, 8])
def test_a_match_does_not_depend_on_its_place_in_the_batch(batch, waves):
    tf, f0, f1, _, _ = batch
    o0, o1 = _run(tf, f0, f1, waves)
    perm = torch.randperm(MMAX, generator=torch.Generator(device="cpu").manual_seed(5)).cuda()
    assert not torch.equal(perm // 8, torch.arange(MMAX, device="cuda") // 8)        # matches change workgroup and wave
    p0, p1 = _run(tf, f0[perm], f1[perm], waves)
    for k in range(MMAX):
        assert torch.equal(p0[k], o0[perm[k]]) and torch.equal(p1[k], o1[perm[k]]), (waves, k, int(perm[k]))


@pytest.mark.parametrize("n", [1, 3])
def test_forward_is_bit_identical_between_four_and_eight_waves(n):
    from test_e2e_golden import build_model, load
    rc, img0, img1, _ = load("e2e_batch8")
    dev = "cuda:0"
    keys = ("b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f", "conf_matrix")
    model = build_model(rc, 0.0, dev)
    outs = {}
    for waves in (4, 8):
        with ops.debug_switch(fine_waves=waves):
            data = {"image0": torch.from_numpy(img0[:n]).to(dev), "image1": torch.from_numpy(img1[:n]).to(dev)}
            model(data)
            torch.cuda.synchronize()
        outs[waves] = {k: data[k].detach().clone() for k in keys}
    assert len(outs[4]["mconf"]) > 50 * n
    for k in keys:
        assert torch.equal(outs[4][k], outs[8][k]), k
