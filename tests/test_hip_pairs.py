"""Feature banks on the GPU (loftr_amd/pairs.py, csrc/bank.hip): the slot-indexed kernels against their stacked-map originals,
``LoFTR.match_pairs`` against ``LoFTR.forward`` on the image-level golden cases (bit for bit with the HIP backbone), the reference
goldens through a bank, the pair-list driver under a budget that forces evictions, and the guards."""
import copy
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from _cases import GOLDEN_DIR, TOL_CONF, TOL_PX, compare_to_golden

_spec = importlib.util.spec_from_file_location("make_golden_e2e", os.path.join(GOLDEN_DIR, "make_golden_e2e.py"))
E2E = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(E2E)

DEV = "cuda:0"
KEYS = ("b_ids", "i_ids", "j_ids", "m_bids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f", "conf_matrix")
INPUTS = ("image0", "image1", "mask0", "mask1", "scale0", "scale1")


def load(name):
    g = dict(np.load(os.path.join(GOLDEN_DIR, f"{name}.npz")))
    rc = json.loads(str(g["recipe"]))
    img0, img1 = E2E.images_from_golden(g)
    return rc, img0, img1, g, E2E.extras(rc, img0, img1)


def build_model(rc, thr):
    from loftr_amd import LoFTR
    cfg = E2E.e2e_cfg(thr, rc)
    model = LoFTR(copy.deepcopy(cfg)).eval()
    model.load_state_dict(E2E.e2e_state_dict(model, cfg, rc["bn_strength"], rc.get("coarse_gain", 1.0)), strict=True)
    return model.to(DEV)


def sub(g, tag):
    d = {k.split("/", 1)[1]: v for k, v in g.items() if isinstance(k, str) and k.startswith(tag + "/")}
    d.update({k: v for k, v in g.items() if k.startswith("conf_")})
    return d


def forward(model, img0, img1, extras=None):
    data = {"image0": img0, "image1": img1}
    data.update(extras or {})
    model(data)
    return data


def assert_same(fwd, got, tag):
    """match_pairs left what forward left: same keys in the same order (the batch inputs aside), same values bit for bit."""
    assert [k for k in fwd if k not in INPUTS] == [k for k in got if k not in INPUTS], tag
    for k in ("bs", "hw0_i", "hw1_i", "hw0_c", "hw1_c", "hw0_f", "hw1_f", "W"):
        assert fwd[k] == got[k], (tag, k)
    for k in KEYS + ("conf_matrix_with_bin", "gt_mask", "_match_counts", "mask0", "mask1", "scale0", "scale1"):
        assert (k in fwd) == (k in got), (tag, k)
        if k in fwd and fwd[k] is not None:
            a, b = fwd[k], got[k]
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (tag, k)


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---- 1. kernels ---------------------------------------------------------------------------------------------------------
def _fine_inputs(n, L, Cc=256, Cf=128, M=300, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    feat_c = torch.randn(2 * n, L, Cc, device=DEV, generator=g)
    ids = [torch.randint(0, hi, (M,), device=DEV, generator=g) for hi in (n, L, L)]
    w = dict(down_w=torch.randn(Cf, Cc, device=DEV, generator=g) * 0.05, down_b=torch.randn(Cf, device=DEV, generator=g),
             merge_w=torch.randn(Cf, 2 * Cf, device=DEV, generator=g) * 0.05, merge_b=torch.randn(Cf, device=DEV, generator=g))
    return feat_c[:n], feat_c[n:], ids, w


@pytest.mark.gpu
@pytest.mark.parametrize("channels_last", [True, False])
def test_pos_encode_flatten_gather_equals_the_stacked_maps(channels_last):
    from loftr_amd import ops
    g = torch.Generator(device=DEV).manual_seed(1)
    bank = torch.randn(6, 60, 80, 256, device=DEV, generator=g).permute(0, 3, 1, 2)       # [6, 256, 60, 80] channels-last view
    if not channels_last:
        bank = bank.contiguous()
    pe = torch.randn(256, 64, 96, device=DEV, generator=g)
    ids = [5, 0, 5, 2, 2]
    got = ops.pos_encode_flatten_gather(bank, ids, pe)
    want = ops.pos_encode_flatten(bank[torch.tensor(ids, device=DEV)], pe)
    assert torch.equal(got, want)
    out = torch.full((2 * len(ids), 60 * 80, 256), float("nan"), device=DEV)
    ops.pos_encode_flatten_gather(bank, ids, pe, out=out[len(ids):])
    assert torch.equal(out[len(ids):], want) and torch.isnan(out[:len(ids)]).all()


@pytest.mark.gpu
def test_fine_preprocess_gather_equals_the_stacked_maps():
    from loftr_amd import ops
    n, hc, wc = 4, 12, 16
    g = torch.Generator(device=DEV).manual_seed(2)
    bank0 = torch.randn(7, 4 * hc, 4 * wc, 128, device=DEV, generator=g).permute(0, 3, 1, 2)
    bank1 = torch.randn(3, 4 * hc, 4 * wc, 128, device=DEV, generator=g).permute(0, 3, 1, 2)
    s0, s1 = [6, 1, 6, 0], [2, 2, 0, 1]
    c0, c1, (b, i, j), w = _fine_inputs(n, hc * wc)
    got = ops.fine_preprocess_gather(bank0, s0, bank1, s1, c0, c1, b, i, j, (hc, wc), (hc, wc), 5, 4, **w)
    want = ops.fine_preprocess(bank0[torch.tensor(s0, device=DEV)], bank1[torch.tensor(s1, device=DEV)], c0, c1, b, i, j,
                               (hc, wc), (hc, wc), 5, 4, **w)
    for a, e in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, e)


@pytest.mark.gpu
def test_gather_kernels_on_a_bank_past_2_31_elements():
    """220 fine maps of a 640 x 480 image: 2.16e9 elements (8.6 GB); the used images sit in the last slots, whose offsets only a 64-bit
    product reaches.  The same memory viewed as a 128-channel coarse bank checks the position-encoding gather."""
    from loftr_amd import ops
    S, H, W, Cf = 220, 240, 320, 128
    assert S * H * W * Cf > 2 ** 31
    store = torch.empty(S, H, W, Cf, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    used = [219, 217, 218]
    for s in used:
        store[s].normal_(generator=g)
    bank = store.permute(0, 3, 1, 2)
    pe = torch.randn(Cf, H, W, device=DEV, generator=g)
    ids = [219, 217, 219]
    got = ops.pos_encode_flatten_gather(bank, ids, pe)
    assert torch.equal(got, ops.pos_encode_flatten(bank[torch.tensor(ids, device=DEV)], pe))
    del got
    n, hc, wc = 2, H // 4, W // 4
    c0, c1, (b, i, j), w = _fine_inputs(n, hc * wc, Cf=Cf, seed=4)
    s0, s1 = [219, 218], [217, 219]
    got = ops.fine_preprocess_gather(bank, s0, bank, s1, c0, c1, b, i, j, (hc, wc), (hc, wc), 5, 4, **w)
    want = ops.fine_preprocess(bank[torch.tensor(s0, device=DEV)], bank[torch.tensor(s1, device=DEV)], c0, c1, b, i, j,
                               (hc, wc), (hc, wc), 5, 4, **w)
    for a, e in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, e)
    del store, bank
    torch.cuda.empty_cache()


# ---- 2. match_pairs == forward, bit for bit ------------------------------------------------------------------------------
def _bank_of(model, images, extras, side, capacity=None, first=0):
    from loftr_amd import FeatureBank
    k = images.shape[0]
    bank = FeatureBank(model, capacity or k, tuple(images.shape[2:]))
    m, s = extras.get("mask" + side), extras.get("scale" + side)
    slots = bank.add(images, mask=m, scale=s, slots=list(range(first, first + k)))
    return bank, slots


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["e2e_batch8", "e2e_outdoor_840", "e2e_unequal", "e2e_ot", "e2e_r16_4"])
def test_match_pairs_equals_forward(name):
    rc, i0, i1, g, ex = load(name)
    img0, img1 = _cuda(i0), _cuda(i1)
    extras = {k: _cuda(v) for k, v in ex.items()}
    for thr in (0.0, 0.2):
        model = build_model(rc, thr)
        assert model.backbone_impl == "hip"
        fwd = forward(model, img0, img1, extras)
        n = img0.shape[0]
        if img0.shape == img1.shape:               # one bank holding both image sets
            bank, ids0 = _bank_of(model, img0, extras, "0", capacity=2 * n)
            ids1 = bank.add(img1, mask=extras.get("mask1"), scale=extras.get("scale1"))
            got = model.match_pairs(bank, ids0, bank, ids1)
        else:                                      # two banks of different image sizes (and capacities)
            bank0, ids0 = _bank_of(model, img0, extras, "0")
            bank1, ids1 = _bank_of(model, img1, extras, "1", capacity=n + 2, first=2)
            got = model.match_pairs(bank0, ids0, bank1, ids1)
        torch.cuda.synchronize()
        if thr == 0.0:
            assert fwd["mconf"].numel() > 50, name
        assert_same(fwd, got, (name, thr))


@pytest.mark.gpu
def test_reuse_list_in_chunks_equals_forward_on_each_chunk():
    """12 pairs over the 16 images of e2e_batch8 (repeats, a reversed pair, a self-pair), as chunks of 8 (persistent coarse transformer)
    and 4 (launches), each against forward on that chunk's stacked images."""
    from loftr_amd import FeatureBank
    rc, i0, i1, g, _ = load("e2e_batch8")
    images = torch.cat([_cuda(i0), _cuda(i1)])
    model = build_model(rc, 0.0)
    bank = FeatureBank(model, 20, tuple(images.shape[2:]))
    slots = bank.add(images, slots=list(range(4, 20)))
    pairs = np.array([[0, 8], [1, 9], [2, 10], [3, 11], [0, 12], [8, 0], [5, 5], [4, 13], [6, 14], [7, 15], [0, 9], [3, 3]])
    for rows in (range(0, 8), range(8, 12)):
        p = pairs[rows.start:rows.stop]
        fwd = forward(model, images[p[:, 0]], images[p[:, 1]])
        got = model.match_pairs(bank, [slots[a] for a in p[:, 0]], bank, [slots[b] for b in p[:, 1]])
        assert fwd["mconf"].numel() > 50
        assert_same(fwd, got, rows)


# ---- 3. the reference goldens through a bank --------------------------------------------------------------------------------
def _dist_to_ref64(d, g):
    """(max |d mconf|, max |d mkpts1_f|) of a result against the reference's float64 forward on the common matches."""
    r = sub(g, "ref64")
    key = lambda x: list(zip(np.asarray(x["b_ids"]).tolist(), np.asarray(x["i_ids"]).tolist(), np.asarray(x["j_ids"]).tolist()))
    pos = {k: n for n, k in enumerate(key(r))}
    common = [(n, pos[k]) for n, k in enumerate(key(d)) if k in pos]
    a, b = np.array([c[0] for c in common]), np.array([c[1] for c in common])
    dc = np.abs(np.asarray(d["mconf"])[a].astype(np.float64) - r["mconf"][b]).max()
    dp = np.abs(np.asarray(d["mkpts1_f"])[a].astype(np.float64) - r["mkpts1_f"][b]).max()
    return dc, dp


@pytest.mark.gpu
@pytest.mark.parametrize("name,impl", [("e2e_batch8", "hip"), ("e2e_batch", "torch")])
def test_bank_matches_the_reference_golden(name, impl):
    """The tolerance rule of test_e2e_golden.py:test_forward_from_images_matches_reference (2x the reference's own fp32-vs-fp64
    noise where that exceeds the north-star bar; 3.3x for the MIOpen backbone)."""
    from loftr_amd import FeatureBank
    rc, i0, i1, g, _ = load(name)
    model = build_model(rc, 0.0)
    model.backbone_impl = impl
    img0, img1 = _cuda(i0), _cuda(i1)
    n = img0.shape[0]
    bank = FeatureBank(model, 2 * n, tuple(img0.shape[2:]))
    ids0, ids1 = bank.add(img0), bank.add(img1)
    data = model.match_pairs(bank, ids0, bank, ids1)
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in data.items() if v is not None}
    noise_conf, noise_px = _dist_to_ref64(sub(g, "thr0"), g)
    tol_px = max(TOL_PX, (3.3 if impl == "torch" else 2.0) * noise_px)
    tol_conf = max(TOL_CONF, 2.0 * noise_conf)
    rep = compare_to_golden(out, sub(g, "thr0"), 0.0, tol_conf=tol_conf, tol_px=tol_px, max_flips=2)
    assert rep["M_out"] > 100


# ---- 4. the pair-list driver ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_match_pair_list_with_evictions_equals_forward_per_chunk():
    from loftr_amd import FeatureBank
    from loftr_amd.pairs import Extract, match_pair_list, plan_pair_list
    rc, i0, i1, g, _ = load("e2e_batch8")
    images = torch.cat([_cuda(i0), _cuda(i1)])
    images = torch.cat([images, images[:8].flip(-1)])                # 24 distinct images on 16 slots
    model = build_model(rc, 0.0)
    rng = np.random.default_rng(5)
    pairs = rng.integers(0, 24, (40, 2))
    hw = tuple(images.shape[2:])
    budget = 16 * FeatureBank.image_bytes(model, hw)
    planned = sum(len(st.images) for st in plan_pair_list(pairs, 16, 8, 16) if isinstance(st, Extract))
    assert planned > len(np.unique(pairs)) > 16                     # the budget forces evictions and re-extractions
    ran, real = [], model.backbone.forward_hip

    def spy(x, *a, **kw):
        ran.append(x.shape[0])
        return real(x, *a, **kw)
    model.backbone.forward_hip = spy
    stats, chunks = {}, []
    for rows, data in match_pair_list(model, pairs, lambda ids: {"image": images[ids]}, hw, budget_bytes=budget, stats=stats):
        chunks.append((rows, {k: data[k].clone() for k in KEYS}))
    del model.backbone.forward_hip
    assert sum(ran) == planned == stats["images_extracted"] and stats["n_slots"] == 16
    assert [r.start for r, _ in chunks] == list(range(0, 40, 8))
    for rows, got in chunks:
        p = pairs[rows.start:rows.stop]
        fwd = forward(model, images[p[:, 0]], images[p[:, 1]])
        for k in KEYS:
            assert torch.equal(fwd[k], got[k]), (rows, k)


# ---- 5. guards -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_guards():
    from loftr_amd import FeatureBank, _lib, ops
    rc, i0, i1, g, _ = load("e2e_batch")
    model = build_model(rc, 0.0)
    img = _cuda(i0)
    bank = FeatureBank(model, 4, tuple(img.shape[2:]))
    ids = bank.add(img)
    model.match_pairs(bank, ids, bank, ids)
    # out-of-range / empty slots: raised on the host before any launch
    with pytest.raises(_lib.LoftrHipError):
        model.match_pairs(bank, [0], bank, [4])
    with pytest.raises(_lib.LoftrHipError):
        model.match_pairs(bank, [0], bank, [3])
    with pytest.raises(_lib.LoftrHipError):
        ops.pos_encode_flatten_gather(bank.coarse_map(), [9], model.pos_encoding.pe[0])
    # .train()
    model.train()
    with pytest.raises(_lib.LoftrHipError):
        model.match_pairs(bank, ids, bank, ids)
    with pytest.raises(_lib.LoftrHipError):
        bank.add(img)
    model.eval()
    # weights changed after add
    with torch.no_grad():
        model.backbone.layer1[0].conv1.weight.mul_(1.0)
    with pytest.raises(_lib.LoftrHipError, match="other backbone weights"):
        model.match_pairs(bank, ids, bank, ids)
    ids = bank.add(img, slots=ids)
    model.match_pairs(bank, ids, bank, ids)
    # a bank not on the model's device
    bank.coarse, bank.fine = bank.coarse.cpu(), bank.fine.cpu()
    with pytest.raises(_lib.LoftrHipError):
        model.match_pairs(bank, ids, bank, ids)
