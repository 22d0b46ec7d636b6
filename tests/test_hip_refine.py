"""Track refinement on the GPU (csrc/refine_gpu.hip, loftr_amd/pairs.py, loftr_amd/refinement.py): the centres kernel
against the host routine, the window gather at given centres against the existing gathers (aligned: the slot-indexed twin; unaligned:
ops.fine_preprocess on a zero-padded, shifted copy of the map), ``LoFTR.refine_points`` against the forward it must reproduce, the
pair-list driver against ``refine_points`` on the planned chunks, and ``SfmResult.refine_tracks`` against the oracles.  Everything runs
on fine maps of 32 x 48 pixels (coarse 8 x 12, images 64 x 96) or a little larger."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

import _refine_cases as cases
import _refine_oracle as oracle
from _cases import GOLDEN_DIR

_spec = importlib.util.spec_from_file_location("make_golden_e2e", os.path.join(GOLDEN_DIR, "make_golden_e2e.py"))
E2E = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(E2E)

DEV = "cuda:0"
HW = (64, 96)
RECIPE = dict(bn_strength=0.3, temp_bug_fix=True)
KEYS = ("pts0", "pts1_start", "pts1", "expec_f", "ok")


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---- 1. the centres --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scales", [False, True])
def test_refine_centres_equals_the_host_routine(scales):
    from loftr_amd import ops
    pts0, pts1, b_ids = cases.centre_points()
    reps = 12                                                           # more than one block of 256 rows
    pts0, pts1, b_ids = np.tile(pts0, (reps, 1)), np.tile(pts1, (reps, 1)), np.sort(np.tile(b_ids, reps))
    sc = (cases.SCALE0, cases.SCALE1) if scales else (None, None)
    geo = (cases.N_PAIRS, cases.HW0_F, cases.HW1_F, cases.HW0_C, cases.HW1_C, cases.STRIDE, cases.S)
    host = ops.refine_centres(*(torch.from_numpy(a) for a in (pts0, pts1, b_ids)), *geo, *(None if s is None else torch.from_numpy(s) for s in sc))
    got = ops.refine_centres(_cuda(pts0), _cuda(pts1), _cuda(b_ids), *geo, *(None if s is None else _cuda(s) for s in sc))
    assert len(b_ids) > 256 and (host["ok"] == 0).any() and (host["ok"] == 1).any()
    for k, v in host.items():
        assert got[k].dtype == v.dtype and torch.equal(got[k].cpu(), v), k


# ---- 2. / 3. the window gather -----------------------------------------------------------------------------------------------------
def _fine_inputs(n, L, Cc=256, Cf=128, M=300, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    feat_c = torch.randn(2 * n, L, Cc, device=DEV, generator=g)
    ids = [torch.randint(0, hi, (M,), device=DEV, generator=g) for hi in (n, L, L)]
    w = dict(down_w=torch.randn(Cf, Cc, device=DEV, generator=g) * 0.05, down_b=torch.randn(Cf, device=DEV, generator=g),
             merge_w=torch.randn(Cf, 2 * Cf, device=DEV, generator=g) * 0.05, merge_b=torch.randn(Cf, device=DEV, generator=g))
    return feat_c[:n], feat_c[n:], ids, w


def _centres_of(cell, wc, stride, offset=(0, 0)):
    return torch.stack([(cell % wc) * stride + offset[0], (cell // wc) * stride + offset[1]], 1).to(torch.int32).contiguous()


@pytest.mark.gpu
def test_gather_at_aligned_centres_equals_the_slot_gather():
    """The inputs of test_fine_preprocess_gather_equals_the_stacked_maps: two banks of 7 and 3 slots, repeated and distinct slots."""
    from loftr_amd import ops
    n, hc, wc = 4, 12, 16
    g = torch.Generator(device=DEV).manual_seed(2)
    bank0 = torch.randn(7, 4 * hc, 4 * wc, 128, device=DEV, generator=g).permute(0, 3, 1, 2)
    bank1 = torch.randn(3, 4 * hc, 4 * wc, 128, device=DEV, generator=g).permute(0, 3, 1, 2)
    s0, s1 = [6, 1, 6, 0], [2, 2, 0, 1]
    c0, c1, (b, i, j), w = _fine_inputs(n, hc * wc)
    want = ops.fine_preprocess_gather(bank0, s0, bank1, s1, c0, c1, b, i, j, (hc, wc), (hc, wc), 5, 4, **w)
    got = ops.fine_preprocess_gather_at(bank0, s0, bank1, s1, c0, c1, b, i, j, _centres_of(i, wc, 4), _centres_of(j, wc, 4),
                                        (hc, wc), (hc, wc), 5, 4, **w)
    for a, e in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, e)


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [(1, 0), (0, 3), (2, 2), (3, 1), (0, 0), (3, 3)])
def test_gather_at_unaligned_centres_equals_the_gather_on_a_shifted_map(offset):
    """Centres stride * cell + offset for EVERY cell of the grid (all corners and edges); offset (0, 0) has the centre (0, 0) and offset
    (3, 3) the centre (extent - 1, extent - 1).  The comparison is ops.fine_preprocess on the map zero-padded by `stride` pixels on every
    side and shifted by the offset: there the same window is the aligned window of cell (cy + 1, cx + 1) of an (hc + 2) x (wc + 2)
    grid, and feat_c is scattered so that this cell holds the feature of the cell passed to gather_at.  The window radius (2) is below
    the padding (4), so the zeros outside the map agree on both sides."""
    from loftr_amd import ops
    n, hc, wc, stride, Cf = 2, 8, 12, 4, 128
    hf, wf = stride * hc, stride * wc
    g = torch.Generator(device=DEV).manual_seed(6)
    store0, store1 = (torch.randn(k, hf, wf, Cf, device=DEV, generator=g) for k in (3, 2))
    s0, s1 = [2, 0], [1, 1]
    L = hc * wc
    c0, c1, _, w = _fine_inputs(n, L, seed=7)
    cell = torch.arange(L, device=DEV)
    b = torch.repeat_interleave(torch.arange(n, device=DEV), L)
    i, j = cell.repeat(n), cell.flip(0).repeat(n)
    ox, oy = offset
    at0, at1 = _centres_of(i, wc, stride, offset), _centres_of(j, wc, stride, offset)
    assert 0 <= int(at0.min()) and int(at0[:, 0].max()) < wf and int(at0[:, 1].max()) < hf
    got = ops.fine_preprocess_gather_at(store0.permute(0, 3, 1, 2), s0, store1.permute(0, 3, 1, 2), s1, c0, c1, b, i, j, at0, at1,
                                        (hc, wc), (hc, wc), 5, stride, **w)

    def shifted(store, slots):
        big = torch.zeros(n, hf + 2 * stride, wf + 2 * stride, Cf, device=DEV)
        big[:, stride - oy:stride - oy + hf, stride - ox:stride - ox + wf] = store[torch.tensor(slots, device=DEV)]
        return big.permute(0, 3, 1, 2)

    def scattered(feat_c):
        big = torch.zeros(n, (hc + 2) * (wc + 2), feat_c.shape[2], device=DEV)
        big[:, ((cell // wc + 1) * (wc + 2) + cell % wc + 1)] = feat_c
        return big
    up = lambda ids: (ids // wc + 1) * (wc + 2) + ids % wc + 1
    want = ops.fine_preprocess(shifted(store0, s0), shifted(store1, s1), scattered(c0), scattered(c1), b, up(i), up(j),
                               (hc + 2, wc + 2), (hc + 2, wc + 2), 5, stride, **w)
    for a, e in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, e)


# ---- 4. refine_points reproduces the forward ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from loftr_amd import LoFTR
    cfg = E2E.e2e_cfg(0.0, RECIPE)
    m = LoFTR(copy.deepcopy(cfg)).eval()
    m.load_state_dict(E2E.e2e_state_dict(m, cfg, RECIPE["bn_strength"]), strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def images():
    """6 images of 64 x 96."""
    from loftr_amd.synth import make_images
    i0, i1 = make_images(1234, 3, *HW)
    return _cuda(np.concatenate([i0, i1]))


def _extras(n):
    """MegaDepth-style masks (valid rectangles of 48 x 96 and 64 x 72 pixels) and scales for n pairs."""
    m0, m1 = torch.zeros(n, 8, 12, dtype=torch.bool, device=DEV), torch.zeros(n, 8, 12, dtype=torch.bool, device=DEV)
    m0[:, :6, :], m1[:, :, :9] = True, True
    return dict(mask0=m0, mask1=m1, scale0=torch.tensor([[1.9, 1.9]] * n, device=DEV), scale1=torch.tensor([[1.25, 1.5]] * n, device=DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("n,extras", [(1, False), (3, False), (3, True)])
def test_refine_points_reproduces_the_forward(model, images, n, extras):
    """match_pairs, then refine_points at its coarse points: the same windows, the same coarse features, the same fine level.  This
    pins the scale, sign and window conventions of the new path to the forward that the goldens pin to the reference."""
    from loftr_amd import FeatureBank
    ex = _extras(n) if extras else {}
    bank = FeatureBank(model, 2 * n, HW)
    ids0 = bank.add(images[:n], mask=ex.get("mask0"), scale=ex.get("scale0"))
    ids1 = bank.add(images[3:3 + n], mask=ex.get("mask1"), scale=ex.get("scale1"))
    data = model.match_pairs(bank, ids0, bank, ids1)
    M = data["b_ids"].shape[0]
    print(f"n = {n}, extras = {extras}: {M} matches")
    assert M > 0 and data["mkpts1_c"].shape[0] == M
    got = model.refine_points(bank, ids0, bank, ids1, data["b_ids"], data["mkpts0_c"], data["mkpts1_c"])
    assert got["ok"].all()
    for k, ref in (("pts0", "mkpts0_c"), ("pts1_start", "mkpts1_c"), ("expec_f", "expec_f"), ("pts1", "mkpts1_f")):
        assert got[k].dtype == data[ref].dtype and torch.equal(got[k], data[ref]), (k, ref)
    assert torch.isfinite(got["pts1"]).all() and not torch.equal(got["pts1"], got["pts1_start"])
    # a row that is not ok is NaN and leaves the others as they were
    pts1 = data["mkpts1_c"].clone()
    pts1[0, 0] = float("nan")
    bad = model.refine_points(bank, ids0, bank, ids1, data["b_ids"], data["mkpts0_c"], pts1)
    assert bad["ok"].tolist() == [0] + [1] * (M - 1) and torch.isnan(bad["pts1"][0]).all() and torch.isnan(bad["expec_f"][0]).all()
    assert torch.equal(bad["pts1"][1:], got["pts1"][1:]) and torch.equal(bad["expec_f"][1:], got["expec_f"][1:])


# ---- 5. / 6. the driver and the tracks ------------------------------------------------------------------------------------------------
def _by_hand(model, images, pairs, pair_offsets, pts0, pts1, n_slots, batch_size):
    """refine_points on the chunks plan_pair_list yields, on a bank of its own -> the concatenated results, the extractions."""
    from loftr_amd import FeatureBank
    from loftr_amd.pairs import Extract, plan_pair_list
    bank = FeatureBank(model, n_slots, HW)
    out, extracted = [], 0
    for st in plan_pair_list(pairs, n_slots, batch_size, 16):
        if isinstance(st, Extract):
            bank.add(images[st.images], slots=st.slots)
            extracted += len(st.images)
            continue
        jobs = slice(int(pair_offsets[st.rows.start]), int(pair_offsets[st.rows.stop]))
        b_ids = np.repeat(np.arange(len(st.rows)), np.diff(pair_offsets[st.rows.start:st.rows.stop + 1]))
        out.append(model.refine_points(bank, st.slots0, bank, st.slots1, torch.from_numpy(b_ids), pts0[jobs], pts1[jobs]))
    return {k: torch.cat([o[k] for o in out]) for k in KEYS}, extracted


@pytest.mark.gpu
def test_refine_pair_list_equals_refine_points_on_the_planned_chunks(model, images):
    """5 pairs, batch_size 2 and a budget of 4 slots.  plan_pair_list needs 2 * batch_size slots, which already hold 4 images, so the
    eviction takes a fifth and a sixth image: the pairs run over 6 images."""
    from loftr_amd import FeatureBank
    from loftr_amd.pairs import refine_pair_list
    pairs = np.array([[0, 1], [2, 3], [4, 5], [1, 0], [3, 5]])
    pair_offsets = np.array([0, 7, 7, 12, 20, 23])                       # a pair without a job among them
    g = torch.Generator(device=DEV).manual_seed(8)
    pts0, pts1 = (torch.rand(23, 2, device=DEV, generator=g) * torch.tensor([95.0, 63.0], device=DEV) for _ in range(2))
    want, extracted = _by_hand(model, images, pairs, pair_offsets, pts0, pts1, 4, 2)
    assert extracted > 6                                                # the budget forced an eviction and a second extraction
    stats, slices, got = {}, [], []
    for jobs, res in refine_pair_list(model, pairs, pair_offsets, pts0, pts1, lambda ids: {"image": images[ids]}, HW,
                                      budget_bytes=4 * FeatureBank.image_bytes(model, HW), batch_size=2, stats=stats):
        slices.append((jobs.start, jobs.stop))
        got.append(res)
    assert slices == [(0, 7), (7, 20), (20, 23)] and stats["n_slots"] == 4 and stats["images_extracted"] == extracted
    for k in KEYS:
        assert torch.equal(torch.cat([r[k] for r in got]), want[k]), k
    assert want["ok"].all() and torch.isfinite(want["pts1"]).all()


@pytest.mark.gpu
def test_refine_tracks_end_to_end(model, images):
    from loftr_amd import FeatureBank
    sfm = cases.build_sfm(cases.SCENE4, device=DEV, image_hw=HW)
    load = lambda ids: {"image": images[ids]}
    kw = dict(max_std=0.5, max_shift_px=6.0)
    view, ref = sfm.refine_tracks(model, load, batch_size=2, budget_bytes=4 * FeatureBank.image_bytes(model, HW), **kw)
    host = sfm.to_host()
    plan = oracle.plan(host)
    for k in ("pairs", "pair_offsets", "job_ref_kp", "job_query_kp", "job_track"):
        assert np.array_equal(getattr(ref.plan, k).cpu().numpy(), plan[k]), k
    res, _ = _by_hand(model, images, plan["pairs"], plan["pair_offsets"], sfm.keypoints[_cuda(plan["job_ref_kp"])],
                      sfm.keypoints[_cuda(plan["job_query_kp"])], 4, 2)
    res = {k: v.cpu().numpy() for k, v in res.items()}
    want_kp, want_state, accepted = oracle.apply(host["keypoints"], plan["job_ref_kp"], plan["job_query_kp"], res, HW, kw["max_std"],
                                                 kw["max_shift_px"])
    print("states:", np.bincount(want_state, minlength=5).tolist(), "std:", res["expec_f"][:, 2].round(3).tolist())
    assert np.array_equal(view.keypoints.cpu().numpy().view(np.int32), want_kp.view(np.int32))
    assert np.array_equal(ref.kp_state.cpu().numpy(), want_state) and np.array_equal(ref.job_std.cpu().numpy(), res["expec_f"][:, 2])
    for s, name in enumerate(("n_untouched", "n_ref_moved", "n_query_accepted", "n_query_rejected", "n_ref_kept")):
        assert ref.stats[name] == int((want_state == s).sum()), name
    assert ref.stats["n_jobs"] == plan["stats"]["n_jobs"] == len(accepted) and ref.stats["n_untouched"] > 0
    assert 0 < accepted.sum() < len(accepted)                            # queries are accepted and queries are rejected
    outside = ref.kp_state == 0                                          # a keypoint outside every job keeps its bits
    assert torch.equal(view.keypoints[outside], sfm.keypoints[outside])
    assert view.is_refined and view.track_id is sfm.track_id
    K = torch.tensor([[80.0, 0, 48], [0, 80.0, 32], [0, 0, 1]], dtype=torch.float64).repeat(4, 1, 1)
    T = torch.eye(4, dtype=torch.float64).repeat(4, 1, 1)
    T[:, 0, 3] = torch.arange(4, dtype=torch.float64) * 0.1
    pts = view.triangulate(K, T)
    assert pts.xyz.shape[0] == int(sfm.track_ok.sum())
