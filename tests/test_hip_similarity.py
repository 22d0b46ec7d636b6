"""Batched 3D similarity RANSAC on the GPU (csrc/similarity_gpu.hip: ops.estimate_similarities, ops.transform_model;
loftr_amd.alignment; evaluation.register_depth): for every problem of a batch, the result of the host estimator
loftr_estimate_similarity (evaluation.estimate_similarity_native) with the same seed -- same n_inliers, same inlier mask, and the
float64 BITS of s, R and t.  The host estimator is the reference here (tests/test_similarity.py checks it against a numpy oracle)."""
import copy

import numpy as np
import pytest
import torch

import _similarity_cases as SC
import _similarity_oracle as O
from loftr_amd import _lib, alignment, evaluation as EV, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR, CONF = SC.THR, SC.CONF


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


@pytest.fixture(scope="module")
def grid():
    """Per mode: tags, problems and the host estimator's results for the two seeds (computed once, never modified)."""
    out = {}
    for with_scale in (True, False):
        tags, probs = SC.problems(with_scale)
        host = {seed: [EV.estimate_similarity_native(a, b, with_scale, THR, CONF, seed) for a, b in probs] for seed in (0, 11)}
        out[with_scale] = (tags, probs, host)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_equal_to_host(bids, host, got):
    s, R, t, inl, n = (x.cpu().numpy() for x in got)
    assert s.dtype == R.dtype == t.dtype == np.float64
    for b, ref in enumerate(host):
        mask = inl[bids == b]
        if ref is None:
            assert n[b] == -1 and not mask.any() and not R[b].any() and not t[b].any() and s[b] == 0, (b, n[b])
            continue
        assert n[b] == ref[3].sum(), (b, n[b], ref[3].sum())
        assert np.array_equal(mask, ref[3]), (b, np.flatnonzero(mask != ref[3])[:10])
        assert np.array_equal(_bits(s[b]), _bits(ref[0])), (b, s[b], ref[0])
        assert np.array_equal(_bits(R[b]), _bits(ref[1])), (b, np.abs(R[b] - ref[1]).max())
        assert np.array_equal(_bits(t[b]), _bits(ref[2])), (b, np.abs(t[b] - ref[2]).max())


@pytest.mark.parametrize("with_scale", [True, False])
@pytest.mark.parametrize("seed", [0, 11])
def test_identical_to_the_host_estimator_on_a_ragged_batch(grid, seed, with_scale):
    """The batch of tests/_similarity_cases.py problems(): its docstring says why each problem is there."""
    tags, probs, host = grid[with_scale]
    assert 5500 <= sum(len(p[0]) for p in probs) <= 7000
    src, dst, bids = SC.batch(probs)
    got = ops.estimate_similarities(*_dev((src, dst, bids)), len(probs), with_scale, THR, CONF, seed)
    _assert_equal_to_host(bids, host[seed], got)
    # the batch holds what it claims to hold (properties of the host results, the reference of this test)
    ref = dict(zip(tags, host[seed]))
    for tag in ("m0", "m2", "empty", "collinear"):
        assert ref[tag] is None, tag
    assert ref["m3"][3].sum() == 3 and ref["m4"][3].sum() >= 3
    # 0.9^3 -> log(1e-3) / log(1 - 0.729) <= 6 iterations; 0.16^3 -> 1 683 > the cap of 1 000
    assert ref["early"][3].mean() >= 0.9 and 0.1 <= ref["capped"][3].mean() <= 0.16
    assert ref["coplanar"][3].mean() >= 0.65 and ref["m1300"][3].sum() == 780 and ref["m1100"][3].sum() >= 600
    assert ref["noise"] is None or ref["noise"][3].sum() < 10                         # (three random pairs are no similar triangles)
    a, b = probs[tags.index("adoption")]
    fit = O.umeyama(a, b, with_scale)
    assert ref["adoption"][3].all() and (O.residual(*fit, a, b) <= THR).sum() < len(a)     # the fit over all loses inliers
    if not with_scale:
        assert all(r is None or r[0] == 1.0 for r in host[seed])


def test_repeat_calls_poisoned_memory_and_untouched_inputs(grid):
    from conftest import poison_gpu_memory
    tags, probs, host = grid[True]
    t = _dev(SC.batch(probs))
    P, M = len(probs), t[0].shape[0]
    before = [x.clone() for x in t]
    a = ops.estimate_similarities(*t, P, True, THR, CONF, 11)
    b = ops.estimate_similarities(*t, P, True, THR, CONF, 11)
    poison_gpu_memory(big_gib=1, small_blocks=256)
    c = ops.estimate_similarities(*t, P, True, THR, CONF, 11)
    f32 = ops.estimate_similarities(t[0].float(), t[1].float(), t[2], P, True, THR, CONF, 11)      # f32 inputs are widened
    assert f32[0].dtype == torch.float64
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    for x, y in zip(t, before):
        assert torch.equal(x, y)
    assert a[0].shape == (P,) and a[1].shape == (P, 3, 3) and a[2].shape == (P, 3) and all(x.dtype == torch.float64 for x in a[:3])
    assert a[3].dtype == torch.bool and a[3].shape == (M,) and a[4].dtype == torch.int64 and a[4].shape == (P,)
    # the same workspace twice, poisoned in between, through the raw entry point
    lib = _lib.load()
    ws = torch.full((lib.loftr_estimate_similarity_batched_workspace_bytes(M, P),), 0xFF, dtype=torch.uint8, device=DEV)
    outs = []
    for k in range(2):
        s, R, tt = (torch.full(sh, float("nan"), dtype=torch.float64, device=DEV) for sh in ((P,), (P, 9), (P, 3)))
        inl, n = torch.full((M,), 0xFF, dtype=torch.uint8, device=DEV), torch.full((P,), -7, dtype=torch.int64, device=DEV)
        st = lib.loftr_estimate_similarity_batched(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), M, P, 1, THR, CONF, 11, s.data_ptr(),
                                                   R.data_ptr(), tt.data_ptr(), inl.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   torch.cuda.current_stream().cuda_stream)
        assert st == 0
        outs.append((s, R.reshape(P, 3, 3), tt, inl.view(torch.bool), n))
        if k == 0:
            ws.fill_(0x7F)
    for x, y, z in zip(a, outs[0], outs[1]):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_refusals_leave_the_outputs_unwritten(grid):
    tags, probs, host = grid[True]
    t = _dev(SC.batch(probs[6:9]))
    M, P = t[0].shape[0], 3
    lib = _lib.load()
    ws = torch.empty(lib.loftr_estimate_similarity_batched_workspace_bytes(M, P), dtype=torch.uint8, device=DEV)

    def raw(bids=None, ws_bytes=None):
        s, R, tt = (torch.full(sh, 7.0, dtype=torch.float64, device=DEV) for sh in ((P,), (P, 9), (P, 3)))
        inl, n = torch.full((M,), 7, dtype=torch.uint8, device=DEV), torch.full((P,), 7, dtype=torch.int64, device=DEV)
        st = lib.loftr_estimate_similarity_batched(t[0].data_ptr(), t[1].data_ptr(), (t[2] if bids is None else bids).data_ptr(), M, P, 1, THR, CONF,
                                                   0, s.data_ptr(), R.data_ptr(), tt.data_ptr(), inl.data_ptr(), n.data_ptr(), ws.data_ptr(),
                                                   ws.numel() if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return st, bool((s == 7).all() and (R == 7).all() and (tt == 7).all() and (inl == 7).all() and (n == 7).all())

    assert raw(bids=t[2].flip(0).contiguous()) == (-1, True)                          # not grouped by ascending problem
    bad = t[2].clone(); bad[-1] = P
    assert raw(bids=bad) == (-1, True)                                                # id >= P
    bad = t[2].clone(); bad[0] = -1
    assert raw(bids=bad) == (-1, True)
    assert raw(ws_bytes=ws.numel() - 1) == (-3, True)                                 # short workspace
    st, untouched = raw()
    assert st == 0 and not untouched
    call = lambda *a: ops.estimate_similarities(*a, True, THR, CONF)
    with pytest.raises(_lib.LoftrHipError):
        call(t[0].cpu(), t[1], t[2], P)
    with pytest.raises(_lib.LoftrHipError):
        call(t[0], t[1], t[2].flip(0), P)
    with pytest.raises(_lib.LoftrHipError):
        call(t[0], t[1], t[2], 2)                                                     # problem ids beyond P
    with pytest.raises(_lib.LoftrHipError):
        call(t[0], t[1][:-1], t[2], P)
    got = call(*t, P)                                                                 # still fine after the refusals
    _assert_equal_to_host(t[2].cpu().numpy(), host[0][6:9], got)


def test_empty_batch_and_no_correspondences():
    z3, b = torch.zeros(0, 3, dtype=torch.float64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV)
    s, R, t, inl, n = ops.estimate_similarities(z3, z3, b, 3)
    assert n.tolist() == [-1, -1, -1] and inl.shape == (0,) and not R.any() and not t.any() and not s.any()
    s, R, t, inl, n = ops.estimate_similarities(z3, z3, b, 0)
    assert s.shape == (0,) and R.shape == (0, 3, 3) and t.shape == (0, 3) and n.shape == (0,)


def test_per_problem_form_matches_the_host_estimator(grid):
    tags, probs, host = grid[True]
    for tag in ("m2", "m4", "m257", "collinear"):
        a, b = probs[tags.index(tag)]
        ref, got = EV.estimate_similarity_native(a, b, True, THR, CONF, 4), EV.estimate_similarity_native_gpu(a, b, True, THR, CONF, 4)
        assert (ref is None) == (got is None), tag
        if ref is not None:
            assert ref[0] == got[0] and all(np.array_equal(x, y) for x, y in zip(ref[1:], got[1:])), tag


# ---- moving a model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_transform_model_equals_the_host_routine(N, n):
    """N around the 256-thread block, n = 65 beyond a wave; every third image unposed with NaN rows, NaN points; out of place and in
    place."""
    case = [torch.from_numpy(np.ascontiguousarray(a)) for a in SC.model_case(N, n)]
    want_xyz, want_T = ops.transform_model(*case)
    dev = [a.to(DEV) for a in case]
    keep = [a.clone() for a in dev]
    got_xyz, got_T = ops.transform_model(*dev)
    same = lambda a, b: a.cpu().numpy().tobytes() == b.numpy().tobytes()              # bits, NaN included
    assert got_xyz.is_cuda and got_T.is_cuda and same(got_xyz, want_xyz) and same(got_T, want_T)
    assert all(same(a, b.cpu()) for a, b in zip(dev, keep))                           # inputs untouched
    a, b = ops.transform_model(*dev, out_xyz=dev[0], out_T=dev[1])                    # in place
    assert a is dev[0] and b is dev[1] and same(a, want_xyz) and same(b, want_T)
    e = ops.transform_model(dev[0][:0], dev[1][:0], dev[2][:0], *dev[3:])
    assert e[0].shape == (0, 3) and e[1].shape == (0, 4, 4)


# ---- alignment --------------------------------------------------------------------------------------------------------------------
def test_align_equals_the_cpu_chain():
    """The CPU test's scene (scene_b reconstructed on the CPU -- tests/test_hip_registration.py pins the GPU reconstruction to those
    bits -- with its tensors moved to the device): align_centres and Reconstruction.align, GPU against CPU."""
    s, rec, al_sc = SC.alignment_case()
    ref, known = torch.from_numpy(al_sc["ref"]), torch.from_numpy(al_sc["known"])
    rec_g = copy.copy(rec)
    rec_g.T_cam_from_world, rec_g.posed = rec.T_cam_from_world.to(DEV), rec.posed.to(DEV)
    rec_g.points = copy.copy(rec.points)
    rec_g.points.xyz = rec.points.xyz.to(DEV)
    same = lambda a, b: a.cpu().numpy().tobytes() == b.numpy().tobytes()
    for thresh, with_scale in ((SC.ALIGN_THR, True), (float("inf"), True), (SC.ALIGN_THR, False)):
        want = alignment.align_centres(rec.T_cam_from_world, rec.posed, ref, known, thresh, with_scale)
        got = alignment.align_centres(rec_g.T_cam_from_world, rec_g.posed, ref.to(DEV), known.to(DEV), thresh, with_scale)
        for k in ("s", "R", "t", "inliers", "n_inliers"):
            assert getattr(got, k).is_cuda and torch.equal(getattr(got, k).cpu(), getattr(want, k)), (thresh, with_scale, k)
        # rms is a sum in torch's order: not pinned to the bit; NaN on both sides without a model (the rigid fit: the frames differ in scale)
        assert got.rms.is_cuda and (np.isnan(float(want.rms)) == np.isnan(float(got.rms)) == (int(want.n_inliers) < 0))
        assert int(want.n_inliers) < 0 or abs(float(got.rms) - float(want.rms)) <= 1e-12
    assert int(want.n_inliers) == -1                                                  # the last case is the one without a model
    want2, want_al = rec.align(ref, known, thresh=SC.ALIGN_THR)
    got2, got_al = rec_g.align(ref.to(DEV), known.to(DEV), thresh=SC.ALIGN_THR)
    assert int(want_al.n_inliers) == 8 and torch.equal(got_al.inliers.cpu(), want_al.inliers)
    assert got2.T_cam_from_world.is_cuda and same(got2.T_cam_from_world, want2.T_cam_from_world) and same(got2.points.xyz, want2.points.xyz)
    # fewer than three known images: no model on either side, the reconstruction itself comes back
    two = torch.zeros(12, dtype=torch.bool)
    two[[1, 4]] = True
    none_g, al_g = rec_g.align(ref.to(DEV), two.to(DEV), thresh=SC.ALIGN_THR)
    assert none_g is rec_g and int(al_g.n_inliers) == -1 and not al_g.inliers.any() and not al_g.R.any()


# ---- register_depth ---------------------------------------------------------------------------------------------------------------
def _forward():
    from test_e2e_golden import _bench_data, build_model, load
    rc, img0, img1, g = load("e2e_batch")
    net = build_model(rc, 0.0, DEV)
    data = _bench_data(g, img0, img1, DEV)
    net(data)
    return data, img0


def _assert_register_depth_equals_host(data, N):
    bids = data["m_bids"].cpu().numpy()
    x0, v0 = ops.lift_keypoints(data["mkpts0_f"], data["m_bids"], data["depth0"], data["K0"])
    x1, v1 = ops.lift_keypoints(data["mkpts1_f"], data["m_bids"], data["depth1"], data["K1"])
    valid = (v0 & v1).cpu().numpy()
    x0, x1 = x0.cpu().numpy(), x1.cpu().numpy()
    assert data["n_lifted"].tolist() == [int(valid[bids == b].sum()) for b in range(N)]
    inl = data["inliers"].cpu().numpy()
    assert not inl[~valid].any()
    R, t, n = data["R_3d"].cpu().numpy(), data["t_3d"].cpu().numpy(), data["n_inliers"].cpu().numpy()
    for b in range(N):
        sel = valid & (bids == b)
        ref = EV.estimate_similarity_native(x0[sel], x1[sel], False, THR, CONF, 0)
        if ref is None:
            assert n[b] == -1 and not inl[sel].any() and not R[b].any() and not t[b].any()
            continue
        assert ref[0] == 1.0 and n[b] == ref[3].sum() and np.array_equal(inl[sel], ref[3])
        assert np.array_equal(R[b], ref[1].astype(np.float32)) and np.array_equal(t[b], ref[2].astype(np.float32))     # bits after the f32 cast
    return valid


def test_register_depth_on_a_real_forward():
    """evaluation.register_depth on the output of the forward over the 3-pair golden case.

    (a) The batch as tests/test_hip_absolute_pose.py builds it, with the synthetic depth map (and its zero block) on both sides: keys,
    shapes, dtypes, n_lifted, dropped matches are never inliers, and per pair the host estimator's result on that pair's lifted, valid
    correspondences, bit for bit after the f32 cast.
    (b) Ground truth.  The golden forward runs random weights on synthetic images: its matches obey no camera geometry, so the batch has
    no true pose to compare with.  The test gives it one: the forward's own mkpts0_f and m_bids are kept, the scene is a plane seen by
    camera 0, each pair gets a true rigid motion T_0to1, both depth maps are that plane's exact depth per pixel, and 70 % of the
    keypoints in image 1 become the projections of the moved points plus 0.5 px noise (the others keep the forward's own mkpts1_f:
    outliers).  On this batch register_depth equals the host estimator as in (a), and its largest rotation error and largest centre
    error against T_0to1 over the batch's pairs are at most those of evaluation.localize (defaults: 3 px) on the same batch.  Both
    estimators see the same pixel noise; the 3D-3D fit also sees image 1's depth, which is why it is expected to be no worse."""
    data, img0 = _forward()
    N, M = img0.shape[0], data["mkpts0_f"].shape[0]
    H, W = img0.shape[2:]
    assert M > 100
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.stack([3 + 0.004 * xx + 0.003 * yy + 0.5 * b for b in range(N)]).astype(np.float32)
    depth[:, H // 4:H // 2, W // 4:W // 2] = 0.0
    K0 = np.stack([np.array([[500.0 + 10 * b, 0, W / 2], [0, 505.0, H / 2 - b], [0, 0, 1]], np.float32) for b in range(N)])
    K1 = K0[::-1].copy()
    data.update(depth0=torch.from_numpy(depth).to(DEV), depth1=torch.from_numpy(depth[::-1].copy()).to(DEV), K0=torch.from_numpy(K0).to(DEV),
                K1=torch.from_numpy(K1).to(DEV))
    before = {k: data[k].clone() for k in ("mkpts0_f", "mkpts1_f", "m_bids")}
    assert EV.register_depth(data) is data
    assert data["R_3d"].shape == (N, 3, 3) and data["R_3d"].dtype == torch.float32 and data["R_3d"].is_cuda
    assert data["t_3d"].shape == (N, 3) and data["t_3d"].dtype == torch.float32
    assert data["inliers"].shape == (M,) and data["inliers"].dtype == torch.bool
    assert data["n_inliers"].shape == (N,) and data["n_inliers"].dtype == torch.int64
    assert data["n_lifted"].shape == (N,) and data["n_lifted"].dtype == torch.int64
    for k, v in before.items():
        assert torch.equal(data[k], v)
    valid = _assert_register_depth_equals_host(data, N)
    assert 0 < valid.sum() < M                                                        # some matches fall into a zero block
    # (b) a planar scene with a true motion per pair
    rng = np.random.default_rng(77)
    bids = data["m_bids"].cpu().numpy()
    k0 = data["mkpts0_f"].cpu().numpy().astype(np.float64)
    k1 = data["mkpts1_f"].cpu().numpy().astype(np.float64)
    K0d, K1d = K0.astype(np.float64), K1.astype(np.float64)
    nrm, dist = np.array([0.15, -0.1, 1.0]), 4.0                                       # the plane nrm . X = dist in camera 0
    pix = np.stack([xx, yy, np.ones_like(xx)], -1).reshape(-1, 3).astype(np.float64)
    d0, d1, T_gt = [], [], []
    for b in range(N):
        R = O.rot(rng.standard_normal(3), np.radians(rng.uniform(5, 15)))
        t = rng.uniform(-0.4, 0.4, 3)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        T_gt.append(T)
        n1, dist1 = R @ nrm, dist + (R @ nrm) @ t                                      # the same plane in camera 1
        d0.append((dist / (pix @ np.linalg.inv(K0d[b]).T @ nrm)).reshape(H, W))
        d1.append((dist1 / (pix @ np.linalg.inv(K1d[b]).T @ n1)).reshape(H, W))
        sel = np.flatnonzero(bids == b)
        z = dist / (np.c_[k0[sel], np.ones(len(sel))] @ np.linalg.inv(K0d[b]).T @ nrm)
        X1 = (np.c_[k0[sel], np.ones(len(sel))] @ np.linalg.inv(K0d[b]).T * z[:, None]) @ R.T + t
        p = X1 @ K1d[b].T
        p = p[:, :2] / p[:, 2:] + 0.5 * rng.standard_normal((len(sel), 2))
        good = rng.random(len(sel)) < 0.7
        k1[sel[good]] = p[good]
    assert min(np.min(d0), np.min(d1)) > 1.0                                           # the plane is in front of both cameras everywhere
    geo = {"bs": N, "m_bids": data["m_bids"], "mkpts0_f": data["mkpts0_f"], "mkpts1_f": torch.from_numpy(k1.astype(np.float32)).to(DEV),
           "depth0": torch.from_numpy(np.stack(d0).astype(np.float32)).to(DEV), "depth1": torch.from_numpy(np.stack(d1).astype(np.float32)).to(DEV),
           "K0": data["K0"], "K1": data["K1"]}
    loc = EV.localize(dict(geo))
    EV.register_depth(geo)
    _assert_register_depth_equals_host(geo, N)
    e3d, epnp = [], []
    for b in range(N):
        assert int(geo["n_inliers"][b]) >= 3 and int(loc["n_inliers"][b]) >= 3, b
        e3d.append(EV.absolute_pose_error(T_gt[b], geo["R_3d"][b], geo["t_3d"][b]))
        epnp.append(EV.absolute_pose_error(T_gt[b], loc["R_abs"][b], loc["t_abs"][b]))
        print(f"pair {b}: register_depth {e3d[b][0]:.5f} deg, {e3d[b][1]:.6f}; localize {epnp[b][0]:.5f} deg, {epnp[b][1]:.6f}; "
              f"inliers {int(geo['n_inliers'][b])} / {int(loc['n_inliers'][b])} of {(bids == b).sum()}, lifted {int(geo['n_lifted'][b])}")
    for k in (0, 1):
        assert max(e[k] for e in e3d) <= max(e[k] for e in epnp), (k, e3d, epnp)
