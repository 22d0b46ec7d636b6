"""Batched absolute pose on the GPU (csrc/absolute_pose_gpu.hip: ops.estimate_absolute_poses, ops.lift_keypoints; evaluation.localize):
for every pair of a batch, the result of the host estimator loftr_estimate_absolute_pose (evaluation.estimate_absolute_pose_native)
with the same seed -- same n_inliers, same inlier mask, R and t equal after the float32 rounding.  The host estimator is the reference
here (tests/test_absolute_pose.py checks it against a numpy oracle); parity against OpenCV's solvePnPRansac stays unpinned."""
import os

import numpy as np
import pytest
import torch

from loftr_amd import _lib, evaluation as EV, ops
import _absolute_pose_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR, CONF = 3.0, 0.999
K_SKEW = np.array([[540.0, 1.5, 310.0], [0, 515.0, 250.0], [0, 0, 1]])


def _pairs():
    """A ragged batch of about 6 000 matches: the smallest shapes at which each stage can go wrong.  257 and 513 cross the 256-wide
    strided sums of the refit and the scorer's 512-match LDS tile; 3 is the sample size and 4 the refit's minimum."""
    rng = np.random.default_rng(2026)
    tags, pairs = [], []

    def add(tag, sc):
        tags.append(tag)
        pairs.append((sc["X"], sc["kpts"], np.asarray(sc["K"], np.float32)))
    add("m0", O.make_scene(rng, 0))
    add("m2", O.make_scene(rng, 2))
    add("m3", O.make_scene(rng, 3))
    add("m4", O.make_scene(rng, 4, 0.3))
    add("m257", O.make_scene(rng, 257, 0.5, 0.3, K=K_SKEW))
    add("empty", O.make_scene(rng, 0))                                                # an empty pair between two non-empty ones
    add("m513", O.make_scene(rng, 513, 0.5, 0.3))
    add("early", O.make_scene(rng, 700, 0.3, 0.05))                                   # stops after a few iterations
    add("capped", O.make_scene(rng, 1500, 0.5, 0.85))                                 # runs all 1000
    add("collinear", O.make_collinear_scene())
    add("planar", O.make_scene(rng, 300, 0.5, 0.3, planar=True, K=K_SKEW))
    add("adoption", O.make_adoption_scene(rng, THR))                                  # refit rejected by the adoption rule
    add("m1100", O.make_scene(rng, 1100, 0.5, 0.4))
    add("noise", dict(X=np.c_[rng.uniform(-3, 3, 300), rng.uniform(-2, 2, 300), rng.uniform(2, 8, 300)].astype(np.float32),
                      kpts=np.c_[rng.uniform(0, 640, 300), rng.uniform(0, 480, 300)].astype(np.float32), K=O.K_DEFAULT))
    add("m1300", O.make_scene(rng, 1300, 0.0, 0.4))
    return tags, pairs


def _batch(pairs):
    return (np.concatenate([p[0] for p in pairs]).reshape(-1, 3), np.concatenate([p[1] for p in pairs]).reshape(-1, 2),
            np.concatenate([np.full(len(p[0]), b, np.int64) for b, p in enumerate(pairs)]), np.stack([p[2] for p in pairs]))


def _dev(batch):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in batch]


@pytest.fixture(scope="module")
def grid():
    """Tags, pairs and the host estimator's results for the two seeds (computed once, never modified)."""
    tags, pairs = _pairs()
    host = {seed: [EV.estimate_absolute_pose_native(X, k, K, THR, CONF, seed) for X, k, K in pairs] for seed in (0, 11)}
    return tags, pairs, host


def _assert_equal_to_host(bids, host, got):
    R, t, inl, n = (x.cpu().numpy() for x in got)
    for b, ref in enumerate(host):
        mask = inl[bids == b]
        if ref is None:
            assert n[b] == -1 and not mask.any() and not R[b].any() and not t[b].any(), (b, n[b])
            continue
        assert n[b] == ref[2].sum(), (b, n[b], ref[2].sum())
        assert np.array_equal(mask, ref[2]), (b, np.flatnonzero(mask != ref[2])[:10])
        assert np.array_equal(R[b], ref[0].astype(np.float32)), (b, np.abs(R[b] - ref[0]).max())
        assert np.array_equal(t[b], ref[1].astype(np.float32)), (b, np.abs(t[b] - ref[1]).max())


@pytest.mark.parametrize("seed", [0, 11])
def test_identical_to_the_host_estimator_on_a_ragged_batch(grid, seed):
    tags, pairs, host = grid
    assert 5500 <= sum(len(p[0]) for p in pairs) <= 7000
    batch = _batch(pairs)
    got = ops.estimate_absolute_poses(*_dev(batch), THR, CONF, seed)
    _assert_equal_to_host(batch[2], host[seed], got)
    # the batch holds what it claims to hold (properties of the host results, the reference of this test)
    ref = dict(zip(tags, host[seed]))
    for tag in ("m0", "m2", "empty", "collinear"):
        assert ref[tag] is None, tag
    assert ref["m3"][2].sum() == 3 and ref["m4"][2].sum() >= 3
    # 0.9^3 -> log(1e-3) / log(1 - 0.729) <= 6 iterations; 0.16^3 -> 1 683 > the cap of 1 000
    assert ref["early"][2].mean() >= 0.9 and 0.1 <= ref["capped"][2].mean() <= 0.16
    assert ref["planar"][2].mean() >= 0.65 and ref["m1300"][2].sum() == 780 and ref["noise"][2].sum() < 30
    X, k, K = pairs[tags.index("adoption")]
    Ro, to = O.fit_pose(K, X, k, ref["adoption"][0], ref["adoption"][1])
    assert ref["adoption"][2].all() and (O.residual(K, Ro, to, X, k) <= THR).sum() < len(X)       # the fit over all loses inliers


def test_repeat_calls_poisoned_memory_and_untouched_inputs(grid):
    from conftest import poison_gpu_memory
    tags, pairs, host = grid
    t = _dev(_batch(pairs))
    before = [x.clone() for x in t]
    a = ops.estimate_absolute_poses(*t, THR, CONF, 11)
    b = ops.estimate_absolute_poses(*t, THR, CONF, 11)
    poison_gpu_memory(big_gib=1, small_blocks=256)
    c = ops.estimate_absolute_poses(*t, THR, CONF, 11)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    for x, y in zip(t, before):
        assert torch.equal(x, y)
    P, M = len(pairs), t[0].shape[0]
    assert a[0].shape == (P, 3, 3) and a[0].dtype == torch.float32 and a[1].shape == (P, 3) and a[1].dtype == torch.float32
    assert a[2].dtype == torch.bool and a[2].shape == (M,) and a[3].dtype == torch.int64 and a[3].shape == (P,)
    # the same workspace twice, through the raw entry point
    lib = _lib.load()
    ws = torch.empty(lib.loftr_estimate_absolute_pose_batched_workspace_bytes(M, P), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        R, tt = torch.zeros(P, 9, device=DEV), torch.zeros(P, 3, device=DEV)
        inl, n = torch.zeros(M, dtype=torch.uint8, device=DEV), torch.zeros(P, dtype=torch.int64, device=DEV)
        st = lib.loftr_estimate_absolute_pose_batched(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), M, t[3].data_ptr(), P, THR, CONF, 11,
                                                      R.data_ptr(), tt.data_ptr(), inl.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      torch.cuda.current_stream().cuda_stream)
        assert st == 0
        outs.append((R.reshape(P, 3, 3), tt, inl.view(torch.bool), n))
    for x, y, z in zip(a, outs[0], outs[1]):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_refusals_leave_the_outputs_unwritten(grid):
    tags, pairs, host = grid
    t = _dev(_batch(pairs[6:9]))
    M, P = t[0].shape[0], 3
    lib = _lib.load()
    ws = torch.empty(lib.loftr_estimate_absolute_pose_batched_workspace_bytes(M, P), dtype=torch.uint8, device=DEV)

    def raw(bids=None, ws_bytes=None):
        R, tt = torch.full((P, 9), 7.0, device=DEV), torch.full((P, 3), 7.0, device=DEV)
        inl, n = torch.full((M,), 7, dtype=torch.uint8, device=DEV), torch.full((P,), 7, dtype=torch.int64, device=DEV)
        st = lib.loftr_estimate_absolute_pose_batched(t[0].data_ptr(), t[1].data_ptr(), (t[2] if bids is None else bids).data_ptr(), M, t[3].data_ptr(),
                                                      P, THR, CONF, 0, R.data_ptr(), tt.data_ptr(), inl.data_ptr(), n.data_ptr(), ws.data_ptr(),
                                                      ws.numel() if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return st, bool((R == 7).all() and (tt == 7).all() and (inl == 7).all() and (n == 7).all())

    assert raw(bids=t[2].flip(0).contiguous()) == (-1, True)                          # not grouped by ascending pair
    bad = t[2].clone(); bad[-1] = P
    assert raw(bids=bad) == (-1, True)                                                # id >= P
    bad = t[2].clone(); bad[0] = -1
    assert raw(bids=bad) == (-1, True)
    assert raw(ws_bytes=ws.numel() - 1) == (-3, True)                                 # short workspace
    st, untouched = raw()
    assert st == 0 and not untouched
    call = lambda *a: ops.estimate_absolute_poses(*a, THR, CONF)
    with pytest.raises(_lib.LoftrHipError):
        call(t[0].cpu(), t[1], t[2], t[3])
    with pytest.raises(_lib.LoftrHipError):
        call(t[0], t[1], t[2].flip(0), t[3])
    with pytest.raises(_lib.LoftrHipError):
        call(t[0], t[1], t[2], t[3][:2])                                              # pair ids beyond K
    with pytest.raises(_lib.LoftrHipError):
        call(t[0], t[1][:-1], t[2], t[3])
    got = call(*t)                                                                    # still fine after the refusals
    _assert_equal_to_host(t[2].cpu().numpy(), host[0][6:9], got)


def test_empty_batch_and_no_matches():
    z3, z2 = torch.zeros(0, 3, device=DEV), torch.zeros(0, 2, device=DEV)
    b = torch.zeros(0, dtype=torch.int64, device=DEV)
    R, t, inl, n = ops.estimate_absolute_poses(z3, z2, b, torch.eye(3, device=DEV).repeat(3, 1, 1), THR, CONF)
    assert n.tolist() == [-1, -1, -1] and inl.shape == (0,) and not R.any() and not t.any()
    R, t, inl, n = ops.estimate_absolute_poses(z3, z2, b, torch.zeros(0, 3, 3, device=DEV), THR, CONF)
    assert R.shape == (0, 3, 3) and t.shape == (0, 3) and n.shape == (0,)
    X, v = ops.lift_keypoints(z2, b, torch.ones(2, 6, 8, device=DEV), torch.eye(3, device=DEV).repeat(2, 1, 1))
    assert X.shape == (0, 3) and v.shape == (0,) and v.dtype == torch.bool


def test_per_pair_form_matches_the_host_estimator(grid):
    tags, pairs, host = grid
    for tag in ("m2", "m4", "m257", "collinear"):
        X, k, K = pairs[tags.index(tag)]
        ref, got = EV.estimate_absolute_pose_native(X, k, K, THR, CONF, 4), EV.estimate_absolute_pose_native_gpu(X, k, K, THR, CONF, 4)
        assert (ref is None) == (got is None), tag
        if ref is not None:
            assert np.array_equal(ref[2], got[2]) and np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1]), tag


# ---- lifting --------------------------------------------------------------------------------------------------------------------
def _lift_case():
    """700 keypoints over 3 pairs with 38 x 54 depth maps (three blocks of the kernel's grid; even sizes, so that the border keypoints
    dw - 0.5 / dh - 0.5 round half-to-even out of the map): inside, at exact halves, on the border, outside, negative, and over a
    block of zero depth; skewed intrinsics."""
    rng = np.random.default_rng(7)
    P, dh, dw, M = 3, 38, 54, 700
    depth = rng.uniform(1, 9, (P, dh, dw)).astype(np.float32)
    depth[:, 10:20, 15:30] = 0.0
    kpts = np.c_[rng.uniform(-3, dw + 2, M), rng.uniform(-3, dh + 2, M)].astype(np.float32)
    kpts[:40] = np.floor(kpts[:40]) + 0.5
    kpts[40] = (dw - 0.5, 5.0); kpts[41] = (5.0, dh - 0.5); kpts[42] = (-1.0, 5.0); kpts[43] = (5.0, -0.75); kpts[44] = (17.2, 12.9)
    kpts[45] = (dw - 1.0, dh - 1.0); kpts[46] = (0.0, 0.0); kpts[47] = (float(dw), 3.0); kpts[48] = (-0.5, -0.5); kpts[49] = (0.5, 1.5)
    bids = np.sort(rng.integers(0, P, M)).astype(np.int64)
    K = np.stack([np.array([[41.0 + b, 0.25 * b, 26.5 - b], [0, 43.0 - b, 18.25 + b], [0, 0, 1]], np.float32) for b in range(P)])
    T = np.tile(np.eye(4, dtype=np.float32), (P, 1, 1))
    for b in range(P):
        T[b, :3, :3] = O.rot(rng.standard_normal(3), 0.3 + 0.2 * b).astype(np.float32)
        T[b, :3, 3] = rng.uniform(-2, 2, 3).astype(np.float32)
    return kpts, bids, depth, K, T


def test_lift_keypoints_equals_the_float32_oracle_bit_for_bit():
    kpts, bids, depth, K, T = _lift_case()
    d = _dev((kpts, bids, depth, K, T))
    for with_T in (False, True):
        X, v = ops.lift_keypoints(*d[:4], d[4] if with_T else None)
        Xo, vo = O.lift(kpts, bids, depth, K, T if with_T else None)
        assert X.dtype == torch.float32 and v.dtype == torch.bool
        assert np.array_equal(v.cpu().numpy(), vo)
        assert np.array_equal(X.cpu().numpy().view(np.uint32), Xo.view(np.uint32)), np.abs(X.cpu().numpy() - Xo).max()
    v, X = v.cpu().numpy(), X.cpu().numpy()
    assert 100 < v.sum() < len(v) - 100
    # out-of-map, border (x = dw - 0.5 rounds to dw), negative and zero-depth keypoints: invalid, zero rows
    assert not v[[40, 41, 42, 43, 44, 47]].any() and not X[~v].any()
    assert v[[45, 46, 48, 49]].all()                                                  # corners; -0.5 rounds to -0 and 0.5 to 0: inside
    # the result with T is the result without T, transformed (float32, the oracle's operation order)
    X0 = ops.lift_keypoints(*d[:4])[0].cpu().numpy()
    t = T[bids]
    XT = np.stack([t[:, i, 0] * X0[:, 0] + t[:, i, 1] * X0[:, 1] + t[:, i, 2] * X0[:, 2] + t[:, i, 3] for i in range(3)], 1)
    assert np.array_equal(X[v], XT[v])


def test_lift_keypoints_matches_the_reference_fixture():
    """Device lift -> T_0to1 -> K1 projection (float32 numpy) against the reference's float32 w_kpts0, under the tolerance of
    tests/test_absolute_pose.py: 2 x the reference's own float32-vs-float64 distance, floored at one float32 ulp of 640 px."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lift_warp.npz"))
    N, L = g["kpts0"].shape[:2]
    bids = np.repeat(np.arange(N), L)
    X, valid = ops.lift_keypoints(*_dev((g["kpts0"].reshape(-1, 2), bids, g["depth0"], g["K0"])))
    X, valid = X.cpu().numpy(), valid.cpu().numpy()
    assert np.array_equal(valid, g["nonzero"].reshape(-1))
    f = np.float32
    T, K1 = g["T_0to1"][bids], g["K1"][bids]
    Y = np.einsum("nij,nj->ni", T[:, :3, :3], X).astype(f) + T[:, :3, 3]
    h = np.einsum("nij,nj->ni", K1, Y).astype(f)
    w = h[:, :2] / (h[:, 2:] + f(1e-4))
    ref32, ref64 = g["w_kpts0_f32"].reshape(-1, 2)[valid], g["w_kpts0_f64"].reshape(-1, 2)[valid]
    tol = max(2 * np.abs(ref32.astype(np.float64) - ref64).max(), 2.0 ** -14)
    assert np.abs(w[valid].astype(np.float64) - ref32).max() <= tol


# ---- localize -------------------------------------------------------------------------------------------------------------------
def test_localize_on_a_real_forward():
    """evaluation.localize on the output of the forward over the 3-pair golden case with a synthetic depth map that has a zero block:
    keys, shapes, dtypes; n_lifted; dropped matches are never inliers; per pair the host estimator's result on that pair's lifted, valid
    matches; db_side = 1 swaps the roles."""
    from test_e2e_golden import _bench_data, build_model, load
    rc, img0, img1, g = load("e2e_batch")
    net = build_model(rc, 0.0, DEV)
    data = _bench_data(g, img0, img1, DEV)
    net(data)
    N, M = img0.shape[0], data["mkpts0_f"].shape[0]
    H, W = img0.shape[2:]
    assert M > 100
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.stack([3 + 0.004 * xx + 0.003 * yy + 0.5 * b for b in range(N)]).astype(np.float32)
    depth[:, H // 4:H // 2, W // 4:W // 2] = 0.0
    K0 = np.stack([np.array([[500.0 + 10 * b, 0, W / 2], [0, 505.0, H / 2 - b], [0, 0, 1]], np.float32) for b in range(N)])
    K1 = K0[::-1].copy()
    data.update(depth0=torch.from_numpy(depth).to(DEV), K0=torch.from_numpy(K0).to(DEV), K1=torch.from_numpy(K1).to(DEV))
    before = {k: data[k].clone() for k in ("mkpts0_f", "mkpts1_f", "m_bids")}
    assert EV.localize(data) is data
    assert data["R_abs"].shape == (N, 3, 3) and data["R_abs"].dtype == torch.float32 and data["R_abs"].is_cuda
    assert data["t_abs"].shape == (N, 3) and data["t_abs"].dtype == torch.float32
    assert data["inliers"].shape == (M,) and data["inliers"].dtype == torch.bool
    assert data["n_inliers"].shape == (N,) and data["n_inliers"].dtype == torch.int64
    assert data["n_lifted"].shape == (N,) and data["n_lifted"].dtype == torch.int64
    for k, v in before.items():
        assert torch.equal(data[k], v)
    bids = data["m_bids"].cpu().numpy()
    X, valid = ops.lift_keypoints(data["mkpts0_f"], data["m_bids"], data["depth0"], data["K0"])
    X, valid, k1 = X.cpu().numpy(), valid.cpu().numpy(), data["mkpts1_f"].cpu().numpy()
    assert 0 < valid.sum() < M                                                        # some matches fall into the zero block
    assert data["n_lifted"].tolist() == [int(valid[bids == b].sum()) for b in range(N)]
    inl = data["inliers"].cpu().numpy()
    assert not inl[~valid].any()
    host = [EV.estimate_absolute_pose_native(X[valid & (bids == b)], k1[valid & (bids == b)], K1[b], 3.0, 0.999, 0) for b in range(N)]
    got = (data["R_abs"], data["t_abs"], data["inliers"][torch.from_numpy(valid).to(DEV)], data["n_inliers"])
    _assert_equal_to_host(bids[valid], host, got)
    # the roles swapped: the same matches with image 1 as the database image
    swapped = {"bs": N, "m_bids": data["m_bids"], "mkpts0_f": data["mkpts1_f"], "mkpts1_f": data["mkpts0_f"], "depth1": data["depth0"],
               "K1": data["K0"], "K0": data["K1"]}
    EV.localize(swapped, db_side=1)
    for k in ("R_abs", "t_abs", "inliers", "n_inliers", "n_lifted"):
        assert torch.equal(swapped[k], data[k]), k
    # explicit arguments override the batch's own, and a world transform moves the estimate
    T = torch.eye(4, device=DEV).repeat(N, 1, 1)
    T[:, :3, 3] = torch.tensor([0.5, -0.25, 1.0], device=DEV)
    moved = EV.localize(dict(swapped), db_side=1, T_world_from_db=T, seed=0)
    assert torch.equal(moved["n_lifted"], data["n_lifted"]) and moved["R_abs"].shape == (N, 3, 3)
