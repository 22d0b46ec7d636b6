"""Batched homography / fundamental-matrix RANSAC on the GPU (csrc/geometry_gpu.hip, ops.estimate_geometry): for every pair of a batch,
the result of the host estimator loftr_estimate_geometry (evaluation.estimate_homography_native / estimate_fundamental_native) with the
same seed -- same n_inliers, same inlier mask, the matrix equal after the float32 rounding.  The host estimator is the reference here
(tests/test_geometry.py checks it against a numpy oracle); parity against OpenCV stays unpinned."""
import numpy as np
import pytest
import torch

from loftr_amd import _lib, evaluation as EV, ops
import _geometry_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODELS = ("homography", "fundamental")
SIZE = {"homography": 4, "fundamental": 7}
THR = {"homography": 3.0, "fundamental": 1.0}
CONF = 0.999
HOST = {"homography": EV.estimate_homography_native, "fundamental": EV.estimate_fundamental_native}
GPU1 = {"homography": EV.estimate_homography_native_gpu, "fundamental": EV.estimate_fundamental_native_gpu}


def _collinear(rng, n=60):
    t = rng.uniform(0, 1, n)
    return np.c_[100 + 400 * t, 80 + 300 * t].astype(np.float32), np.c_[120 + 380 * t, 90 + 290 * t].astype(np.float32)


def _pairs(model):
    """A ragged batch of about 6 000 matches: the smallest shapes at which each stage can go wrong.  257 and 513 cross the 256-wide
    strided sums of the refit and the scorer's 512-match LDS tile; 8 is the fundamental refit's minimum."""
    rng = np.random.default_rng(2025 + len(model))
    s, thr = SIZE[model], THR[model]
    pair = lambda n, noise, out: O.make_pair(rng, model, n, noise, out, thr)[:2]
    tags, pairs = [], []
    def add(tag, p):
        tags.append(tag)
        pairs.append(p)
    add("m0", pair(0, 0.0, 0.0))
    add("s-1", pair(s - 1, 0.0, 0.0))
    add("s", pair(s, 0.0, 0.0))
    add("m8", pair(8, 0.3, 0.0))
    add("m257", pair(257, 0.5, 0.3))
    add("empty", pair(0, 0.0, 0.0))                                                   # an empty pair between two non-empty ones
    add("m513", pair(513, 0.5, 0.3))
    add("early", pair(700, 0.3, 0.05))                                                # stops after a few iterations
    add("capped", pair(1500, 0.5, 0.85))                                              # runs all 1000
    add("collinear", _collinear(rng))
    add("adoption", O.make_adoption_pair(rng, model, thr)[:2])                        # refit rejected by the adoption rule
    add("m1100", pair(1100, 0.5, 0.4))
    add("noise", (np.c_[rng.uniform(0, 640, 300), rng.uniform(0, 480, 300)].astype(np.float32),
                  np.c_[rng.uniform(0, 640, 300), rng.uniform(0, 480, 300)].astype(np.float32)))
    add("m1300", pair(1300, 0.0, 0.4))
    return tags, pairs


def _batch(pairs):
    return (np.concatenate([p[0] for p in pairs]).reshape(-1, 2), np.concatenate([p[1] for p in pairs]).reshape(-1, 2),
            np.concatenate([np.full(len(p[0]), b, np.int64) for b, p in enumerate(pairs)]))


def _dev(batch):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in batch]


@pytest.fixture(scope="module")
def grids():
    """Per model: tags, pairs and the host estimator's results for the two seeds (computed once, never modified)."""
    out = {}
    for model in MODELS:
        tags, pairs = _pairs(model)
        host = {seed: [HOST[model](p0, p1, THR[model], CONF, seed) for p0, p1 in pairs] for seed in (0, 11)}
        out[model] = (tags, pairs, host)
    return out


def _assert_equal_to_host(pairs, host, got):
    mat, inl, n = (x.cpu().numpy() for x in got)
    bids = _batch(pairs)[2]
    for b, ref in enumerate(host):
        mask = inl[bids == b]
        if ref is None:
            assert n[b] == -1 and not mask.any() and not mat[b].any(), (b, n[b])
            continue
        assert n[b] == ref[1].sum(), (b, n[b], ref[1].sum())
        assert np.array_equal(mask, ref[1]), (b, np.flatnonzero(mask != ref[1])[:10])
        assert np.array_equal(mat[b], ref[0].astype(np.float32)), (b, np.abs(mat[b] - ref[0]).max())


@pytest.mark.parametrize("seed", [0, 11])
@pytest.mark.parametrize("model", MODELS)
def test_identical_to_the_host_estimator_on_a_ragged_batch(grids, model, seed):
    tags, pairs, host = grids[model]
    assert 5000 <= sum(len(p[0]) for p in pairs) <= 7000
    got = ops.estimate_geometry(*_dev(_batch(pairs)), len(pairs), model, THR[model], CONF, seed)
    _assert_equal_to_host(pairs, host[seed], got)
    # the batch holds what it claims to hold (properties of the host results, the reference of this test)
    ref = dict(zip(tags, host[seed]))
    for tag in ("m0", "s-1", "empty"):
        assert ref[tag] is None
    assert ref["s"] is not None and ref["s"][1].sum() == SIZE[model]
    assert ref["early"][1].mean() >= 0.9 and ref["capped"][1].mean() <= 0.2           # 0.9^7 -> <= 12 iterations; 0.2^4 -> the cap
    if model == "homography":
        assert ref["collinear"] is None
    p0, p1 = pairs[tags.index("adoption")]
    fit = (O.fit_homography if model == "homography" else O.fit_fundamental)(p0, p1)
    assert ref["adoption"][1].all() and (O.residual(model, fit, p0, p1) <= THR[model]).sum() < len(p0)   # the fit over all loses inliers


@pytest.mark.parametrize("model", MODELS)
def test_repeat_calls_poisoned_memory_and_untouched_inputs(grids, model):
    from conftest import poison_gpu_memory
    tags, pairs, host = grids[model]
    t = _dev(_batch(pairs))
    before = [x.clone() for x in t]
    a = ops.estimate_geometry(*t, len(pairs), model, THR[model], CONF, 11)
    b = ops.estimate_geometry(*t, len(pairs), model, THR[model], CONF, 11)
    poison_gpu_memory(big_gib=1, small_blocks=256)
    c = ops.estimate_geometry(*t, len(pairs), model, THR[model], CONF, 11)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    for x, y in zip(t, before):
        assert torch.equal(x, y)
    assert a[0].shape == (len(pairs), 3, 3) and a[0].dtype == torch.float32 and a[1].dtype == torch.bool and a[1].shape == t[2].shape
    assert a[2].dtype == torch.int64 and a[2].shape == (len(pairs),)
    # the same workspace twice, through the raw entry point
    lib, M, P, kind = _lib.load(), t[0].shape[0], len(pairs), MODELS.index(model)
    ws = torch.empty(lib.loftr_estimate_geometry_batched_workspace_bytes(M, P, kind), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        mat, inl, n = torch.zeros(P, 9, device=DEV), torch.zeros(M, dtype=torch.uint8, device=DEV), torch.zeros(P, dtype=torch.int64, device=DEV)
        st = lib.loftr_estimate_geometry_batched(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), M, P, kind, THR[model], CONF, 11, mat.data_ptr(),
                                                 inl.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert st == 0
        outs.append((mat.reshape(P, 3, 3), inl.view(torch.bool), n))
    for x, y, z in zip(a, outs[0], outs[1]):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_refusals_leave_the_outputs_unwritten(grids):
    tags, pairs, host = grids["fundamental"]
    t = _dev(_batch(pairs[6:9]))
    M, P = t[0].shape[0], 3
    lib = _lib.load()
    ws = torch.empty(lib.loftr_estimate_geometry_batched_workspace_bytes(M, P, 1), dtype=torch.uint8, device=DEV)

    def raw(bids=None, model=1, ws_bytes=None):
        mat, inl, n = torch.full((P, 9), 7.0, device=DEV), torch.full((M,), 7, dtype=torch.uint8, device=DEV), torch.full((P,), 7, dtype=torch.int64, device=DEV)
        st = lib.loftr_estimate_geometry_batched(t[0].data_ptr(), t[1].data_ptr(), (t[2] if bids is None else bids).data_ptr(), M, P, model, 1.0, CONF, 0,
                                                 mat.data_ptr(), inl.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return st, bool((mat == 7).all() and (inl == 7).all() and (n == 7).all())

    assert raw(bids=t[2].flip(0).contiguous()) == (-1, True)                          # not grouped by ascending pair
    bad = t[2].clone(); bad[-1] = P
    assert raw(bids=bad) == (-1, True)                                                # id >= P
    bad = t[2].clone(); bad[0] = -1
    assert raw(bids=bad) == (-1, True)
    assert raw(ws_bytes=ws.numel() - 1) == (-3, True)                                 # short workspace
    assert raw(model=2) == (-1, True)
    st, untouched = raw()
    assert st == 0 and not untouched
    call = lambda *a, model="fundamental": ops.estimate_geometry(*a, P, model, 1.0, CONF)
    with pytest.raises(_lib.LoftrHipError):
        call(t[0].cpu(), t[1], t[2])
    with pytest.raises(_lib.LoftrHipError):
        call(t[0], t[1], t[2].flip(0))
    with pytest.raises(_lib.LoftrHipError):
        call(t[0].reshape(-1), t[1], t[2])
    with pytest.raises(_lib.LoftrHipError):
        call(t[0], t[1], t[2][:-1])
    with pytest.raises(_lib.LoftrHipError):
        call(*t, model="essential")
    assert call(*t)[2].shape == (P,)                                                  # still fine after the refusals


def test_empty_batch_and_no_matches():
    z = torch.zeros(0, 2, device=DEV)
    b = torch.zeros(0, dtype=torch.int64, device=DEV)
    for model in MODELS:
        mat, inl, n = ops.estimate_geometry(z, z, b, 3, model, 1.0, CONF)
        assert n.tolist() == [-1, -1, -1] and inl.shape == (0,) and not mat.any()
        mat, inl, n = ops.estimate_geometry(z, z, b, 0, model, 1.0, CONF)
        assert mat.shape == (0, 3, 3) and n.shape == (0,)


@pytest.mark.parametrize("model", MODELS)
def test_per_pair_form_matches_the_host_estimator(grids, model):
    tags, pairs, host = grids[model]
    for tag in ("s-1", "m8", "m257", "collinear"):
        p0, p1 = pairs[tags.index(tag)]
        ref, got = HOST[model](p0, p1, THR[model], CONF, 4), GPU1[model](p0, p1, THR[model], CONF, 4)
        assert (ref is None) == (got is None), tag
        if ref is not None:
            assert np.array_equal(ref[1], got[1]) and np.array_equal(ref[0], got[0]), tag


@pytest.mark.parametrize("model", MODELS)
def test_verify_matches_on_a_real_forward(model):
    """evaluation.verify_matches on the output of the forward over the 3-pair golden case: keys, shapes, dtypes, and per pair the host
    estimator's result on that pair's matches."""
    from test_e2e_golden import _bench_data, build_model, load
    rc, img0, img1, g = load("e2e_batch")
    net = build_model(rc, 0.0, DEV)
    data = _bench_data(g, img0, img1, DEV)
    net(data)
    N, M = img0.shape[0], data["mkpts0_f"].shape[0]
    assert M > 100
    assert EV.verify_matches(data, model=model) is data
    key = "H" if model == "homography" else "F"
    assert data[key].shape == (N, 3, 3) and data[key].dtype == torch.float32 and data[key].is_cuda
    assert data["inliers"].shape == (M,) and data["inliers"].dtype == torch.bool
    assert data["n_inliers"].shape == (N,) and data["n_inliers"].dtype == torch.int64
    p0, p1, bids = (data[k].cpu().numpy() for k in ("mkpts0_f", "mkpts1_f", "m_bids"))
    pairs = [(p0[bids == b], p1[bids == b]) for b in range(N)]
    host = [HOST[model](a, b, THR[model], CONF, 0) for a, b in pairs]
    _assert_equal_to_host(pairs, host, (data[key], data["inliers"], data["n_inliers"]))
