"""GPU tests of the model lookup (csrc/model_lookup_gpu.hip): the kernels against the defining host routine, bit for bit, on
the random and hand-written cases, partial waves and blocks, a block-count scan of more than one scan block, the table stress cases,
empty queries, chunked adds, device-side error reporting; and the chain atlas -> triangulation -> model -> poses against the CPU chain."""
import numpy as np
import pytest
import torch

from loftr_amd import LocalizationModel, QueryLocalizer, QueryPoses, _lib, build as build_mod
import _model_lookup_cases as MC
import _model_lookup_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def _both(case, what):
    got, want = MC.run_gpu(case), MC.run_host(case)
    MC.assert_same(got, want, what)
    return got


def test_random_queries_equal_the_host_routine(lib):
    got = _both(MC.random_case(), "random")
    assert got["counts"][0] > 100 and got["counts"][4 + O.FUSED] > 100 and got["counts"][3] == 0


def test_hand_written_cases(lib):
    case, want_reason, _, kept = MC.hand_case()
    got = _both(case, "hand")
    assert got["match_reason"].tolist() == want_reason and got["match"].tolist() == kept["match"]
    case, want_reason = MC.edge_case()
    assert _both(case, "edges")["match_reason"].tolist() == want_reason


@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 1025])
def test_prefixes_that_fill_no_wave_or_block(lib, M):
    _both(MC.prefix(MC.random_case(), M), f"prefix {M}")


def test_block_counts_beyond_one_scan_block(lib):
    """M = 256 * 1024 + 1 matches: 1025 block counts, so the scan of the block counts takes two scan blocks."""
    case = MC.tiled(MC.random_case(), 256 * 1024 + 1)
    got = _both(case, "tiled")
    assert len(got["match_reason"]) == 256 * 1024 + 1 and got["counts"][0] > 30000


def test_table_stress(lib):
    got = _both(MC.same_key_case(4096), "same key")
    assert got["match"].tolist() == [0] and got["counts"][4 + O.FUSED] == 4095           # equal confidence: the smallest index
    for vary in ("query", "point"):
        got = _both(MC.key_bits_case(vary), vary + " bits")
        assert got["counts"][0] == 1500 and (got["conf"] == 0.5).all()


@pytest.mark.parametrize("Q", [1, 3, 1025])
def test_empty_queries_first_last_and_in_the_middle(lib, Q):
    got = _both(MC.empty_queries_case(Q), f"Q = {Q}")
    n = np.diff(got["q_offsets"])
    assert len(n) == Q and (Q == 1 or (n[0] == 0 and n[-1] == 0)) and n.sum() == got["counts"][0] > 0


def test_nothing_to_do(lib):
    case, *_ = MC.hand_case()
    none = MC.make_queries(np.zeros((0, 2)), np.zeros((0, 2)), [], [], [], [], 0)
    for qq in (none, dict(none, Q=5), dict(none, Q=2, row_db=case["q"]["row_db"], row_query=case["q"]["row_query"])):
        got = _both(dict(model=case["model"], q=qq), "empty")
        assert got["counts"][0] == 0 and got["q_offsets"].tolist() == [0] * (qq["Q"] + 1)


# ---- the Python layer on the device ----------------------------------------------------------------------------------------------------------
def _model(case, dev="cuda"):
    m = case["model"]
    t = lambda k: torch.from_numpy(m[k]).to(dev)
    return LocalizationModel(t("kp_offsets"), t("keypoints"), t("kp_point"), t("xyz"), m["image_hw"], m["cell_px"])


def _add_rows(loc, q, r0, r1, dev="cuda", **over):
    sel = (q["rows"] >= r0) & (q["rows"] < r1)
    data = {"mkpts0_f": torch.from_numpy(q["kpts_q"][sel]).to(dev), "mkpts1_f": torch.from_numpy(q["kpts_db"][sel]).to(dev),
            "mconf": torch.from_numpy(q["conf"][sel]).to(dev), "m_bids": torch.from_numpy(q["rows"][sel].astype(np.int64) - r0).to(dev)}
    data.update(over)
    loc.add(q["row_query"][r0:r1], q["row_db"][r0:r1], data, db_side=1, mask=None if q["mask"] is None else torch.from_numpy(q["mask"][sel]).to(dev))


@pytest.mark.parametrize("rows_per_add", [1, 7])
def test_chunked_adds_equal_one_call(lib, rows_per_add):
    """1 / 7 rows per add: with 7, queries are split across calls."""
    case = MC.random_case()
    q, model = case["q"], _model(case)
    R = len(q["row_db"])
    one, many = QueryLocalizer(model, q["Q"]), QueryLocalizer(model, q["Q"])
    _add_rows(one, q, 0, R)
    for r0 in range(0, R, rows_per_add):
        _add_rows(many, q, r0, min(R, r0 + rows_per_add))
    (a, sa), (b, sb) = one.correspondences(), many.correspondences()
    want = MC.run_host(case)
    for k in MC.FIELDS:
        assert a[k].is_cuda and torch.equal(a[k], b[k]) and np.array_equal(a[k].cpu().numpy(), want[k], equal_nan=True), (rows_per_add, k)
    assert sa == sb and sa["n_correspondences"] == want["counts"][0]


def test_device_side_errors_surface_as_value_errors(lib):
    case, *_ = MC.hand_case()
    q, model = case["q"], _model(case)
    bids = torch.from_numpy(q["rows"].astype(np.int64)).cuda()
    for edit, pat in ((lambda b: b.__setitem__(15, 3), r"rows outside \[0, R\).*device"), (lambda b: b.__setitem__(0, -1), r"rows outside \[0, R\).*device"),
                      (lambda b: b.__setitem__(5, 1), "rows that do not ascend.*device")):
        b = bids.clone()
        edit(b)
        loc = QueryLocalizer(model, 2)
        _add_rows(loc, q, 0, 3, m_bids=b)                                # nothing waits: the ids live on the device
        with pytest.raises(ValueError, match=pat):
            loc.solve(np.tile(np.eye(3), (2, 1, 1)))
    # an id that is in range for the whole list but not for its own add
    loc = QueryLocalizer(model, 2)
    first = bids[:int((q["rows"] < 2).sum())]
    _add_rows(loc, q, 0, 2, m_bids=torch.where(first == 1, 2, first))
    _add_rows(loc, q, 2, 3)
    with pytest.raises(ValueError, match=r"rows outside \[0, R\).*device"):
        loc.correspondences()
    # the bits the Python layer checks on the host before they reach the kernels, straight through ops
    from loftr_amd import ops
    m = case["model"]
    inv, gh, gw = O.grid(m["image_hw"], m["cell_px"])
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for over, bit in ((dict(row_query=np.array([0, 0, 2], np.int32)), O.ST_QUERY), (dict(row_query=np.array([1, 0, 1], np.int32)), O.ST_QUERY),
                      (dict(row_db=np.array([0, 2, 0], np.int32)), O.ST_IMAGE), (dict(row_db=np.array([0, 0, -1], np.int32)), O.ST_IMAGE),
                      (dict(row_query=np.array([0, 0, 2], np.int32), row_db=np.array([5, 0, 0], np.int32)), O.ST_QUERY | O.ST_IMAGE)):
        qq = dict(q, **over)
        out = ops.model_lookup(model.kp_offsets, model.kp_cell, model.kp_point, model.xyz, gh, gw, float(inv),
                               *[dev(qq[k]) for k in ("kpts_db", "kpts_q", "conf", "rows", "mask", "row_db", "row_query")], 2)
        assert int(out["counts"][3].cpu()) == bit == O.lookup(m, qq)["status"], over
    # the model's own bits
    t = lambda k: torch.from_numpy(m[k]).cuda()
    with pytest.raises(ValueError, match="ascend strictly"):
        LocalizationModel(t("kp_offsets"), t("keypoints")[[1, 0, 2, 3]], t("kp_point"), t("xyz"), MC.HW, MC.CELL)
    with pytest.raises(ValueError, match=r"kp_point outside \[-1, P\)"):
        LocalizationModel(t("kp_offsets"), t("keypoints"), torch.tensor([0, -1, 2, 1], dtype=torch.int32).cuda(), t("xyz"), MC.HW, MC.CELL)


def test_mixed_devices_are_refused(lib):
    case, *_ = MC.hand_case()
    m, q = case["model"], case["q"]
    t = lambda k: torch.from_numpy(m[k])
    with pytest.raises(_lib.LoftrHipError, match="different devices"):
        LocalizationModel(t("kp_offsets").cuda(), t("keypoints"), t("kp_point").cuda(), t("xyz").cuda(), MC.HW, MC.CELL)
    gpu, cpu = _model(case), _model(case, "cpu")
    with pytest.raises(_lib.LoftrHipError, match="no silent fallback"):
        _add_rows(QueryLocalizer(gpu, 2), q, 0, 3, dev="cpu")
    with pytest.raises(_lib.LoftrHipError, match="no silent fallback"):
        _add_rows(QueryLocalizer(cpu, 2), q, 0, 3, dev="cuda")
    with pytest.raises(_lib.LoftrHipError, match="no silent fallback"):
        _add_rows(QueryLocalizer(gpu, 2), q, 0, 3, mconf=torch.from_numpy(q["conf"]))
    loc = QueryLocalizer(gpu, 2)
    _add_rows(loc, q, 0, 3)
    with pytest.raises(_lib.LoftrHipError, match="no silent fallback"):
        loc.solve(torch.zeros(2, 3, 3))


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
def test_chain_on_the_gpu_equals_the_cpu_chain(lib):
    """GPU atlas -> triangulate -> LocalizationModel -> QueryLocalizer.solve against the CPU chain: the correspondences bit for bit; R, t,
    inliers and n_inliers equal, as tests/test_hip_absolute_pose.py asserts for the estimator alone."""
    Kq = MC.query_scene()["K"]
    cpu_model, _, _ = MC.build_model("cpu")
    want = MC.localize_scene(cpu_model).solve(Kq, thresh_px=3.0, conf=0.999, seed=0)
    gpu_model, _, _ = MC.build_model("cuda")
    assert gpu_model.kp_cell.is_cuda and torch.equal(gpu_model.kp_cell.cpu(), cpu_model.kp_cell) and torch.equal(gpu_model.kp_point.cpu(), cpu_model.kp_point)
    for rows_per_add in (5, 3):
        got = MC.localize_scene(gpu_model, rows_per_add).solve(Kq, thresh_px=3.0, conf=0.999, seed=0)
        assert isinstance(got, QueryPoses) and got.R.is_cuda and got.n_corr.tolist() == [60] * 8
        for k in QueryPoses.FIELDS:
            g, w = getattr(got, k).cpu(), getattr(want, k)
            assert g.dtype == w.dtype and torch.equal(g, w), (rows_per_add, k)
        assert got.stats == want.stats
        assert (got.n_inliers > 0).all()
    host = got.to_host()
    assert set(host) == set(QueryPoses.FIELDS) | {"stats"} and host["R"].shape == (8, 3, 3)
