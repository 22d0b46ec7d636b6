"""CPU tests of the model lookup (csrc/model_lookup.hip): the defining host routine against the independent oracle
(tests/_model_lookup_oracle.py), every array and count equal; the hand-written cases; the guards of the Python layer; and the
localisation of eight query cameras against the triangulated model of _triangulation_cases.sfm_scene(), end to end."""
import numpy as np
import pytest
import torch

from loftr_amd import KeypointAtlas, LocalizationModel, QueryLocalizer, QueryPoses, _lib, build as build_mod, ops
from loftr_amd.evaluation import estimate_absolute_pose_native
import _model_lookup_cases as MC
import _model_lookup_oracle as O
import _triangulation_cases as TC


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


# ---- the host routine against the oracle ---------------------------------------------------------------------------------------------------
def test_random_queries_equal_the_oracle(lib):
    case = MC.random_case()
    got, want = MC.run_host(case), MC.run_oracle(case)
    MC.assert_same(got, want, "random")
    c, q = want["counts"], case["q"]
    assert all(c[k] > 0 for k in ("kept", "masked", "nonfinite", "negative_conf", "outside", "no_keypoint", "no_point", "fused")), c
    n = np.diff(got["q_offsets"])
    assert n[1] == 0 and n[2] == 0 and (n[[0, 3, 4, 5, 6, 7, 8]] > 0).all(), n       # no row; rows that all miss
    # the duplicated rows of query 4: of two equal matches the first is kept, never both
    in4 = q["row_query"][q["rows"]] == 4
    assert (got["match_reason"][in4] == O.FUSED).sum() >= (got["match_reason"][in4] == O.KEPT).sum() > 0
    # no (query, point) twice
    pairs = list(zip(got["q_ids"].tolist(), got["point"].tolist()))
    assert len(set(pairs)) == len(pairs) and (np.diff(got["match"]) > 0).all() and (np.diff(got["q_ids"]) >= 0).all()


def test_one_match_of_every_reason(lib):
    case, want_reason, want_counts, kept = MC.hand_case()
    got = MC.run_host(case)
    MC.assert_same(got, MC.run_oracle(case), "hand")
    assert got["match_reason"].tolist() == want_reason
    assert {name: got["counts"][4 + i] for i, name in enumerate(O.REASONS)} == want_counts and got["counts"][0] == 4
    for k, v in kept.items():
        assert np.array_equal(got[k], np.asarray(v, got[k].dtype)), (k, got[k])
    assert np.array_equal(got["kpts"], case["q"]["kpts_q"][kept["match"]])


def test_binary_search_edges(lib):
    case, want_reason = MC.edge_case()
    got = MC.run_host(case)
    MC.assert_same(got, MC.run_oracle(case), "edges")
    assert got["match_reason"].tolist() == want_reason
    # the kept matches found THEIR image's keypoint: every keypoint has its own point
    hits = {(1, 7): 0, (2, 3): 1, (2, 512): 4, (3, 10): 5, (5, 0): 6, (5, 10): 7}
    rows = case["q"]["rows"][got["match"]]
    cells = [int(O.cell_of(case["q"]["kpts_db"][m], *O.grid(MC.HW, MC.CELL))) for m in got["match"]]
    assert [hits[(int(case["q"]["row_db"][r]), c)] for r, c in zip(rows, cells)] == got["point"].tolist()


@pytest.mark.parametrize("name", ["same_key", "query_bits", "point_bits", "empty_1", "empty_3", "empty_1025"])
def test_table_and_offset_cases_equal_the_oracle(lib, name):
    case = {"same_key": lambda: MC.same_key_case(), "query_bits": lambda: MC.key_bits_case("query"), "point_bits": lambda: MC.key_bits_case("point"),
            "empty_1": lambda: MC.empty_queries_case(1), "empty_3": lambda: MC.empty_queries_case(3),
            "empty_1025": lambda: MC.empty_queries_case(1025)}[name]()
    got = MC.run_host(case)
    MC.assert_same(got, MC.run_oracle(case), name)
    if name == "same_key":
        assert got["match"].tolist() == [0] and got["counts"][4 + O.FUSED] == 4095
    if name in ("query_bits", "point_bits"):
        assert got["counts"][0] == 1500 and (got["conf"] == 0.5).all()


def test_every_error_bit(lib):
    case, *_ = MC.hand_case()
    m, q = case["model"], case["q"]
    inv, gh, gw = O.grid(m["image_hw"], m["cell_px"])
    cell, status = ops.model_cells_host(m["kp_offsets"], m["keypoints"], m["kp_point"], 2, gh, gw, float(inv))
    assert status == 0 and cell.tolist() == [5, 40, 100, 5]

    def run(**over):
        qq = dict(q, **over)
        bits = O.lookup(m, qq)["status"]
        with pytest.raises(_lib.LoftrHipError, match="status -1"):
            ops.model_lookup_host(m["kp_offsets"], cell, m["kp_point"], m["xyz"], gh, gw, float(inv), qq["kpts_db"], qq["kpts_q"], qq["conf"],
                                  qq["rows"], qq["mask"], qq["row_db"], qq["row_query"], qq["Q"])
        return bits

    edit = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]]).astype(a.dtype)
    assert run(rows=edit(q["rows"], 15, 3)) == O.ST_ROW
    assert run(rows=edit(q["rows"], 0, -1)) == O.ST_ROW
    assert run(rows=edit(q["rows"], 5, 1)) == O.ST_UNSORTED
    assert run(row_query=np.array([0, 0, 2], np.int32)) == O.ST_QUERY
    assert run(row_query=np.array([-1, 0, 1], np.int32)) == O.ST_QUERY
    assert run(row_query=np.array([1, 0, 1], np.int32)) == O.ST_QUERY                        # descending
    assert run(row_db=np.array([0, 2, 0], np.int32)) == O.ST_IMAGE
    assert run(row_db=np.array([0, -1, 0], np.int32)) == O.ST_IMAGE
    assert run(Q=1) == O.ST_QUERY
    # the model's bits
    kp = m["keypoints"].copy()
    kp[[0, 1]] = kp[[1, 0]]                                                                  # cells 40, 5, 100: not ascending
    assert ops.model_cells_host(m["kp_offsets"], kp, m["kp_point"], 2, gh, gw, float(inv))[1] == 16 == O.model_cells(m["kp_offsets"], kp, m["kp_point"], 2, MC.HW, MC.CELL)[1]
    kp = m["keypoints"].copy()
    kp[1] = kp[0]                                                                            # the same cell twice
    assert ops.model_cells_host(m["kp_offsets"], kp, m["kp_point"], 2, gh, gw, float(inv))[1] == 16
    kp[1] = [-3.0, 1.0]                                                                      # outside the grid
    assert ops.model_cells_host(m["kp_offsets"], kp, m["kp_point"], 2, gh, gw, float(inv))[1] == 16
    kp[1] = [np.nan, 1.0]
    assert ops.model_cells_host(m["kp_offsets"], kp, m["kp_point"], 2, gh, gw, float(inv))[1] == 16
    for bad in (2, -2):
        pt = m["kp_point"].copy()
        pt[2] = bad
        assert ops.model_cells_host(m["kp_offsets"], m["keypoints"], pt, 2, gh, gw, float(inv))[1] == 32 == O.model_cells(m["kp_offsets"], m["keypoints"], pt, 2, MC.HW, MC.CELL)[1]
    # image 1 starts anew: its cell 5 after image 0's cell 100 is no descent
    assert O.model_cells(m["kp_offsets"], m["keypoints"], m["kp_point"], 2, MC.HW, MC.CELL) == ([5, 40, 100, 5], 0)


def test_no_query_no_match_no_row(lib):
    case, *_ = MC.hand_case()
    q = case["q"]
    none = MC.make_queries(np.zeros((0, 2)), np.zeros((0, 2)), [], [], [], [], 0)
    for name, qq in (("nothing", none), ("queries without rows", dict(none, Q=5)),
                     ("rows without matches", dict(none, Q=2, row_db=q["row_db"], row_query=q["row_query"])),
                     ("an empty mask", dict(none, Q=3, mask=np.zeros(0, np.uint8)))):
        got = MC.run_host(dict(model=case["model"], q=qq))
        MC.assert_same(got, MC.run_oracle(dict(model=case["model"], q=qq)), name)
        assert got["counts"][0] == 0 and got["q_offsets"].tolist() == [0] * (qq["Q"] + 1) and got["pts3d"].shape == (0, 3)


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def _model(case):
    m = case["model"]
    return LocalizationModel(m["kp_offsets"], m["keypoints"], m["kp_point"], m["xyz"], m["image_hw"], m["cell_px"])


def _data(q, sel, base):
    return {"mkpts0_f": torch.from_numpy(q["kpts_q"][sel]), "mkpts1_f": torch.from_numpy(q["kpts_db"][sel]), "mconf": torch.from_numpy(q["conf"][sel]),
            "m_bids": torch.from_numpy(q["rows"][sel].astype(np.int64) - base)}


def _localizer(case, rows_per_add):
    q = case["q"]
    loc = QueryLocalizer(_model(case), q["Q"])
    R = len(q["row_db"])
    for r0 in range(0, max(R, 1), rows_per_add):
        r1 = min(R, r0 + rows_per_add)
        sel = (q["rows"] >= r0) & (q["rows"] < r1)
        loc.add(q["row_query"][r0:r1], q["row_db"][r0:r1], _data(q, sel, r0), db_side=1, mask=None if q["mask"] is None else torch.from_numpy(q["mask"][sel]))
    return loc


@pytest.mark.parametrize("rows_per_add", [1, 7, 1000])
def test_query_localizer_equals_the_oracle_however_the_rows_are_chunked(lib, rows_per_add):
    case = MC.random_case()
    out, stats = _localizer(case, rows_per_add).correspondences()
    want = MC.run_oracle(case)
    for k in MC.FIELDS:
        assert np.array_equal(out[k].numpy(), want[k], equal_nan=True), (rows_per_add, k)
    assert stats["n_correspondences"] == want["C"] and stats["n_matches"] == len(case["q"]["conf"]) and "n_bad_row" not in stats
    assert {k: stats["n_" + k] for k in O.REASONS if k != "bad_row"} == {k: v for k, v in want["counts"].items() if k != "bad_row"}


def test_db_side_0_swaps_the_roles(lib):
    case, *_ = MC.hand_case()
    q = case["q"]
    loc = QueryLocalizer(_model(case), 2)
    d = _data(q, slice(None), 0)
    d["mkpts0_f"], d["mkpts1_f"] = d["mkpts1_f"], d["mkpts0_f"]
    loc.add(q["row_query"], q["row_db"], d, db_side=0, mask=torch.from_numpy(q["mask"]).bool())
    out, _ = loc.correspondences()
    assert out["match"].tolist() == [2, 12, 14, 15]


def test_guards_of_add_and_the_constructors(lib):
    case, *_ = MC.hand_case()
    m, q = case["model"], case["q"]
    model = _model(case)
    assert model.kp_cell.tolist() == [5, 40, 100, 5] and model.device.type == "cpu" and (model.gh, model.gw) == (19, 27)
    args = lambda **over: {**dict(kp_offsets=m["kp_offsets"], keypoints=m["keypoints"], kp_point=m["kp_point"], xyz=m["xyz"], image_hw=MC.HW,
                                  cell_px=MC.CELL), **over}
    for over, exc, pat in ((dict(kp_offsets=np.array([0, 3, 5])), ValueError, "kp_offsets must start"),
                           (dict(kp_offsets=np.array([1, 3, 4])), ValueError, "kp_offsets must start"),
                           (dict(kp_offsets=np.array([0, 4, 3, 4])), ValueError, "kp_offsets must start"),
                           (dict(kp_offsets=np.array([0.0, 3.0, 4.0])), ValueError, "integers"),
                           (dict(kp_point=m["kp_point"].astype(np.float32)), ValueError, "integers"),
                           (dict(keypoints=m["keypoints"][:3]), ValueError, "expected kp_offsets"),
                           (dict(xyz=m["xyz"][:, :2]), ValueError, "expected kp_offsets"),
                           (dict(kp_point=np.array([0, -1, 2, 1], np.int32)), ValueError, r"kp_point outside \[-1, P\)"),
                           (dict(keypoints=m["keypoints"][[1, 0, 2, 3]]), ValueError, "ascend strictly"),
                           (dict(cell_px=0.0), ValueError, "positive"),
                           (dict(keypoints=torch.from_numpy(m["keypoints"]).to("meta")), _lib.LoftrHipError, "different devices")):
        with pytest.raises(exc, match=pat):
            LocalizationModel(**args(**over))
    with pytest.raises(ValueError, match="LocalizationModel"):
        QueryLocalizer(object(), 2)
    with pytest.raises(ValueError, match="n_queries"):
        QueryLocalizer(model, -1)
    good = _data(q, slice(None), 0)
    rq, rd = q["row_query"], q["row_db"]
    bad_calls = (
        (dict(db_side=2), ValueError, "db_side"),
        (dict(query_ids=[0, 0, 2]), ValueError, "query ids outside"),
        (dict(query_ids=[0, 1, 0]), ValueError, "must not descend"),
        (dict(query_ids=[0.0, 0.0, 1.0]), ValueError, "integer array"),
        (dict(query_ids=[0, 0]), ValueError, "database image ids"),
        (dict(db_image_ids=[0, 2, 0]), ValueError, "database image ids outside"),
        (dict(data={k: v for k, v in good.items() if k != "mconf"}), ValueError, "lacks"),
        (dict(data=dict(good, mconf=good["mconf"][:3])), ValueError, "expected mkpts0_f"),
        (dict(data=dict(good, m_bids=good["m_bids"].float())), ValueError, "m_bids must be integers"),
        (dict(data=dict(good, m_bids=good["m_bids"] + 1)), ValueError, r"m_bids outside \[0, 3\)"),
        (dict(data=dict(good, m_bids=good["m_bids"].flip(0))), ValueError, "m_bids must ascend"),
        (dict(mask=torch.ones(3, dtype=torch.bool)), ValueError, "mask must be bool"),
        (dict(mask=torch.ones(16)), ValueError, "mask must be bool"),
        (dict(data=dict(good, mconf=good["mconf"].to("meta"))), _lib.LoftrHipError, "no silent fallback"),
    )
    for over, exc, pat in bad_calls:
        loc = QueryLocalizer(model, 2)
        kw = {**dict(query_ids=rq, db_image_ids=rd, data=good, db_side=1, mask=None), **over}
        with pytest.raises(exc, match=pat):
            loc.add(**kw)
        assert loc.n_rows == 0 and loc.n_matches == 0
    loc = QueryLocalizer(model, 2)
    with pytest.raises(ValueError, match="but no row"):
        loc.add([], [], good)
    loc.add([1], [0], _data(q, q["rows"] == 2, 2))
    with pytest.raises(ValueError, match="must not descend"):                                # ... from one call to the next
        loc.add([0], [0], _data(q, q["rows"] == 0, 0))
    with pytest.raises(ValueError, match=r"K_query \[2,3,3\]"):
        loc.solve(np.zeros((3, 3, 3)))
    with pytest.raises(_lib.LoftrHipError, match="no silent fallback"):
        loc.solve(torch.zeros(2, 3, 3, device="meta"))


def test_from_atlas_needs_the_grid_geometry(lib):
    model, sfm, pts = MC.build_model("cpu")
    xyz, has = pts.keypoint_xyz(sfm)
    assert torch.equal(model.kp_point >= 0, has) and torch.equal(model.xyz[model.kp_point[has].long()], xyz[has])
    assert sfm.image_hw == TC.SFM_HW and sfm.cell_px == TC.SFM_CELL and "image_hw" not in sfm.FIELDS
    bare = type(sfm)(sfm.stats, **{k: getattr(sfm, k) for k in sfm.FIELDS})
    with pytest.raises(ValueError, match="grid geometry"):
        LocalizationModel.from_atlas(bare, pts)
    from loftr_amd import triangulate_tracks
    s = TC.scene()
    loose = triangulate_tracks(*[torch.from_numpy(np.ascontiguousarray(s[k])) for k in ("offsets", "obs_image", "obs_xy", "K", "T")])
    with pytest.raises(ValueError, match="no tracks"):
        LocalizationModel.from_atlas(sfm, loose)


# ---- end to end over sfm_scene() -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def localized(lib):
    """The eight queries through the CPU chain: computed once, left unchanged."""
    model, _, _ = MC.build_model("cpu")
    res = MC.localize_scene(model).solve(MC.query_scene()["K"], thresh_px=3.0, conf=0.999, seed=0)
    return model, res, MC.run_oracle(MC.scene_as_case(model))


def test_scene_correspondences_equal_the_oracle(localized):
    model, res, want = localized
    assert isinstance(res, QueryPoses) and res.stats["n_matches"] == 8 * 300 and res.stats["n_correspondences"] == 8 * 60
    assert res.n_corr.tolist() == [60] * 8                                                   # every 3D point once per query
    got = res.to_host()
    for k in MC.FIELDS:
        assert np.array_equal(got[k], want[k]), k
    assert res.stats["n_kept"] + res.stats["n_fused"] + res.stats["n_no_point"] == 2400 and res.stats["n_no_keypoint"] == 0
    assert torch.equal(res.match_inlier.nonzero().squeeze(1), res.match[res.inliers].long())


def test_scene_poses_equal_the_host_estimator_on_the_oracles_correspondences(localized):
    _, res, want = localized
    qs = MC.query_scene()
    for q in range(MC.N_QUERIES):
        sl = slice(int(want["q_offsets"][q]), int(want["q_offsets"][q + 1]))
        R, t, inl = estimate_absolute_pose_native(want["pts3d"][sl], want["kpts"][sl], qs["K"][q], 3.0, 0.999, 0)
        assert np.array_equal(res.R[q].numpy(), R.astype(np.float32)) and np.array_equal(res.t[q].numpy(), t.astype(np.float32)), q
        assert np.array_equal(res.inliers[sl].numpy(), inl) and int(res.n_inliers[q]) == int(inl.sum()), q


def test_scene_poses_are_within_twice_the_ground_truth_baseline(localized):
    """The baseline already carries the query-side snapping error (2 px cells); the model adds the database-side one, averaged over up
    to five views: two independent errors of similar size give about sqrt(2), so 2 x is the bar.  The per-query figures are printed
    before they are asserted (profiles/model_localize_accuracy.txt; tools/micro/model_localize_accuracy.py prints the same report)."""
    _, res, want = localized
    rows = MC.accuracy_figures(res, want)
    print(MC.accuracy_report(rows))
    for r in rows:
        assert r["n"] >= 3 and r["n_gt"] >= 3, r                                             # both localised
        assert r["R_err"] <= 2 * r["R_gt"] and r["c_err"] <= 2 * r["c_gt"], r
