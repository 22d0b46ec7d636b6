"""Inputs shared by the model-lookup tests (tests/test_model_lookup.py on the CPU, tests/test_hip_model_lookup.py on the GPU): seeded
random queries over a small model, one match of every reason, the binary-search edges, the table stress cases, the localisation scene
over _triangulation_cases.sfm_scene(), and the runners that bring the host routine, the kernels and the oracle to one form."""
import functools

import numpy as np

import _model_lookup_oracle as O
import _triangulation_cases as TC

HW, CELL = (38.0, 54.0), 2.0                      # a 19 x 27 grid
GH, GW = 19, 27
FIELDS = ("pts3d", "kpts", "q_ids", "match", "point", "conf", "q_offsets", "match_reason")


def centre(cell, frac=(0.5, 0.5), gw=GW):
    """A position inside cell cy * gw + cx of a grid of 2 px cells."""
    cy, cx = divmod(int(cell), gw)
    return [(cx + frac[0]) * CELL, (cy + frac[1]) * CELL]


def make_model(cells_per_image, kp_point, xyz, rng=None, hw=HW):
    """cells_per_image: ascending cell ids of every image's keypoints; positions random inside the cell (the centre without rng)."""
    gw = int(hw[1] / CELL)
    kp = [centre(c, rng.uniform(0.05, 0.95, 2) if rng is not None else (0.5, 0.5), gw) for cells in cells_per_image for c in cells]
    off = np.cumsum([0] + [len(c) for c in cells_per_image]).astype(np.int64)
    return dict(kp_offsets=off, keypoints=np.array(kp, np.float32).reshape(-1, 2), kp_point=np.asarray(kp_point, np.int32),
                xyz=np.asarray(xyz, np.float32).reshape(-1, 3), image_hw=hw, cell_px=CELL)


def make_queries(kpts_db, kpts_q, conf, rows, row_db, row_query, Q, mask=None):
    return dict(kpts_db=np.asarray(kpts_db, np.float32).reshape(-1, 2), kpts_q=np.asarray(kpts_q, np.float32).reshape(-1, 2),
                conf=np.asarray(conf, np.float32).reshape(-1), rows=np.asarray(rows, np.int32).reshape(-1),
                mask=None if mask is None else np.asarray(mask, np.uint8).reshape(-1), row_db=np.asarray(row_db, np.int32).reshape(-1),
                row_query=np.asarray(row_query, np.int32).reshape(-1), Q=int(Q))


# ---- seeded random queries ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(seed=11, per_row=40):
    """12 images on the 19 x 27 grid (image 3 without a keypoint, image 7 with one), 150 points, a third of the keypoints without one.
    9 queries: query 1 has no row, the rows of query 2 all miss (they point at image 3 and at empty cells), every row of query 4 comes
    twice; confidences from {0.25, 0.5, 0.75, -0.0}, so that ties are everywhere; masked, non-finite, negative and outside matches mixed in."""
    rng = np.random.default_rng(seed)
    n_images, P = 12, 150
    cells = []
    for i in range(n_images):
        n = 0 if i == 3 else 1 if i == 7 else int(rng.integers(120, 260))
        cells.append(np.sort(rng.choice(GH * GW, n, replace=False)))
    K = sum(len(c) for c in cells)
    kp_point = np.where(rng.random(K) < 0.33, -1, rng.integers(0, P, K))
    model = make_model(cells, kp_point, rng.standard_normal((P, 3)), rng)
    row_query, row_db, copy_of_previous = [], [], []
    for q, n_rows in enumerate((3, 0, 2, 4, 3, 1, 5, 2, 3)):
        dbs = [3] + [0] * (n_rows - 1) if q == 2 else rng.integers(0, n_images, n_rows).tolist()
        for d in dbs:
            for copy in ((False, True) if q == 4 else (False,)):
                row_query.append(q); row_db.append(d); copy_of_previous.append(copy)
    kd, kq, conf, rows = [], [], [], []
    for r, (q, d) in enumerate(zip(row_query, row_db)):
        if copy_of_previous[r]:
            kd += kd[-per_row:]; kq += kq[-per_row:]; conf += conf[-per_row:]; rows += [r] * per_row
            continue
        empty = np.setdiff1d(np.arange(GH * GW), cells[d])
        for _ in range(per_row):
            u = rng.random()
            if q == 2 or u < 0.15 or len(cells[d]) == 0:
                p = centre(rng.choice(empty), rng.uniform(0.05, 0.95, 2))                  # no keypoint there
            elif u < 0.25:
                p = rng.uniform(-6, 1.2, 2) * np.array(HW[::-1])                           # mostly outside the grid
            else:
                p = centre(rng.choice(cells[d]), rng.uniform(0.0, 0.999, 2))
            kd.append(p)
            kq.append(rng.uniform(-50, 900, 2))                                            # the query point needs no grid
            conf.append(rng.choice([0.25, 0.5, 0.75, -0.0]))
            rows.append(r)
    kd, kq, conf = np.array(kd, np.float32), np.array(kq, np.float32), np.array(conf, np.float32)
    M = len(conf)
    for arr, val, n in ((kd, np.nan, 6), (kq, np.inf, 6), (conf, -np.inf, 3), (conf, np.nan, 3), (conf, -0.5, 12)):
        idx = rng.choice(M, n, replace=False)
        if arr.ndim == 2:
            arr[idx, rng.integers(0, 2, n)] = val
        else:
            arr[idx] = val
    mask = (rng.random(M) > 0.1).astype(np.uint8)
    return dict(model=model, q=make_queries(kd, kq, conf, rows, row_db, row_query, 9, mask))


# ---- one match of every reason --------------------------------------------------------------------------------------------------------------
def hand_case():
    """-> (case, expected reason per match, expected counts).  Image 0 has keypoints at cells 5 (point 0), 40 (no point) and 100 (point 1),
    image 1 at cell 5 (point 1).  Two queries."""
    model = make_model([[5, 40, 100], [5]], [0, -1, 1, 1], [[1, 2, 3], [4, 5, 6]])
    c5, c40, c100, c41 = centre(5), centre(40), centre(100), centre(41)
    nan, inf = float("nan"), float("inf")
    qp = [300.5, 200.25]
    m = [  # (kpts_db, kpts_q, conf, row, mask, reason); rows: 0 = (query 0, image 0), 1 = (query 0, image 1), 2 = (query 1, image 0)
        (c5, qp, 0.5, 0, 1, O.FUSED),                 # 0: (query 0, point 0); loses to match 2
        (c5, qp, 0.9, 0, 0, O.MASKED),                # 1: would win, but masked
        (c5, [1.0, 2.0], 0.7, 0, 1, O.KEPT),          # 2: (query 0, point 0)
        ([nan, 3.0], qp, 0.5, 0, 1, O.NONFINITE),     # 3
        (c5, [inf, 3.0], 0.5, 0, 1, O.NONFINITE),     # 4: the query point counts too
        (c5, qp, nan, 0, 1, O.NONFINITE),             # 5
        (c5, qp, -0.25, 0, 1, O.NEG_CONF),            # 6
        ([-0.5, 3.0], qp, 0.5, 0, 1, O.OUTSIDE),      # 7
        ([3.0, 38.0], qp, 0.5, 0, 1, O.OUTSIDE),      # 8: y = H is the first row outside
        (c41, qp, 0.5, 0, 1, O.NO_KEYPOINT),          # 9
        (c40, qp, 0.5, 0, 1, O.NO_POINT),             # 10
        (c100, [-20.0, 5000.0], -0.0, 0, 1, O.FUSED),  # 11: (query 0, point 1): -0.0 is not negative and the query point needs no grid, but 12 wins
        (c5, qp, 0.7, 1, 1, O.KEPT),                  # 12: (query 0, point 1) through image 1: the smaller index of the tie with 13
        (c5, qp, 0.7, 1, 1, O.FUSED),                 # 13
        (c100, qp, 0.1, 2, 1, O.KEPT),                # 14: point 1 for ANOTHER query
        (c5, qp, 0.1, 2, 1, O.KEPT),                  # 15: (query 1, point 0)
    ]
    want = [r for *_, r in m]
    q = make_queries([x[0] for x in m], [x[1] for x in m], [x[2] for x in m], [x[3] for x in m], [0, 1, 0], [0, 0, 1], 2, [x[4] for x in m])
    counts = dict(kept=4, bad_row=0, masked=1, nonfinite=3, negative_conf=1, outside=2, no_keypoint=1, no_point=1, fused=3)
    kept = dict(match=[2, 12, 14, 15], point=[0, 1, 1, 0], q_ids=[0, 0, 1, 1], q_offsets=[0, 2, 4],
                pts3d=[[1, 2, 3], [4, 5, 6], [4, 5, 6], [1, 2, 3]], conf=[0.7, 0.7, 0.1, 0.1])
    return dict(model=model, q=q), want, counts, kept


# ---- binary-search edges ----------------------------------------------------------------------------------------------------------------
def edge_case():
    """Images: 0 without a keypoint, 1 with one (cell 7), 2 with cells 3, 9, 20, 512 (the grid's last), 3 with cell 10, 4 without, 5 with
    cells 0 and 10.  Every keypoint has its own point.  -> (case, expected reason per match)."""
    model = make_model([[], [7], [3, 9, 20, 512], [10], [], [0, 10]], list(range(8)), np.arange(24).reshape(8, 3))
    probes = [  # (image, cell, reason)
        (0, 7, O.NO_KEYPOINT),        # an image with no keypoint, first in the model
        (4, 10, O.NO_KEYPOINT),       # ... and between two others: cell 10 is held by BOTH neighbours (images 3 and 5)
        (1, 7, O.KEPT), (1, 6, O.NO_KEYPOINT), (1, 8, O.NO_KEYPOINT),          # one keypoint: hit, below, above
        (2, 3, O.KEPT), (2, 512, O.KEPT),                                       # first and last cell of a range
        (2, 2, O.NO_KEYPOINT), (2, 10, O.NO_KEYPOINT), (2, 19, O.NO_KEYPOINT), (2, 21, O.NO_KEYPOINT),   # before, between, after
        (2, 7, O.NO_KEYPOINT),        # held by the previous image only
        (2, 10, O.NO_KEYPOINT),       # held by the next image only
        (3, 10, O.KEPT), (3, 512, O.NO_KEYPOINT), (3, 0, O.NO_KEYPOINT),        # cell 512 ends the previous image, cell 0 starts image 5
        (5, 0, O.KEPT), (5, 10, O.KEPT), (5, 512, O.NO_KEYPOINT),
    ]
    rows = list(range(len(probes)))
    q = make_queries([centre(c, (0.01, 0.99)) for _, c, _ in probes], [[10.0 * i, 5.0] for i in rows], [0.5] * len(rows), rows,
                     [im for im, _, _ in probes], [0] * len(rows), 1)
    return dict(model=model, q=q), [r for _, _, r in probes]


# ---- table stress ---------------------------------------------------------------------------------------------------------------------------
def same_key_case(n=4096):
    """n candidates of ONE (query, point) with equal confidence: the smallest index must win."""
    model = make_model([[5]], [0], [[1, 2, 3]])
    q = make_queries([centre(5)] * n, np.arange(2 * n).reshape(n, 2), [0.5] * n, [0] * n, [0], [0], 1)
    return dict(model=model, q=q)


def key_bits_case(vary, n=1500):
    """Keys that differ only in the query bits (vary = 'query': n queries of one row each, all reaching point 0) or only in the point
    bits (vary = 'point': one query and one row, n keypoints with a point each); every key comes twice, the later one more confident."""
    if vary == "query":
        model = make_model([[5]], [0], [[1, 2, 3]])
        pos, rows = [centre(5)] * (2 * n), np.repeat(np.arange(n), 2)
        conf = np.tile([0.25, 0.5], n)
        return dict(model=model, q=make_queries(pos, np.arange(4 * n).reshape(2 * n, 2), conf, rows, [0] * n, list(range(n)), n))
    hw = (80.0, 80.0)                                                    # a 40 x 40 grid
    model = make_model([list(range(n))], list(range(n)), np.arange(3 * n).reshape(n, 3), hw=hw)
    pos = [centre(c, gw=40) for c in range(n)] * 2
    return dict(model=model, q=make_queries(pos, np.arange(4 * n).reshape(2 * n, 2), [0.25] * n + [0.5] * n, [0] * (2 * n), [0], [0], 1))


def empty_queries_case(Q):
    """Q queries of which only a few have rows: the first, the last and stretches in the middle stay empty."""
    rng = np.random.default_rng(Q)
    model = make_model([[5, 9, 30], [9, 11]], [0, 1, 2, 1, 3], rng.standard_normal((4, 3)))
    busy = sorted({Q // 3, Q // 2, Q - 2} & set(range(1, Q - 1))) if Q > 2 else ([0] if Q == 1 else [])
    row_query = [q for q in busy for _ in range(2)]
    row_db = [0, 1] * len(busy)
    kd, kq, conf, rows = [], [], [], []
    for r, d in enumerate(row_db):
        for c in ((5, 9, 30, 31) if d == 0 else (9, 11, 12)):
            kd.append(centre(c)); kq.append(rng.uniform(0, 500, 2)); conf.append(rng.choice([0.5, 0.75])); rows.append(r)
    return dict(model=model, q=make_queries(kd, kq, conf, rows, row_db, row_query, Q))


def prefix(case, M):
    """The first M matches of a case (same rows, same model)."""
    q = case["q"]
    sub = {k: (None if q[k] is None else q[k][:M]) for k in ("kpts_db", "kpts_q", "conf", "rows", "mask")}
    return dict(model=case["model"], q=dict(q, **sub))


def tiled(case, M):
    """A case of exactly M matches: the matches of `case` repeated row block after row block (rows and queries keep ascending)."""
    q = case["q"]
    m0, R, Q = len(q["conf"]), len(q["row_db"]), q["Q"]
    reps = -(-M // m0)
    t = lambda a: np.concatenate([a] * reps)[:M]
    rows = np.concatenate([q["rows"] + i * R for i in range(reps)])[:M].astype(np.int32)
    row_query = np.concatenate([q["row_query"] + i * Q for i in range(reps)]).astype(np.int32)
    return dict(model=case["model"], q=dict(kpts_db=t(q["kpts_db"]), kpts_q=t(q["kpts_q"]), conf=t(q["conf"]), rows=rows,
                                             mask=None if q["mask"] is None else t(q["mask"]), row_db=np.concatenate([q["row_db"]] * reps),
                                             row_query=row_query, Q=Q * reps))


# ---- runners: one form for the host routine, the kernels and the oracle ---------------------------------------------------------------------
def _trim(out):
    C = int(out["counts"][0])
    res = {k: (out[k][:C] if k not in ("q_offsets", "match_reason") else out[k]) for k in FIELDS}
    res["counts"] = [int(v) for v in out["counts"]]
    return res


def run_host(case):
    from loftr_amd import ops
    m, q = case["model"], case["q"]
    inv, gh, gw = O.grid(m["image_hw"], m["cell_px"])
    cell, status = ops.model_cells_host(m["kp_offsets"], m["keypoints"], m["kp_point"], len(m["xyz"]), gh, gw, float(inv))
    assert status == 0, status
    return _trim(ops.model_lookup_host(m["kp_offsets"], cell, m["kp_point"], m["xyz"], gh, gw, float(inv), q["kpts_db"], q["kpts_q"], q["conf"],
                                       q["rows"], q["mask"], q["row_db"], q["row_query"], q["Q"]))


def run_gpu(case, timings=None):
    import torch
    from loftr_amd import ops
    m, q = case["model"], case["q"]
    inv, gh, gw = O.grid(m["image_hw"], m["cell_px"])
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    mo = [dev(m[k]) for k in ("kp_offsets", "keypoints", "kp_point", "xyz")]
    cell, status = ops.model_cells(mo[0], mo[1], mo[2], len(m["xyz"]), gh, gw, float(inv))
    out = ops.model_lookup(mo[0], cell, mo[2], mo[3], gh, gw, float(inv), *[dev(q[k]) for k in ("kpts_db", "kpts_q", "conf", "rows", "mask",
                                                                                                 "row_db", "row_query")], q["Q"], timings=timings)
    assert int(status.cpu()) == 0
    return _trim({k: v.cpu().numpy() for k, v in out.items()})


def run_oracle(case):
    return O.lookup(case["model"], case["q"])


def assert_same(got, want, what):
    """got: a runner's dict; want: another runner's dict or the oracle's."""
    for k in FIELDS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w), (what, k)
    if isinstance(want["counts"], dict):                                 # the oracle's
        c = got["counts"]
        assert c[0] == want["C"] and c[3] == 0 and c[1] == c[2] == 0 and not any(c[13:]), (what, c)
        assert {name: c[4 + i] for i, name in enumerate(O.REASONS)} == want["counts"], (what, c, want["counts"])
        assert sum(c[4:13]) == len(got["match_reason"]), (what, c)
    else:
        assert got["counts"] == want["counts"], (what, got["counts"], want["counts"])


# ---- the localisation scene -----------------------------------------------------------------------------------------------------------------
N_QUERIES = 8


@functools.lru_cache(maxsize=None)
def query_scene(seed=17):
    """Eight query cameras drawn like the cameras of sfm_scene() (f in [450, 650], principal point (800, 600), up to 8 degrees about a
    random axis, centres on the 4-unit baseline), each matched against all five database images: row (q, d) holds the 60 points, the
    database side at the atlas's snapped positions, the query side snapped to 2 px cell centres.
    -> dict(K [8,3,3], T [8,4,4], rows = [(q, d, kpts_db, kpts_q, conf)], px_q)."""
    s = TC.sfm_scene()
    rng = np.random.default_rng(seed)
    cams = [TC.camera(rng.uniform(450, 650), (rng.uniform(-2, 2), rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)),
                      TC.rotation(rng.standard_normal(3), rng.uniform(0, 8)), pp=(800.0, 600.0)) for _ in range(N_QUERIES)]
    K, T = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    snap = lambda p: (np.floor(p / TC.SFM_CELL) * TC.SFM_CELL + TC.SFM_CELL / 2).astype(np.float32)
    px_q = [snap(np.stack([TC.project(K[q], T[q], x) for x in s["X"]])) for q in range(N_QUERIES)]
    rows = [(q, d, s["px"][d], px_q[q], rng.uniform(0.5, 1.0, len(s["X"])).astype(np.float32)) for q in range(N_QUERIES) for d in range(5)]
    return dict(K=K, T=T, rows=rows, px_q=px_q)


def build_model(device):
    """sfm_scene() -> atlas -> triangulate (default 4 px) -> LocalizationModel on `device`; -> (model, sfm, pts)."""
    from loftr_amd import LocalizationModel
    s = TC.sfm_scene()
    sfm = TC.run_atlas(device)
    pts = sfm.triangulate(s["K"], s["T"])
    return LocalizationModel.from_atlas(sfm, pts), sfm, pts


def localize_scene(model, rows_per_add=5):
    """query_scene() through QueryLocalizer on the model's device, `rows_per_add` rows per add -> QueryLocalizer (before solve)."""
    import torch
    from loftr_amd import QueryLocalizer
    qs = query_scene()
    loc = QueryLocalizer(model, N_QUERIES)
    rows = qs["rows"]
    for i in range(0, len(rows), rows_per_add):
        chunk = rows[i:i + rows_per_add]
        t = lambda j, dt: torch.from_numpy(np.concatenate([r[j] for r in chunk]).astype(dt)).to(model.device)
        bids = torch.from_numpy(np.repeat(np.arange(len(chunk)), [len(r[4]) for r in chunk])).to(model.device)
        loc.add([r[0] for r in chunk], [r[1] for r in chunk], {"mkpts0_f": t(3, np.float32), "mkpts1_f": t(2, np.float32),
                                                               "mconf": t(4, np.float32), "m_bids": bids}, db_side=1)
    return loc


def scene_as_case(model):
    """query_scene() and a LocalizationModel as the dicts the oracle takes."""
    qs = query_scene()
    rows = qs["rows"]
    m = dict(kp_offsets=model.kp_offsets.cpu().numpy(), keypoints=model.keypoints.cpu().numpy(), kp_point=model.kp_point.cpu().numpy(),
             xyz=model.xyz.cpu().numpy(), image_hw=model.image_hw, cell_px=model.cell_px)
    q = make_queries(np.concatenate([r[2] for r in rows]), np.concatenate([r[3] for r in rows]), np.concatenate([r[4] for r in rows]),
                     np.repeat(np.arange(len(rows)), [len(r[4]) for r in rows]), [r[1] for r in rows], [r[0] for r in rows], N_QUERIES)
    return dict(model=m, q=q)


# ---- accuracy of the localised poses ----------------------------------------------------------------------------------------------------------
def accuracy_figures(res, want):
    """Per query: (inliers, rotation error, centre error) of the model's pose and of the same estimator on the same correspondences
    with the ground-truth points in place of the triangulated ones."""
    from loftr_amd.evaluation import absolute_pose_error, estimate_absolute_pose_native
    s, qs = TC.sfm_scene(), query_scene()
    # ground truth of a correspondence: the scene point whose snapped projection in the query image is the correspondence's query point
    rows = []
    for q in range(N_QUERIES):
        sl = slice(int(want["q_offsets"][q]), int(want["q_offsets"][q + 1]))
        index = {tuple(p): i for i, p in enumerate(qs["px_q"][q].tolist())}
        X_gt = np.array([s["X"][index[tuple(p)]] for p in want["kpts"][sl].tolist()])
        R, t, inl = estimate_absolute_pose_native(X_gt, want["kpts"][sl], qs["K"][q], 3.0, 0.999, 0)
        base = absolute_pose_error(qs["T"][q], R, t)
        got = absolute_pose_error(qs["T"][q], res.R[q].numpy(), res.t[q].numpy())
        rows.append(dict(q=q, n=int(res.n_inliers[q]), R_err=got[0], c_err=got[1], n_gt=int(inl.sum()), R_gt=base[0], c_gt=base[1]))
    return rows


def accuracy_report(rows):
    lines = ["localisation against the triangulated model (tests/_model_lookup_cases.py query_scene(): 8 query cameras x 5 database rows x 60",
             "points of sfm_scene(), 2 px cells, triangulation at 4 px, estimator at 3 px / 0.999 / seed 0); baseline = the same estimator on the same",
             "correspondences with the ground-truth points; required: rotation and centre error <= 2 x the baseline's",
             "query  inliers  rot_deg   centre    | baseline: inliers  rot_deg   centre    | ratio rot  centre"]
    for r in rows:
        lines.append(f"{r['q']:5d}  {r['n']:7d}  {r['R_err']:.5f}  {r['c_err']:.6f}  |           {r['n_gt']:7d}  {r['R_gt']:.5f}  {r['c_gt']:.6f}  |"
                     f"     {r['R_err'] / r['R_gt']:5.2f}  {r['c_err'] / r['c_gt']:6.2f}")
    rr, rc = [r["R_err"] / r["R_gt"] for r in rows], [r["c_err"] / r["c_gt"] for r in rows]
    lines.append(f"ratio of the rotation error: median {np.median(rr):.2f}, worst {max(rr):.2f}; of the centre error: median {np.median(rc):.2f}, worst {max(rc):.2f}")
    return "\n".join(lines)
