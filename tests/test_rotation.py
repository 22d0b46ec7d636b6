"""CPU checks of rotation averaging over the view graph (loftr_amd/rotations.py, csrc/rotation.hip): the host routine against
the independent numpy oracle (tests/_rotation_oracle.py), the gauge and the edges of the rule, planted outliers, averaging against
chaining, invariance under a permutation and a reversal of the edges, duplicates, invalid edges, two components, every error bit, and
the chain SfmResult.rotation_averaging -> without_rows -> reconstruct(rotations=True) on a pair list with one wrongly matched row."""
import math
import os

import numpy as np
import pytest
import torch

import _rotation_cases as RC
import _rotation_oracle as RO
import loftr_amd
from loftr_amd import _lib, build as build_mod, ops, rotations
from loftr_amd.evaluation import global_rotation_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTS = ("in_graph", "edge_state", "support", "tree", "edge_use")
# Host routine against the oracle's dense-solve leg, conjugate gradients tightened (pcg_tol = 1e-12, 500 iterations) so that the solver
# is not what differs.  MEASURED: the largest distance over ORACLE_SCENES; the assertion allows ten times that (numpy sums in another
# order).  Anything above 1e-6 would be another algorithm, not rounding.
MEASURED_R, MEASURED_CHORD = 1.4e-15, 1.4e-15            # measured 1.33e-15 (R) and 1.33e-15 (edge_chord); profiles/rotation_accuracy.txt
TOL_R, TOL_CHORD = 10 * MEASURED_R, 10 * MEASURED_CHORD
TIGHT = dict(pcg_iters=500, pcg_tol=1e-12)
MAX_ERR_DEG = 10.0


@pytest.fixture(scope="module", autouse=True)
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def oracle_scenes():
    return RC.outlier_scenes() + RC.chain_scenes() + [RC.hub_scene(), RC.two_components(), RC.with_duplicates(RC.make_scene("d", 20, 3, 5))[0]]


ORACLE_SCENES = oracle_scenes()


@pytest.fixture(scope="module")
def oracle_runs():
    """The oracle's dense leg on every scene, computed once and shared."""
    return {sc.name: RO.average(*sc.args, solver="dense") for sc in ORACLE_SCENES}


def counts_of(rot):
    return [0 if k == "error_bits" else rot.stats[k] for k in ops.ROTATION_NAMES]


def err_deg(chord):
    return np.degrees(2.0 * np.arcsin(np.clip(chord / 2.0, 0.0, 1.0)))


@pytest.mark.parametrize("sc", ORACLE_SCENES, ids=[s.name for s in ORACLE_SCENES])
def test_host_routine_against_the_oracle(sc, oracle_runs):
    want = oracle_runs[sc.name]
    got = loftr_amd.average_rotations(*sc.args, **TIGHT)
    host = got.to_host()
    for k in INTS:
        assert np.array_equal(host[k], want[k]), (sc.name, k)
    skip = ops.ROTATION_NAMES.index("n_pcg_iters")                        # (the dense leg runs no conjugate gradients)
    assert [c for i, c in enumerate(counts_of(got)) if i != skip] == [c for i, c in enumerate(want["counts"]) if i != skip]
    m, j = want["in_graph"], ~np.isnan(want["edge_chord"])
    d_R, d_chord = np.abs(host["R"][m] - want["R"][m]).max(), np.abs(host["edge_chord"][j] - want["edge_chord"][j]).max()
    print(f"{sc.name}: max |R - oracle| = {d_R:.3e}, max |chord - oracle| = {d_chord:.3e}")
    assert np.isnan(host["R"][~m]).all() and np.isnan(host["edge_chord"][~j]).all()
    assert d_R <= TOL_R and d_chord <= TOL_CHORD, (sc.name, d_R, d_chord)
    for k, (a, b) in enumerate(zip((got.stats[n] for n in ops.ROTATION_INFO), want["info"])):
        assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (sc.name, ops.ROTATION_INFO[k], a, b)
    # the other leg: the same conjugate gradients at the defaults; every count, the iterations included
    want = RO.average(*sc.args, solver="pcg")
    got = loftr_amd.average_rotations(*sc.args)
    assert counts_of(got) == want["counts"], sc.name
    assert np.abs(got.R.numpy()[m] - want["R"][m]).max() <= TOL_R
    assert np.array_equal(got.edge_state.numpy(), want["edge_state"])


def test_noise_free_graph():
    sc = RC.make_scene("exact", 25, 3, 7, chords=6, noise_deg=0.0)
    rot = loftr_amd.average_rotations(*sc.args)
    assert bool(rot.edge_ok.all()) and rot.stats["n_iters"] == 1 and rot.stats["status_name"] == "converged"
    assert rot.stats["last_step"] < 1e-12 and rot.stats["max_ok_chord"] < 1e-12
    assert float(global_rotation_errors(rot.R, sc.R_gt).max()) < math.degrees(1e-12)
    G = sc.R_gt[rot.root]                                                  # the gauge: R[root] = I, so R_i = R_gt_i R_gt_root^T
    assert np.abs(rot.R.numpy() - sc.R_gt @ G.T).max() < 1e-12


def test_gauge_and_the_edges_of_the_rule():
    sc = RC.chain_scenes()[0]
    rot = loftr_amd.average_rotations(*sc.args)
    assert rot.R[rot.root].numpy().tobytes() == np.eye(3).tobytes()
    forced = loftr_amd.average_rotations(*sc.args, root=3)
    assert forced.root == 3 and forced.R[3].numpy().tobytes() == np.eye(3).tobytes()
    # max_iters = 0: the start values along the tree, which the oracle chains with matrices
    start = loftr_amd.average_rotations(*sc.args, max_iters=0)
    want = RO.average(*sc.args)
    assert start.stats["n_iters"] == 0 and start.stats["status_name"] == "max_iters" and start.stats["cost_start"] == start.stats["cost_end"]
    assert np.abs(start.R.numpy() - want["R_start"]).max() <= TOL_R and np.array_equal(start.tree.numpy(), want["tree"])
    # nothing to do
    none = loftr_amd.average_rotations(np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)), np.zeros(0, np.int32), 1)
    assert none.stats["status_name"] == "nothing" and none.root == 0 and none.R.numpy().tobytes() == np.eye(3)[None].tobytes()
    assert none.in_graph.tolist() == [True] and none.stats["n_components"] == 1
    none = loftr_amd.average_rotations(np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)), np.zeros(0, np.int32), 4)
    assert none.stats["status_name"] == "nothing" and none.in_graph.tolist() == [True, False, False, False] and bool(torch.isnan(none.R[1:]).all())
    none = loftr_amd.average_rotations(np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)), np.zeros(0, np.int32), 0)
    assert none.stats["status_name"] == "nothing" and none.root == -1 and none.R.shape == (0, 3, 3)


OUTLIERS = RC.outlier_scenes()


@pytest.mark.parametrize("sc", OUTLIERS, ids=[s.name for s in OUTLIERS])
def test_planted_outliers(sc, oracle_runs):
    assert 5 <= sc.n <= 64 and sc.planted.any()
    # the condition, on the oracle alone: good edges below half of the threshold, planted ones above twice it
    o = oracle_runs[sc.name]
    e = err_deg(o["edge_chord"])
    print(f"{sc.name}: oracle good edges <= {e[~sc.planted].max():.2f} deg, planted >= {e[sc.planted].min():.2f} deg")
    assert e[~sc.planted].max() < MAX_ERR_DEG / 2 and e[sc.planted].min() > 2 * MAX_ERR_DEG
    rot = loftr_amd.average_rotations(*sc.args)
    assert np.array_equal((rot.edge_state == 3).numpy(), sc.planted) and np.array_equal(rot.edge_ok.numpy(), ~sc.planted)
    assert not (rot.tree.numpy() & sc.planted).any()
    deg = rot.edge_err_deg.numpy()
    assert deg[~sc.planted].max() < MAX_ERR_DEG < deg[sc.planted].min()


CHAINS = RC.chain_scenes()


@pytest.mark.parametrize("sc", CHAINS, ids=[s.name for s in CHAINS])
def test_averaging_beats_chaining(sc, oracle_runs):
    o = oracle_runs[sc.name]
    tree_o, avg_o = (float(global_rotation_errors(o[k], sc.R_gt).max()) for k in ("R_start", "R"))
    assert tree_o >= 2 * avg_o                                            # the condition, on the oracle alone
    start, rot = loftr_amd.average_rotations(*sc.args, max_iters=0), loftr_amd.average_rotations(*sc.args)
    tree, avg = (float(global_rotation_errors(r.R, sc.R_gt).max()) for r in (start, rot))
    print(f"{sc.name}: largest error to the truth {tree:.2f} deg (tree) -> {avg:.2f} deg (averaged)")
    assert avg < tree and rot.stats["cost_end"] < rot.stats["cost_start"]


def test_permutation_and_reversal_leave_the_verdict():
    sc = RC.outlier_scenes()[2]
    base = loftr_amd.average_rotations(*sc.args)
    E = sc.edge_weight.shape[0]
    perm = np.random.default_rng(3).permutation(E)
    im, R = sc.edge_image[perm].copy(), sc.edge_R[perm].copy()
    flip = np.arange(E) % 3 == 0                                           # every third edge stored as (b, a, R^T)
    im[flip] = im[flip][:, ::-1]
    R[flip] = np.transpose(R[flip], (0, 2, 1))
    rot = loftr_amd.average_rotations(im, R, sc.edge_weight[perm], sc.n)
    assert np.array_equal(rot.support.numpy(), base.support.numpy()[perm])
    assert np.array_equal(rot.edge_state.numpy(), base.edge_state.numpy()[perm])
    back = np.zeros(E, bool)
    back[perm] = rot.tree.numpy()                                          # the tree, mapped back through the permutation
    assert np.array_equal(back, base.tree.numpy())
    assert rot.root == base.root and np.abs(rot.R.numpy() - base.R.numpy()).max() < 1e-9


def test_duplicates_the_heavier_is_used_and_both_are_judged():
    base = RC.make_scene("d", 20, 3, 5)
    sc, idx = RC.with_duplicates(base)
    E0 = base.edge_weight.shape[0]
    rot = loftr_amd.average_rotations(*sc.args)
    use = rot.edge_use.numpy()
    heavier_second = sc.edge_weight[E0:] > sc.edge_weight[idx]
    assert heavier_second.any() and (~heavier_second).any()
    assert np.array_equal(use[E0:], heavier_second) and np.array_equal(use[idx], ~heavier_second)
    assert rot.stats["n_duplicate"] == idx.size and rot.stats["n_used"] == E0
    assert bool((rot.edge_state == 2).all()) and not bool(torch.isnan(rot.edge_chord).any())
    assert not (rot.tree.numpy() & ~use).any() and not rot.support.numpy()[~use].any()
    tie = sc.edge_weight.copy()
    tie[E0:] = tie[idx]                                                   # equal weights: the lowest index
    rot = loftr_amd.average_rotations(sc.edge_image, sc.edge_R, tie, sc.n)
    assert rot.edge_use.numpy()[idx].all() and not rot.edge_use.numpy()[E0:].any()


def test_invalid_edges_are_no_error():
    sc = RC.make_scene("inv", 14, 3, 9)
    R, w = sc.edge_R.copy(), sc.edge_weight.copy()
    R[0] = 0.0                                                            # what pairwise_poses leaves for a refused model
    R[5, 1, 2] = np.nan
    R[9] = R[9] @ np.diag([1.0, 1.0, -1.0])                               # a reflection
    R[13] = 1.1 * R[13]
    w[17] = 0
    bad = [0, 5, 9, 13, 17]
    rot = loftr_amd.average_rotations(sc.edge_image, R, w, sc.n)
    assert rot.stats["n_invalid"] == 5 and rot.edge_state[bad].tolist() == [0] * 5 and bool(torch.isnan(rot.edge_chord[bad]).all())
    assert not rot.edge_use[bad].any() and not rot.tree[bad].any() and rot.support[bad].tolist() == [0] * 5
    rest = np.setdiff1d(np.arange(w.shape[0]), bad)
    assert bool((rot.edge_state[rest] == 2).all()) and bool(rot.in_graph.all())


def test_two_components():
    sc = RC.two_components()
    rot = loftr_amd.average_rotations(*sc.args)
    assert rot.root < 10 and rot.in_graph.tolist() == [True] * 10 + [False] * 6 and rot.stats["n_components"] == 2
    assert bool(torch.isnan(rot.R[10:]).all()) and not bool(torch.isnan(rot.R[:10]).any())
    second = sc.edge_image[:, 0] >= 10
    assert rot.edge_state[second].tolist() == [1] * int(second.sum()) and bool(torch.isnan(rot.edge_chord[second]).all())
    assert bool((rot.edge_state[~second] == 2).all()) and rot.stats["n_tree"] == 14
    other = loftr_amd.average_rotations(*sc.args, root=12)                # the smaller component, when asked for
    assert other.in_graph.tolist() == [False] * 10 + [True] * 6


def test_every_error_bit_raises(monkeypatch):
    sc = RC.make_scene("err", 9, 3, 61)
    texts = dict(ops.ROTATION_ERRORS)
    im = sc.edge_image.copy()
    im[4, 1] = sc.n
    with pytest.raises(ValueError, match="edge_image outside"):
        loftr_amd.average_rotations(im, sc.edge_R, sc.edge_weight, sc.n)
    im = sc.edge_image.copy()
    im[2, 1] = im[2, 0]
    with pytest.raises(ValueError, match="joins an image to itself"):
        loftr_amd.average_rotations(im, sc.edge_R, sc.edge_weight, sc.n)
    for root in (sc.n, -2):
        with pytest.raises(ValueError, match="root outside"):
            loftr_amd.average_rotations(*sc.args, root=root)
    graph = rotations.view_graph

    def shuffled(*a):
        off, adj, use = graph(*a)
        adj = adj.clone()
        adj[[0, 1]] = adj[[1, 0]]
        return off, adj, use
    monkeypatch.setattr(rotations, "view_graph", shuffled)
    with pytest.raises(ValueError, match="group the edges by image"):
        loftr_amd.average_rotations(*sc.args)
    monkeypatch.setattr(rotations, "view_graph", graph)
    assert sorted(texts) == [1, 2, 4, 8]
    for name, args, bit in RC.error_cases():                               # the host routine: the bits, and nothing else written
        out = ops.rotation_averaging_host(*args)
        assert out["counts"][1] & bit and out["counts"].tolist() == [0, int(out["counts"][1])] + [0] * 14, name
        assert all(not np.ascontiguousarray(out[k]).view(np.uint8).any() for k in out if k != "counts"), name
    for kw in (dict(loss_deg=0.0), dict(cycle_deg=-1.0), dict(max_err_deg=200.0), dict(pcg_tol=1.0), dict(max_iters=-1), dict(pcg_iters=1.5)):
        with pytest.raises(ValueError):
            loftr_amd.average_rotations(*sc.args, **kw)
    with pytest.raises(ValueError, match="must hold integers"):
        loftr_amd.average_rotations(sc.edge_image, sc.edge_R, sc.edge_weight.astype(np.float32), sc.n)


class _FakeGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: enough for the device check, which runs before any data is touched."""
    @property
    def is_cuda(self):
        return True


def test_mixed_devices_are_an_error():
    sc = RC.make_scene("mix", 6, 2, 1)
    tensors = [torch.from_numpy(x) for x in sc.args[:3]]
    for i in range(3):
        mixed = list(tensors)
        mixed[i] = tensors[i].as_subclass(_FakeGpu)
        with pytest.raises(_lib.LoftrHipError, match="GPU and CPU arguments mixed.*no silent fallback"):
            loftr_amd.average_rotations(*mixed, sc.n)


def test_global_rotation_errors_removes_the_free_rotation():
    rng = np.random.default_rng(2)
    R_gt = np.stack([RC.random_rotation(rng) for _ in range(7)])
    G = RC.random_rotation(rng)
    R = R_gt @ G.T
    assert float(global_rotation_errors(R, R_gt).max()) < 1e-6
    R[3] = RC.rot_from_quat([math.cos(math.radians(4.0)), math.sin(math.radians(4.0)), 0.0, 0.0]) @ R[3]   # 8 degrees
    mask = np.arange(7) != 3
    e = global_rotation_errors(R, R_gt, mask=mask)
    assert math.isnan(float(e[3])) and float(e[mask].max()) < 1e-6
    e = global_rotation_errors(R, R_gt)
    assert 6.0 < float(e[3]) < 8.0 and float(e[mask].max()) < 2.0
    R[5] = np.nan
    assert math.isnan(float(global_rotation_errors(R, R_gt)[5]))


# ---- the chain: a pair list with one wrongly matched row -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def false_row():
    return RC.false_row_atlas("cpu")


def test_rotation_averaging_rejects_the_false_row(false_row):
    sfm, s = false_row
    _, _, ninl = sfm.pairwise_poses(s["K"])
    assert int(ninl[RC.FALSE_ROW]) > RC.FALSE_POINTS // 2                  # coherent with a wrong geometry: a majority of the row's matches fits its model
    rot = sfm.rotation_averaging(s["K"])
    assert torch.nonzero(~rot.edge_ok).reshape(-1).tolist() == [RC.FALSE_ROW] and int(rot.edge_state[RC.FALSE_ROW]) == 3
    assert float(rot.edge_err_deg[RC.FALSE_ROW]) > 20.0 and not bool(rot.tree[RC.FALSE_ROW]) and bool(rot.in_graph.all())
    truth = s["T"][:, :3, :3]
    assert float(global_rotation_errors(rot.R, truth).max()) < 3.0           # (2 px cells: the five-point rotations are a degree or two off)


def test_without_rows_regrows_only_what_the_row_touched(false_row):
    sfm, s = false_row
    n_rows = sfm.row_images.shape[0]
    rows_ok = torch.arange(n_rows) != RC.FALSE_ROW
    sfm2, done = sfm.without_rows(rows_ok)
    assert int(sfm.track_ok.sum()) == 60 - RC.FALSE_POINTS                 # the false row made every track it touched inconsistent
    assert bool(sfm2.track_ok.all()) and sfm2.stats["n_rows_removed"] == 1
    off, image, local = sfm2.tracks()
    for t in range(off.numel() - 1):                                       # only consistent tracks
        ims = image[off[t]:off[t + 1]].tolist()
        assert len(set(ims)) == len(ims)
    members = lambda r, ok=None: {frozenset(np.nonzero(r.track_id.numpy() == t)[0].tolist())
                                  for t in range(r.track_len.numel()) if ok is None or bool(ok[t])}
    assert members(sfm, sfm.track_ok) <= members(sfm2)                     # the tracks the row never touched keep their members
    assert len(members(sfm2)) == 60 and all(len(m) == 5 for m in members(sfm2))
    per_row = (sfm2.row_offsets[1:] - sfm2.row_offsets[:-1]).tolist()
    assert per_row[RC.FALSE_ROW] == 0 and sum(per_row) == sfm2.matches.shape[0] == sfm.matches.shape[0] - RC.FALSE_POINTS
    assert sfm.track_id.numel() == sfm2.track_id.numel() and int(sfm.track_ok.sum()) == 60 - RC.FALSE_POINTS       # the input is left untouched
    same, _ = sfm.without_rows(torch.ones(n_rows, dtype=torch.bool))      # nothing rejected: the split alone
    assert torch.equal(same.track_id, sfm.split()[0].track_id)
    with pytest.raises(ValueError, match=r"expected rows_ok \[10\]"):
        sfm.without_rows(rows_ok[:5])


def test_reconstruct_with_rotations(false_row):
    sfm, s = false_row
    kw = dict(min_corr=6, min_inliers=6)
    before = sfm.reconstruct(s["K"], **kw)                                 # computed before the keyword is passed anywhere
    rec = sfm.reconstruct(s["K"], rotations=True, **kw)
    assert rec.rotations is not None and rec.stats["rotations"]["n_outlier"] == 1 and rec.sfm is not None and bool(rec.sfm.track_ok.all())
    assert rec.stats["init_row"] != RC.FALSE_ROW and bool(rec.posed.all())
    assert rec.points.stats["n_ok"] > before.points.stats["n_ok"]          # the tracks the false row spoiled are back
    custom = sfm.reconstruct(s["K"], rotations=dict(max_err_deg=8.0), **kw)
    assert custom.stats["rotations"]["max_err_deg"] == 8.0
    after = sfm.reconstruct(s["K"], **kw)                                  # the default is unchanged, bit for bit
    assert after.rotations is None and "rotations" not in after.stats
    assert after.T_cam_from_world.numpy().tobytes() == before.T_cam_from_world.numpy().tobytes()
    assert after.points.xyz.numpy().tobytes() == before.points.xyz.numpy().tobytes() and after.stats["init_row"] == before.stats["init_row"]
