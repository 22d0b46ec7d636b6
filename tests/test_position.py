"""Global positioning, CPU side: the host routine loftr_global_positions_host against the independent numpy oracle
(tests/_position_oracle.py), against ground truth, and through SfmResult.reconstruct_global.  The kernels are compared with the host
routine bit for bit in tests/test_hip_position.py."""
import functools

import numpy as np
import pytest
import torch

import _position_cases as PC
import _position_oracle as PO
import _rotation_cases as RC
import loftr_amd
from loftr_amd import evaluation, ops_global, positions

# Host routine against the oracle's conjugate-gradient leg (the same rule in numpy: dense blocks, numpy sums in another order).
# MEASURED: the largest distance over ORACLE_SCENES and the further cases (profiles/position_accuracy.txt); the assertions allow ten
# times that.  xyz is fp32: a double that moves by 1e-14 can cross a rounding boundary, so one unit in the last place at |x| < 4.
MEASURED_C, MEASURED_D = 5.3e-14, 4.0e-15               # measured 5.24e-14 (centres) and 4.00e-15 (depth_scale)
TOL_C, TOL_D, TOL_XYZ = 10 * MEASURED_C, 10 * MEASURED_D, 2.0 ** -22
# Noise-free scenes with exact rotations: the largest centre error of the ORACLE after a similarity, measured 8.13e-8 on the ring and
# 1.24e-7 on the line (pixels are stored in fp32, and the refinement ends on ftol = 1e-7, not at the minimum); ten times the larger one.
MEASURED_EXACT = 1.3e-7
TOL_EXACT = 10 * MEASURED_EXACT


@functools.lru_cache(maxsize=None)
def scene(name):
    return {"small": PC.small, "ring": PC.ring, "line": PC.line, "exact_ring": lambda: PC.exact("ring"), "exact_line": lambda: PC.exact("line"),
            **{s.name: (lambda s=s: s) for s in PC.further_cases()}}[name]()


@functools.lru_cache(maxsize=None)
def oracle(name, solver="pcg"):
    return PO.positions(*scene(name).args, solver=solver)


@functools.lru_cache(maxsize=None)
def host(name):
    return positions.global_positions(*scene(name).args)


def counts_of(got):
    return [0 if k == "error_bits" else got.stats[k] for k in ops_global.POSITION_NAMES]


def centre_error(centres, sc, state):
    idx = np.nonzero(state > 0)[0]
    return PO.align_error(np.asarray(centres)[idx], sc.c_gt[idx])


ORACLE_SCENES = ("small", "ring", "line", "exact_ring", "exact_line", "no_observations", "one_usable", "outside_graph", "no_direction")


@pytest.mark.parametrize("name", ORACLE_SCENES)
def test_host_routine_against_the_oracle(name):
    got, want = host(name), oracle(name)
    g = got.to_host()
    assert counts_of(got) == want["counts"][:13], name                     # every count, the trials and the iterations included
    for k in ("obs_state", "cam_state", "point_active"):
        assert np.array_equal(g[k], want[k]), (name, k)
    m, a = g["cam_state"] > 0, g["point_active"]
    assert np.isnan(g["centres"][~m]).all() and np.isnan(g["xyz"][~a]).all() and not np.isnan(g["centres"][m]).any()
    d_c = np.abs(g["centres"][m] - want["centres"][m]).max()
    d_x = np.abs(g["xyz"][a] - want["xyz"][a]).max()
    d_d = np.abs(g["depth_scale"] - want["depth_scale"]).max()
    print(f"{name}: max |centres - oracle| = {d_c:.3e}, |xyz - oracle| = {d_x:.3e}, |depth_scale - oracle| = {d_d:.3e}")
    assert d_c <= TOL_C and d_d <= TOL_D and d_x <= TOL_XYZ, (name, d_c, d_x, d_d)
    for k, (x, y) in enumerate(zip((got.stats[n] for n in ops_global.POSITION_INFO), want["info"])):
        assert abs(x - y) <= 1e-9 * max(1.0, abs(y)), (name, ops_global.POSITION_INFO[k], x, y)
    assert torch.equal(got.posed, got.cam_state >= 2)
    T = got.T_cam_from_world.numpy()
    R = scene(name).R
    p = g["cam_state"] >= 2
    assert np.isnan(T[~p]).all() and np.array_equal(T[p][:, :3, :3], R[p]) and np.array_equal(T[p][:, 3], np.tile([0, 0, 0, 1.0], (p.sum(), 1)))
    assert np.abs(T[p][:, :3, 3] + np.einsum("nij,nj->ni", R[p], g["centres"][p])).max() <= 1e-14


@pytest.mark.parametrize("name", ("exact_ring", "exact_line"))
def test_noise_free_scene_gives_the_truth(name):
    sc, got, want = scene(name), host(name), oracle(name)
    e_host, e_oracle = centre_error(got.centres.numpy(), sc, got.cam_state.numpy()), centre_error(want["centres"], sc, want["cam_state"])
    print(f"{name}: centre error after a similarity: host {e_host:.3e}, oracle {e_oracle:.3e}")
    assert e_oracle <= MEASURED_EXACT and e_host <= TOL_EXACT
    assert got.stats["n_negative_scale"] == 0 and bool((got.obs_state[got.obs_state > 0] == 1).all())      # d > 0 on every active observation
    assert bool((got.depth_scale[got.obs_state > 0] > 0).all())


@pytest.mark.parametrize("name", ("ring", "line"))
def test_accuracy_against_ground_truth(name):
    """Noise (0.5 px, 0.5 degrees on the rotations) and 7 % gross outliers, on a ring and on a straight line of cameras (the case
    pairwise directions cannot solve): the host routine is at most 1.1 times as far from the truth as the dense oracle."""
    sc, got, dense = scene(name), host(name), oracle(name, "dense")
    e_host, e_dense = centre_error(got.centres.numpy(), sc, got.cam_state.numpy()), centre_error(dense["centres"], sc, dense["cam_state"])
    print(f"{name}: largest centre error after a similarity: host {e_host:.4f}, dense oracle {e_dense:.4f}")
    assert e_host <= 1.1 * e_dense + TOL_C
    assert sc.outlier.sum() >= 0.04 * sc.outlier.size
    # the Huber weights of the planted outliers, from the routine's outputs
    g = got.to_host()
    v = PO.bearings(sc.obs_xy.astype(np.float64), sc.obs_image, sc.K, sc.R)
    track = np.repeat(np.arange(len(sc.offsets) - 1), np.diff(sc.offsets))
    r = v - g["depth_scale"][:, None] * (g["xyz"][track].astype(np.float64) - g["centres"][sc.obs_image])
    nr = np.linalg.norm(r, axis=1)
    weight = np.where(nr <= 0.1, 1.0, 0.1 / np.maximum(nr, 1e-300))
    assert (weight[sc.outlier & (g["obs_state"] > 0)] < 1.0).all()
    assert np.median(weight[~sc.outlier]) == 1.0


def test_renumbering_the_tracks():
    """Tracks in another order: a point's own sums do not move; a camera's list, and with it the order of its osum64, does.  Only the
    rounding of those sums differs (1e-16 relative), carried through a reduced system whose condition stays below 1e6 on this scene."""
    sc = scene("small")
    rng = np.random.default_rng(0)
    perm = rng.permutation(len(sc.offsets) - 1)
    idx = np.concatenate([np.arange(sc.offsets[t], sc.offsets[t + 1]) for t in perm])
    off = np.concatenate([[0], np.cumsum(np.diff(sc.offsets)[perm])]).astype(np.int64)
    a = sc.args
    got = positions.global_positions(off, sc.obs_image[idx], sc.obs_xy[idx], *a[3:])
    ref = host("small")
    assert counts_of(got) == counts_of(ref)
    assert np.abs(got.centres.numpy() - ref.centres.numpy()).max() <= 1e-9
    assert np.abs(got.xyz.numpy() - ref.xyz.numpy()[perm]).max() <= 1e-6 and np.array_equal(got.obs_state.numpy(), ref.obs_state.numpy()[idx])


def test_further_cases():
    got = host("no_observations")                                         # a camera with no observations keeps its place along the tree
    want = oracle("no_observations")
    assert got.cam_state.tolist() == [3, 2, 2, 2, 1] and got.stats["n_chained"] == 1 and not bool(got.posed[4])
    assert np.abs(got.centres.numpy()[4] - want["start"]["centres"][4]).max() <= TOL_C
    got = host("one_usable")                                              # a point with one usable observation is not active
    assert not bool(got.point_active[3]) and got.obs_state[scene("one_usable").offsets[3]:scene("one_usable").offsets[4]].tolist() == [0] * 4
    assert bool(torch.isnan(got.xyz[3]).all()) and got.stats["n_active_points"] == 39
    got = host("outside_graph")                                           # an image outside the graph
    assert got.cam_state.tolist() == [3, 2, 2, 2, 0] and bool(torch.isnan(got.centres[4]).all()) and got.stats["n_in_graph"] == 4
    assert bool((got.obs_state[torch.from_numpy(scene("outside_graph").obs_image == 4)] == 0).all())
    got = host("no_direction")                                            # tree edges with t = 0 or not finite are counted, the call goes on
    assert got.stats["n_tree_no_direction"] == 2 and got.stats["status_name"] == "converged"


def test_no_iterations_returns_the_start_values():
    sc = scene("small")
    got = positions.global_positions(*sc.args, max_iters=0)
    want = oracle("small")["start"]
    assert got.stats["n_trials"] == 0 and got.stats["status_name"] == "max_iters" and got.stats["cost_start"] == got.stats["cost_end"]
    assert np.abs(got.centres.numpy() - want["centres"]).max() <= TOL_C and np.abs(got.depth_scale.numpy() - want["d"]).max() <= TOL_D
    assert np.abs(got.xyz.numpy() - want["X"].astype(np.float32)).max() <= TOL_XYZ
    step = np.linalg.norm(np.diff(got.centres.numpy(), axis=0), axis=1)    # a path: unit steps from the root at 0
    assert np.abs(step - 1.0).max() <= 1e-12 and got.centres[0].tolist() == [0.0, 0.0, 0.0]
    one = positions.global_positions(*sc.args, huber=0.0, max_iters=1)     # the square: every weight is 1
    assert one.stats["n_trials"] == 1
    none = positions.global_positions(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, 2), np.float32), sc.K[:1], sc.R[:1],
                                      np.ones(1, np.uint8), 0, np.zeros((0, 2), np.int32), np.zeros((0, 3)))
    assert none.stats["status_name"] == "nothing" and none.cam_state.tolist() == [3] and none.centres.tolist() == [[0.0, 0.0, 0.0]]


@pytest.mark.parametrize("name,sc,bit", PC.error_cases(), ids=[c[0] for c in PC.error_cases()])
def test_every_error_bit_raises(name, sc, bit):
    text = dict(ops_global.POSITION_ERRORS)[bit]
    with pytest.raises(ValueError) as err:
        positions.global_positions(*sc.args)
    assert text in str(err.value)


def test_error_bits_leave_every_other_output_zero():
    from loftr_amd import _tracks
    sc = scene("small")
    cam_offsets, cam_obs = _tracks.group_by_image(sc.obs_image, sc.n)
    args = [sc.offsets, sc.obs_image, sc.obs_xy, cam_offsets, cam_obs, sc.K, sc.R, sc.in_graph, sc.tree_image, sc.tree_t, sc.root]
    ok = ops_global.global_positions_host(*args)
    assert ok["counts"][1] == 0 and ok["cam_state"].any()
    for name, edit in (("list_swapped", lambda o, c: c.__setitem__([0, 1], c[[1, 0]])), ("list_outside", lambda o, c: c.__setitem__(3, len(c))),
                       ("list_offsets", lambda o, c: o.__setitem__(2, o[2] + 1)), ("list_end", lambda o, c: o.__setitem__(-1, o[-1] - 1))):
        a = list(args)
        a[3], a[4] = cam_offsets.copy(), cam_obs.copy()
        edit(a[3], a[4])
        out = ops_global.global_positions_host(*a)
        assert out["counts"][1] == 4, name                                 # a grouping that is not the stable one
        assert not any(out[k].any() for k in out if k != "counts") and out["counts"].sum() == 4, name
    a = list(args)
    a[1] = sc.obs_image.copy(); a[1][0] = -1
    a[10] = sc.n
    out = ops_global.global_positions_host(*a)
    assert out["counts"][1] & 1 and out["counts"][1] & 8 and not any(out[k].any() for k in out if k != "counts")


def test_mixed_devices_and_bad_arguments_are_errors():
    sc = scene("small")
    with pytest.raises(ValueError, match="pcg_tol"):
        positions.global_positions(*sc.args, pcg_tol=1.0)
    with pytest.raises(ValueError, match="max_iters"):
        positions.global_positions(*sc.args, max_iters=-1)
    with pytest.raises(ValueError, match="must hold integers"):
        positions.global_positions(sc.offsets.astype(np.float64), *sc.args[1:])
    with pytest.raises(loftr_amd._lib.LoftrHipError, match="expected numpy arrays"):
        ops_global.global_positions_host(*[torch.zeros(1)] * 10, 0)
    assert loftr_amd.global_positions is positions.global_positions and loftr_amd.GlobalPositions is positions.GlobalPositions


# ---- the chain: a pair list with one wrongly matched row -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def false_row():
    return RC.false_row_atlas("cpu")


def test_reconstruct_global(false_row):
    sfm, s = false_row
    kw = dict(min_corr=6, min_inliers=6)
    ref = sfm.reconstruct(s["K"], rotations=True, **kw)
    rec = sfm.reconstruct_global(s["K"], **kw)
    assert rec.rotations is not None and torch.nonzero(~rec.rotations.edge_ok).reshape(-1).tolist() == [RC.FALSE_ROW]     # the row is rejected
    assert rec.stats["rows_removed"]["n_tracks"] == 60 and rec.sfm is not None and bool(rec.sfm.track_ok.all())
    in_graph = rec.rotations.in_graph
    assert bool(in_graph.all()) and bool(rec.posed[in_graph].all())        # every image of the root's component ends posed
    assert rec.positions is not None and rec.stats["positions"]["status_name"] == "converged" and rec.stats["positions"]["n_free"] == 4
    assert bool(rec.positions.posed.all()) and rec.round_registered.tolist() == [0] * 5
    root = rec.rotations.root
    assert rec.stats["init"] == (root, None)                               # the adjustments held the root, by name
    assert rec.T_cam_from_world[root].numpy().tobytes() == rec.positions.T_cam_from_world[root].numpy().tobytes()
    T_gt = torch.from_numpy(s["T"])
    rot_g, c_g = evaluation.trajectory_errors(rec.T_cam_from_world, rec.posed, T_gt)
    rot_i, c_i = evaluation.trajectory_errors(ref.T_cam_from_world, ref.posed, T_gt)
    print(f"reconstruct_global: rot {rot_g.max():.4f} deg, centre {c_g.max():.5f}; reconstruct(rotations=True): rot {rot_i.max():.4f} deg, "
          f"centre {c_i.max():.5f}")
    assert rot_g.max() <= 2.0 * rot_i.max() and c_g.max() <= 2.0 * c_i.max()
    assert rec.points.stats["n_ok"] == ref.points.stats["n_ok"] == 60
    with pytest.raises(ValueError, match=r"expected K \[5,3,3\]"):
        sfm.reconstruct_global(s["K"][:4])


def test_global_positions_of_a_pair_list(false_row):
    sfm, s = false_row
    rot = sfm.rotation_averaging(s["K"])
    sfm2, _ = sfm.without_rows(rot.edge_ok | (rot.edge_state < 2))
    pos = sfm2.global_positions(s["K"], rot, max_iters=5)
    assert pos.stats["max_iters"] == 5 and pos.root == rot.root and pos.cam_state[rot.root] == 3
    assert pos.stats["n_tracks"] == 60 and pos.stats["n_tree_no_direction"] == 0
    _, c_err = evaluation.trajectory_errors(pos.T_cam_from_world, pos.posed, torch.from_numpy(s["T"]))
    print(f"pair list, 5 trials: largest centre error after a similarity {c_err.max():.4f} (the cameras span 4 units)")
    assert np.isfinite(c_err).all() and bool(pos.posed.all())             # (recorded, not judged: test_reconstruct_global judges the chain)
    refined = sfm2._relabelled(sfm2.track_id)
    refined.is_refined = True
    with pytest.raises(ValueError, match="refined view"):
        refined.global_positions(s["K"], rot)


def test_reconstruct_tracks_from_a_start_reproduces_the_loop(false_row):
    """reconstruct_tracks(start=...) from the incremental loop's own state after the initial pair: the same result bit for bit."""
    from loftr_amd.registration import reconstruct_tracks
    sfm, s = false_row
    sfm2, _ = sfm.split()
    K = torch.from_numpy(s["K"]).to(torch.float64)
    R, t, ninl = sfm2.pairwise_poses(K)
    row = 0
    a, b = sfm2.row_images[row].tolist()
    offsets, image, local = sfm2.tracks()
    xy = sfm2.keypoints[sfm2.kp_offsets[image] + local]
    kw = dict(min_corr=6, min_inliers=6, thresh_px=4.0)
    ref = reconstruct_tracks(offsets, image.to(torch.int32), xy, K, (a, b, R[row], t[row]), **kw)
    T = torch.full((5, 4, 4), float("nan"), dtype=torch.float64)
    T[a] = torch.eye(4, dtype=torch.float64)
    T[b] = torch.eye(4, dtype=torch.float64)
    T[b, :3, :3], tb = R[row].to(torch.float64), t[row].to(torch.float64)
    T[b, :3, 3] = tb / float(torch.linalg.norm(tb))
    posed = torch.zeros(5, dtype=torch.bool)
    posed[a] = posed[b] = True
    got = reconstruct_tracks(offsets, image.to(torch.int32), xy, K, None, start=(T, posed), **kw)
    assert got.T_cam_from_world.numpy().tobytes() == ref.T_cam_from_world.numpy().tobytes()
    assert got.points.xyz.numpy().tobytes() == ref.points.xyz.numpy().tobytes() and torch.equal(got.posed, ref.posed)
    assert torch.equal(got.round_registered, ref.round_registered) and got.stats["rounds"] == ref.stats["rounds"]
    assert got.stats["init"] == (a, None) and ref.stats["init"] == (a, b)
    named = reconstruct_tracks(offsets, image.to(torch.int32), xy, K, None, start=(T, posed, a), **kw)      # the fixed image by name
    assert named.T_cam_from_world.numpy().tobytes() == ref.T_cam_from_world.numpy().tobytes()
    other = reconstruct_tracks(offsets, image.to(torch.int32), xy, K, None, start=(T, posed, b), **kw)      # another gauge: b stays put
    assert other.T_cam_from_world[b].numpy().tobytes() == T[b].numpy().tobytes()
    assert other.T_cam_from_world[a].numpy().tobytes() != T[a].numpy().tobytes()
    with pytest.raises(ValueError, match="init must be None"):
        reconstruct_tracks(offsets, image.to(torch.int32), xy, K, (a, b, R[row], t[row]), start=(T, posed), **kw)
    unposed = int(torch.nonzero(~posed)[0])
    with pytest.raises(ValueError, match="fixed image of start must be a posed image"):
        reconstruct_tracks(offsets, image.to(torch.int32), xy, K, None, start=(T, posed, unposed), **kw)
    far = T.clone()
    far[b] = torch.eye(4, dtype=torch.float64)                            # both at the origin, looking the same way: nothing triangulates
    with pytest.raises(ValueError, match=r"the 2 posed images of start \(fixed: \d\) triangulate nothing"):
        reconstruct_tracks(offsets, image.to(torch.int32), xy, K, None, start=(far, posed), **kw)
