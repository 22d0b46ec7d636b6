"""Global positioning on the GPU (csrc/position_gpu.hip): every output of the kernels is bit for bit the host routine's, at
the wave and chunk edges of the observation count, of one camera's list and of the camera count (a tree wider and deeper than the
start workgroup), on the further cases of tests/test_position.py, and through the chain of SfmResult.reconstruct_global.  The iteration
limits are small so that the fixed launch schedule stays short."""
import numpy as np
import pytest
import torch

import _position_cases as PC
import _rotation_cases as RC
from loftr_amd import _tracks, ops_global, positions

pytestmark = pytest.mark.gpu

SHORT = dict(max_iters=3, pcg_iters=4, min_cam_obs=1)


def ops_args(sc):
    cam_offsets, cam_obs = _tracks.group_by_image(np.clip(sc.obs_image, 0, sc.n - 1), sc.n)          # (as positions.global_positions does)
    return [np.ascontiguousarray(x) for x in (sc.offsets, sc.obs_image, sc.obs_xy, cam_offsets, cam_obs, sc.K, sc.R, sc.in_graph, sc.tree_image,
                                              sc.tree_t)]


def both(sc, **kw):
    """-> the host routine's outputs; asserts that the kernels give the same bytes in every output."""
    a = ops_args(sc)
    want = ops_global.global_positions_host(*a, sc.root, **kw)
    got = ops_global.global_positions(*[torch.from_numpy(x).cuda() for x in a], sc.root, **kw)
    torch.cuda.synchronize()
    assert list(got) == list(want)
    for k in want:
        assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), (sc.name, k, kw)
    return want


@pytest.mark.parametrize("N", (2, 63, 64, 65, 4095, 4096, 4097))
def test_observation_counts_at_the_wave_and_chunk_edges(N):
    sc = PC.sized(N)
    out = both(sc, **SHORT)
    assert out["counts"][1] == 0 and out["counts"][4] == N and out["counts"][0] >= 1


@pytest.mark.parametrize("count", (1, 64, 65, 4097))
def test_one_camera_list_at_the_wave_edges(count):
    sc = PC.one_camera_list(count)
    out = both(sc, **SHORT)
    assert out["counts"][1] == 0 and out["cam_state"].tolist() == [3, 2, 2] and int((sc.obs_image == 1).sum()) == count


@pytest.mark.parametrize("n,tree", ((2, "path"), (3, "path"), (64, "star"), (65, "path"), (1025, "path"), (1025, "star")))
def test_camera_counts(n, tree):
    """1025 cameras: a path is deeper than the start workgroup has threads, a star wider."""
    sc = PC.many_cameras(n, tree)
    out = both(sc, **SHORT)
    assert out["counts"][1] == 0 and out["counts"][10] == (n - 1 if tree == "path" else 1) and out["counts"][11] == n


@pytest.mark.parametrize("sc", PC.further_cases() + [PC.small(), PC.ring()], ids=lambda s: s.name)
@pytest.mark.parametrize("huber", (0.0, 0.1))
def test_further_cases_and_both_losses(sc, huber):
    both(sc, huber=huber, max_iters=3, pcg_iters=4)
    both(sc, huber=huber, **SHORT)


LARGE = PC.large_further_cases()


@pytest.mark.parametrize("sc", LARGE, ids=lambda s: s.name)
@pytest.mark.parametrize("min_cam_obs", (1, 8))
def test_further_cases_at_the_edge_sizes(sc, min_cam_obs):
    """NaN pixels on every 7th observation, a leaf outside the graph, a camera without observations and two tree edges without a
    direction, at 4097 observations, in a camera list of 4097 and among 1025 cameras (a path and a star): inactive observations and
    cameras that are outside or chained only sit in the middle and at the tail of waves and chunks, the counters run over many waves."""
    out = both(sc, max_iters=5, pcg_iters=4, min_cam_obs=min_cam_obs)
    state = out["cam_state"]
    assert out["counts"][1] == 0 and out["counts"][8] == 2 and state[-1] == 0 and (state == 0).sum() == 1 and (state == 1).sum() >= 1
    assert 0 < out["counts"][4] < len(sc.obs_image) and (out["obs_state"][::7] == 0).all() and not out["point_active"].all()
    assert (out["counts"][6] > 0) == (out["counts"][0] > 0)               # trials iff a camera is free
    start = both(sc, max_iters=0, pcg_iters=4, min_cam_obs=min_cam_obs)   # the start values alone
    assert start["counts"][0] == 0 and np.array_equal(start["cam_state"], state)
    assert both(sc, huber=0.0, max_iters=2, pcg_iters=1, min_cam_obs=min_cam_obs)["counts"][1] == 0


_LARGE_ERRORS = PC.error_cases(lambda: PC.many_cameras(1025, "path")) + PC.error_cases(lambda: PC.sized(4097, n=6))


@pytest.mark.parametrize("name,sc,bit", _LARGE_ERRORS, ids=[f"{c[1].name}-{c[0]}" for c in _LARGE_ERRORS])
def test_error_bits_at_the_edge_sizes(name, sc, bit):
    out = both(sc, **SHORT)
    assert out["counts"][1] & bit and out["counts"].sum() == out["counts"][1] and not any(out[k].any() for k in out if k != "counts")


@pytest.mark.parametrize("pcg_iters", (0, 1))
def test_few_conjugate_gradient_iterations(pcg_iters):
    out = both(PC.small(), max_iters=3, pcg_iters=pcg_iters, min_cam_obs=1)
    assert out["counts"][3] <= 3 * pcg_iters
    start = both(PC.small(), max_iters=0, pcg_iters=4)
    assert start["counts"][0] == 0 and start["info"][0] == start["info"][1]


@pytest.mark.parametrize("name,sc,bit", PC.error_cases(), ids=[c[0] for c in PC.error_cases()])
def test_error_bits(name, sc, bit):
    out = both(sc, **SHORT)
    assert out["counts"][1] & bit and out["counts"].sum() == out["counts"][1] and not any(out[k].any() for k in out if k != "counts")


def test_a_bad_grouping():
    sc = PC.small()
    a = ops_args(sc)
    a[4] = a[4].copy()
    a[4][[0, 1]] = a[4][[1, 0]]
    want = ops_global.global_positions_host(*a, sc.root, **SHORT)
    got = ops_global.global_positions(*[torch.from_numpy(x).cuda() for x in a], sc.root, **SHORT)
    assert want["counts"][1] == 4 and all(got[k].cpu().numpy().tobytes() == want[k].tobytes() for k in want)


def test_wrapper_and_timings():
    sc = PC.small()
    timings = []
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() if isinstance(x, np.ndarray) else x for x in sc.args]
    got = positions.global_positions(*dev, timings=timings, **SHORT)
    want = positions.global_positions(*sc.args, **SHORT)
    assert [s for s, _ in timings] == list(ops_global.POSITION_STAGES) and all(ms >= 0 for _, ms in timings)
    for k in positions.GlobalPositions.FIELDS:
        assert getattr(got, k).is_cuda and getattr(got, k).cpu().numpy().tobytes() == getattr(want, k).numpy().tobytes(), k
    assert {k: v for k, v in got.stats.items()} == want.stats


def test_reconstruct_global_chain_matches_the_cpu_chain():
    kw = dict(min_corr=6, min_inliers=6, positions_kw=dict(max_iters=3, pcg_iters=4))
    sfm_c, s = RC.false_row_atlas("cpu")
    sfm_g, _ = RC.false_row_atlas("cuda")
    cpu, gpu = sfm_c.reconstruct_global(s["K"], **kw), sfm_g.reconstruct_global(s["K"], **kw)
    assert gpu.T_cam_from_world.is_cuda and gpu.positions.centres.is_cuda
    assert gpu.positions.centres.cpu().numpy().tobytes() == cpu.positions.centres.numpy().tobytes()
    assert gpu.T_cam_from_world.cpu().numpy().tobytes() == cpu.T_cam_from_world.numpy().tobytes()          # the same poses bit for bit
    assert torch.equal(gpu.posed.cpu(), cpu.posed) and gpu.points.xyz.cpu().numpy().tobytes() == cpu.points.xyz.numpy().tobytes()
