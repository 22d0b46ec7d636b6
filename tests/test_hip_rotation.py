"""GPU tests of rotation averaging: the kernels of csrc/rotation_gpu.hip against the host routine, every output equal bit for
bit (R, edge_chord and info compared as 64-bit words, all integers and the counts), at the sizes where the kernels can go wrong: no
edge, one edge, 63 / 64 / 65 / 67 images (the wave edges of the per-node and per-edge launches), a hub with 70 neighbours (the
neighbour-list steps of 64 lanes), 1 366 images (3 n = 4 098 crosses the 4096-term chunk of the ordered sums and the tree is deeper
than the 1024 threads of the start-value workgroup), the planted-outlier scenes, duplicates, two components, max_iters = 0,
pcg_iters = 1, a run that ends on max_iters, the error bits raised on the device, and average_rotations /
SfmResult.rotation_averaging / reconstruct(rotations=True) on the CPU against the GPU."""
import numpy as np
import pytest
import torch

import _rotation_cases as RC
import loftr_amd
from loftr_amd import ops

pytestmark = pytest.mark.gpu
OUT = ("R", "in_graph", "edge_state", "edge_chord", "support", "tree", "edge_use", "counts", "info")
ERRORS = RC.error_cases()
OUTLIERS = RC.outlier_scenes()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def run_both(args, dev, timings=None):
    host = ops.rotation_averaging_host(*args)
    gpu = ops.rotation_averaging(*[torch.from_numpy(x).to(dev) for x in args[:6]], *args[6:], timings=timings)
    return host, {k: v.cpu() for k, v in gpu.items()}


def words(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def same(gpu, host, what=""):
    assert set(gpu) == set(host) == set(OUT)
    for k in OUT:
        h = torch.from_numpy(host[k])
        assert gpu[k].dtype == h.dtype and gpu[k].shape == h.shape, (what, k)
        assert torch.equal(words(gpu[k]), words(h)), (what, k, gpu[k].reshape(-1).tolist()[:24], h.reshape(-1).tolist()[:24])


def stat(out, name):
    return int(out["counts"][ops.ROTATION_NAMES.index(name)])


def test_no_edge_and_one_edge(dev):
    empty = RC.Scene("empty", np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)), np.zeros(0, np.int32), 3, None, None)
    host, gpu = run_both(RC.ops_args(empty), dev)
    same(gpu, host, "E = 0")
    assert stat(gpu, "status") == 3 and stat(gpu, "n_in_graph") == 1 and stat(gpu, "root") == 0
    none = RC.Scene("none", np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)), np.zeros(0, np.int32), 0, None, None)
    host, gpu = run_both(RC.ops_args(none), dev)
    same(gpu, host, "n = 0")
    assert stat(gpu, "status") == 3 and stat(gpu, "root") == -1
    host, gpu = run_both(RC.ops_args(RC.make_scene("one", 2, 1, 3)), dev)
    same(gpu, host, "n = 2")
    assert stat(gpu, "status") == 0 and stat(gpu, "n_in_graph") == 2 and stat(gpu, "n_ok") == 1


@pytest.mark.parametrize("n", (63, 64, 65, 67))
def test_wave_edges(dev, n):
    host, gpu = run_both(RC.ops_args(RC.make_scene("w", n, 3, 70 + n, planted=5)), dev)
    assert stat(host, "error_bits") == 0 and stat(host, "n_in_graph") == n and stat(host, "n_outlier") == 5 and stat(host, "status") == 0
    same(gpu, host, n)


def test_hub_of_70(dev):
    sc = RC.hub_scene()
    timings = []
    host, gpu = run_both(RC.ops_args(sc), dev, timings)
    assert stat(host, "error_bits") == 0 and int(host["support"].max()) >= 2 and np.array_equal(host["edge_state"] == 3, sc.planted)
    same(gpu, host, "hub")
    assert [t[0] for t in timings] == list(ops.ROTATION_STAGES) and all(t[1] >= 0 for t in timings)


def test_1366_images_cross_the_sum_chunk_and_the_start_workgroup(dev):
    host, gpu = run_both(RC.ops_args(RC.make_scene("long", 1366, 2, 81), root=0, max_iters=6), dev)
    assert stat(host, "error_bits") == 0 and stat(host, "n_in_graph") == 1366 and stat(host, "tree_depth") > 1024 // 2
    assert stat(host, "n_iters") >= 2 and stat(host, "root") == 0
    same(gpu, host, "1366")


@pytest.mark.parametrize("sc", OUTLIERS, ids=[s.name for s in OUTLIERS])
def test_planted_outliers(dev, sc):
    host, gpu = run_both(RC.ops_args(sc), dev)
    assert np.array_equal(host["edge_state"] == 3, sc.planted)
    same(gpu, host, sc.name)


def test_duplicates_two_components_and_the_iteration_limits(dev):
    dup, idx = RC.with_duplicates(RC.make_scene("d", 20, 3, 5))
    host, gpu = run_both(RC.ops_args(dup), dev)
    assert stat(host, "n_duplicate") == idx.size
    same(gpu, host, "duplicates")
    host, gpu = run_both(RC.ops_args(RC.two_components()), dev)
    assert stat(host, "n_in_graph") == 10 and stat(host, "n_components") == 2 and int((host["edge_state"] == 1).sum()) > 0
    same(gpu, host, "two components")
    noisy = RC.chain_scenes()[0]
    for kw, status in ((dict(max_iters=0), 1), (dict(pcg_iters=1), None), (dict(max_iters=2), 1), (dict(pcg_iters=0), 0)):
        host, gpu = run_both(RC.ops_args(noisy, **kw), dev)
        assert status is None or stat(host, "status") == status, (kw, stat(host, "status"))
        same(gpu, host, kw)


@pytest.mark.parametrize("name,args,bit", ERRORS, ids=[e[0] for e in ERRORS])
def test_error_bits_raised_on_the_device(dev, name, args, bit):
    host, gpu = run_both(args, dev)
    assert stat(host, "error_bits") & bit
    same(gpu, host, name)
    for k in OUT:
        if k != "counts":
            assert not words(gpu[k]).any(), (name, k)
    assert gpu["counts"].tolist() == [0, stat(host, "error_bits")] + [0] * 14


def test_average_rotations_cpu_against_gpu(dev):
    sc = OUTLIERS[2]
    cpu = loftr_amd.average_rotations(*sc.args)
    gpu = loftr_amd.average_rotations(*[torch.from_numpy(x).to(dev) for x in sc.args[:3]], sc.n)
    assert gpu.R.is_cuda and gpu.root == cpu.root and gpu.stats == cpu.stats
    a, b = cpu.to_host(), gpu.to_host()
    for k in loftr_amd.GlobalRotations.FIELDS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert torch.equal(gpu.edge_ok.cpu(), cpu.edge_ok) and torch.equal(gpu.edge_ok.cpu(), torch.from_numpy(~sc.planted))
    with pytest.raises(loftr_amd._lib.LoftrHipError, match="mixed"):
        loftr_amd.average_rotations(torch.from_numpy(sc.edge_image).to(dev), sc.edge_R, sc.edge_weight, sc.n)


def test_sfm_chain_cpu_against_gpu(dev):
    """SfmResult.rotation_averaging and reconstruct(rotations=True) on the pair list with one wrongly matched row: the same rejected
    rows and the same final poses on both sides, bit for bit."""
    (cpu, s), (gpu, _) = RC.false_row_atlas("cpu"), RC.false_row_atlas("cuda")
    rc, rg = cpu.rotation_averaging(s["K"]), gpu.rotation_averaging(s["K"])
    assert rg.R.is_cuda and rg.stats == rc.stats and torch.nonzero(~rg.edge_ok).reshape(-1).tolist() == [RC.FALSE_ROW]
    a, b = rc.to_host(), rg.to_host()
    for k in loftr_amd.GlobalRotations.FIELDS:
        assert a[k].tobytes() == b[k].tobytes(), k
    kw = dict(min_corr=6, min_inliers=6, rotations=True)
    c, g = cpu.reconstruct(s["K"], **kw), gpu.reconstruct(s["K"], **kw)
    assert g.stats["rotations"] == c.stats["rotations"] and g.stats["init_row"] == c.stats["init_row"] and bool(g.posed.all())
    assert torch.equal(g.sfm.track_id.cpu(), c.sfm.track_id) and torch.equal(g.rotations.edge_state.cpu(), c.rotations.edge_state)
    assert g.T_cam_from_world.cpu().numpy().tobytes() == c.T_cam_from_world.numpy().tobytes()
    assert g.points.stats["n_ok"] == c.points.stats["n_ok"] == 60
