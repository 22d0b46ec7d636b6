"""GPU tests of track splitting: the kernels of csrc/split_gpu.hip against the host routine, torch.equal on every output and
count, over the hand cases, the seeded random graphs, edge and keypoint counts around a wave, a workgroup and several workgroups, one
inconsistent component whose member list reaches 1 / 2 / 63 / 64 / 65 keypoints, the descending chain under 0 / 1 / 32 rounds, a run
whose last rounds are no-ops, the error bits raised on the device, and SfmResult.split / reconstruct(split=True) GPU against CPU."""
import pytest
import torch

import _split_cases as SC
import loftr_amd
from loftr_amd import ops

pytestmark = pytest.mark.gpu
HAND = SC.hand()
ERRORS = SC.errors()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def run_both(args, dev, timings=None):
    host = ops.split_tracks_host(*args)
    gpu = ops.split_tracks(*[torch.from_numpy(x).to(dev) for x in args[:5]], *args[5:], timings=timings)
    return host, {k: v.cpu() for k, v in gpu.items()}


def same(gpu, host, what=""):
    assert set(gpu) == set(host) == set(SC.OUT)
    for k in SC.OUT:
        assert gpu[k].dtype == torch.from_numpy(host[k]).dtype and torch.equal(gpu[k], torch.from_numpy(host[k])), \
            (what, k, gpu[k].tolist()[:40], host[k].tolist()[:40])


@pytest.mark.parametrize("name,args,want", HAND, ids=[h[0] for h in HAND])
def test_hand_cases(dev, name, args, want):
    host, gpu = run_both(args, dev)
    same(gpu, host, name)
    for k in SC.OUT:
        assert gpu[k].tolist() == want[k], (name, k)


@pytest.mark.parametrize("seed", (1, 2, 3, 4))
def test_random_graphs(dev, seed):
    for min_len, max_rounds in ((2, 32), (3, 32), (1, 2), (2, 0)):
        host, gpu = run_both(SC.random_args(seed, min_len, max_rounds), dev)
        assert host["counts"][1] == 0 and host["counts"][6] > 0
        same(gpu, host, (seed, min_len, max_rounds))


@pytest.mark.parametrize("E", (0, 1, 63, 64, 65, 255, 256, 257, 4097))
def test_edge_counts(dev, E):
    host, gpu = run_both(SC.sized(E, 300), dev)
    assert host["counts"][1] == 0 and host["counts"][2:6].sum() == E
    same(gpu, host, E)


@pytest.mark.parametrize("K", (1, 257, 4097))
def test_keypoint_counts(dev, K):
    host, gpu = run_both(SC.sized(2 * K, K), dev)
    assert host["counts"][1] == 0 and host["counts"][7] == K
    same(gpu, host, K)


@pytest.mark.parametrize("members", (1, 2, 63, 64, 65))
def test_one_component_by_list_length(dev, members):
    args = SC.one_component(members, extra_edges=3 * members, seed=members)
    host, gpu = run_both(args, dev)
    assert host["counts"][1] == 0 and host["counts"][10] == members and host["counts"][5] == 0          # the list reaches every image
    assert host["counts"][4] >= (1 if members > 1 else 0)                                               # the second keypoint of the last image conflicts
    same(gpu, host, members)


@pytest.mark.parametrize("max_rounds", (0, 1, 32))
def test_descending_chain_by_rounds(dev, max_rounds):
    args = SC.case(SC.CHAIN, SC.CHAIN_IMAGES, [0] * 11, [0], 10, max_rounds=max_rounds)
    host, gpu = run_both(args, dev)
    assert host["counts"][9] == min(max_rounds, 9) and (host["counts"][5] > 0) == (max_rounds < 9)
    same(gpu, host, max_rounds)


def test_the_last_rounds_are_no_ops(dev):
    timings = []
    args = SC.random_args(3, 2, 32)
    host, gpu = run_both(args, dev, timings=timings)
    used = int(host["counts"][9])
    assert 0 < used < 31 and not host["round_accepted"][used:].any() and host["counts"][5] == 0
    same(gpu, host)
    assert [s for s, _ in timings] == list(ops.SPLIT_STAGES) and all(ms >= 0 for _, ms in timings)


@pytest.mark.parametrize("name,args,bits", ERRORS, ids=[e[0] for e in ERRORS])
def test_error_bits_on_the_device(dev, name, args, bits):
    host, gpu = run_both(args, dev)
    assert gpu["counts"].tolist() == [0, bits] + [0] * 14
    same(gpu, host, name)                                                 # nothing is written beyond the counts
    for k in SC.OUT[:4]:
        assert not gpu[k].any(), k
    with pytest.raises(ValueError, match="split_tracks"):
        loftr_amd.split_tracks(*[torch.from_numpy(x).to(dev) for x in args[:5]], *args[5:])


def test_ops_takes_gpu_tensors_only(dev):
    args = HAND[0][1]
    with pytest.raises(loftr_amd._lib.LoftrHipError, match="numpy arrays"):
        ops.split_tracks_host(*[torch.from_numpy(x).to(dev) for x in args[:5]], *args[5:])
    mixed = [torch.from_numpy(x).to(dev) for x in args[:5]]
    mixed[2] = mixed[2].cpu()
    with pytest.raises(loftr_amd._lib.LoftrHipError, match="GPU and CPU arguments mixed"):
        loftr_amd.split_tracks(*mixed, *args[5:])


@pytest.fixture(scope="module")
def atlases(dev):
    return SC.run_atlas("cpu"), SC.run_atlas(dev)


def test_sfm_split_gpu_against_cpu(atlases):
    cpu, gpu = atlases
    c2, cdone = cpu.split()
    g2, gdone = gpu.split()
    assert gdone.track_id_new.is_cuda and cdone.stats == gdone.stats and cdone.stats["n_rescued"] > 0
    for k in loftr_amd.Split.FIELDS:
        assert torch.equal(getattr(gdone, k).cpu(), getattr(cdone, k)), k
    for k in cpu.FIELDS:
        assert torch.equal(getattr(g2, k).cpu(), getattr(c2, k)), k
    assert bool(g2.track_ok.all())


def test_reconstruct_with_split_gpu_against_cpu(atlases):
    cpu, gpu = atlases
    K = SC.noisy_scene()["K"]
    rc, rg = cpu.reconstruct(K, split=True), gpu.reconstruct(K, split=True)
    assert rc.stats["split"] == rg.stats["split"] and bool(rg.posed.all()) and torch.equal(rg.posed.cpu(), rc.posed)
    assert torch.equal(rg.sfm.track_id.cpu(), rc.sfm.track_id) and torch.equal(rg.points.offsets.cpu(), rc.points.offsets)
    assert rg.points.stats["n_ok"] >= gpu.reconstruct(K).points.stats["n_ok"]
