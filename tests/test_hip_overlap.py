"""The view-overlap kernels (csrc/overlap_gpu.hip) against the host routine (csrc/overlap.hip, itself held to the numpy oracle by
tests/test_overlap.py): torch.equal on overlap, n_vis and counts.  Cases: the scenes and the hand-placed boundaries; the lane, wave and
tile edges of the target tile (LOFTR_OVERLAP_TILE = 256 targets per block); one source with a number of usable points at the edges of
the staged chunk (256 entries) and beyond several chunks; one source and more sources than a tile; a list whose every entry is unusable;
the error bits found on the device; and the two Python entries, GPU against CPU."""
import numpy as np
import pytest
import torch

import _overlap_cases as OC
import loftr_amd
from loftr_amd import build as build_mod, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def lib():
    build_mod.build(verbose=False)


def both(c):
    cpu = ops.view_overlap(*OC.tensors(c))
    gpu = ops.view_overlap(*OC.tensors(c, "cuda"))
    for k in ("overlap", "n_vis", "counts"):
        assert gpu[k].is_cuda and gpu[k].dtype == cpu[k].dtype and torch.equal(gpu[k].cpu(), cpu[k]), k
    return cpu


def test_scenes():
    for c in (OC.scene_a(), OC.scene_b(), OC.spoiled()):
        out = both(c)
        assert out["counts"][1] == 0 and out["counts"][4] > 0


@pytest.mark.parametrize("name,c,want", OC.hand_cases(), ids=[h[0] for h in OC.hand_cases()])
def test_hand_placed_boundaries(name, c, want):
    assert both(c)["overlap"].tolist() == want


@pytest.mark.parametrize("name,c", OC.empty_cases(), ids=[e[0] for e in OC.empty_cases()])
def test_empty_tables(name, c):
    assert both(c)["counts"][1] == 0


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257])
def test_target_tile_edges(m):
    out = both(OC.sized(3, m, 300, 100, seed=m, unusable=0.1))
    assert out["counts"][3] == m and out["counts"][4] > 0


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_chunk_edges_of_one_source(count):
    out = both(OC.exactly_usable(count))
    assert out["n_vis"].tolist() == [count] and (out["overlap"].max() > 0 if count >= 63 else count > 0 or not out["overlap"].any())


@pytest.mark.parametrize("n", [1, 257])
def test_source_counts(n):
    out = both(OC.sized(n, 5, 200, 20, seed=n))
    assert out["counts"][2] == n


def test_a_list_without_a_usable_entry():
    c = OC.sized(2, 70, 100, [300, 40], seed=9)
    c["point_ok"][:] = 0
    out = both(c)
    assert out["counts"].tolist() == [0, 0, 2, 70, 0, 0, 0, 0]
    c = OC.sized(2, 70, 100, [300, 40], seed=9)
    c["xyz"][:, 1] = np.inf
    assert both(c)["counts"].tolist() == [0, 0, 2, 70, 0, 0, 0, 0]


@pytest.mark.parametrize("name,c,bits", OC.bad_lists(), ids=[b[0] for b in OC.bad_lists()])
def test_error_bits_on_the_device(name, c, bits):
    out = both(c)                                                                        # nothing beyond the zeroed outputs
    assert out["counts"].tolist() == [0, bits, 0, 0, 0, 0, 0, 0] and not out["overlap"].any() and not out["n_vis"].any()
    with pytest.raises(ValueError, match="found on the device"):
        loftr_amd.view_overlap(*OC.tensors(c, "cuda")[:11])


def test_stage_timings_are_reported():
    timings = []
    ops.view_overlap(*OC.tensors(OC.scene_a(), "cuda"), timings=timings)
    assert [s for s, _ in timings] == list(ops.OVERLAP_STAGES) and all(ms >= 0 for _, ms in timings)


def test_propose_pairs_gpu_equals_cpu():
    rec, sfm, _ = OC.ring_reconstruction()
    rec_g, sfm_g, _ = OC.ring_reconstruction("cuda")
    pairs, score = rec.propose_pairs(sfm, top_k=4, min_shared=20)
    pairs_g, score_g = rec_g.propose_pairs(sfm_g, top_k=4, min_shared=20)
    assert pairs_g.is_cuda and torch.equal(pairs_g.cpu(), pairs) and torch.equal(score_g.cpu(), score) and [0, 23] in pairs.tolist()


def test_propose_for_poses_gpu_equals_cpu():
    model, *args, _ = OC.ring_model()
    model_g, *args_g, _ = OC.ring_model("cuda")
    ids, score = model.propose_for_poses(*args, top_k=5, min_shared=10)
    ids_g, score_g = model_g.propose_for_poses(*args_g, top_k=5, min_shared=10)
    assert ids_g.is_cuda and torch.equal(ids_g.cpu(), ids) and torch.equal(score_g.cpu(), score) and (ids >= 0).any()
