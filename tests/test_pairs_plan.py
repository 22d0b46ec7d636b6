"""Schedules of pair lists on a feature bank (loftr_amd/pairs.py: plan_pair_list), checked by replaying them on the host: every row is
matched once and in input order, from slots that hold its images; residency stays within the bank; the images of the chunk being
matched are never evicted; with room for every image each is extracted exactly once, in full groups.  Run on synthetic lists and on
the image structure of the reference's ScanNet-1500 and MegaDepth-1500 test lists (tests/golden/pair_lists.npz)."""
import math
import os

import numpy as np
import pytest

from loftr_amd.pairs import Extract, Match, plan_pair_list

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_lists.npz")


def _fixture(name):
    g = np.load(GOLDEN)
    return g[name + "_pairs"], int(g[name + "_images"])


def replay(pairs, n_slots, batch_size=8, extract_batch=16):
    """Run the plan against a model of the bank; returns (steps, images extracted, extract groups)."""
    pairs = np.asarray(pairs)
    steps = plan_pair_list(pairs, n_slots, batch_size, extract_batch)
    slot_of, image_in = {}, {}                       # image -> slot, slot -> image
    next_row, extracted, groups = 0, 0, 0
    pending_chunk = None
    for st in steps:
        if isinstance(st, Extract):
            assert 1 <= len(st.images) <= extract_batch and len(st.images) == len(st.slots) == len(set(st.slots))
            chunk = pairs[next_row:next_row + batch_size].reshape(-1)
            for x, s in zip(st.images, st.slots):
                assert 0 <= s < n_slots
                assert x not in slot_of, "image extracted while resident"
                old = image_in.pop(s, None)
                if old is not None:
                    assert old not in set(chunk.tolist()), "evicted an image of the chunk about to be matched"
                    del slot_of[old]
                slot_of[x], image_in[s] = s, x
            extracted += len(st.images)
            groups += 1
            assert len(slot_of) <= n_slots
        else:
            assert isinstance(st, Match)
            assert st.rows.start == next_row and 1 <= len(st.rows) <= batch_size, "rows out of order"
            assert len(st.rows) == batch_size or st.rows.stop == len(pairs)
            for r, s0, s1 in zip(st.rows, st.slots0, st.slots1):
                assert image_in.get(s0) == pairs[r, 0] and image_in.get(s1) == pairs[r, 1], "chunk image not resident"
            next_row = st.rows.stop
    assert next_row == len(pairs), "not every row matched"
    return steps, extracted, groups


def _synthetic(seed, P=200, U=60):
    rng = np.random.default_rng(seed)
    return rng.integers(0, U, (P, 2))


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("n_slots", [16, 24, 40, 1000])
@pytest.mark.parametrize("batch_size,extract_batch", [(8, 16), (4, 5), (8, 3)])
def test_synthetic_lists(seed, n_slots, batch_size, extract_batch):
    pairs = _synthetic(seed)
    if n_slots < 2 * batch_size:
        return
    U = len(np.unique(pairs))
    _, extracted, groups = replay(pairs, n_slots, batch_size, extract_batch)
    assert U <= extracted <= 2 * len(pairs)
    if n_slots >= U:
        assert extracted == U and groups == math.ceil(U / extract_batch)


@pytest.mark.parametrize("name,U", [("scannet", 2596), ("megadepth", 806)])
def test_reference_lists_with_room_for_every_image(name, U):
    pairs, n = _fixture(name)
    assert pairs.shape == (1500, 2) and pairs.dtype == np.int32 and n == U == len(np.unique(pairs))
    _, extracted, groups = replay(pairs, U)
    assert extracted == U and groups == math.ceil(U / 16)


@pytest.mark.parametrize("name", ["scannet", "megadepth"])
@pytest.mark.parametrize("n_slots", [16, 64, 300])
def test_reference_lists_under_a_budget(name, n_slots):
    pairs, U = _fixture(name)
    _, extracted, _ = replay(pairs, n_slots)
    assert U <= extracted <= 2 * len(pairs)


def test_reuse_saves_extractions_on_megadepth():
    pairs, U = _fixture("megadepth")
    assert replay(pairs, 300)[1] < 2 * len(pairs) * 0.6


def test_lookahead_never_evicts_an_earlier_next_use():
    # chunks of 1 pair: [0,1] [2,3] [0,1] [4,5] ... on 2 slots per chunk + 2 spare: the look-ahead after chunk 0 may bring 2, 3 in,
    # but bringing 4, 5 in later would have to evict 0 / 1, which are used again before them
    pairs = np.array([[0, 1], [2, 3], [0, 1], [4, 5], [0, 1]])
    steps, extracted, _ = replay(pairs, 4, batch_size=1, extract_batch=8)
    assert extracted == 6
    first = steps[0]
    assert isinstance(first, Extract) and first.images == [0, 1, 2, 3]


def test_single_chunk_and_self_pairs():
    steps, extracted, groups = replay(np.array([[3, 3], [3, 7], [7, 3]]), 16)
    assert extracted == 2 and groups == 1 and len(steps) == 2


@pytest.mark.parametrize("bad", [np.zeros((4, 3), int), np.zeros(8, int), np.array([[0, -1]]), np.array([[0.0, 1.0]]),
                                 np.array([[0, 2 ** 40]])])
def test_bad_pairs_raise(bad):
    with pytest.raises(ValueError):
        plan_pair_list(bad, 64)


def test_too_few_slots_raise():
    with pytest.raises(ValueError):
        plan_pair_list(np.zeros((4, 2), int), 15, batch_size=8)
    with pytest.raises(ValueError):
        plan_pair_list(np.zeros((4, 2), int), 64, batch_size=0)
