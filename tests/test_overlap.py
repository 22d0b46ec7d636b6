"""View overlap and pair proposals on the CPU: the host routine loftr_view_overlap_host against the numpy statement of the
rule (tests/_overlap_oracle.py) with exact equality on overlap, n_vis and counts; the hand-placed points on every boundary of the
predicate; the selection rules; the ValueErrors; and the behavioural case -- a ring of cameras matched as an open chain must get its
closing pair proposed and nothing further than three steps apart."""
import math

import numpy as np
import pytest
import torch

import _overlap_cases as OC
import _overlap_oracle as OO
import loftr_amd
from loftr_amd import build as build_mod, ops, proposals


@pytest.fixture(scope="module", autouse=True)
def lib():
    build_mod.build(verbose=False)


def host(c):
    out = ops.view_overlap(*OC.tensors(c))
    return out["overlap"].numpy(), out["n_vis"].numpy(), out["counts"].numpy()


def assert_equals_oracle(c):
    got, want = host(c), OO.view_overlap(*OC.oracle_args(c))
    for g, w, name in zip(got, want, ("overlap", "n_vis", "counts")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name
    return got


def test_scenes_equal_the_oracle():
    o, n_vis, counts = assert_equals_oracle(OC.scene_a())
    assert counts[1] == 0 and counts[2] == counts[3] == 5 and counts[0] == n_vis.sum() > 0 and counts[4] == np.count_nonzero(o) > 5
    assert (np.diag(o) <= n_vis).all() and (o <= n_vis[:, None]).all()
    o, n_vis, counts = assert_equals_oracle(OC.scene_b())
    assert counts[2] == counts[3] == 12 and 0 < counts[4] < 144                          # the tight angle and scale reject some pairs
    loose = dict(OC.scene_b(), cos_min=-1.0, max_scale2=math.inf, border=0.0)
    o2 = assert_equals_oracle(loose)[0]
    assert (o2 >= o).all() and o2.sum() > o.sum()


def test_spoiled_scene_equals_the_oracle():
    c = OC.spoiled()
    o, n_vis, counts = assert_equals_oracle(c)
    assert counts[2] == 12 - 3 and counts[3] == 12 - 7
    assert (o[[1, 2, 3]] == 0).all() and (n_vis[[1, 2, 3]] == 0).all() and (o[:, [4, 5, 6, 7, 8, 9, 10]] == 0).all()
    clean = host(OC.scene_b())
    assert n_vis.sum() < np.delete(clean[1], [1, 2, 3]).sum()                            # the unusable entries are not counted


@pytest.mark.parametrize("name,c,want", OC.hand_cases(), ids=[h[0] for h in OC.hand_cases()])
def test_hand_placed_boundaries(name, c, want):
    o = assert_equals_oracle(c)[0]
    assert o.tolist() == want


@pytest.mark.parametrize("name,c", OC.empty_cases(), ids=[e[0] for e in OC.empty_cases()])
def test_empty_tables(name, c):
    o, n_vis, counts = assert_equals_oracle(c)
    assert o.shape == (len(c["src_ok"]), len(c["tgt_ok"])) and counts[1] == 0 and counts[5:].tolist() == [0, 0, 0]


@pytest.mark.parametrize("name,c,bits", OC.bad_lists(), ids=[b[0] for b in OC.bad_lists()])
def test_error_bits(name, c, bits):
    o, n_vis, counts = assert_equals_oracle(c)
    assert counts.tolist() == [0, bits, 0, 0, 0, 0, 0, 0] and not o.any() and not n_vis.any()
    with pytest.raises(ValueError, match="vis_point must lie in" if bits & 1 else "vis_offsets must start at 0"):
        loftr_amd.view_overlap(*OC.tensors(c)[:11])


def test_sized_cases_equal_the_oracle():
    assert_equals_oracle(OC.sized(3, 5, 300, 100, seed=4, unusable=0.2))
    o, n_vis, _ = assert_equals_oracle(OC.exactly_usable(65))
    assert n_vis.tolist() == [65] and o.max() > 0
    o, n_vis, counts = assert_equals_oracle(OC.exactly_usable(0))
    assert n_vis.tolist() == [0] and not o.any() and counts[2] == 1


def test_python_entry_takes_the_angle_and_scale():
    c = OC.scene_b()
    t = OC.tensors(c)[:11]
    t[4], t[5], t[7], t[8] = (x.reshape(-1, s, s) for x, s in zip((t[4], t[5], t[7], t[8]), (3, 4, 3, 4)))
    res = loftr_amd.view_overlap(*t, max_angle_deg=20.0, max_scale=1.3, border_px=4.0)
    assert isinstance(res, loftr_amd.Overlap) and np.array_equal(res.overlap.numpy(), host(c)[0])
    assert res.stats["n_sources"] == 12 and res.stats["n_visible"] == int(res.n_vis.sum()) and "error_bits" not in res.stats
    assert res.to_host()["overlap"].shape == (12, 12)
    for kw in (dict(max_angle_deg=-1.0), dict(max_angle_deg=181.0), dict(max_angle_deg=float("nan")), dict(max_scale=0.5),
               dict(max_scale=float("nan")), dict(border_px=-1.0), dict(border_px=float("inf"))):
        with pytest.raises(ValueError, match="must"):
            loftr_amd.view_overlap(*t, **kw)
    with pytest.raises(ValueError, match="must hold integers"):
        loftr_amd.view_overlap(t[0].double(), *t[1:])
    with pytest.raises(ValueError, match="expected K_src"):
        loftr_amd.view_overlap(*t[:4], t[4][:5], *t[5:])


# ---- the selection ------------------------------------------------------------------------------------------------------------------
def test_select_pairs_ordering_ties_and_existing():
    o = torch.tensor([[9, 50, 40, 40, 0],
                      [50, 9, 40, 35, 31],
                      [45, 40, 9, 40, 29],
                      [40, 60, 40, 9, 30],
                      [90, 31, 90, 30, 9]], dtype=torch.int32)
    # scores: (0,1) 50, (0,2) 40, (0,3) 40, (0,4) 0, (1,2) 40, (1,3) 35, (1,4) 31, (2,3) 40, (2,4) 29, (3,4) 30
    pairs, score = proposals.select_pairs(o, top_k=2, min_shared=30)
    # image 0: 1 (50), then the tie 2 / 3 at 40 -> 2; image 1: 0, 2; image 2: the tie 0 / 1 / 3 at 40 -> 0, 1; image 3: 0, 2; image 4: 1 (31), 3 (30)
    assert pairs.dtype == torch.int64 and pairs.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 4], [2, 3], [3, 4]]
    assert score.tolist() == [50, 40, 40, 40, 31, 40, 30]
    for existing in ([[0, 1], [3, 2]], [[1, 0], [2, 3]], torch.tensor([[0, 1], [2, 3], [1, 0]], dtype=torch.int32)):
        pairs, score = proposals.select_pairs(o, existing=existing, top_k=2, min_shared=30)
        # image 0: 2, 3; image 1: 2, 3 (35); image 2: 0, 1; image 3: 0, 1; image 4: 1, 3
        assert pairs.tolist() == [[0, 2], [0, 3], [1, 2], [1, 3], [1, 4], [3, 4]] and score.tolist() == [40, 40, 40, 35, 31, 30]
    pairs, score = proposals.select_pairs(o, top_k=1, min_shared=41)
    assert pairs.tolist() == [[0, 1]] and score.tolist() == [50]
    pairs, score = proposals.select_pairs(o, top_k=9, min_shared=0)                      # more than there are: every pair, the diagonal never
    assert pairs.tolist() == [[a, b] for a in range(5) for b in range(a + 1, 5)]
    pairs, score = proposals.select_pairs(o, top_k=3, min_shared=1000)
    assert pairs.shape == (0, 2) and score.shape == (0,)
    assert proposals.select_pairs(torch.zeros((0, 0), dtype=torch.int32))[0].shape == (0, 2)
    for bad, kw in ((o[:, :4], {}), (o.float(), {}), (o, dict(top_k=0)), (o, dict(top_k=2.0)), (o, dict(min_shared=-1)), (o, dict(existing=[0, 1])),
                    (o, dict(existing=torch.zeros((2, 2))))):
        with pytest.raises(ValueError):
            proposals.select_pairs(bad, **kw)


def test_select_database_ordering_ties_and_padding():
    o = torch.tensor([[40, 0, 5],
                      [70, 0, 5],
                      [40, 0, 5],
                      [10, 0, 6]], dtype=torch.int32)                                    # 4 database images x 3 queries
    ids, score = proposals.select_database(o, top_k=3, min_shared=10)
    assert ids.dtype == torch.int64 and ids.tolist() == [[1, 0, 2], [-1, -1, -1], [-1, -1, -1]]
    assert score.tolist() == [[70, 40, 40], [0, 0, 0], [0, 0, 0]]
    ids, score = proposals.select_database(o, top_k=6, min_shared=5)                     # top_k beyond the database: padded
    assert ids.tolist() == [[1, 0, 2, 3, -1, -1], [-1] * 6, [3, 0, 1, 2, -1, -1]] and score[2].tolist() == [6, 5, 5, 5, 0, 0]
    ids, _ = proposals.select_database(o, top_k=1, min_shared=0)
    assert ids.tolist() == [[1], [0], [3]]
    assert proposals.select_database(torch.zeros((0, 2), dtype=torch.int32), top_k=2)[0].tolist() == [[-1, -1], [-1, -1]]
    assert proposals.select_database(torch.zeros((3, 0), dtype=torch.int32), top_k=2)[0].shape == (0, 2)


def test_propose_pairs_builds_the_lists_of_the_posed_images():
    rec, sfm, want = OC.ring_reconstruction()
    o = host(want)[0]
    pairs, score = rec.propose_pairs(sfm, top_k=4, min_shared=20)
    p2, s2 = proposals.select_pairs(torch.from_numpy(o), existing=sfm.row_images, top_k=4, min_shared=20)
    assert torch.equal(pairs, p2) and torch.equal(score, s2) and len(pairs) > 10
    got = {tuple(p) for p in pairs.tolist()}
    assert (0, 23) in got and not any(5 in p for p in got)                               # the closing pair; the image without a pose is in no pair
    assert not got & {tuple(r) for r in sfm.row_images.tolist()}
    tight, _ = rec.propose_pairs(sfm, top_k=4, min_shared=20, max_angle_deg=10.0)        # the keywords reach view_overlap
    assert len(tight) < len(pairs)
    rec.points.offsets = None
    with pytest.raises(ValueError, match="carry no tracks"):
        rec.propose_pairs(sfm)


def test_propose_for_poses_builds_the_lists_of_the_database_images():
    model, K_db, T_db, K_q, T_q, hw, want = OC.ring_model()
    o = host(want)[0]
    ids, score = model.propose_for_poses(K_db, T_db, K_q, T_q, hw, top_k=5, min_shared=10)
    i2, s2 = proposals.select_database(torch.from_numpy(o), top_k=5, min_shared=10)
    assert ids.shape == (9, 5) and torch.equal(ids, i2) and torch.equal(score, s2) and (ids[:, 0] >= 0).sum() >= 5
    with pytest.raises(ValueError, match="K_db holds"):
        model.propose_for_poses(K_db[:3], T_db[:3], K_q, T_q, hw)


# ---- the behavioural case -----------------------------------------------------------------------------------------------------------
def test_a_ring_matched_as_a_chain_gets_its_closing_pair():
    c, existing = OC.ring_scene()
    res = loftr_amd.view_overlap(*OC.tensors(c)[:11], max_angle_deg=45.0, max_scale=2.0)
    pairs, score = loftr_amd.select_pairs(res, existing=torch.from_numpy(existing), top_k=4, min_shared=20)
    got = {tuple(p) for p in pairs.tolist()}
    step = lambda a, b: min((a - b) % 24, (b - a) % 24)
    print(f"visible per camera {res.n_vis.float().mean():.0f}, proposals {len(got)}, largest ring distance {max(step(a, b) for a, b in got)}")
    assert (0, 23) in got
    assert all(step(a, b) <= 3 for a, b in got)
    assert not got & {tuple(e) for e in existing.tolist()} and (score >= 20).all()
