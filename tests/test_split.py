"""Track splitting on the CPU: the host routine loftr_split_tracks_host against the set-based oracle (tests/_split_oracle.py)
with exact equality on every array and count, over the hand cases (whose expected results are written out in tests/_split_cases.py) and
seeded random graphs; the properties of the rule; SfmResult.split and reconstruct(split=True) on the atlas of a noisy pair list."""
import numpy as np
import pytest
import torch

import _split_cases as SC
import _split_oracle as SO
import loftr_amd
from loftr_amd import ops

HAND = SC.hand()
ERRORS = SC.errors()
SEEDS = (1, 2, 3, 4)


def same(got, want, what=""):
    for k in SC.OUT:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k, np.asarray(got[k]).tolist(), np.asarray(want[k]).tolist())


@pytest.mark.parametrize("name,args,want", HAND, ids=[h[0] for h in HAND])
def test_hand_cases(name, args, want):
    got = ops.split_tracks_host(*args)
    same(got, want, name)                                                 # what is written out
    same(got, SO.split(*args), name)                                      # the oracle agrees with what is written out
    assert got["track_id_new"].dtype == np.int32 and got["edge_state"].dtype == np.uint8 and got["counts"].dtype == np.int64


@pytest.mark.parametrize("name,args,bits", ERRORS, ids=[e[0] for e in ERRORS])
def test_error_bits(name, args, bits):
    got = ops.split_tracks_host(*args)
    assert got["counts"].tolist() == [0, bits] + [0] * 14
    for k in SC.OUT[:4]:
        assert not got[k].any(), k                                        # nothing but the counts is written
    same(got, SO.split(*args), name)
    with pytest.raises(ValueError, match="split_tracks: " + {1: "edge_kp outside", 2: "track_id outside", 4: "kp_image must not descend",
                                                              8: "edge_conf must be finite"}[bits & -bits]):
        loftr_amd.split_tracks(*args)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("min_len,max_rounds", [(2, 32), (3, 32), (1, 2), (2, 0)])
def test_random_graphs_against_the_oracle(seed, min_len, max_rounds):
    args = SC.random_args(seed, min_len, max_rounds)
    got = ops.split_tracks_host(*args)
    assert got["counts"][1] == 0 and got["counts"][6] > 0                 # the generator makes inconsistent tracks
    same(got, SO.split(*args), seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_visiting_order_of_a_phase_does_not_matter(seed):
    args = SC.random_args(seed)
    want = ops.split_tracks_host(*args)
    for s in range(3):
        same(SO.split(*args, rng=np.random.default_rng(100 * seed + s)), want, (seed, s))


def _partition(ids):
    groups = {}
    for k, t in enumerate(np.asarray(ids).tolist()):
        if t >= 0:
            groups.setdefault(t, []).append(k)
    return sorted(groups.values())


@pytest.mark.parametrize("seed", SEEDS)
def test_properties(seed):
    edges, conf, kp_image, track_id, track_ok, n = SC.random_graph(seed)
    frozen = [g for g in _partition(track_id) if track_ok[track_id[g[0]]] and len(g) >= 2]            # (shorter than min_track_len: not numbered)
    assert len(frozen) > 3
    full = ops.split_tracks_host(edges, conf, kp_image, track_id, track_ok, n, 2, 32)
    assert full["counts"][5] == 0 and 0 < full["counts"][9] < 32          # it finishes, and the last rounds are no-ops
    for max_rounds in (0, 1, 2, 32):
        got = ops.split_tracks_host(edges, conf, kp_image, track_id, track_ok, n, 2, max_rounds)
        parts = _partition(got["track_id_new"])
        for g in frozen:                                                  # a consistent track keeps its members exactly
            assert g in parts, (max_rounds, g)
        free = (track_id >= 0) & (track_ok[np.maximum(track_id, 0)] == 0)
        for g in parts:
            if g in frozen:
                continue
            assert free[g].all()                                          # a grown track holds free keypoints only
            assert len(set(kp_image[g].tolist())) == len(g), (max_rounds, g)                   # and visits an image at most once
            assert len(set(track_id[g].tolist())) == 1                    # and stays inside one input track
        assert (got["track_id_new"][track_id < 0] == -1).all()
        if max_rounds == 0:
            assert (got["track_id_new"][free] == -1).all() and (got["edge_state"][got["edge_state"] != 0] == 3).all()
        assert got["counts"][0] == len(parts) and got["track_len_new"][:len(parts)].tolist() == [len(g) for g in sorted(parts, key=lambda g: g[0])]
        assert got["counts"][2:6].sum() == len(edges) and got["counts"][9] == (got["round_accepted"] > 0).sum()
    # an input without inconsistent tracks comes back with the same partition (min_track_len = 1: a torn keypoint is a track of one)
    ok = np.ones_like(track_ok)
    got = ops.split_tracks_host(edges, conf, kp_image, track_id, ok, n, 1, 32)
    assert _partition(got["track_id_new"]) == _partition(track_id) and got["counts"][2] == len(edges) and got["counts"][6:11].tolist() == [0] * 5


def test_zero_confidences_and_negative_zero():
    """-0.0 packs as +0.0: with every confidence zero of either sign the lower edge wins"""
    args = SC.case([(0, 2, -0.0), (2, 1, 0.0)], [0, 0, 1], [0, 0, 0], [0], 2)
    got = ops.split_tracks_host(*args)
    assert got["track_id_new"].tolist() == [0, -1, 0] and got["edge_state"].tolist() == [1, 2]
    same(got, SO.split(*args))


# ---- SfmResult.split / reconstruct(split=True) on the atlas of a noisy pair list ------------------------------------------------------
@pytest.fixture(scope="module")
def sfm():
    return SC.run_atlas("cpu")


def _consistent(sfm):
    off, image, _ = sfm.tracks(consistent_only=False)
    off, image = off.tolist(), image.tolist()
    return all(len(set(image[a:b])) == b - a for a, b in zip(off[:-1], off[1:]))


def test_sfm_split(sfm):
    assert not bool(sfm.track_ok.all()) and not _consistent(sfm)          # the generator really produces inconsistent tracks
    before = int(sfm.tracks(consistent_only=True)[0][-1])
    sfm2, done = sfm.split()
    assert isinstance(done, loftr_amd.Split) and done.stats["n_open"] == 0 and done.stats["n_inconsistent_tracks"] == int((~sfm.track_ok).sum())
    assert bool(sfm2.track_ok.all()) and _consistent(sfm2) and sfm2.track_ok.numel() == sfm2.track_len.numel() == done.stats["n_tracks"]
    after = int(sfm2.tracks(consistent_only=True)[0][-1])
    assert after >= before and after == before + done.stats["n_rescued"] and done.stats["n_rescued"] > 0
    assert sfm2.track_len.tolist() == torch.bincount(sfm2.track_id[sfm2.track_id >= 0].long()).tolist()
    for k in sfm.FIELDS:
        if k not in ("track_id", "track_len", "track_ok"):
            assert getattr(sfm2, k) is getattr(sfm, k), k
    assert sfm2.image_hw == sfm.image_hw and sfm2.cell_px == sfm.cell_px and bool(sfm.track_ok.all()) is False      # the input is untouched
    # the oracle on the same atlas
    e = sfm.edge_keypoints().numpy()
    want = SO.split(e, sfm.match_conf.numpy(), sfm.keypoint_image().numpy(), sfm.track_id.numpy(), sfm.track_ok.numpy(), 8)
    assert np.array_equal(done.track_id_new.numpy(), want["track_id_new"]) and np.array_equal(done.edge_state.numpy(), want["edge_state"])
    assert np.array_equal(done.round_accepted.numpy(), want["round_accepted"])
    # an undistorted view splits like the original: no pixel is read
    view = sfm.undistorted(torch.from_numpy(SC.noisy_scene()["K"]), torch.zeros(8, dtype=torch.float64))
    v2, vdone = view.split()
    assert v2.is_undistorted and torch.equal(vdone.track_id_new, done.track_id_new) and v2.keypoints is view.keypoints
    # splitting a split result changes nothing but the (identical) numbering
    sfm3, again = sfm2.split()
    assert torch.equal(sfm3.track_id, sfm2.track_id) and again.stats["n_inconsistent_tracks"] == 0


def test_edge_keypoints_index_the_rows_images(sfm):
    e = sfm.edge_keypoints()
    img = sfm.keypoint_image()[e.long()]
    row = torch.repeat_interleave(torch.arange(sfm.row_images.shape[0]), sfm.row_offsets[1:] - sfm.row_offsets[:-1])
    assert torch.equal(img, sfm.row_images.long()[row]) and e.dtype == torch.int32
    assert torch.equal(sfm.track_id[e[:, 0].long()], sfm.track_id[e[:, 1].long()])           # an atlas edge never spans two tracks


def _fields(rec):
    out = {"posed": rec.posed, "T": rec.T_cam_from_world, "K": rec.K, "xyz": rec.points.xyz, "status": rec.points.status,
           "inlier": rec.points.obs_inlier, "offsets": rec.points.offsets}
    return out, {k: v for k, v in rec.stats.items()}


def test_reconstruct_without_split_is_unchanged(sfm):
    K = SC.noisy_scene()["K"]
    a, b = sfm.reconstruct(K), sfm.reconstruct(K, split=False)
    fa, sa = _fields(a)
    fb, sb = _fields(b)
    for k in fa:
        assert torch.equal(fa[k], fb[k], ) or (fa[k].is_floating_point() and torch.equal(torch.nan_to_num(fa[k]), torch.nan_to_num(fb[k]))), k
    assert sa == sb and "split" not in sa and a.sfm is None and b.sfm is None


def test_reconstruct_with_split_poses_every_image(sfm):
    s = SC.noisy_scene()
    base = sfm.reconstruct(s["K"])
    rec = sfm.reconstruct(s["K"], split=True)
    assert bool(rec.posed.all()) and rec.stats["split"]["n_rescued"] > 0 and rec.stats["split"]["n_open"] == 0
    assert rec.sfm is not None and bool(rec.sfm.track_ok.all()) and rec.points.offsets.numel() - 1 == rec.sfm.track_len.numel()
    assert rec.points.stats["n_ok"] >= base.points.stats["n_ok"]          # at least as many points as the run without the split


def test_value_errors():
    e, c, im, tid, ok, n, _, _ = SC.hand()[0][1]
    for kw, msg in ((dict(min_track_len=0), "min_track_len"), (dict(max_rounds=-1), "max_rounds"), (dict(max_rounds=2.0), "max_rounds"),
                    (dict(min_track_len=True), "min_track_len")):
        with pytest.raises(ValueError, match=msg):
            loftr_amd.split_tracks(e, c, im, tid, ok, n, **kw)
    with pytest.raises(ValueError, match="n_images"):
        loftr_amd.split_tracks(e, c, im, tid, ok, -1)
    with pytest.raises(ValueError, match="edge_kp must hold integers"):
        loftr_amd.split_tracks(e.astype(np.float32), c, im, tid, ok, n)
    with pytest.raises(ValueError, match="track_id must hold integers"):
        loftr_amd.split_tracks(e, c, im, tid.astype(np.float64), ok, n)
    done = loftr_amd.split_tracks(torch.from_numpy(e).long(), torch.from_numpy(c).double(), im.tolist(), tid, ok.astype(bool), n)   # converted
    assert done.track_id_new.tolist() == [0, -1, 0] and done.stats["n_rescued"] == 2 and done.track_len_new.tolist() == [2]
    assert done.to_host()["stats"]["largest_component"] == 2
