"""Keypoint atlas on the GPU (csrc/atlas_gpu.hip): every output must equal the defining host routine's bit for bit -- on the cases of
tests/test_atlas.py, whatever the chunking and the starting capacity, and on the matches of a real pair-list run."""
import copy
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _atlas_cases as AC
from _cases import GOLDEN_DIR

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

_HOST = {}


def host(key, n, hw, rows, **kw):
    """The host routine's result, computed once per case."""
    if key not in _HOST:
        _HOST[key] = AC.run(n, hw, rows, device="cpu", **kw)
    return _HOST[key]


# ---- (a), (b): random rows, three cell sizes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cell_px", [2.0, 0.5, 16.0])
def test_random_rows_equal_the_host_routine(cell_px):
    n, hw, rows = AC.random_case()
    AC.assert_same(AC.run(n, hw, rows, cell_px, device=DEV), host(("random", cell_px), n, hw, rows, cell_px=cell_px), cell_px)


def test_chunking_and_growth_do_not_matter():
    n, hw, rows = AC.random_case()
    want = host(("random", 2.0), n, hw, rows, cell_px=2.0)
    AC.assert_same(AC.run(n, hw, rows, device=DEV, chunk=1), want, "one row per add")
    AC.assert_same(AC.run(n, hw, rows, device=DEV, chunk=7), want, "7 rows per add")
    AC.assert_same(AC.run(n, hw, rows, device=DEV, chunk=7, capacity=64), want, "grown from 64 matches")


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def test_invalid_observations_are_counted_by_reason():
    n, hw, rows, expect = AC.invalid_case()
    got = AC.run(n, hw, rows, device=DEV)
    assert got["stats"] == expect
    AC.assert_same(got, host("invalid", n, hw, rows))


def test_empty_atlas_and_rows_without_matches():
    from loftr_amd import KeypointAtlas
    got = KeypointAtlas(4, (10, 10), device=DEV).finalize().to_host()
    assert got["stats"]["n_keypoints"] == 0 and list(got["kp_offsets"]) == [0] * 5 and list(got["row_offsets"]) == [0]
    a = KeypointAtlas(4, (10, 10), device=DEV)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    a.add([[0, 1], [2, 3]], {"mkpts0_f": z(0, 2), "mkpts1_f": z(0, 2), "mconf": z(0), "m_bids": z(0, dt=torch.long)})
    s = a.finalize()
    assert s.row_offsets.tolist() == [0, 0, 0] and s.matches.shape == (0, 2) and s.track_len.numel() == 0 and s.kp_offsets.tolist() == [0] * 5


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_track_len", [2, 3])
def test_tracks_by_hand(min_track_len):
    n, hw, rows, want = AC.track_case()
    got = AC.run(n, hw, rows, device=DEV, min_track_len=min_track_len, chunk=4)
    w = want[min_track_len]
    assert got["track_id"].tolist() == w["track_id"] and got["track_len"].tolist() == w["track_len"] and got["track_ok"].tolist() == w["track_ok"]
    AC.assert_same(got, host(("tracks", min_track_len), n, hw, rows, min_track_len=min_track_len, chunk=4))


def test_tracks_csr_view_on_the_device():
    from loftr_amd import KeypointAtlas
    n, hw, rows, _ = AC.track_case()
    a = KeypointAtlas(n, hw, device=DEV)
    for ids, k0, k1, c, bids, _ in AC.chunks(rows, 5):
        a.add(ids, {"mkpts0_f": torch.from_numpy(k0).to(DEV), "mkpts1_f": k1, "mconf": c, "m_bids": bids})      # host and device inputs mix
    s = a.finalize()
    off, image, local = s.tracks()
    assert off.is_cuda and off.tolist() == [0, 9, 13, 15] and image.tolist() == list(range(13)) + [16, 17] and local.tolist() == [0] * 15
    off, image, local = s.tracks(consistent_only=False)
    assert off.tolist() == [0, 9, 13, 17, 19] and image[13:17].tolist() == [13, 13, 14, 15] and local[13:17].tolist() == [0, 1, 0, 0]


# ---- (e) ---------------------------------------------------------------------------------------------------------------------
def test_table_stress_equals_the_host_routine():
    n, hw, rows = AC.stress_case()
    got = AC.run(n, hw, rows, device=DEV, chunk=16)
    AC.assert_same(got, host("stress", n, hw, rows, chunk=16))
    ro = got["row_offsets"]
    assert ro[2] - ro[1] == 1 and (np.diff(ro[2:]) == 40).all()


# ---- guards that need the device ---------------------------------------------------------------------------------------------
def test_device_side_guards():
    from loftr_amd import KeypointAtlas
    d = {"mkpts0_f": torch.ones(2, 2, device=DEV), "mkpts1_f": torch.ones(2, 2, device=DEV), "mconf": torch.ones(2, device=DEV)}
    for bids, what in (([0, 2], "outside"), ([-1, 0], "outside"), ([1, 0], "ascend")):
        a = KeypointAtlas(5, (10, 10), device=DEV)
        a.add([[0, 1], [1, 2]], dict(d, m_bids=torch.tensor(bids, device=DEV)))     # device ids: no readback in add ...
        with pytest.raises(ValueError, match=what):
            a.finalize()                                                            # ... the kernel's finding is raised here
    with pytest.raises(ValueError, match="max_bytes"):
        KeypointAtlas(5, (10, 10), device=DEV, max_bytes=8 * 5 * 25 - 1)
    KeypointAtlas(5, (10, 10), device=DEV, max_bytes=8 * 5 * 25)


# ---- a real forward ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair_list_run():
    """Model and images of the e2e_batch8 golden (24 images), 16 pair-list rows without self-pairs, matched once; the chunks are kept."""
    from loftr_amd import LoFTR, evaluation
    from loftr_amd.pairs import match_pair_list
    spec = importlib.util.spec_from_file_location("make_golden_e2e", os.path.join(GOLDEN_DIR, "make_golden_e2e.py"))
    E2E = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(E2E)
    g = dict(np.load(os.path.join(GOLDEN_DIR, "e2e_batch8.npz")))
    rc = json.loads(str(g["recipe"]))
    i0, i1 = E2E.images_from_golden(g)
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    images = torch.cat([cuda(i0), cuda(i1)])
    images = torch.cat([images, images[:8].flip(-1)])
    cfg = E2E.e2e_cfg(0.0, rc)
    model = LoFTR(copy.deepcopy(cfg)).eval()
    model.load_state_dict(E2E.e2e_state_dict(model, cfg, rc["bn_strength"], rc.get("coarse_gain", 1.0)), strict=True)
    model = model.to(DEV)
    rng = np.random.default_rng(11)
    a = rng.integers(0, 24, 16)
    pairs = np.stack([a, (a + rng.integers(1, 24, 16)) % 24], 1)
    hw = tuple(images.shape[2:])
    chunks = []
    for rows, data in match_pair_list(model, pairs, lambda ids: {"image": images[ids]}, hw):
        evaluation.verify_matches(data)
        chunks.append((pairs[rows.start:rows.stop], {k: data[k] for k in ("mkpts0_f", "mkpts1_f", "mconf", "m_bids", "inliers")}))
    return hw, chunks


@pytest.mark.parametrize("masked", [False, True])
def test_real_pair_list_equals_the_host_routine(pair_list_run, masked):
    from loftr_amd import KeypointAtlas
    hw, chunks = pair_list_run
    res = {}
    for dev in (DEV, "cpu"):
        atlas = KeypointAtlas(24, hw, cell_px=2.0, device=dev)
        for ids, data in chunks:
            atlas.add(ids, {k: v.to(dev) for k, v in data.items()}, mask=data["inliers"].to(dev) if masked else None)
        res[dev] = atlas.finalize(min_track_len=2)
    got, want = res[DEV].to_host(), res["cpu"].to_host()
    AC.assert_same(got, want, masked)
    assert got["stats"]["n_matches"] == sum(d["mconf"].numel() for _, d in chunks) > 0
    off, ro, ri, tid = got["kp_offsets"], got["row_offsets"], got["row_images"], got["track_id"]
    for r in range(len(ri)):
        m = got["matches"][ro[r]:ro[r + 1]]
        assert len(np.unique(m[:, 0])) == len(m) == len(np.unique(m[:, 1]))                       # one-to-one per row
        ga, gb = m[:, 0] + off[ri[r, 0]], m[:, 1] + off[ri[r, 1]]
        assert (m >= 0).all() and (ga < off[ri[r, 0] + 1]).all() and (gb < off[ri[r, 1] + 1]).all()   # inside the images' keypoint ranges
        assert (tid[ga] >= 0).all() and (tid[ga] == tid[gb]).all()                                 # a kept match joins two keypoints of one track
