"""Keypoint atlas on the CPU: the defining host routine (loftr_atlas_host behind KeypointAtlas(device='cpu')) against the independent
oracle tests/_atlas_oracle.py -- exact equality of every output array and of the counts."""
import numpy as np
import pytest
import torch

import _atlas_cases as AC
from _atlas_oracle import atlas_oracle


def _oracle(n_images, hw, rows, cell_px=2.0, chunk=8, min_track_len=2):
    return atlas_oracle(AC.chunks(rows, chunk), n_images, hw, cell_px, min_track_len)


# ---- (a), (b) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell_px", [2.0, 0.5, 16.0])
def test_random_rows_equal_the_oracle(cell_px):
    n, hw, rows = AC.random_case()
    got = AC.run(n, hw, rows, cell_px)
    AC.assert_same(got, _oracle(n, hw, rows, cell_px), cell_px)
    st = got["stats"]
    assert st["n_rows"] == 30 and st["n_valid"] == st["n_matches"] and 0 < st["n_kept"] < st["n_valid"]
    assert got["row_offsets"][6] == got["row_offsets"][5]            # the row without a match
    if cell_px == 2.0:
        from loftr_amd import KeypointAtlas
        a = KeypointAtlas(n, hw, cell_px, device="cpu")
        assert (a.gh, a.gw) == (19, 27)
    if cell_px == 16.0:
        # several side-0 points share a cell: the mutual-best rule drops matches for side 0 as well as for side 1
        assert st["n_keypoints"] <= 12 * 3 * 4 and st["n_kept"] < st["n_valid"] // 4


def test_matches_are_one_to_one_per_row_and_in_range():
    n, hw, rows = AC.random_case()
    got = AC.run(n, hw, rows, 16.0)
    off, ro, ri = got["kp_offsets"], got["row_offsets"], got["row_images"]
    for r in range(len(ri)):
        m = got["matches"][ro[r]:ro[r + 1]]
        assert len(np.unique(m[:, 0])) == len(m) == len(np.unique(m[:, 1]))
        for side in (0, 1):
            assert (m[:, side] >= 0).all() and (m[:, side] < off[ri[r, side] + 1] - off[ri[r, side]]).all()


def test_chunking_does_not_matter():
    n, hw, rows = AC.random_case()
    want = AC.run(n, hw, rows, chunk=8)
    for chunk in (1, 7, 30):
        AC.assert_same(AC.run(n, hw, rows, chunk=chunk), want, chunk)


# ---- (c) --------------------------------------------------------------------------------------------------------------------
def test_invalid_observations_are_counted_by_reason():
    n, hw, rows, expect = AC.invalid_case()
    got = AC.run(n, hw, rows)
    assert got["stats"] == expect
    AC.assert_same(got, _oracle(n, hw, rows))
    assert np.array_equal(got["score"], np.array([0.9, 0.0, 0.0, 0.0, 0.9, 0.0], np.float32)) and list(got["row_offsets"]) == [0, 3, 3]
    assert np.signbit(got["score"]).sum() == 2                       # the -0.0 confidence is kept as it came (one keypoint per side)


def test_empty_atlas_and_rows_without_matches():
    from loftr_amd import KeypointAtlas
    a = KeypointAtlas(4, (10, 10), device="cpu")
    got = a.finalize().to_host()
    assert got["stats"]["n_keypoints"] == 0 and list(got["kp_offsets"]) == [0] * 5 and list(got["row_offsets"]) == [0]
    a = KeypointAtlas(4, (10, 10), device="cpu")
    empty = {"mkpts0_f": torch.zeros(0, 2), "mkpts1_f": torch.zeros(0, 2), "mconf": torch.zeros(0), "m_bids": torch.zeros(0, dtype=torch.long)}
    a.add([[0, 1], [2, 3]], empty)
    s = a.finalize()
    assert s.row_offsets.tolist() == [0, 0, 0] and s.matches.shape == (0, 2) and s.track_len.numel() == 0
    assert [t.numel() for t in s.tracks()] == [1, 0, 0]


# ---- (d) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_track_len", [2, 3])
def test_tracks_by_hand(min_track_len):
    n, hw, rows, want = AC.track_case()
    got = AC.run(n, hw, rows, min_track_len=min_track_len, chunk=4)
    w = want[min_track_len]
    assert got["track_id"].tolist() == w["track_id"] and got["track_len"].tolist() == w["track_len"] and got["track_ok"].tolist() == w["track_ok"]
    assert got["kp_offsets"].tolist() == list(range(14)) + [15, 16, 17, 18, 19, 19] and got["n_obs"].tolist() == [1] + [2] * 7 + [1, 3] + [1] * 3 + [1, 1, 2, 2, 1, 1]
    AC.assert_same(got, atlas_oracle(AC.chunks(rows, 4), n, hw, 2.0, min_track_len))


def test_tracks_csr_view():
    from loftr_amd import KeypointAtlas
    n, hw, rows, _ = AC.track_case()
    a = KeypointAtlas(n, hw, device="cpu")
    for ids, k0, k1, c, bids, _ in AC.chunks(rows, 5):
        a.add(ids, {"mkpts0_f": k0, "mkpts1_f": k1, "mconf": c, "m_bids": bids})
    s = a.finalize()
    off, image, local = s.tracks()
    assert off.tolist() == [0, 9, 13, 15] and image.tolist() == list(range(13)) + [16, 17] and local.tolist() == [0] * 15
    off, image, local = s.tracks(consistent_only=False)
    assert off.tolist() == [0, 9, 13, 17, 19] and image[13:17].tolist() == [13, 13, 14, 15] and local[13:17].tolist() == [0, 1, 0, 0]


# ---- (e) --------------------------------------------------------------------------------------------------------------------
def test_table_stress_equals_the_oracle():
    n, hw, rows = AC.stress_case()
    got = AC.run(n, hw, rows, chunk=16)
    AC.assert_same(got, _oracle(n, hw, rows, chunk=16))
    ro = got["row_offsets"]
    assert ro[2] - ro[1] == 1                                        # every match of row 1 shares its side-b cell: one survives
    assert (np.diff(ro[2:]) == 40).all()                             # rows 2..41: the same 40 one-to-one matches every time


# ---- (f) --------------------------------------------------------------------------------------------------------------------
def test_guards_and_bytes_needed():
    from loftr_amd import KeypointAtlas, _lib
    assert KeypointAtlas.bytes_needed(12, (37, 53), 2.0) == 8 * 12 * 19 * 27
    assert KeypointAtlas.bytes_needed(806, (480, 640), 2.0) == 8 * 806 * 240 * 320
    assert KeypointAtlas.bytes_needed(1, (10, 10), 3.0) == 8 * 4 * 4                 # fp32: 10 * (1 / 3) rounds up to 4 cells
    d = {"mkpts0_f": torch.ones(2, 2), "mkpts1_f": torch.ones(2, 2), "mconf": torch.ones(2), "m_bids": torch.tensor([0, 1])}
    new = lambda: KeypointAtlas(5, (10, 10), device="cpu")
    with pytest.raises(ValueError, match="itself"):
        new().add([[0, 1], [2, 2]], d)
    with pytest.raises(ValueError, match=r"outside \[0, 5\)"):
        new().add([[0, 1], [2, 5]], d)
    with pytest.raises(ValueError, match=r"outside \[0, 5\)"):
        new().add([[0, 1], [-1, 2]], d)
    with pytest.raises(ValueError, match=r"m_bids outside \[0, 1\)"):
        new().add([[0, 1]], d)
    with pytest.raises(ValueError, match="ascend"):
        new().add([[0, 1], [1, 2]], dict(d, m_bids=torch.tensor([1, 0])))
    with pytest.raises(ValueError, match="mask"):
        new().add([[0, 1], [1, 2]], d, mask=torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError, match="lacks"):
        new().add([[0, 1], [1, 2]], {"mkpts0_f": torch.ones(2, 2)})
    with pytest.raises(ValueError):
        KeypointAtlas(0, (10, 10), device="cpu")
    with pytest.raises(ValueError):
        KeypointAtlas(2, (10, 10), cell_px=0.0, device="cpu")
    a = new()
    a.add([[0, 1], [1, 2]], d)
    a.finalize()
    with pytest.raises(ValueError, match="finalized"):
        a.add([[0, 1], [1, 2]], d)
    with pytest.raises(ValueError, match="finalized"):
        a.finalize()
    if not torch.cuda.is_available():
        with pytest.raises(_lib.LoftrHipError):                                      # no silent fallback to the host routine
            KeypointAtlas(5, (10, 10))
