"""GPU tests of the track triangulation (csrc/triangulate_gpu.hip): the kernels against the defining host routine, bit for
bit, for every group size; the hand-written tracks; device-side error reporting; block and wave remainders; the atlas end to end."""
import numpy as np
import pytest
import torch

from loftr_amd import Points3D, _lib, build as build_mod, triangulate_tracks
import _triangulation_cases as TC

pytestmark = pytest.mark.gpu
FIELDS = Points3D.FIELDS


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def _inputs(s, dev=None):
    t = [torch.from_numpy(np.ascontiguousarray(s[k])) for k in ("offsets", "obs_image", "obs_xy", "K", "T")]
    return [x.to(dev) for x in t] if dev else t


def _same(got, want, what):
    """torch.equal on every field (NaN positions compared by mask) and equal stats."""
    for k in FIELDS:
        g, w = getattr(got, k).cpu(), getattr(want, k)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype.is_floating_point:
            assert torch.equal(torch.isnan(g), torch.isnan(w)), (what, k, "NaN positions")
            g, w = torch.nan_to_num(g, nan=0.0), torch.nan_to_num(w, nan=0.0)
        assert torch.equal(g, w), (what, k, int((g != w).sum()))
    assert got.stats == want.stats, (what, got.stats, want.stats)


@pytest.fixture(scope="module")
def host(lib):
    """The 405-track scene through the host routine: computed once, left unchanged."""
    return triangulate_tracks(*_inputs(TC.scene()), TC.THRESH_PX, TC.MIN_ANGLE_DEG)


@pytest.mark.parametrize("group", [0, 8, 64])
def test_scene_equals_the_host_routine_for_every_group(host, group):
    pts = triangulate_tracks(*_inputs(TC.scene(), "cuda"), TC.THRESH_PX, TC.MIN_ANGLE_DEG, group=group)
    assert pts.xyz.is_cuda and pts.stats["n_ok"] >= 350
    _same(pts, host, f"group {group}")


@pytest.mark.parametrize("group", [0, 8, 64])
def test_hand_written_tracks(lib, group):
    inp, expect = TC.hand_cases()
    pts = triangulate_tracks(*_inputs(inp, "cuda"), TC.THRESH_PX, TC.MIN_ANGLE_DEG, group=group)
    res = pts.to_host()
    res["offsets"] = inp["offsets"]
    TC.check_hand(res, expect)
    _same(pts, triangulate_tracks(*_inputs(inp), TC.THRESH_PX, TC.MIN_ANGLE_DEG), f"hand, group {group}")


def test_no_tracks(lib):
    K, T = TC.camera(500, (0, 0, 0))
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    pts = triangulate_tracks(z(1, torch.int64), z(0, torch.int32), z((0, 2), torch.float32), torch.from_numpy(K[None]).cuda(), torch.from_numpy(T[None]).cuda())
    assert pts.xyz.shape == (0, 3) and pts.stats["n_tracks"] == 0 and pts.stats["n_ok"] == 0


@pytest.mark.parametrize("group", [0, 8, 64])
def test_bad_tracks_surface_as_value_errors(lib, group):
    s = TC.scene()
    off, im, xy, K, T = _inputs(s, "cuda")
    bad = im.clone()
    bad[1234] = 12
    with pytest.raises(ValueError, match="obs_image outside.*device"):
        triangulate_tracks(off, bad, xy, K, T, group=group)
    bad[1234] = -1
    with pytest.raises(ValueError, match="obs_image outside.*device"):
        triangulate_tracks(off, bad, xy, K, T, group=group)
    for edit in (lambda o: o.__setitem__(100, o[99] - 1), lambda o: o.__setitem__(0, 1), lambda o: o.__setitem__(-1, o[-1] + 5),
                 lambda o: o.__setitem__(50, 10 ** 12), lambda o: o.__setitem__(50, -(10 ** 12))):
        o = off.clone()
        edit(o)
        with pytest.raises(ValueError, match="offsets must start at 0.*device"):
            triangulate_tracks(o, im, xy, K, T, group=group)
    with pytest.raises(_lib.LoftrHipError, match="mixed"):                                 # no silent fallback
        triangulate_tracks(off, im.cpu(), xy, K, T)


@pytest.mark.parametrize("n_tracks", [1, 3, 37, 101])
def test_track_counts_that_fill_no_wave_or_block(host, n_tracks):
    """8-lane groups: 8 tracks per wave, 32 per block; 64-lane groups: 4 per block.  1, 3, 37 and 101 tracks leave idle groups in the last
    wave and block of both launches; the prefix of the scene must give the prefix of the result."""
    s = TC.scene()
    n_obs = int(s["offsets"][n_tracks])
    sub = dict(offsets=s["offsets"][:n_tracks + 1], obs_image=s["obs_image"][:n_obs], obs_xy=s["obs_xy"][:n_obs], K=s["K"], T=s["T"])
    for group in (0, 8, 64):
        pts = triangulate_tracks(*_inputs(sub, "cuda"), TC.THRESH_PX, TC.MIN_ANGLE_DEG, group=group)
        for k in FIELDS:
            g, w = getattr(pts, k).cpu(), getattr(host, k)[:n_obs if k == "obs_inlier" else n_tracks]
            assert torch.equal(torch.nan_to_num(g.float(), nan=-7.0), torch.nan_to_num(w.float(), nan=-7.0)), (n_tracks, group, k)
        assert sum(pts.stats["n_" + n] for n in ("ok", "too_short", "no_hypothesis", "small_angle", "bad_camera")) == n_tracks


def test_atlas_end_to_end(lib):
    s = TC.sfm_scene()
    want = TC.run_atlas("cpu").triangulate(s["K"], s["T"], thresh_px=0.9)
    sfm = TC.run_atlas("cuda")
    got = sfm.triangulate(s["K"], s["T"], thresh_px=0.9)
    assert got.xyz.is_cuda and 0 < got.stats["n_ok"] and got.stats["n_tracks"] == len(s["X"])
    _same(got, want, "atlas")
    for k in ("offsets", "image", "keypoint"):
        assert torch.equal(getattr(got, k).cpu(), getattr(want, k)), k
    xyz, has = got.keypoint_xyz(sfm)
    wxyz, whas = want.keypoint_xyz(TC.run_atlas("cpu"))
    assert torch.equal(has.cpu(), whas) and torch.equal(torch.nan_to_num(xyz.cpu(), nan=-7.0), torch.nan_to_num(wxyz, nan=-7.0))
