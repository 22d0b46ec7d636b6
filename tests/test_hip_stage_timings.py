"""GPU tests of the timed paths of atlas_finalize, triangulate_tracks and model_lookup (csrc/stage_timer.h): a call with ``timings``
records an event at every stage boundary and waits for the stream; it must name the stages in order, give finite times >= 0 and
leave every output as the untimed call does, bit for bit.  Per routine the smallest multi-image case of its case table and one empty
case (M = 0 or T = 0), where some boundaries are never reached."""
import math

import numpy as np
import pytest
import torch

from loftr_amd import KeypointAtlas, _lib, build as build_mod, ops
import _atlas_cases as AC
import _model_lookup_cases as MC
import _triangulation_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def _atlas(case, timings):
    """invalid_case() (3 images, 15 matches in 2 rows) or no add at all -> to_host() of the SfmResult."""
    n_images, hw, rows = AC.invalid_case()[:3]
    atlas = KeypointAtlas(n_images, hw, 2.0, device="cuda")
    for ids, k0, k1, c, bids, mask in AC.chunks(rows if case == "small" else [], 8):
        data = {"mkpts0_f": torch.from_numpy(k0).cuda(), "mkpts1_f": torch.from_numpy(k1).cuda(), "mconf": torch.from_numpy(c).cuda(),
                "m_bids": torch.from_numpy(bids).cuda()}
        atlas.add(ids, data, mask=None if mask is None else torch.from_numpy(mask).cuda())
    out = atlas.finalize(timings=timings).to_host()
    assert out["stats"]["n_matches"] == (15 if case == "small" else 0)
    return out


def _triangulation(case, timings):
    """hand_cases() (12 tracks over 10 cameras) or T = 0 -> every output of ops.triangulate_tracks."""
    s = TC.hand_cases()[0]
    if case == "empty":
        s = dict(s, offsets=np.zeros(1, np.int64), obs_image=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2), np.float32))
    args = [torch.from_numpy(np.ascontiguousarray(s[k])).cuda() for k in ("offsets", "obs_image", "obs_xy", "K", "T")]
    out = ops.triangulate_tracks(*args, TC.THRESH_PX, TC.COS_MIN, timings=timings)
    assert out["status"].numel() == (12 if case == "small" else 0)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _model_lookup(case, timings):
    """hand_case() (16 matches against 2 images) or its first 0 matches -> the trimmed outputs and the counts."""
    c = MC.hand_case()[0]
    out = MC.run_gpu(c if case == "small" else MC.prefix(c, 0), timings=timings)
    assert len(out["match_reason"]) == (16 if case == "small" else 0)
    return out


ROUTINES = {"atlas_finalize": (_atlas, ops.ATLAS_STAGES), "triangulate_tracks": (_triangulation, ops.TRI_STAGES),
            "model_lookup": (_model_lookup, ops.MODEL_STAGES)}


@pytest.mark.parametrize("case", ["small", "empty"])
@pytest.mark.parametrize("routine", sorted(ROUTINES))
def test_a_timed_call_names_its_stages_and_changes_no_output(lib, routine, case):
    run, stages = ROUTINES[routine]
    timings = []
    timed, plain = run(case, timings), run(case, None)
    assert [name for name, _ in timings] == list(stages), timings
    assert all(isinstance(ms, float) and math.isfinite(ms) and ms >= 0.0 for _, ms in timings), timings
    assert sorted(timed) == sorted(plain)
    for k, want in plain.items():
        got = timed[k]
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (routine, case, k)
        else:
            assert got == want, (routine, case, k, got, want)
