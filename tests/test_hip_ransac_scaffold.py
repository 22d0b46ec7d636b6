"""The device scaffold shared by the three batched RANSAC estimators (csrc/ransac_gpu.h: sample kernel, work list, 512-match score tile,
workspace, replay driver, 256-lane refit tree) at the shapes where a shared scaffold can go wrong: per model (five-point, homography,
fundamental matrix, P3P) one ragged batch whose pairs hold s - 1, s, s + 1 matches (s = the model's sample size), 255, 256, 257 (the
refit's lane count) and 511, 512, 513, 1025 (the score tile), with an empty pair in the middle; 0.3 px noise, 30 % outliers, seeds 0 and
11.  The assertions are those of the estimators' own "identical to the host estimator" tests: same n_inliers, same inlier mask, the model
equal after the float32 rounding."""
import numpy as np
import pytest

from loftr_amd import evaluation as EV, ops
import _absolute_pose_oracle as AO
import _geometry_oracle as GO
import test_hip_absolute_pose as TA
import test_hip_geometry as TG
import test_hip_pose as TP

pytestmark = pytest.mark.gpu
NOISE, OUTLIERS, SEEDS = 0.3, 0.3, (0, 11)
SAMPLE = {"five_point": 5, "homography": 4, "fundamental": 7, "p3p": 3}


def _counts(s):
    c = [s - 1, s, s + 1, 255, 256, 257, 511, 512, 513, 1025]
    return c[:5] + [0] + c[5:]                                                         # an empty pair in the middle of the batch


def _build(model):
    """-> pairs of the model's test module, the host estimator's results per seed."""
    rng = np.random.default_rng(31 + SAMPLE[model])
    if model == "five_point":
        pairs = [TP._pair(rng, n, NOISE, OUTLIERS) for n in _counts(5)]
        host = {seed: [EV.estimate_pose_native(*p, TP.THR, conf=TP.CONF, seed=seed) for p in pairs] for seed in SEEDS}
    elif model == "p3p":
        scenes = [AO.make_scene(rng, n, NOISE, OUTLIERS) for n in _counts(3)]
        pairs = [(sc["X"], sc["kpts"], np.asarray(sc["K"], np.float32)) for sc in scenes]
        host = {seed: [EV.estimate_absolute_pose_native(*p, TA.THR, TA.CONF, seed) for p in pairs] for seed in SEEDS}
    else:
        pairs = [GO.make_pair(rng, model, n, NOISE, OUTLIERS, TG.THR[model])[:2] for n in _counts(SAMPLE[model])]
        host = {seed: [TG.HOST[model](*p, TG.THR[model], TG.CONF, seed) for p in pairs] for seed in SEEDS}
    return pairs, host


@pytest.fixture(scope="module")
def built():
    """Per model, built on first use: the pairs and the host results for the two seeds (computed once, never modified)."""
    cache = {}

    def get(model):
        if model not in cache:
            cache[model] = _build(model)
        return cache[model]
    return get


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("model", list(SAMPLE))
def test_identical_to_the_host_estimator_at_the_scaffold_edges(built, model, seed):
    pairs, host = built(model)
    s, ref = SAMPLE[model], host[seed]
    if model == "five_point":
        TP._compare(pairs, TP._on_gpu(TP._batch(pairs), seed), seed, host=ref)
    elif model == "p3p":
        batch = TA._batch(pairs)
        TA._assert_equal_to_host(batch[2], ref, ops.estimate_absolute_poses(*TA._dev(batch), TA.THR, TA.CONF, seed))
    else:
        got = ops.estimate_geometry(*TG._dev(TG._batch(pairs)), len(pairs), model, TG.THR[model], TG.CONF, seed)
        TG._assert_equal_to_host(pairs, ref, got)
    # the batch holds what it claims to hold (properties of the host results, the reference of this test): no model below the sample
    # size or for the empty pair; at the edges of the lanes and of the tile a model that holds a good part of the 70 % true inliers
    # (0.3 px of noise on both images against the five-point threshold of 0.5 px leaves about three quarters of them) and few others
    assert [len(p[0]) for p in pairs] == [s - 1, s, s + 1, 255, 256, 0, 257, 511, 512, 513, 1025]
    assert ref[0] is None and ref[5] is None
    assert all(r is not None and 0.3 * len(p[0]) <= r[-1].sum() <= 0.8 * len(p[0]) for p, r in zip(pairs[6:], ref[6:]))
