"""Inputs shared by the similarity tests (tests/test_similarity.py on the CPU, tests/test_hip_similarity.py on the GPU): the ragged batch
of estimation problems, the models to move, and the alignment case on tests/_bundle_cases.py scene_b."""
import functools

import numpy as np

import _bundle_cases as BC
import _similarity_oracle as O

THR, CONF = 0.05, 0.999
ALIGN_THR = 0.05            # scene_b's reconstruction sits within 0.0034 of the truth (profiles/registration_accuracy.txt), times a scale <= 2
MIN_CORR = MIN_INLIERS = 6  # as tests/test_registration.py


def problems(with_scale):
    """A ragged batch of about 6 300 correspondences: the smallest shapes at which each stage can go wrong.
    m0, m2: fewer than a sample (no model); m3: the sample size and the refit's minimum; m4: one spare correspondence; empty: a problem
    without correspondences between two that have some (start offsets); m257: crosses the 256 strided partials of the refit's sums (one
    thread owns two correspondences); m513: crosses the scorer's 512-correspondence LDS tile; early: >= 90 % inliers, the adaptive
    stop ends the replay after a few iterations; capped: an inlier share of 0.10-0.16, the replay runs all 1000; collinear: every
    sample degenerate (no model); coplanar: a rank-2 cross-covariance in the refit as well; adoption: the refit is rejected by the
    adoption rule; noise: no structure at all; m1100, m1300: three and more tiles, several correspondences per thread."""
    rng = np.random.default_rng(2027)
    tags, out = [], []

    def add(tag, sc):
        tags.append(tag)
        out.append((np.ascontiguousarray(sc["src"], np.float64), np.ascontiguousarray(sc["dst"], np.float64)))
    mk = lambda *a, **k: O.make_scene(rng, *a, with_scale=with_scale, thresh=THR, **k)
    add("m0", mk(0))
    add("m2", mk(2))
    add("m3", mk(3))
    add("m4", mk(4, 0.005))
    add("m257", mk(257, 0.008, 0.3))
    add("empty", mk(0))
    add("m513", mk(513, 0.008, 0.3))
    add("early", mk(700, 0.005, 0.05))
    add("capped", mk(1500, 0.008, 0.85))
    add("collinear", O.make_collinear_scene())
    add("coplanar", mk(300, 0.008, 0.3, planar=True))
    add("adoption", O.make_adoption_scene(rng, THR, with_scale=with_scale))
    add("m1100", mk(1100, 0.008, 0.4))
    add("noise", dict(src=rng.uniform(-3, 3, (300, 3)), dst=rng.uniform(-3, 3, (300, 3))))
    add("m1300", mk(1300, 0.0, 0.4))
    return tags, out


def batch(probs):
    return (np.concatenate([p[0] for p in probs]).reshape(-1, 3), np.concatenate([p[1] for p in probs]).reshape(-1, 3),
            np.concatenate([np.full(len(p[0]), b, np.int64) for b, p in enumerate(probs)]))


def model_case(N, n, seed=5):
    """A model to move: N points (f32, some NaN rows), n poses (f64) of which every third is not posed and holds NaN, one similarity."""
    rng = np.random.default_rng(seed + 1000 * N + n)
    xyz = rng.uniform(-5, 5, (N, 3)).astype(np.float32)
    xyz[::7] = np.nan
    T = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        T[i, :3, :3], T[i, :3, 3] = O.rot(rng.standard_normal(3), rng.uniform(0, np.pi)), rng.uniform(-4, 4, 3)
    posed = np.ones(n, bool)
    posed[2::3] = False
    T[~posed] = np.nan
    s, R, t = O.random_similarity(rng)
    return xyz, T, posed, np.array([s]), R, t


@functools.lru_cache(maxsize=None)
def alignment_case():
    """scene_b reconstructed on the CPU (12 cameras, all posed), and reference positions in another frame: one image unknown, a quarter
    of the images (3) grossly wrong.  -> (scene, Reconstruction, alignment scene)."""
    import loftr_amd
    s = BC.scene_b()
    R = s["T_true"][1, :3, :3] @ s["T_true"][0, :3, :3].T
    t = s["T_true"][1, :3, 3] - R @ s["T_true"][0, :3, 3]
    rec = loftr_amd.reconstruct_tracks(s["offsets"], s["obs_image"], s["obs_xy"], s["K"], (0, 1, R, t), min_corr=MIN_CORR, min_inliers=MIN_INLIERS)
    return s, rec, O.make_alignment_scene(s["T_true"], np.random.default_rng(31), ALIGN_THR)
