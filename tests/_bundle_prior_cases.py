"""Inputs of the position-prior tests (tests/test_bundle_prior.py on the CPU, tests/test_hip_bundle_prior.py on the GPU):
the scenes of _bundle_cases, _bundle_focal_cases and _bundle_shared_cases with measured camera positions -- the true centres plus
N(0, sigma) per axis -- and no fixed camera, the scaled scene the feature exists for, and the synthetic problems for the edges."""
import copy
import functools

import numpy as np
import torch

import _bundle_cases as BC
import _bundle_focal_cases as FC
import _bundle_shared_cases as SC
import _triangulation_cases as TC

SIGMA = 0.02                                                                    # position noise of the priors, world units


def centres(T):
    return -np.einsum("nji,nj->ni", T[:, :3, :3], T[:, :3, 3])


def with_priors(s, sigma=SIGMA, seed=41):
    """A copy of scene dict s with prior_xyz [n,3] = true centres + N(0, sigma), prior_sigma = sigma, prior_mask all true, and NO fixed
    camera."""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    rng = np.random.default_rng(seed)
    s["prior_xyz"] = centres(s["T_true"]) + sigma * rng.standard_normal((len(s["K"]), 3))
    s["prior_sigma"], s["prior_mask"] = float(sigma), np.ones(len(s["K"]), bool)
    s["fixed"] = np.zeros(len(s["K"]), bool)
    return s


def scaled(s, factor):
    """s with its starting poses and points scaled about their centroid (the mean of the true camera centres and points together):
    reprojection cannot see it, a gauge freedom."""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    m = np.concatenate([centres(s["T_true"]), s["X_true"]]).mean(0)
    T = s["T_cam_from_world"]
    c = m + factor * (centres(T) - m)
    T[:, :3, 3] = -np.einsum("nij,nj->ni", T[:, :3, :3], c)
    s["xyz"] = (m + factor * (s["xyz"].astype(np.float64) - m)).astype(np.float32)
    return s


@functools.lru_cache(maxsize=None)
def prior_case(name):
    """'scene_a' / 'scene_b': the pose scenes; 'focal': the detuned scene A (every image may refine); 'shared': scene B in three bodies;
    'scaled': scene B (generator seed 13) shrunk by 0.95 about its centroid -- each with priors and no fixed camera."""
    if name in ("scene_a", "scene_b"):
        return with_priors(getattr(BC, name)())
    if name == "focal":
        return with_priors(FC.focal_case("scene_a"))
    if name == "shared":
        return with_priors(SC.shared_case("bodies"))
    if name == "scaled":
        return scaled(with_priors(BC.scene_b(seed=13)), 0.95)
    raise KeyError(name)


def mode_kwargs(name, s):
    """The keywords of loftr_amd.bundle_adjust that select the mode of case `name`."""
    if name == "focal":
        return dict(refine_focal=True)
    if name == "shared":
        return dict(refine_focal=True, camera_ids=s["camera_ids"])
    return {}


def prior_kwargs(s):
    return dict(position_prior=s["prior_xyz"], prior_sigma=s["prior_sigma"], prior_mask=s["prior_mask"])


def centre_rms(T, T_true, which=None):
    d = centres(T) - centres(T_true)
    d = d if which is None else d[np.asarray(which, bool)]
    return float(np.sqrt((d * d).sum(1).mean()))


def centre_max(T, T_true):
    return float(np.linalg.norm(centres(T) - centres(T_true), axis=1).max())


# ---- synthetic problems for the edges -----------------------------------------------------------------------------------------------------
def many_cameras(n_prior, n_plain=0, n_fixed=0, seed=51):
    """n_fixed fixed cameras, then n_plain free cameras without a prior, then n_prior free cameras with one; every camera sees two of
    8 points (below 16 cameras: all of 4 points), so that each has observations and the problem stays tiny per camera.
    -> scene dict with priors (prior_mask false for the first n_fixed + n_plain) and `fixed`."""
    n = n_fixed + n_plain + n_prior
    rng = np.random.default_rng(seed)
    tracks = [[] for _ in range(8)]
    for i in range(n):
        for j in (i % 8, (3 * i + 1) % 8 if (3 * i + 1) % 8 != i % 8 else (i + 2) % 8):
            tracks[j].append(i)
    if n < 16:                                                           # too few cameras to fill eight tracks: four that all see
        tracks = [list(range(n))] * 4
    s = BC.synthetic(n, tracks, seed=seed, n_fixed=n_fixed)
    s["prior_xyz"] = centres(s["T_true"]) + SIGMA * rng.standard_normal((n, 3))
    s["prior_sigma"] = float(SIGMA)
    s["prior_mask"] = np.arange(n) >= n_fixed + n_plain
    return s


def one_camera_many_obs(n_obs, seed=52):
    """Camera 0 fixed, camera 1 free with a prior and exactly n_obs observations (n_obs tracks seen by both)."""
    s = with_priors(BC.all_see_all(2, n_obs, seed=seed, n_fixed=1))
    s["fixed"][0] = True
    return s


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------
def refine_chain(device):
    """sfm_scene() through the atlas and SfmResult.reconstruct on `device`; image 4 is then declared unposed (a NaN pose, as an image
    that never registered has); reference positions = true centres + N(0, 0.005); align alone and align(refine=...).
    -> (scene, reconstruction, reference positions, aligned, refined, alignment)."""
    s, sfm = TC.sfm_scene(), TC.run_atlas(device)
    rec = sfm.reconstruct(s["K"], min_corr=6, min_inliers=6)
    rec = copy.copy(rec)
    rec.posed, rec.T_cam_from_world = rec.posed.clone(), rec.T_cam_from_world.clone()
    rec.posed[4] = False
    rec.T_cam_from_world[4] = float("nan")
    ref = torch.from_numpy(centres(s["T"]) + 0.005 * np.random.default_rng(61).standard_normal((5, 3))).to(rec.posed.device)
    aligned, al = rec.align(ref, thresh=0.05)
    refined, al2 = rec.align(ref, thresh=0.05, refine=dict(sfm=sfm, sigma=0.005))
    assert torch.equal(al.inliers, al2.inliers) and torch.equal(al.R, al2.R)
    return s, rec, ref, aligned, refined, al
