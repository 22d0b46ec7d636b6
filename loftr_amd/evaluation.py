"""Lightning-free evaluation caller of the matching path.

Mirrors what the reference's ``PL_LoFTR.test_step`` / ``test_epoch_end`` do around ``matcher(batch)``
(src/lightning/lightning_loftr.py:95-111, 205-249) with the same function names, batch-dict keys, return
structure and ``LoFTR_pred_eval.npy`` dump format, so an evaluation script can swap

    from src.utils.metrics import compute_symmetrical_epipolar_errors, compute_pose_errors, aggregate_metrics

for ``from loftr_amd.evaluation import ...``.

* per-match epipolar errors: HIP kernel ``loftr_epipolar_errors`` (csrc/eval.hip), device tensors in, device
  tensor out -- no host round trip between the matcher and its first consumer;
* aggregation (AUC / precision over a dataset: a few thousand scalars, once per dataset) is host-side numpy like
  the reference's;
* pose estimation (metrics.py:71-140) is OpenCV in the reference (`cv2.findEssentialMat` RANSAC + `cv2.recoverPose`):
  used when cv2 is importable; otherwise `estimate_pose_native` -- the library's own five-point RANSAC + cheirality
  (csrc/pose.hip: Nister's solver, Sampson distance, OpenCV's documented parameters; host code like cv2's), or
  `estimate_pose_native_gpu` -- the same estimator with the same results, the whole batch in one GPU call.  PARITY
  UNPINNED against OpenCV (absent from this image; its sampling sequence cannot be reproduced): tests/test_pose.py
  checks the solver on exact data and the recovered pose on synthetic scenes with known ground truth;
* beyond the reference's evaluation: geometric verification without intrinsics (`verify_matches`: homography / fundamental
  matrix, csrc/geometry*.hip) and metric localisation from matches and a depth map (`localize`: lifting + P3P RANSAC,
  csrc/absolute_pose*.hip), each one GPU call per batch with a host estimator that defines the result;
* poses of queries localised against a triangulated model (`loftr_amd.localization.QueryLocalizer.solve`, no depth maps) are scored
  with `absolute_pose_error` and `localization_recall`, like `localize`'s.
"""
import os

import numpy as np
import torch

from . import ops


# ---- per-batch metrics ------------------------------------------------------------------------------------
def compute_symmetrical_epipolar_errors(data):
    """metrics.py:50-68.  Update: data['epi_errs'] float32 [M] (device tensor)."""
    data.update({"epi_errs": ops.epipolar_errors(data["mkpts0_f"], data["mkpts1_f"], data["m_bids"],
                                                 data["T_0to1"].to(torch.float32), data["K0"].to(torch.float32),
                                                 data["K1"].to(torch.float32))})


def _angle_deg(cosine):
    return float(np.degrees(np.arccos(np.clip(cosine, -1.0, 1.0))))


def relative_pose_error(T_0to1, R, t, ignore_gt_t_thr=0.0):
    """metrics.py:12-28 -> (t_err, R_err) in degrees: angle between the translation directions (sign-ambiguous, so
    folded to [0, 90]; ignored when the ground-truth baseline is shorter than `ignore_gt_t_thr`) and the geodesic
    angle between the rotations."""
    gt_R, gt_t = T_0to1[:3, :3], T_0to1[:3, 3]
    baseline = np.linalg.norm(gt_t)
    if baseline < ignore_gt_t_thr:
        t_err = 0
    else:
        ang = _angle_deg(np.dot(t, gt_t) / (np.linalg.norm(t) * baseline))
        t_err = min(ang, 180.0 - ang)
    R_err = abs(_angle_deg((np.trace(R.T @ gt_R) - 1.0) / 2.0))
    return t_err, R_err


def _normalise(kpts, K):
    """pixels -> normalised camera coordinates (the reference indexes K[[0,1],[2,2]] / K[[0,1],[0,1]], metrics.py:75-76)."""
    return (kpts - K[:2, 2][None]) / np.array([K[0, 0], K[1, 1]])[None]


def estimate_pose_cv2(kpts0, kpts1, K0, K1, thresh, conf=0.99999):
    """metrics.py:71-100: OpenCV 5-point RANSAC on normalised points (threshold = pixels / mean focal length as the
    reference computes it), then the cheirality vote over the returned essential matrices.  Needs cv2."""
    import cv2
    if len(kpts0) < 5:
        return None
    n0, n1 = _normalise(kpts0, K0), _normalise(kpts1, K1)
    focal = np.mean([K0[0, 0], K1[1, 1], K0[0, 0], K1[1, 1]])          # (sic) the reference's choice of entries
    E, mask = cv2.findEssentialMat(n0, n1, np.eye(3), threshold=thresh / focal, prob=conf, method=cv2.RANSAC)
    if E is None:
        return None
    candidates = []
    for Ei in np.split(E, len(E) // 3):
        votes, R, t, _ = cv2.recoverPose(Ei, n0, n1, np.eye(3), 1e9, mask=mask)
        candidates.append((votes, R, t[:, 0]))
    votes, R, t = max(candidates, key=lambda c: c[0], default=(0, None, None))   # first maximum, like the reference's `>`
    return None if votes <= 0 else (R, t, mask.ravel() > 0)


def _cfg_get(config, path, default):
    node = config
    for key in path:
        if node is None:
            return default
        node = node.get(key) if isinstance(node, dict) else getattr(node, key, None)
    return default if node is None else node


def estimate_pose_native(kpts0, kpts1, K0, K1, thresh, conf=0.99999, seed=0):
    """estimate_pose (metrics.py:72-98) on the library's own five-point RANSAC + cheirality (csrc/pose.hip, host code;
    parity against cv2 unpinned).  Returns (R [3,3], t [3], inlier mask [M] bool) or None like the reference."""
    import ctypes as C
    from . import _lib
    k0 = np.ascontiguousarray(kpts0, np.float32).reshape(-1, 2)
    k1 = np.ascontiguousarray(kpts1, np.float32).reshape(-1, 2)
    M = k0.shape[0]
    if M < 5:
        return None
    K0c, K1c = np.ascontiguousarray(K0, np.float32), np.ascontiguousarray(K1, np.float32)
    R, t = np.empty((3, 3), np.float32), np.empty(3, np.float32)
    inl = np.zeros(M, np.uint8)
    n = C.c_long(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().loftr_estimate_pose(ptr(k0), ptr(k1), M, ptr(K0c), ptr(K1c), float(thresh), float(conf), int(seed),
                                               ptr(R), ptr(t), ptr(inl), C.byref(n)), "loftr_estimate_pose")
    if n.value < 0:
        return None
    return R.astype(np.float64), t.astype(np.float64), inl.astype(bool)


def estimate_pose_native_gpu(kpts0, kpts1, K0, K1, thresh, conf=0.99999, seed=0):
    """estimate_pose_native on the GPU (ops.estimate_poses, csrc/pose_gpu.hip): the same result for the same seed -- same
    inlier mask, R and t equal after the float32 rounding.  Called on one pair it takes host arrays like estimate_pose_native;
    passed as compute_pose_errors' estimator it is the explicit form of on_missing='native_gpu' and runs the whole batch in
    one call."""
    k0 = np.ascontiguousarray(kpts0, np.float32).reshape(-1, 2)
    if k0.shape[0] < 5:
        return None
    k0 = torch.as_tensor(k0).cuda()
    k1 = torch.as_tensor(np.ascontiguousarray(kpts1, np.float32).reshape(-1, 2)).cuda()
    K = [torch.as_tensor(np.ascontiguousarray(k, np.float32)).reshape(1, 3, 3).cuda() for k in (K0, K1)]
    R, t, inl, n = ops.estimate_poses(k0, k1, torch.zeros(k0.shape[0], dtype=torch.int64, device=k0.device), K[0], K[1], thresh, conf,
                                      seed)
    if int(n[0]) < 0:
        return None
    return R[0].cpu().numpy().astype(np.float64), t[0].cpu().numpy().astype(np.float64), inl.cpu().numpy()


def _poses_native_gpu(data, pixel_thr, conf):
    """The batch path of estimate_pose_native_gpu: one ops.estimate_poses call for every pair of `data` -> per pair
    (R, t, inlier mask) or None, as the per-pair estimators return them."""
    dev = data["mkpts0_f"].device if data["mkpts0_f"].is_cuda else torch.device("cuda")
    f32 = lambda k: data[k].to(device=dev, dtype=torch.float32)
    m_bids = data["m_bids"].to(device=dev, dtype=torch.int64)
    R, t, inl, n = ops.estimate_poses(f32("mkpts0_f"), f32("mkpts1_f"), m_bids, f32("K0"), f32("K1"), pixel_thr, conf)
    R, t, inl, n, bids = R.cpu().numpy(), t.cpu().numpy(), inl.cpu().numpy(), n.cpu().numpy(), m_bids.cpu().numpy()
    return [None if n[b] < 0 else (R[b].astype(np.float64), t[b].astype(np.float64), inl[bids == b]) for b in range(len(n))]


# ---- geometric verification without intrinsics (csrc/geometry.hip, csrc/geometry_gpu.hip) -------------------------------
def _geometry_native(kpts0, kpts1, model, thresh, conf, seed):
    import ctypes as C
    from . import _lib
    k0 = np.ascontiguousarray(kpts0, np.float32).reshape(-1, 2)
    k1 = np.ascontiguousarray(kpts1, np.float32).reshape(-1, 2)
    M = k0.shape[0]
    if M < (4 if model == "homography" else 7):
        return None
    mat, inl, n = np.zeros(9, np.float32), np.zeros(M, np.uint8), C.c_long(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().loftr_estimate_geometry(ptr(k0), ptr(k1), M, ops.GEOMETRY_MODELS[model], float(thresh), float(conf), int(seed),
                                                   ptr(mat), ptr(inl), C.byref(n)), "loftr_estimate_geometry")
    if n.value < 0:
        return None
    return mat.reshape(3, 3).astype(np.float64), inl.astype(bool)


def _geometry_native_gpu(kpts0, kpts1, model, thresh, conf, seed):
    k0 = np.ascontiguousarray(kpts0, np.float32).reshape(-1, 2)
    if k0.shape[0] < (4 if model == "homography" else 7):
        return None
    k0 = torch.as_tensor(k0).cuda()
    k1 = torch.as_tensor(np.ascontiguousarray(kpts1, np.float32).reshape(-1, 2)).cuda()
    mat, inl, n = ops.estimate_geometry(k0, k1, torch.zeros(k0.shape[0], dtype=torch.int64, device=k0.device), 1, model, thresh, conf, seed)
    if int(n[0]) < 0:
        return None
    return mat[0].cpu().numpy().astype(np.float64), inl.cpu().numpy()


def estimate_homography_native(kpts0, kpts1, thresh=3.0, conf=0.999, seed=0):
    """Homography x1 ~ H x0 of one pair from pixel matches [M,2] (numpy): 4-point RANSAC + least-squares refit, the library's
    own host estimator (csrc/geometry.hip; parity against cv2.findHomography unpinned).  thresh is the forward transfer error in
    pixels.  Returns (H [3,3] with unit Frobenius norm, inlier mask [M] bool), or None without a model (fewer than 4 matches, only
    degenerate samples, fewer than 4 inliers)."""
    return _geometry_native(kpts0, kpts1, "homography", thresh, conf, seed)


def estimate_fundamental_native(kpts0, kpts1, thresh=1.0, conf=0.999, seed=0):
    """Fundamental matrix x1^T F x0 = 0 of one pair from pixel matches [M,2] (numpy): 7-point RANSAC + rank-2 least-squares
    refit, the library's own host estimator (csrc/geometry.hip; parity against cv2.findFundamentalMat unpinned).  thresh is the
    Sampson distance in pixels.  Returns (F [3,3] with unit Frobenius norm, inlier mask [M] bool), or None without a model."""
    return _geometry_native(kpts0, kpts1, "fundamental", thresh, conf, seed)


def estimate_homography_native_gpu(kpts0, kpts1, thresh=3.0, conf=0.999, seed=0):
    """estimate_homography_native on the GPU (ops.estimate_geometry): the same result for the same seed -- same inlier mask, H equal
    after the float32 rounding."""
    return _geometry_native_gpu(kpts0, kpts1, "homography", thresh, conf, seed)


def estimate_fundamental_native_gpu(kpts0, kpts1, thresh=1.0, conf=0.999, seed=0):
    """estimate_fundamental_native on the GPU (ops.estimate_geometry): the same result for the same seed."""
    return _geometry_native_gpu(kpts0, kpts1, "fundamental", thresh, conf, seed)


def verify_matches(data, model="fundamental", thresh_px=None, conf=0.999, seed=0):
    """Geometric verification of every pair of the batch dict that forward / match_pairs leaves, in one GPU call (ops.estimate_geometry):
    no intrinsics needed, the keypoints stay on the device.  Update: data['inliers'] bool [M] in match order, data['F'] (model
    'fundamental') or data['H'] ('homography') float32 [N,3,3] with unit Frobenius norm (zero where no model was found) and
    data['n_inliers'] int64 [N] (-1 there).  N is data['bs'].
    Defaults: thresh_px = 1.0 px Sampson distance for the fundamental matrix, 3.0 px transfer error for the homography, conf 0.999,
    seed 0.  They are this project's choice (common settings of such verifiers); nothing in the reference fixes them."""
    if thresh_px is None:
        thresh_px = 3.0 if model == "homography" else 1.0
    N = int(data["bs"]) if "bs" in data else int(data["image0"].shape[0])
    mat, inl, n = ops.estimate_geometry(data["mkpts0_f"].to(torch.float32), data["mkpts1_f"].to(torch.float32), data["m_bids"].to(torch.int64),
                                        N, model, thresh_px, conf, seed)
    data.update({"inliers": inl, "H" if model == "homography" else "F": mat, "n_inliers": n})
    return data


def focal_errors(focal, K_gt):
    """Relative focal error per image, |f / f_gt - 1| with f_gt the mean of the two diagonal entries of ``K_gt [n,3,3]``: ``focal [n]``
    (e.g. ``ViewGraphCalibration.focal``), or ``[n,3,3]`` intrinsics, read the same way.  numpy in, numpy out (tensors are copied)."""
    to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    f, Kg = to_np(focal).astype(np.float64), to_np(K_gt).astype(np.float64)
    if f.ndim == 3:
        f = 0.5 * (f[:, 0, 0] + f[:, 1, 1])
    if Kg.ndim != 3 or Kg.shape[1:] != (3, 3) or f.shape != (Kg.shape[0],):
        raise ValueError(f"focal_errors: expected focal [n] (or [n,3,3]) and K_gt [n,3,3], got {f.shape}, {Kg.shape}")
    return np.abs(f / (0.5 * (Kg[:, 0, 0] + Kg[:, 1, 1])) - 1.0)


# ---- absolute pose from matches and depth (csrc/absolute_pose.hip, csrc/absolute_pose_gpu.hip) ---------------------------
def estimate_absolute_pose_native(pts3d, kpts, K, thresh=3.0, conf=0.999, seed=0):
    """Camera pose x_cam = R X + t of one image from 2D-3D matches (numpy: pts3d [M,3], kpts [M,2] pixels, K [3,3]): P3P RANSAC + a
    Gauss-Newton refit on the reprojection error, the library's own host estimator (csrc/absolute_pose.hip; parity against
    cv2.solvePnPRansac unpinned).  thresh is the reprojection error in pixels; t is in the units of pts3d.
    Returns (R [3,3], t [3], inlier mask [M] bool), or None without a model (fewer than 3 matches, only degenerate samples)."""
    import ctypes as C
    from . import _lib
    X = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
    k = np.ascontiguousarray(kpts, np.float32).reshape(-1, 2)
    M = X.shape[0]
    if M < 3:
        return None
    Kc = np.ascontiguousarray(K, np.float32).reshape(3, 3)
    R, t, inl, n = np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros(M, np.uint8), C.c_long(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().loftr_estimate_absolute_pose(ptr(X), ptr(k), M, ptr(Kc), float(thresh), float(conf), int(seed), ptr(R), ptr(t),
                                                        ptr(inl), C.byref(n)), "loftr_estimate_absolute_pose")
    if n.value < 0:
        return None
    return R.reshape(3, 3).astype(np.float64), t.astype(np.float64), inl.astype(bool)


def estimate_absolute_pose_native_gpu(pts3d, kpts, K, thresh=3.0, conf=0.999, seed=0):
    """estimate_absolute_pose_native on the GPU (ops.estimate_absolute_poses): the same result for the same seed -- same inlier mask,
    R and t equal after the float32 rounding."""
    X = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
    if X.shape[0] < 3:
        return None
    X = torch.as_tensor(X).cuda()
    k = torch.as_tensor(np.ascontiguousarray(kpts, np.float32).reshape(-1, 2)).cuda()
    Kc = torch.as_tensor(np.ascontiguousarray(K, np.float32)).reshape(1, 3, 3).cuda()
    R, t, inl, n = ops.estimate_absolute_poses(X, k, torch.zeros(X.shape[0], dtype=torch.int64, device=X.device), Kc, thresh, conf, seed)
    if int(n[0]) < 0:
        return None
    return R[0].cpu().numpy().astype(np.float64), t[0].cpu().numpy().astype(np.float64), inl.cpu().numpy()


def localize(data, db_side=0, depth=None, K_db=None, K_query=None, T_world_from_db=None, thresh_px=3.0, conf=0.999, seed=0):
    """Metric pose of the query image of every pair of the batch dict that forward / match_pairs leaves, from the matches and the depth
    map of the other (database) image, in GPU calls only: the database keypoints are lifted to 3D (ops.lift_keypoints: nearest depth,
    the reference's warp_kpts arithmetic), matches without depth are dropped, and the query camera is resected from the 2D-3D
    matches (ops.estimate_absolute_poses: P3P RANSAC + Gauss-Newton refit), one call for the whole batch.
    db_side 0: image 0 is the database image (defaults data['depth0'], data['K0'], query intrinsics data['K1']); db_side 1: the roles
    swapped (data['depth1'], data['K1'], data['K0']).  T_world_from_db [N,4,4] (database camera to world) puts the 3D points into a
    world frame; without it they stay in the database camera's frame and (R, t) estimates T_0to1 (db_side 0) / T_1to0 (db_side 1), with
    a metric translation.
    Update: data['R_abs'] float32 [N,3,3], data['t_abs'] float32 [N,3] (x_query = R X + t; zero where no model was found),
    data['inliers'] bool [M] in match order (False for dropped matches), data['n_inliers'] int64 [N] (-1 without a model) and
    data['n_lifted'] int64 [N] (matches with a valid depth).  N is data['bs'].
    Defaults: thresh_px = 3.0 px reprojection error, conf 0.999, seed 0.  They are this project's choice (common settings of such
    localisers); nothing in the reference fixes them."""
    if db_side not in (0, 1):
        raise ValueError(f"localize: db_side must be 0 or 1, got {db_side!r}")
    d, q = str(db_side), str(1 - db_side)
    N = int(data["bs"]) if "bs" in data else int(data["image0"].shape[0])
    f32 = lambda t: t.to(torch.float32)
    depth = f32(data["depth" + d] if depth is None else depth)
    K_db = f32(data["K" + d] if K_db is None else K_db)
    K_query = f32(data["K" + q] if K_query is None else K_query)
    T = None if T_world_from_db is None else f32(T_world_from_db)
    m_bids = data["m_bids"].to(torch.int64)
    pts3d, valid = ops.lift_keypoints(f32(data["mkpts" + d + "_f"]), m_bids, depth, K_db, T)
    keep = valid.nonzero().squeeze(1)                        # boolean selection keeps the grouping by ascending pair
    R, t, inl, n = ops.estimate_absolute_poses(pts3d[keep], f32(data["mkpts" + q + "_f"])[keep], m_bids[keep], K_query, thresh_px, conf, seed)
    inliers = torch.zeros_like(valid)
    inliers[keep] = inl
    n_lifted = torch.zeros(N, dtype=torch.int64, device=valid.device).index_add_(0, m_bids, valid.to(torch.int64))
    data.update({"R_abs": R, "t_abs": t, "inliers": inliers, "n_inliers": n, "n_lifted": n_lifted})
    return data


# ---- 3D similarity between two point sets (csrc/similarity.hip, csrc/similarity_gpu.hip) ----------------------
def estimate_similarity_native(src, dst, with_scale=True, thresh=0.05, conf=0.999, seed=0):
    """dst ~ s R src + t from 3D-3D correspondences (numpy: src [M,3], dst [M,3]): RANSAC over 3-point Kabsch / Umeyama closed forms
    + the same closed form as the refit, the library's own host estimator (csrc/similarity.hip).  with_scale=False fits a rigid
    motion (s == 1.0 exactly).  thresh is the distance |s R src + t - dst| in the units of dst.
    Returns (s, R [3,3], t [3], inlier mask [M] bool) in float64, or None without a model (fewer than 3 correspondences, only
    degenerate samples)."""
    import ctypes as C
    from . import _lib
    a = np.ascontiguousarray(src, np.float64).reshape(-1, 3)
    b = np.ascontiguousarray(dst, np.float64).reshape(-1, 3)
    M = a.shape[0]
    if b.shape[0] != M:
        raise ValueError(f"estimate_similarity_native: src and dst differ in length ({M} and {b.shape[0]})")
    if M < 3:
        return None
    s, R, t, inl, n = np.zeros(1), np.zeros(9), np.zeros(3), np.zeros(M, np.uint8), C.c_long(-1)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().loftr_estimate_similarity(ptr(a), ptr(b), M, int(bool(with_scale)), float(thresh), float(conf), int(seed), ptr(s),
                                                     ptr(R), ptr(t), ptr(inl), C.byref(n)), "loftr_estimate_similarity")
    if n.value < 0:
        return None
    return float(s[0]), R.reshape(3, 3), t, inl.astype(bool)


def estimate_similarity_native_gpu(src, dst, with_scale=True, thresh=0.05, conf=0.999, seed=0):
    """estimate_similarity_native on the GPU (ops.estimate_similarities): the same result for the same seed, bit for bit."""
    a = np.ascontiguousarray(src, np.float64).reshape(-1, 3)
    b = np.ascontiguousarray(dst, np.float64).reshape(-1, 3)
    if b.shape[0] != a.shape[0]:
        raise ValueError(f"estimate_similarity_native_gpu: src and dst differ in length ({a.shape[0]} and {b.shape[0]})")
    if a.shape[0] < 3:
        return None
    a, b = torch.as_tensor(a).cuda(), torch.as_tensor(b).cuda()
    s, R, t, inl, n = ops.estimate_similarities(a, b, torch.zeros(a.shape[0], dtype=torch.int64, device=a.device), 1, with_scale, thresh, conf, seed)
    if int(n[0]) < 0:
        return None
    return float(s[0]), R[0].cpu().numpy(), t[0].cpu().numpy(), inl.cpu().numpy()


def register_depth(data, thresh=0.05, conf=0.999, seed=0, depth0=None, depth1=None, K0=None, K1=None):
    """Rigid motion between the two cameras of every pair of the batch dict that forward / match_pairs leaves, from the matches and a
    depth map on BOTH sides (RGB-D streams, ScanNet), in GPU calls only: the keypoints of each side are lifted to 3D in their own
    camera's frame (ops.lift_keypoints), matches without depth on either side are dropped, and a rigid 3D-3D fit
    (ops.estimate_similarities with with_scale=False) runs for the whole batch in one call.  Unlike the five-point path it is metric
    and does not degenerate on planar scenes, small baselines or pure rotation.
    depth0 / depth1 / K0 / K1 default to the batch's own entries.
    Update: data['R_3d'] float32 [N,3,3], data['t_3d'] float32 [N,3] (x_1 = R x_0 + t, an estimate of T_0to1; zero where no model was
    found), data['inliers'] bool [M] in match order (False for dropped matches), data['n_inliers'] int64 [N] (-1 without a model) and
    data['n_lifted'] int64 [N] (matches with a valid depth on both sides).  N is data['bs'].
    Defaults: thresh = 0.05 in the units of the depth (5 cm for metric depth), conf 0.999, seed 0.  They are this project's choice
    (a common setting for indoor RGB-D registration); nothing in the reference fixes them."""
    N = int(data["bs"]) if "bs" in data else int(data["image0"].shape[0])
    f32 = lambda t: t.to(torch.float32)
    m_bids = data["m_bids"].to(torch.int64)
    x0, v0 = ops.lift_keypoints(f32(data["mkpts0_f"]), m_bids, f32(data["depth0"] if depth0 is None else depth0), f32(data["K0"] if K0 is None else K0))
    x1, v1 = ops.lift_keypoints(f32(data["mkpts1_f"]), m_bids, f32(data["depth1"] if depth1 is None else depth1), f32(data["K1"] if K1 is None else K1))
    valid = v0 & v1
    keep = valid.nonzero().squeeze(1)                        # boolean selection keeps the grouping by ascending pair
    _, R, t, inl, n = ops.estimate_similarities(x0[keep], x1[keep], m_bids[keep], N, False, thresh, conf, seed)
    inliers = torch.zeros_like(valid)
    inliers[keep] = inl
    n_lifted = torch.zeros(N, dtype=torch.int64, device=valid.device).index_add_(0, m_bids, valid.to(torch.int64))
    data.update({"R_3d": R.to(torch.float32), "t_3d": t.to(torch.float32), "inliers": inliers, "n_inliers": n, "n_lifted": n_lifted})
    return data


def trajectory_errors(T_est, posed, T_gt, thresh=None, with_scale=True, conf=0.999, seed=0):
    """Errors of estimated camera poses against the truth after aligning the two frames by a similarity of the camera centres (the
    reconstruction's frame and scale are arbitrary): T_est [n,4,4], T_gt [n,4,4] camera-from-world, posed [n] bool.
    thresh None: one least-squares fit (Umeyama) over all posed images; otherwise the robust fit of alignment.align_centres with that
    threshold (units of the truth), which tolerates grossly wrong poses.
    -> (rot_deg [n], centre_err [n]) float64 numpy, NaN for images without a pose; with fewer than 3 posed images, or without a
    model, every entry is NaN."""
    from .alignment import align_centres, fit_centres
    T = torch.as_tensor(np.asarray(T_est.cpu() if isinstance(T_est, torch.Tensor) else T_est, np.float64))
    G = np.asarray(T_gt.cpu() if isinstance(T_gt, torch.Tensor) else T_gt, np.float64)
    p = torch.as_tensor(np.asarray(posed.cpu() if isinstance(posed, torch.Tensor) else posed).astype(bool))
    n = T.shape[0]
    rot, cen = np.full(n, np.nan), np.full(n, np.nan)
    ref = torch.as_tensor(-np.einsum("nji,nj->ni", G[:, :3, :3], G[:, :3, 3]))
    al = fit_centres(T, p, ref, p, with_scale) if thresh is None else align_centres(T, p, ref, p, thresh, with_scale, conf, seed)
    if al.n_inliers < 0:
        return rot, cen
    _, T2 = ops.transform_model(torch.zeros(0, 3), T, p, al.s, al.R, al.t)
    T2 = T2.numpy()
    for i in np.flatnonzero(p.numpy()):
        R_e, R_g = T2[i, :3, :3], G[i, :3, :3]
        rot[i] = abs(_angle_deg((np.trace(R_e.T @ R_g) - 1.0) / 2.0))
        cen[i] = np.linalg.norm(-R_e.T @ T2[i, :3, 3] + R_g.T @ G[i, :3, 3])
    return rot, cen


def global_rotation_errors(R, R_gt, mask=None):
    """Angle between estimated and true camera-from-world rotations, degrees per image, after the one free rotation is removed:
    ``R [n,3,3]`` is defined up to ``R_i G`` (rotation averaging fixes ``R[root] = I``), so ``G`` is taken as the chordal mean of
    ``R_i^T R_gt_i`` over the images of ``mask`` (default: those with a finite ``R``), the 3 x 3 polar factor with ``det = +1``, computed
    with torch on the host.  Images outside the mask get NaN."""
    R = torch.as_tensor(R, dtype=torch.float64).cpu()
    R_gt = torch.as_tensor(R_gt, dtype=torch.float64).cpu()
    m = torch.isfinite(R).reshape(R.shape[0], -1).all(1) if mask is None else torch.as_tensor(mask).cpu().bool()
    out = torch.full((R.shape[0],), float("nan"), dtype=torch.float64)
    if not bool(m.any()):
        return out
    U, _, Vh = torch.linalg.svd((R[m].transpose(1, 2) @ R_gt[m]).sum(0))
    D = torch.diag(torch.tensor([1.0, 1.0, float(torch.sign(torch.linalg.det(U @ Vh)))], dtype=torch.float64))
    G = U @ D @ Vh
    rel = (R[m] @ G) @ R_gt[m].transpose(1, 2)
    # the chord |R - I|_F = 2 sqrt(2) sin(angle / 2) keeps its precision near zero, where acos of the trace loses it
    chord = (rel - torch.eye(3, dtype=torch.float64)).reshape(-1, 9).norm(dim=1)
    out[m] = torch.rad2deg(2.0 * torch.asin((chord / (2.0 * 2.0 ** 0.5)).clamp(max=1.0)))
    return out


def absolute_pose_error(T_gt, R, t):
    """(rotation error in degrees, distance between the camera centres in the units of the depth) of an estimate x_cam = R X + t
    against the ground truth T_gt [4,4] or [3,4] (same convention): the geodesic angle of R^T R_gt and |R^T t - R_gt^T t_gt|, the two
    figures the localisation benchmarks (Aachen, InLoc) threshold."""
    T_gt = np.asarray(T_gt.cpu() if isinstance(T_gt, torch.Tensor) else T_gt, np.float64)
    R = np.asarray(R.cpu() if isinstance(R, torch.Tensor) else R, np.float64)
    t = np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t, np.float64)
    gt_R, gt_t = T_gt[:3, :3], T_gt[:3, 3]
    R_err = abs(_angle_deg((np.trace(R.T @ gt_R) - 1.0) / 2.0))
    return R_err, float(np.linalg.norm(R.T @ t - gt_R.T @ gt_t))


def localization_recall(t_errs, R_errs, thresholds=((0.25, 2), (0.5, 5), (5, 10))):
    """Fraction of queries localised within each (distance, degrees) pair -- by default the Aachen Day-Night triples
    (0.25 m, 2 deg), (0.5 m, 5 deg), (5 m, 10 deg).  A failed query carries inf errors.  -> {'recall@0.25/2': ...}."""
    t_errs, R_errs = np.asarray(t_errs, np.float64), np.asarray(R_errs, np.float64)
    out = {}
    for dt, dr in thresholds:
        out[f"recall@{dt:g}/{dr:g}"] = float(np.mean((t_errs <= dt) & (R_errs <= dr))) if len(t_errs) else 0.0
    return out


def homography_corner_errors(H, H_gt, hw):
    """Mean corner transfer error per pair in pixels: the four corners of an image of size hw = (h, w) mapped by the estimate and by
    the ground truth, the mean of the four distances (the HPatches protocol of the LoFTR paper; its AUC at 3 / 5 / 10 px is homography_auc(errs)).
    H, H_gt [N,3,3] or [3,3] (any scale); a pair whose estimate is all zero (no model) gets inf."""
    H = np.asarray(H.cpu() if isinstance(H, torch.Tensor) else H, np.float64).reshape(-1, 3, 3)
    G = np.asarray(H_gt.cpu() if isinstance(H_gt, torch.Tensor) else H_gt, np.float64).reshape(-1, 3, 3)
    h, w = hw
    corners = np.array([[0, 0, 1], [w - 1, 0, 1], [w - 1, h - 1, 1], [0, h - 1, 1]], np.float64)
    errs = []
    for A, B in zip(H, G):
        if not A.any():
            errs.append(np.inf)
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            a, b = corners @ A.T, corners @ B.T
            d = np.linalg.norm(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:], axis=1)
        errs.append(float(np.mean(d)) if np.isfinite(d).all() else np.inf)
    return np.array(errs)


_WARNED_NATIVE = []


def compute_pose_errors(data, config=None, estimator=None, on_missing="raise"):
    """metrics.py:103-140.  Update: data['R_errs'], ['t_errs'] (lists of float), ['inliers'] (list of bool arrays) and
    data['pose_estimator'] (which estimator produced them: the AUCs depend on it).

    estimator(kpts0, kpts1, K0, K1, pixel_thr, conf=) -> (R, t, inlier_mask) | None.  Default: OpenCV, as the reference
    uses.  When OpenCV is not importable, `on_missing` decides -- never silently:
      'raise'  (default) ImportError, like the reference's `import cv2`;
      'inf'    record R_err = t_err = inf for every pair (the reference's value for a failed estimate);
      'native' the library's five-point RANSAC (csrc/pose.hip).  PARITY UNPINNED against cv2.findEssentialMat /
               recoverPose (own sampling sequence): a one-time warning says so; passing estimator=estimate_pose_native is
               the explicit form of the same opt-in;
      'native_gpu' the same estimator on the GPU for the whole batch in one call (csrc/pose_gpu.hip): the same R_errs,
               t_errs and inliers as 'native', the same warning; estimator=estimate_pose_native_gpu is its explicit form."""
    pixel_thr = _cfg_get(config, ("TRAINER", "RANSAC_PIXEL_THR"), 0.5)
    conf = _cfg_get(config, ("TRAINER", "RANSAC_CONF"), 0.99999)
    if on_missing not in ("raise", "inf", "native", "native_gpu"):
        raise ValueError(f"on_missing={on_missing!r}: expected 'raise', 'inf', 'native' or 'native_gpu'")
    name = getattr(estimator, "__name__", "custom") if estimator is not None else None
    if estimator is None:
        try:
            import cv2  # noqa: F401
            estimator, name = estimate_pose_cv2, "cv2"
        except ImportError:
            if on_missing == "raise":
                raise ImportError("compute_pose_errors needs OpenCV (cv2.findEssentialMat / recoverPose, metrics.py:72-98); pass "
                                  "on_missing='native' (library five-point RANSAC, parity unpinned) or 'inf', or an estimator")
            if on_missing in ("native", "native_gpu"):
                estimator = estimate_pose_native if on_missing == "native" else estimate_pose_native_gpu
                name = estimator.__name__
                if not _WARNED_NATIVE:
                    _WARNED_NATIVE.append(True)
                    import warnings
                    warnings.warn("OpenCV is not importable: pose errors / AUC come from loftr_amd's five-point RANSAC, whose "
                                  "parity with cv2.findEssentialMat(RANSAC) + recoverPose is unpinned", stacklevel=2)
            else:
                name = "none (inf)"
    data["pose_estimator"] = name
    data.update({"R_errs": [], "t_errs": [], "inliers": []})
    batched = _poses_native_gpu(data, pixel_thr, conf) if estimator is estimate_pose_native_gpu else None
    m_bids = data["m_bids"].cpu().numpy()
    pts0, pts1 = data["mkpts0_f"].cpu().numpy(), data["mkpts1_f"].cpu().numpy()
    K0, K1, T = data["K0"].cpu().numpy(), data["K1"].cpu().numpy(), data["T_0to1"].cpu().numpy()
    for bs in range(K0.shape[0]):
        mask = m_bids == bs
        if batched is not None:
            ret = batched[bs]
        else:
            ret = None if estimator is None else estimator(pts0[mask], pts1[mask], K0[bs], K1[bs], pixel_thr, conf=conf)
        if ret is None:
            data["R_errs"].append(np.inf)
            data["t_errs"].append(np.inf)
            data["inliers"].append(np.array([]).astype(bool))
        else:
            R, t, inliers = ret
            t_err, R_err = relative_pose_error(T[bs], R, t, ignore_gt_t_thr=0.0)
            data["R_errs"].append(R_err)
            data["t_errs"].append(t_err)
            data["inliers"].append(inliers)


# ---- dataset-level aggregation (host, once per dataset) ----------------------------------------------------
def _area_under_recall(sorted_errors, recall, thr):
    """Area (trapezoid rule) under the recall-vs-error step curve from 0 to `thr`, the curve held flat from the last
    error below `thr` up to `thr`."""
    k = int(np.searchsorted(sorted_errors, thr))
    x = np.append(sorted_errors[:k], thr)
    y = np.append(recall[:k], recall[k - 1])
    return float(np.sum(np.diff(x) * (y[1:] + y[:-1]) * 0.5))


def error_auc(errors, thresholds=(5, 10, 20)):
    """metrics.py:143-160: normalised AUC of the cumulative pose-error curve at 5 / 10 / 20 degrees (the reference
    discards its `thresholds` argument in favour of these three)."""
    e = np.concatenate([[0.0], np.sort(np.asarray(list(errors), dtype=np.float64))])
    recall = np.linspace(0, 1, len(e))
    return {f"auc@{t}": _area_under_recall(e, recall, t) / t for t in (5, 10, 20)}


def homography_auc(errors, thresholds=(3, 5, 10)):
    """error_auc's normalised area under the cumulative error curve for homography_corner_errors, at 3 / 5 / 10 px (the HPatches table
    of the LoFTR paper).  error_auc itself keeps the reference's behaviour of ignoring its thresholds, so the same curve and the same
    area routine are evaluated at the thresholds given here."""
    e = np.concatenate([[0.0], np.sort(np.asarray(list(errors), dtype=np.float64))])
    recall = np.linspace(0, 1, len(e))
    return {f"auc@{t}": _area_under_recall(e, recall, t) / t for t in thresholds}


def epidist_prec(errors, thresholds, ret_dict=False):
    """metrics.py:163-174: for each threshold, the mean over pairs of the fraction of that pair's matches whose
    epipolar error is below it (a pair without matches counts 0)."""
    def pair_precision(errs, thr):
        errs = np.asarray(errs)
        return float(np.count_nonzero(errs < thr)) / errs.size if errs.size else 0

    precs = [np.mean([pair_precision(e, thr) for e in errors]) if len(errors) else 0 for thr in thresholds]
    return {f"prec@{t:.0e}": p for t, p in zip(thresholds, precs)} if ret_dict else precs


def aggregate_metrics(metrics, epi_err_thr=5e-4):
    """metrics.py:177-198: one entry per identifier (a DistributedSampler pads the last batch with repeats; a repeat
    overrides the earlier entry but keeps its position), pose AUC of max(R_err, t_err), matching precision at
    `epi_err_thr` (5e-4 ScanNet, 1e-4 MegaDepth)."""
    index_of = {}
    for i, ident in enumerate(metrics["identifiers"]):
        index_of[ident] = i
    keep = list(index_of.values())
    worst = np.maximum(np.asarray(metrics["R_errs"], dtype=np.float64), np.asarray(metrics["t_errs"], dtype=np.float64))[keep]
    out = error_auc(worst)
    out.update(epidist_prec([metrics["epi_errs"][i] for i in keep], [epi_err_thr], ret_dict=True))
    return out


# ---- the loop ----------------------------------------------------------------------------------------------
def _pair_names(batch):
    names = batch.get("pair_names")
    bs = batch["image0"].size(0)
    if names is None:
        return [(f"pair{b}_0", f"pair{b}_1") for b in range(bs)]
    return list(zip(*names))


def compute_metrics(batch, config=None, estimator=None, on_missing="raise"):
    """PL_LoFTR._compute_metrics (lightning_loftr.py:95-111) -> ({'metrics': {...}}, rel_pair_names)."""
    compute_symmetrical_epipolar_errors(batch)
    compute_pose_errors(batch, config, estimator=estimator, on_missing=on_missing)
    rel_pair_names = _pair_names(batch)
    bs = batch["image0"].size(0)
    epi, bids = batch["epi_errs"].cpu().numpy(), batch["m_bids"].cpu().numpy()      # one device->host copy, not one per pair
    metrics = {"identifiers": ["#".join(rel_pair_names[b]) for b in range(bs)],
               "epi_errs": [epi[bids == b] for b in range(bs)],
               "R_errs": batch["R_errs"], "t_errs": batch["t_errs"], "inliers": batch["inliers"]}
    return {"metrics": metrics}, rel_pair_names


@torch.no_grad()
def test_step(matcher, batch, config=None, dump=True, estimator=None, on_missing="raise"):
    """PL_LoFTR.test_step (lightning_loftr.py:205-229): matcher forward, metrics, optional per-pair dumps."""
    matcher(batch)
    ret_dict, rel_pair_names = compute_metrics(batch, config, estimator=estimator, on_missing=on_missing)
    if dump:
        pair_names = _pair_names(batch)
        bids = batch["m_bids"].cpu().numpy()
        host = {k: batch[k].cpu().numpy() for k in ("mkpts0_f", "mkpts1_f", "mconf", "epi_errs")}
        dumps = []
        for b in range(batch["image0"].shape[0]):
            mask = bids == b
            item = {"pair_names": pair_names[b], "identifier": "#".join(rel_pair_names[b])}
            for k, v in host.items():
                item[k] = v[mask]
            for k in ("R_errs", "t_errs", "inliers"):
                item[k] = batch[k][b]
            dumps.append(item)
        ret_dict["dumps"] = dumps
    return ret_dict


def gather(items):
    """src/utils/comm.py:gather as test_epoch_end uses it: the per-rank python lists concatenated in rank order on
    every rank (one process per GPU; metric lists are small host objects -> all_gather_object over the default
    group, RCCL-free: gloo or the object path of nccl).  Identity without an initialised process group."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return list(items)
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, list(items))
    return [x for part in parts for x in part]


def test_epoch_end(outputs, config=None, dump_dir=None):
    """PL_LoFTR.test_epoch_end (lightning_loftr.py:231-249): flatten the per-step metrics, gather them over the
    ranks (duplicates padded in by a DistributedSampler are dropped by identifier in aggregate_metrics), aggregate;
    rank 0 optionally saves ``LoFTR_pred_eval.npy``.  Every rank returns the aggregated metrics."""
    import torch.distributed as dist
    keys = outputs[0]["metrics"].keys()
    metrics = {k: gather([x for o in outputs for x in o["metrics"][k]]) for k in keys}
    epi_thr = _cfg_get(config, ("TRAINER", "EPI_ERR_THR"), 5e-4)
    result = aggregate_metrics(metrics, epi_thr)
    if dump_dir is not None:
        dumps = gather([d for o in outputs for d in o.get("dumps", [])])
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        if rank == 0:
            os.makedirs(dump_dir, exist_ok=True)
            np.save(os.path.join(dump_dir, "LoFTR_pred_eval"), np.array(dumps, dtype=object), allow_pickle=True)
    return result
