"""Georegistration: put a reconstruction into the frame of known camera positions.

``reconstruct`` fixes only the first image of the initial pair; the frame and the scale of what it returns are arbitrary.  With GPS
positions, surveyed centres or a few trusted poses the model moves into their frame::

    rec = sfm.reconstruct(K)
    rec_m, al = rec.align(ref_centres, known=has_gps, thresh=0.5)      # al.s, al.R, al.t, al.inliers, al.rms (units of ref_centres)
    model = LocalizationModel.from_atlas(rec_m.sfm or sfm, rec_m.points)      # query poses come out metric

The transform is the 3D similarity ``ref ~ s R c + t`` between the camera centres ``c = -R_c^T t_c`` of the images that are posed and
known and their reference positions, by RANSAC over 3-point closed forms and a closed-form refit (include/loftr_hip.h).
The host routine ``loftr_estimate_similarity`` defines it (CPU tensors run it), the HIP kernels reproduce it bit for bit (GPU tensors
run them; there is no silent fallback either way), and ``ops.transform_model`` moves poses and points by one text on both sides: the
CPU chain and the GPU chain return the same bits.
"""
import copy

import numpy as np
import torch

from . import _tracks, ops

_ARGS = ("T_cam_from_world", "posed", "ref_centres", "known")


class Alignment:
    """What ``align_centres`` returns (tensors on the device of the input): ``s [] f64``, ``R [3,3] f64``, ``t [3] f64`` with
    ``ref ~ s R c + t`` (zero without a model), ``inliers [n] bool`` (images whose centre agrees with its reference position),
    ``n_inliers [] i64`` (-1 without a model), ``rms [] f64`` (root mean square distance over the inliers, units of the reference;
    NaN without a model), ``stats``: dict of the call's settings.  ``ok`` reads ``n_inliers`` back."""

    FIELDS = ("s", "R", "t", "inliers", "n_inliers", "rms")

    def __init__(self, stats, **tensors):
        self.stats = stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])

    @property
    def ok(self):
        return int(self.n_inliers) >= 0

    def to_host(self):
        """dict of numpy arrays (plus 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out["stats"] = dict(self.stats)
        return out


def camera_centres(T_cam_from_world):
    """[n,3] f64 centres -R_c^T t_c, each a sum of three products taken left to right (elementwise: the same bits on CPU and GPU)."""
    R, t = T_cam_from_world[:, :3, :3], T_cam_from_world[:, :3, 3]
    return -torch.stack([R[:, 0, i] * t[:, 0] + R[:, 1, i] * t[:, 1] + R[:, 2, i] * t[:, 2] for i in range(3)], 1)


def align_centres(T_cam_from_world, posed, ref_centres, known, thresh, with_scale=True, conf=0.999, seed=0):
    """Similarity between the camera centres of a reconstruction and reference positions -> ``Alignment``.

    ``T_cam_from_world [n,4,4]``, ``posed [n]``, ``ref_centres [n,3]``, ``known [n]`` (which rows of ``ref_centres`` hold a position):
    torch tensors on one device.  Source = the centres of the images that are posed and known, destination = their reference
    positions; ``thresh`` is a distance in the units of ``ref_centres`` (``float('inf')``: every image is an inlier of every model,
    which makes the result the plain least-squares fit).  CPU tensors run the host estimator, GPU tensors ONE
    ``ops.estimate_similarities`` call; the same result for one seed.  On the GPU nothing is read back beyond the estimator's own
    replay: the selected images are moved to the front by a stable sort and form problem 0, the others (their centres blanked) are
    problem 1, which has no model."""
    what = "align_centres"
    args = [a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)) for a in (T_cam_from_world, posed, ref_centres, known)]
    gpu = _tracks.one_device(what, _ARGS, args)
    T, posed, ref, known = (a.detach() for a in args)
    dev = T.device
    T, ref, posed, known = T.to(torch.float64), ref.to(torch.float64), posed != 0, known != 0
    n = posed.shape[0] if posed.dim() == 1 else -1
    if tuple(T.shape) != (n, 4, 4) or tuple(ref.shape) != (n, 3) or tuple(known.shape) != (n,):
        raise ValueError(f"{what}: expected T_cam_from_world [n,4,4], posed [n], ref_centres [n,3] and known [n], got {tuple(T.shape)}, "
                         f"{tuple(posed.shape)}, {tuple(ref.shape)}, {tuple(known.shape)}")
    if not (thresh >= 0):
        raise ValueError(f"{what}: thresh must be >= 0, got {thresh}")
    sel = posed & known
    C = camera_centres(T)
    inliers = torch.zeros(n, dtype=torch.bool, device=dev)
    if gpu:
        order = torch.argsort((~sel).to(torch.uint8), stable=True)
        sel_o = sel[order]
        src = torch.where(sel_o[:, None], C[order], torch.full_like(C, float("nan")))
        s, R, t, inl, n_inl = ops.estimate_similarities(src, ref[order], (~sel_o).to(torch.int64), 2, with_scale, thresh, conf, seed)
        s, R, t, n_inl = s[0], R[0], t[0], n_inl[0]
        inliers[order] = inl & sel_o
    else:
        from .evaluation import estimate_similarity_native
        idx = sel.nonzero().squeeze(1)
        est = estimate_similarity_native(C[idx].numpy(), ref[idx].numpy(), with_scale, thresh, conf, seed)
        s, R, t = torch.zeros((), dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
        n_inl = torch.tensor(-1, dtype=torch.int64)
        if est is not None:
            s, R, t = torch.tensor(est[0], dtype=torch.float64), torch.from_numpy(est[1].copy()), torch.from_numpy(est[2].copy())
            inliers[idx] = torch.from_numpy(est[3])
            n_inl = torch.tensor(int(est[3].sum()), dtype=torch.int64)
    e = s * torch.stack([R[i, 0] * C[:, 0] + R[i, 1] * C[:, 1] + R[i, 2] * C[:, 2] for i in range(3)], 1) + t - ref
    e2 = torch.where(inliers, (e * e).sum(1), torch.zeros_like(e[:, 0]))
    rms = torch.where(n_inl > 0, torch.sqrt(e2.sum() / n_inl.clamp(min=1)), torch.full_like(s, float("nan")))
    stats = {"n_images": n, "thresh": float(thresh), "with_scale": bool(with_scale), "conf": float(conf), "seed": int(seed)}
    return Alignment(stats, s=s, R=R, t=t, inliers=inliers, n_inliers=n_inl, rms=rms)


def fit_centres(T_cam_from_world, posed, ref_centres, known, with_scale=True):
    """The plain least-squares similarity (Umeyama) over all posed and known images: ``align_centres`` with an infinite threshold."""
    return align_centres(T_cam_from_world, posed, ref_centres, known, float("inf"), with_scale)


def transformed(rec, s, R, t):
    """``Reconstruction.transformed``: a copy of ``rec`` whose ``T_cam_from_world`` and ``points.xyz`` are moved by X' = s R X + t
    (``ops.transform_model``).  Every other tensor is shared with ``rec``; ``bundle`` stays in the old frame."""
    dev = rec.T_cam_from_world.device
    s, R, t = ((a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, np.float64))).to(dev, torch.float64) for a in (s, R, t))
    xyz, T = ops.transform_model(rec.points.xyz, rec.T_cam_from_world, rec.posed, s.reshape(1), R.reshape(3, 3), t.reshape(3))
    out = copy.copy(rec)
    out.points = copy.copy(rec.points)
    out.points.xyz, out.T_cam_from_world = xyz, T
    return out


def align(rec, ref_centres, known=None, thresh=1.0, with_scale=True, apply=True, conf=0.999, seed=0, refine=None):
    """``Reconstruction.align``: -> ``(rec2, alignment)``.  known None: every row of ``ref_centres`` that is finite.  Without a model
    (``alignment.n_inliers == -1``) or with ``apply=False``, ``rec2`` is ``rec`` itself.  Reads ``n_inliers`` back once.  refine: see
    ``refined``."""
    dev = rec.T_cam_from_world.device
    ref = (ref_centres if isinstance(ref_centres, torch.Tensor) else torch.as_tensor(np.asarray(ref_centres))).to(dev, torch.float64)
    known = torch.isfinite(ref).all(1) if known is None else (known if isinstance(known, torch.Tensor) else torch.as_tensor(np.asarray(known))).to(dev)
    al = align_centres(rec.T_cam_from_world, rec.posed, ref, known, thresh, with_scale, conf, seed)
    if not apply or not al.ok:
        return rec, al
    rec2 = transformed(rec, al.s, al.R, al.t)
    return (rec2 if refine is None else refined(rec2, ref, al, **refine)), al


def refined(rec, ref_centres, al, sfm=None, sigma=1.0, tri=None, **ba):
    """The step after georegistration: a bundle adjustment of the aligned ``rec`` over the tracks of ``sfm`` with NO camera
    fixed and the reference positions of ``al.inliers`` as position priors at ``sigma``, then a triangulation with the adjusted poses
    (``tri``: keyword arguments of ``SfmResult.triangulate``) -> a copy of ``rec`` with the refined ``T_cam_from_world``, ``K``,
    ``points`` and ``bundle``.  An image without a pose has a NaN pose: it is an invalid camera of the adjustment (rule 1), keeps its
    bits, and takes no part in either triangulation."""
    sfm = sfm if sfm is not None else rec.sfm
    if sfm is None:
        raise ValueError("align: refine needs sfm=<the SfmResult of this reconstruction>")
    if rec.K is None:
        raise ValueError("align: refine needs a reconstruction that carries K")
    tri = dict(tri or {})
    dev = rec.T_cam_from_world.device
    tri.setdefault("posed", rec.posed)
    pts = sfm.triangulate(rec.K, rec.T_cam_from_world, **tri)
    res = sfm.adjust(pts, rec.K, rec.T_cam_from_world, fixed=torch.zeros(rec.posed.shape[0], dtype=torch.bool, device=dev),
                     position_prior=ref_centres, prior_mask=al.inliers, prior_sigma=sigma, **ba)
    out = copy.copy(rec)
    out.T_cam_from_world, out.bundle = res.T_cam_from_world, res
    if "K" in res.FIELDS:
        out.K = res.K
    out.points = sfm.triangulate(out.K, out.T_cam_from_world, **tri)
    return out
