"""Pixels without the radial coefficient of their camera: what every stage but the bundle adjustment reads when the lenses distort.

The camera model has one coefficient on normalised coordinates, ``x_d = x (1 + k r^2)``.  ``bundle_adjust(...,
refine_radial=True)`` fits ``k`` on the stored, distorted pixels; triangulation, registration, pose estimation and localisation read
pinhole pixels and get them here::

    xy, ok = loftr_amd.undistort_points(obs_xy, obs_image, res.K, res.radial)

``loftr_undistort_points_host`` defines the result (CPU tensors / numpy arrays run it), the kernel reproduces it bit for bit (GPU tensors
run it; there is no silent fallback either way).  A point beyond the fold of a barrel coefficient, with a NaN anywhere or of a camera
with ``fx = 0`` comes back as ``(NaN, NaN)`` with ``ok = False``; the triangulation rejects pixels that are not finite."""
import numpy as np
import torch

from . import _tracks, ops

_ARGS = ("xy", "image", "K", "radial")


def _convert(what, args, call_gpu, call_host):
    gpu = _tracks.one_device(what, _ARGS, args)
    _tracks.integers(what, "image", args[1])
    if gpu:
        dts = (torch.float32, torch.int32, torch.float64, torch.float64)
        out = call_gpu(*[x.detach().to(dt) for x, dt in zip(args, dts)])
    else:
        dts = (np.float32, np.int32, np.float64, np.float64)
        host = lambda x: x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        out = {k: torch.from_numpy(v) for k, v in call_host(*[np.ascontiguousarray(host(x), dt) for x, dt in zip(args, dts)]).items()}
    bits = int(out["counts"][1])                                                     # the one readback
    if bits and not gpu:
        raise ValueError(f"{what}: " + ops.UNDISTORT_ERRORS[0][1])
    _tracks.raise_error_bits(what, bits, ops.UNDISTORT_ERRORS)
    return out["xy"], out["ok"].view(torch.bool)


def undistort_points(xy, image, K, radial):
    """Distorted pixels -> the pinhole pixels of the same rays: ``(xy [M,2] f32, ok [M] bool)``.

    ``xy [M,2]`` pixels, ``image [M]`` the image of each, ``K [n,3,3]``, ``radial [n]`` the coefficient of each image.  Newton on
    ``r (1 + k r^2) = r_d`` for a fixed 12 iterations; ``ok`` iff everything is finite, ``fx`` and ``fy`` are not zero, the result lies on
    the monotone branch (``1 + 3 k r^2 > 0``) and solves the equation to ``1e-9 (1 + r_d)``; a point that is not ok is ``(NaN, NaN)``.
    ``k = 0`` recomputes the point through ``K``: equal to the input to a rounding, not promised to be its bits.  An ``image`` outside
    ``[0, n)`` raises ValueError.  CPU tensors or numpy arrays run the defining host routine; GPU tensors (all of them, on one device)
    run the kernel."""
    return _convert("undistort_points", [xy, image, K, radial], ops.undistort_points, ops.undistort_points_host)


def distort_points(xy, image, K, radial):
    """Pinhole pixels -> the distorted pixels of the model, from the same text as ``undistort_points`` (host routine only: CPU tensors or
    numpy arrays).  For tests and tools that need to synthesise observations."""
    def no_gpu(*a):
        raise ValueError("distort_points: the host routine only; pass CPU tensors or numpy arrays")
    return _convert("distort_points", [xy, image, K, radial], no_gpu, ops.distort_points_host)
