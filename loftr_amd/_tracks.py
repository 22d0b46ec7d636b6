"""The track table on the Python side: what ``triangulation``, ``bundle`` and ``registration`` check and build before they call ``ops``.

Observations in CSR form (``offsets [T+1]`` over ``obs_image [N]``), once more grouped by image (``cam_offsets [n+1]`` over
``cam_obs [N]``); DESIGN §16, §18, §19.  The kernels report a bad table through error bits in their counts (csrc/tracks_core.h); the host
path refuses the same tables with the same words before it calls the host routine."""
import numpy as np
import torch

from . import ops
from ._lib import LoftrHipError

ERRORS = ops.BUNDLE_ERRORS                  # (bit, what it says); registration's are the same, triangulation raises the first two


def integers(what, name, a):
    """``offsets`` and ``obs_image`` are converted to int64 / int32: refuse what would be rounded on the way."""
    dt = a.dtype if isinstance(a, torch.Tensor) else np.asarray(a).dtype
    if (isinstance(dt, torch.dtype) and (dt.is_floating_point or dt == torch.bool)) or \
            (not isinstance(dt, torch.dtype) and not np.issubdtype(dt, np.integer)):
        raise ValueError(f"{what}: {name} must hold integers, got {dt}")


def one_device(what, names, args):
    """True when every argument is a GPU tensor, False when none is; mixed is an error."""
    gpu = [isinstance(a, torch.Tensor) and a.is_cuda for a in args]
    if any(gpu) and not all(gpu):
        raise LoftrHipError(f"{what}: GPU and CPU arguments mixed (" + ", ".join(f"{n}: {'GPU' if g else 'CPU'}" for n, g in zip(names, gpu))
                            + "); there is no silent fallback: move them to one device")
    return all(gpu)


def check_host(what, offsets, obs_image, n_images):
    """The errors the kernels report through their counts, on numpy arrays [T+1] and [N] before the host routine runs."""
    if obs_image.size and (obs_image.min() < 0 or obs_image.max() >= n_images):
        raise ValueError(f"{what}: " + ERRORS[0][1])
    if offsets.size and (offsets[0] != 0 or offsets[-1] != obs_image.shape[0] or (np.diff(offsets) < 0).any()):
        raise ValueError(f"{what}: " + ERRORS[1][1])


def group_by_image(obs_image, n_images):
    """The observations grouped by image -> (cam_offsets [n+1] i64, cam_obs [N] i32), of the kind of ``obs_image`` (an int32 GPU tensor or
    numpy array): integer plumbing, a stable sort.  Bad image ids are caught by the kernels, so they are only clamped here."""
    n = n_images
    if isinstance(obs_image, torch.Tensor):
        im = obs_image.to(torch.int64)
        cam_obs = torch.sort(im, stable=True).indices.to(torch.int32)
        cam_offsets = torch.zeros(n + 1, dtype=torch.int64, device=im.device)
        if n > 0 and im.numel() and im.dim() == 1:
            cam_offsets[1:] = torch.cumsum(torch.bincount(im.clamp(0, n - 1), minlength=n), 0)
        return cam_offsets, cam_obs
    cam_obs = np.argsort(obs_image, kind="stable").astype(np.int32)
    cam_offsets = np.zeros(n + 1, np.int64)
    if obs_image.ndim == 1:
        cam_offsets[1:] = np.cumsum(np.bincount(obs_image, minlength=n)[:n])
    return cam_offsets, cam_obs


def group_by_camera(camera_ids):
    """The images grouped by camera -> (cam_group [n] i32, group_offsets [G+1] i64, group_cams [n] i32), of the kind of ``camera_ids``
    (an integer tensor or numpy array ``[n]``): the ids are relabelled to dense groups ordered by their smallest member image, then a
    stable sort as in ``group_by_image``.  DESIGN §18.2."""
    if isinstance(camera_ids, torch.Tensor):
        ids = camera_ids.to(torch.int64)
        n, dev = ids.numel(), ids.device
        uniq, inv = torch.unique(ids, return_inverse=True)                 # (sorted by id)
        first = torch.full((uniq.numel(),), n, dtype=torch.int64, device=dev).scatter_reduce(0, inv, torch.arange(n, device=dev), "amin")
        rank = torch.empty_like(first)
        rank[torch.argsort(first)] = torch.arange(uniq.numel(), device=dev)
        group = rank[inv]
        group_cams = torch.sort(group, stable=True).indices.to(torch.int32)
        group_offsets = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=dev)
        group_offsets[1:] = torch.cumsum(torch.bincount(group, minlength=uniq.numel()), 0)
        return group.to(torch.int32), group_offsets, group_cams
    ids = np.asarray(camera_ids).astype(np.int64)
    uniq, first, inv = np.unique(ids, return_index=True, return_inverse=True)
    rank = np.empty(uniq.size, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(uniq.size)
    group = rank[inv.reshape(-1)]
    group_offsets = np.zeros(uniq.size + 1, np.int64)
    group_offsets[1:] = np.cumsum(np.bincount(group, minlength=uniq.size))
    return group.astype(np.int32), group_offsets, np.argsort(group, kind="stable").astype(np.int32)


def raise_error_bits(what, bits, errors=None):
    """The first set error bit of a counts word that was read back -> ValueError (``errors``: the table of the call, ERRORS by default)."""
    for bit, text in errors or ERRORS:
        if bits & bit:
            raise ValueError(f"{what}: {text} (found on the device)")
