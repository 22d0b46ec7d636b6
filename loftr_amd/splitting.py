"""Track splitting: consistent tracks from the components that visit an image twice, on the device.

Rule 4 of the atlas (atlas.py) makes a track of every connected component of the kept matches and marks it
``track_ok = False`` when two of its keypoints lie in one image; every consumer reads ``tracks(consistent_only=True)`` and drops such
a component whole.  LoFTR has no detector, so a chain of rows easily comes back to an image one 2 px cell beside where it left, and
the more rows cover a scene the larger the share of keypoints that is lost this way.  Splitting grows the keypoints of such a
component again along its matches, strongest first, and never joins two components that share an image::

    rec = sfm.reconstruct(K, split=True)                      # the split first; everything after it reads the split atlas
    rec.sfm, rec.stats["split"]                               # the relabelled atlas and the counts

or piece by piece::

    sfm2, split = sfm.split()                                 # split: Split; sfm2 shares every tensor with sfm except the track arrays
    pts = sfm2.triangulate(K, T)                              # every track of sfm2 is consistent

The rule (include/loftr_hip.h) is integer and order-defined, one unsigned 64-bit maximum per decision: the host routine
``loftr_split_tracks_host`` defines it (CPU tensors / numpy arrays run it), the HIP kernels reproduce it bit for bit (GPU tensors run
them; there is no silent fallback either way).
"""
import numpy as np
import torch

from . import _tracks, ops

_ARGS = ("edge_kp", "edge_conf", "kp_image", "track_id", "track_ok")


class Split:
    """What ``split_tracks`` returns (tensors on the device of the input).

    ``track_id_new [K] i32`` (-1: none), ``track_len_new [T'] i32``, ``edge_state [E] u8`` (``ops.SPLIT_STATES``: 0 ignored, 1 internal,
    2 conflict, 3 open), ``round_accepted [max_rounds] i32`` (the edges every round accepted); ``stats``: the counts by name
    (``ops.SPLIT_NAMES``; ``n_open > 0`` means ``max_rounds`` was too small to finish)."""

    FIELDS = ("track_id_new", "track_len_new", "edge_state", "round_accepted")

    def __init__(self, stats, **tensors):
        self.stats = stats
        for k in self.FIELDS:
            setattr(self, k, tensors[k])

    def to_host(self):
        """dict of numpy arrays (plus 'stats')."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out["stats"] = dict(self.stats)
        return out


def _integer(what, name, v, lo):
    if not isinstance(v, int) or isinstance(v, bool) or v < lo:
        raise ValueError(f"{what}: {name} must be an integer >= {lo}, got {v!r}")


def split_tracks(edge_kp, edge_conf, kp_image, track_id, track_ok, n_images, min_track_len=2, max_rounds=32, timings=None):
    """Grow the keypoints of every inconsistent track again into consistent ones -> ``Split``.

    ``edge_kp [E,2]``: the kept matches as GLOBAL keypoint indices (edge ``e`` is match ``e``); ``edge_conf [E]``; ``kp_image [K]``
    (must not descend: keypoints are ordered by image); ``track_id [K]`` (-1: none); ``track_ok [T]``.  CPU tensors or numpy arrays
    run the defining host routine; GPU tensors (all of them, on one device) run the kernels.

    A consistent track keeps its members.  A keypoint of an inconsistent track starts alone; in every round an edge between two
    components that share no image is a candidate, and a candidate that is the strongest (greatest confidence, then lowest edge) at
    BOTH of its components joins them.  At most ``max_rounds`` rounds; a round that accepts nothing ends the procedure.  Components
    of at least ``min_track_len`` keypoints are numbered together with the consistent tracks in ascending smallest keypoint; the
    other keypoints get -1.  One readback; a bad table raises ValueError.  timings: a list that receives (launch class, ms) pairs
    of the GPU launches."""
    what = "split_tracks"
    args = [edge_kp, edge_conf, kp_image, track_id, track_ok]
    gpu = _tracks.one_device(what, _ARGS, args)
    for name, a in zip(_ARGS, args):
        if name not in ("edge_conf", "track_ok"):
            _tracks.integers(what, name, a)
    _integer(what, "n_images", n_images, 0)
    _integer(what, "min_track_len", min_track_len, 1)
    _integer(what, "max_rounds", max_rounds, 0)
    if gpu:
        dts = (torch.int32, torch.float32, torch.int32, torch.int32, None)
        a = [(x.detach() != 0).to(torch.uint8) if dt is None else x.detach().to(dt) for x, dt in zip(args, dts)]
        out = ops.split_tracks(*a, n_images, min_track_len, max_rounds, timings=timings)
    else:
        dts = (np.int32, np.float32, np.int32, np.int32, None)
        host = lambda x: x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        a = [np.ascontiguousarray(host(x) != 0).astype(np.uint8) if dt is None else np.ascontiguousarray(host(x), dt) for x, dt in zip(args, dts)]
        if a[0].ndim != 2:                                                 # (an empty list of edges may come as [0])
            a[0] = a[0].reshape(-1, 2)
        out = {k: torch.from_numpy(v) for k, v in ops.split_tracks_host(*a, n_images, min_track_len, max_rounds).items()}
    word = out["counts"].cpu().tolist()                                    # the one readback
    _tracks.raise_error_bits(what, word[1], ops.SPLIT_ERRORS)
    stats = {name: word[i] for i, name in enumerate(ops.SPLIT_NAMES) if name != "error_bits"}
    stats.update(n_edges=int(out["edge_state"].numel()), n_keypoints=int(out["track_id_new"].numel()), min_track_len=min_track_len,
                 max_rounds=max_rounds)
    return Split(stats, track_id_new=out["track_id_new"], track_len_new=out["track_len_new"][:word[0]], edge_state=out["edge_state"],
                 round_accepted=out["round_accepted"])
