"""Feature banks: run the backbone once per image of a pair list, then match pairs of stored maps.

LoFTR's ResNet-FPN is a function of one image; only the position-encoded coarse transformer onward depends on the pair.
``LoFTR.forward`` recomputes both images of every pair, which is wasted work whenever images repeat across a pair list
(MegaDepth-1500: 1500 pairs over 806 images; a fixed reference frame in a video loop; retrieval pair lists).

* ``FeatureBank`` holds the backbone maps of up to ``capacity`` images of one size in fixed slots, in the layout
  ``backbone.forward_hip`` produces (fp32, channels-last), plus optional coarse masks and scales per slot.
* ``LoFTR.match_pairs(bank0, ids0, bank1, ids1)`` (``match_pairs`` below) matches pair k = (bank0[ids0[k]], bank1[ids1[k]])
  and returns the dict ``forward`` would leave for those images.  The two kernels that read backbone maps have slot-indexed
  variants (csrc/bank.hip); everything after them is the forward's own code (``LoFTR._match_encoded``).  With
  ``backbone_impl = 'hip'`` the result is bit-identical to ``forward`` on the stacked images.
* ``plan_pair_list`` / ``match_pair_list``: a whole pair list under a memory budget -- consecutive chunks of ``batch_size``
  pairs (output order = input order), missing images extracted in groups with look-ahead, Belady eviction.
"""
import bisect
import itertools
from collections import namedtuple

import numpy as np
import torch

from . import ops
from ._lib import LoftrHipError

# the convolution kernels index an activation with 32 bits: images * (H/2) * (W/2) * 256 < 2^31 per backbone call (LoFTR.run_backbone)
_ACT_LIMIT = 2 ** 31 - 1


def _down(n, factor):
    """Size of a map after log2(factor) stride-2 stages (each rounds up, like the backbone's convolutions)."""
    while factor > 1:
        n, factor = (n + 1) // 2, factor // 2
    return n


def _backbone_fingerprint(model):
    """Identity of the backbone weights: (data_ptr, _version) of every parameter and buffer.  Changes when a weight is modified in
    place, replaced or moved."""
    return tuple((t.data_ptr(), t._version) for t in itertools.chain(model.backbone.parameters(), model.backbone.buffers()))


def _model_device(model):
    return next(model.parameters()).device


class FeatureBank:
    """Backbone maps of up to ``capacity`` images of size ``image_hw`` = (H, W), extracted once and matched in any pairing.

    Storage (fp32, channels-last, what ``backbone.forward_hip`` produces): ``coarse [capacity, h_c, w_c, C_c]`` and
    ``fine [capacity, h_f, w_f, C_f]``; ``mask [capacity, h_c, w_c]`` bool and ``scale [capacity, 2]`` once an image with a
    mask / scale has been added.  Masks and scales follow the batch dict of ``LoFTR.forward`` (``mask0`` at coarse resolution,
    ``scale0 = [w, h]``)."""

    EXTRACT_BATCH = 16                         # images per backbone call (at most; the 32-bit activation cap may ask for fewer)

    def __init__(self, model, capacity, image_hw, device=None):
        if int(capacity) < 1:
            raise ValueError(f"FeatureBank: capacity must be positive, got {capacity}")
        self.model = model
        self.device = torch.device(device) if device is not None else _model_device(model)
        self.capacity = int(capacity)
        self.image_hw = (int(image_hw[0]), int(image_hw[1]))
        (self.h_c, self.w_c, cc), (self.h_f, self.w_f, cf) = self.map_shapes(model, self.image_hw)
        self.coarse = torch.empty(self.capacity, self.h_c, self.w_c, cc, device=self.device)
        self.fine = torch.empty(self.capacity, self.h_f, self.w_f, cf, device=self.device)
        self.mask = None
        self.scale = None
        self._fp = [None] * self.capacity       # backbone fingerprint per occupied slot (None: free)
        self._has_mask = [False] * self.capacity
        self._has_scale = [False] * self.capacity
        self.images_extracted = 0
        self.backbone_calls = 0

    @staticmethod
    def map_shapes(model, image_hw):
        """((h_c, w_c, C_c), (h_f, w_f, C_f)) of the backbone maps of one H x W image."""
        cfg = model.config
        res_c, res_f = cfg["resolution"]
        H, W = image_hw
        return ((_down(H, res_c), _down(W, res_c), cfg["coarse"]["d_model"]),
                (_down(H, res_f), _down(W, res_f), cfg["fine"]["d_model"]))

    @classmethod
    def image_bytes(cls, model, image_hw):
        """Device bytes one slot takes (maps, mask, scale)."""
        (hc, wc, cc), (hf, wf, cf) = cls.map_shapes(model, image_hw)
        return 4 * (hc * wc * cc + hf * wf * cf) + hc * wc + 8

    @property
    def bytes_per_image(self):
        return self.image_bytes(self.model, self.image_hw)

    def coarse_map(self):
        """The coarse bank as [capacity, C, h, w] (a channels-last view; what the kernels take)."""
        return self.coarse.permute(0, 3, 1, 2)

    def fine_map(self):
        return self.fine.permute(0, 3, 1, 2)

    def occupied(self):
        return [s for s, fp in enumerate(self._fp) if fp is not None]

    def _free(self, k):
        free = [s for s, fp in enumerate(self._fp) if fp is None]
        if len(free) < k:
            raise LoftrHipError(f"FeatureBank: {k} images to add but {len(free)} free slots of {self.capacity}")
        return free[:k]

    def add(self, images, mask=None, scale=None, slots=None):
        """Run the model's backbone once over ``images`` [k, 1, H, W] and store each image's maps in a slot: the k lowest free
        slots, or ``slots`` (overwritten if occupied).  ``mask`` [k, h_c, w_c] ('0' = padded), ``scale`` [k, 2].
        Returns the slot ids (list of int)."""
        model = self.model
        if model.training:
            raise LoftrHipError("FeatureBank.add: inference only (the backbone's BatchNorm uses batch statistics in .train()); call .eval()")
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[1] != 1 or tuple(images.shape[2:]) != self.image_hw:
            raise ValueError(f"FeatureBank.add: expected images [k, 1, {self.image_hw[0]}, {self.image_hw[1]}], "
                             f"got {tuple(images.shape) if isinstance(images, torch.Tensor) else type(images)}")
        if self.device.type != "cuda":
            raise LoftrHipError(f"FeatureBank.add: the bank is on {self.device}; the HIP path needs a GPU (no CPU fallback)")
        if images.device != self.device or _model_device(model) != self.device:
            raise LoftrHipError(f"FeatureBank.add: images on {images.device}, model on {_model_device(model)}, bank on {self.device}")
        k = images.shape[0]
        if slots is None:
            slots = self._free(k)
        else:
            slots = [int(s) for s in (slots.tolist() if isinstance(slots, torch.Tensor) else slots)]
            if len(slots) != k or len(set(slots)) != k or any(s < 0 or s >= self.capacity for s in slots):
                raise ValueError(f"FeatureBank.add: slots must be {k} distinct ids in [0, {self.capacity}), got {slots}")
        if mask is not None and (mask.shape[0] != k or tuple(mask.shape[1:]) != (self.h_c, self.w_c)):
            raise ValueError(f"FeatureBank.add: mask must be [{k}, {self.h_c}, {self.w_c}], got {tuple(mask.shape)}")
        if scale is not None and tuple(scale.shape) != (k, 2):
            raise ValueError(f"FeatureBank.add: scale must be [{k}, 2], got {tuple(scale.shape)}")
        if k == 0:
            return []
        H, W = self.image_hw
        cap = max(1, _ACT_LIMIT // ((H // 2) * (W // 2) * 256))
        chunk = min(self.EXTRACT_BATCH, cap)
        use_hip = model.backbone_impl == "hip" and images.is_cuda
        run = model.backbone.forward_hip if use_hip else model.backbone
        with torch.no_grad(), torch.cuda.device(self.device):
            slot_t = torch.tensor(slots, dtype=torch.long).to(self.device)
            for i in range(0, k, chunk):
                x = images[i:i + chunk].contiguous(memory_format=torch.channels_last)   # C == 1: a restride, no copy
                fc, ff = run(x)
                self.backbone_calls += 1
                idx = slot_t[i:i + chunk]
                self.coarse.index_copy_(0, idx, fc.permute(0, 2, 3, 1))
                self.fine.index_copy_(0, idx, ff.permute(0, 2, 3, 1))
            if mask is not None:
                if self.mask is None:
                    self.mask = torch.zeros(self.capacity, self.h_c, self.w_c, dtype=torch.bool, device=self.device)
                self.mask.index_copy_(0, slot_t, mask.to(self.device, torch.bool))
            if scale is not None:
                if self.scale is None:
                    self.scale = torch.zeros(self.capacity, 2, dtype=torch.float32, device=self.device)
                self.scale.index_copy_(0, slot_t, scale.to(self.device, torch.float32))
        fp = _backbone_fingerprint(model)
        for s in slots:
            self._fp[s] = fp
            self._has_mask[s] = mask is not None
            self._has_scale[s] = scale is not None
        self.images_extracted += k
        return slots

    def remove(self, slots):
        for s in (slots.tolist() if isinstance(slots, torch.Tensor) else slots):
            if not 0 <= int(s) < self.capacity:
                raise ValueError(f"FeatureBank.remove: slot {s} out of range [0, {self.capacity})")
            self._fp[int(s)] = None
            self._has_mask[int(s)] = self._has_scale[int(s)] = False

    def clear(self):
        self.remove(range(self.capacity))

    def _check(self, ids, model, name):
        """Host-side checks of the slots a match reads: in range, occupied, extracted under the model's current backbone weights."""
        bad = [s for s in ids if not 0 <= s < self.capacity]
        if bad:
            raise LoftrHipError(f"{name}: slot ids out of range [0, {self.capacity}): {bad[:8]}")
        empty = [s for s in ids if self._fp[s] is None]
        if empty:
            raise LoftrHipError(f"{name}: slots hold no image: {empty[:8]}")
        fp = _backbone_fingerprint(model)
        stale = [s for s in ids if self._fp[s] != fp]
        if stale:
            raise LoftrHipError(f"{name}: slots {stale[:8]} were extracted under other backbone weights (changed, replaced or moved "
                                f"since FeatureBank.add); extract them again")


def _host_ids(ids, name):
    if isinstance(ids, torch.Tensor):
        ids = ids.detach().cpu()
        if ids.dim() != 1 or ids.dtype.is_floating_point or ids.dtype == torch.bool:
            raise ValueError(f"{name}: expected a 1-D integer sequence of slot ids, got {tuple(ids.shape)} {ids.dtype}")
        return [int(v) for v in ids.tolist()]
    return [int(v) for v in ids]


def _side_flag(bank, ids, flags, what, name, who):
    have = [flags[s] for s in ids]
    if any(have) and not all(have):
        raise ValueError(f"{who}: some slots of {name} carry a {what} and some do not")
    return all(have)


def _encode_pairs(model, bank0, ids0, bank1, ids1, flags):
    """The front half that ``match_pairs`` and ``refine_points`` share, after ``_pair_guards``: the batch dict of the n pairs (masks and
    scales gathered from the banks, the map extents) and the position-encoded coarse features.  -> (data, feat_c0, feat_c1, t0, t1):
    t0 / t1 are the slot ids as host int32 tensors.  The caller holds ``torch.no_grad()`` and the model's device."""
    n = len(ids0)
    dev = _model_device(model)
    m0, s0, s1 = flags
    # the slot ids go to the kernels as host tensors: the wrappers check them before any launch
    t0, t1 = torch.tensor(ids0, dtype=torch.int32), torch.tensor(ids1, dtype=torch.int32)
    data = {}
    if m0:
        g0, g1 = t0.to(dev, torch.long), t1.to(dev, torch.long)
        data.update(mask0=bank0.mask[g0], mask1=bank1.mask[g1])
    if s0:
        data["scale0"] = bank0.scale[t0.to(dev, torch.long)]
    if s1:
        data["scale1"] = bank1.scale[t1.to(dev, torch.long)]
    data.update({"bs": n, "hw0_i": torch.Size(bank0.image_hw), "hw1_i": torch.Size(bank1.image_hw)})
    data.update({"hw0_c": torch.Size((bank0.h_c, bank0.w_c)), "hw1_c": torch.Size((bank1.h_c, bank1.w_c)),
                 "hw0_f": torch.Size((bank0.h_f, bank0.w_f)), "hw1_f": torch.Size((bank1.h_f, bank1.w_f))})
    model._fine_join = None                               # the fine maps are in the banks: no side stream to join
    pe = model.pos_encoding.pe[0]
    L0, L1, Cc = bank0.h_c * bank0.w_c, bank1.h_c * bank1.w_c, bank0.coarse.shape[3]
    if (bank0.h_c, bank0.w_c) == (bank1.h_c, bank1.w_c):
        # both halves of the ONE [2n, L, C] buffer the coarse transformer runs on in place (as stacked_halves arranges it in forward)
        both = torch.empty(2 * n, L0, Cc, device=dev)
        feat_c0, feat_c1 = both[:n], both[n:]
    else:
        feat_c0 = torch.empty(n, L0, Cc, device=dev)
        feat_c1 = torch.empty(n, L1, Cc, device=dev)
    ops.pos_encode_flatten_gather(bank0.coarse_map(), t0, pe, out=feat_c0)
    ops.pos_encode_flatten_gather(bank1.coarse_map(), t1, pe, out=feat_c1)
    return data, feat_c0, feat_c1, t0, t1


def _pair_guards(model, bank0, ids0, bank1, ids1, who):
    """The checks of a call on n pairs of bank slots -> (bank1, ids0, ids1, flags): the ids as host lists, flags = (the slots carry
    masks, the side-0 slots carry scales, the side-1 slots carry scales)."""
    if model.training:
        raise LoftrHipError(f"{who}: inference only; call .eval()")
    bank1 = bank0 if bank1 is None else bank1
    if ids1 is None:
        raise ValueError(f"{who}: ids1 is required")
    ids0, ids1 = _host_ids(ids0, "ids0"), _host_ids(ids1, "ids1")
    n = len(ids0)
    if n == 0 or len(ids1) != n:
        raise ValueError(f"{who}: ids0 / ids1 must hold the same positive number of slot ids, got {len(ids0)} / {len(ids1)}")
    dev = _model_device(model)
    for tag, bank in (("bank0", bank0), ("bank1", bank1)):
        if not isinstance(bank, FeatureBank):
            raise TypeError(f"{who}: {tag} must be a FeatureBank")
        if bank.coarse.device != dev or bank.fine.device != dev:
            raise LoftrHipError(f"{who}: {tag} is on {bank.coarse.device}, the model on {dev}")
    bank0._check(ids0, model, "ids0")
    bank1._check(ids1, model, "ids1")
    m0 = _side_flag(bank0, ids0, bank0._has_mask, "mask", "ids0", who)
    m1 = _side_flag(bank1, ids1, bank1._has_mask, "mask", "ids1", who)
    if m0 != m1:
        raise ValueError(f"{who}: the slots of one side carry masks and those of the other do not (forward needs both or neither)")
    s0 = _side_flag(bank0, ids0, bank0._has_scale, "scale", "ids0", who)
    s1 = _side_flag(bank1, ids1, bank1._has_scale, "scale", "ids1", who)
    return bank1, ids0, ids1, (m0, s0, s1)


def match_pairs(model, bank0, ids0, bank1=None, ids1=None):
    """LoFTR.match_pairs (see there)."""
    bank1, ids0, ids1, flags = _pair_guards(model, bank0, ids0, bank1, ids1, "match_pairs")
    with torch.no_grad(), torch.cuda.device(_model_device(model)):
        data, feat_c0, feat_c1, t0, t1 = _encode_pairs(model, bank0, ids0, bank1, ids1, flags)
        f0, f1 = bank0.fine_map(), bank1.fine_map()
        model._match_encoded(feat_c0, feat_c1, data,
                             lambda c0, c1: model.fine_preprocess.forward_gather(f0, t0, f1, t1, c0, c1, data))
    return data


def _point_pairs(b_ids, pts0, pts1, n, dev):
    """The checks of the point pairs of ``refine_points`` -> (b_ids i64, pts0 f32, pts1 f32) contiguous on ``dev``.  ``b_ids`` must
    ascend and lie in [0, n): a host sequence is checked for free, a device tensor costs the readback of one flag, here, before
    anything is launched (a pair outside the batch would index the slot tables out of range)."""
    b = b_ids if isinstance(b_ids, torch.Tensor) else torch.as_tensor(np.asarray(b_ids))
    if b.dim() != 1 or b.dtype.is_floating_point or b.dtype == torch.bool:
        raise ValueError(f"refine_points: b_ids must be a 1-D integer sequence, got {tuple(b.shape)} {b.dtype}")
    M = b.shape[0]
    pts = []
    for p, name in ((pts0, "pts0"), (pts1, "pts1")):
        p = p if isinstance(p, torch.Tensor) else torch.as_tensor(np.asarray(p))
        if tuple(p.shape) != (M, 2) or not p.dtype.is_floating_point:
            raise ValueError(f"refine_points: {name} must be a floating-point [{M}, 2] (one point per b_ids entry), got {tuple(p.shape)} {p.dtype}")
        pts.append(p)
    b = b.detach().to(torch.int64)
    if M:
        bad = (b[1:] < b[:-1]).any() | (b[0] < 0) | (b[-1] >= n)
        if bool(bad):
            raise ValueError(f"refine_points: b_ids must ascend and lie in [0, {n})")
    return (b.to(dev).contiguous(), *[p.detach().to(dev, torch.float32).contiguous() for p in pts])


def refine_points(model, bank0, ids0, bank1, ids1, b_ids, pts0, pts1):
    """LoFTR.refine_points (see there)."""
    n = len(ids0) if hasattr(ids0, "__len__") else 0
    dev = _model_device(model)
    b_ids, pts0, pts1 = _point_pairs(b_ids, pts0, pts1, n, dev)
    bank1, ids0, ids1, flags = _pair_guards(model, bank0, ids0, bank1, ids1, "refine_points")
    with torch.no_grad(), torch.cuda.device(dev):
        data, feat_c0, feat_c1, t0, t1 = _encode_pairs(model, bank0, ids0, bank1, ids1, flags)
        feat_c0, feat_c1 = model._coarse_transformer(feat_c0, feat_c1, data)[:2]
        ops.check_transformer_status(dev)
        s = data["hw0_i"][0] / data["hw0_f"][0]                 # FineMatching's scale: image pixels per fine pixel
        stride = data["hw0_f"][0] // data["hw0_c"][0]           # FinePreprocess's stride: fine pixels per coarse cell
        at = ops.refine_centres(pts0, pts1, b_ids, n, data["hw0_f"], data["hw1_f"], data["hw0_c"], data["hw1_c"], stride, s,
                                data.get("scale0"), data.get("scale1"))
        ok = at["ok"]
        if b_ids.shape[0] == 0:
            return {"pts0": at["pts0_s"], "pts1_start": at["pts1_s"], "pts1": at["pts1_s"].clone(),
                    "expec_f": torch.empty(0, 3, device=dev), "ok": ok}
        data.update(b_ids=b_ids, i_ids=at["i_ids"], j_ids=at["j_ids"])
        w0, w1 = model.fine_preprocess.forward_gather_at(bank0.fine_map(), t0, bank1.fine_map(), t1, feat_c0, feat_c1, data,
                                                         at["c0"], at["c1"])
        w0, w1 = model.loftr_fine(w0, w1, inplace=True)
        # reference quirk kept: scale1 is applied iff the side-0 slots carry a scale (fine_matching.py:68)
        expec, pts1_f = ops.fine_match(w0, w1, at["pts1_s"], b_ids, s, data["scale1"] if "scale0" in data else None)
        bad = (ok == 0).unsqueeze(1)
        nan = torch.full((), float("nan"), device=dev)
        return {"pts0": at["pts0_s"], "pts1_start": at["pts1_s"], "pts1": torch.where(bad, nan, pts1_f),
                "expec_f": torch.where(bad, nan, expec), "ok": ok}


# ---- pair lists -----------------------------------------------------------------------------------------------------------
Extract = namedtuple("Extract", "images slots")             # run the backbone on `images` (ids), store them in `slots`
Match = namedtuple("Match", "rows slots0 slots1")           # match pair-list rows `rows` (range) from these slots


def plan_pair_list(pairs, n_slots, batch_size=8, extract_batch=16):
    """Schedule of a pair list on a bank of ``n_slots`` slots (pure host code).  ``pairs`` [P, 2] non-negative image ids.

    Returns a list of Extract(images, slots) and Match(rows, slots0, slots1) steps.  Matches cover consecutive chunks of
    ``batch_size`` rows in input order.  Before a chunk, its missing images are extracted in groups of up to ``extract_batch``;
    the last group is filled with the images the next chunks use, in first-use order (look-ahead).  Eviction is Belady's:
    the resident image whose next use is farthest goes first, never one the current chunk needs; a look-ahead image only
    takes the slot of an image whose next use comes after its own, and the look-ahead stops when no such slot is left."""
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[1] != 2 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"plan_pair_list: pairs must be an integer array [P, 2], got {p.shape} {p.dtype}")
    if p.size and (p.min() < 0 or p.max() > np.iinfo(np.int32).max):
        raise ValueError("plan_pair_list: image ids must be non-negative int32 values")
    batch_size, extract_batch, n_slots = int(batch_size), int(extract_batch), int(n_slots)
    if batch_size < 1 or extract_batch < 1:
        raise ValueError("plan_pair_list: batch_size and extract_batch must be positive")
    if n_slots < 2 * batch_size:
        raise ValueError(f"plan_pair_list: n_slots ({n_slots}) must be at least 2 * batch_size ({2 * batch_size}): "
                         f"one chunk may use that many distinct images")
    P = p.shape[0]
    chunks = [range(c, min(c + batch_size, P)) for c in range(0, P, batch_size)]
    # per chunk: its distinct images in first-use order (row order, side 0 before side 1); per image: the chunks that use it
    chunk_images, uses = [], {}
    for c, rows in enumerate(chunks):
        imgs = list(dict.fromkeys(int(v) for v in p[rows.start:rows.stop].reshape(-1)))
        chunk_images.append(imgs)
        for x in imgs:
            uses.setdefault(x, []).append(c)
    INF = len(chunks)

    def next_use(x, c):
        u = uses[x]
        k = bisect.bisect_left(u, c)
        return u[k] if k < len(u) else INF

    resident = {}                                   # image -> slot (insertion order breaks ties between equal next uses)
    free = list(range(n_slots))
    steps = []
    for c, rows in enumerate(chunks):
        need = chunk_images[c]
        missing = [x for x in need if x not in resident]
        if missing:
            protected = set(need)
            groups, group = [], []

            def victim(limit):
                """The resident image with the farthest next use beyond `limit` that nothing protects (None: none)."""
                best, best_use = None, limit
                for x in resident:
                    if x in protected:
                        continue
                    u = next_use(x, c)
                    if u > best_use:
                        best, best_use = x, u
                return best

            def place(x, limit):
                if free:
                    slot = free.pop(0)
                else:
                    v = victim(limit)
                    if v is None:
                        return False
                    slot = resident.pop(v)
                resident[x] = slot
                protected.add(x)
                group.append((x, slot))
                return True

            for x in missing:                                   # required: evict the farthest next use (c: any image not needed now)
                if not place(x, c):
                    raise AssertionError("plan_pair_list: no slot for an image of the current chunk")   # n_slots >= 2 * batch_size
                if len(group) == extract_batch:
                    groups.append(group)
                    group = []
            if group:                                           # look-ahead fills the last group
                done = False
                for d in range(c + 1, len(chunks)):
                    for x in chunk_images[d]:
                        if x in resident:
                            continue
                        if len(group) == extract_batch or not place(x, d):
                            done = True
                            break
                    if done:
                        break
                groups.append(group)
            for g in groups:
                steps.append(Extract([x for x, _ in g], [s for _, s in g]))
        steps.append(Match(rows, [resident[int(a)] for a in p[rows.start:rows.stop, 0]],
                           [resident[int(b)] for b in p[rows.start:rows.stop, 1]]))
    return steps


def match_pair_list(model, pairs, load, image_hw, budget_bytes=None, batch_size=8, extract_batch=16, stats=None):
    """Match every pair of ``pairs`` [P, 2] (image ids) with the backbone run once per resident image.

    ``load(image_ids)`` returns ``{"image": [k, 1, H, W] fp32 on the model's GPU, "mask": optional [k, h_c, w_c], "scale":
    optional [k, 2]}``.  The bank holds ``budget_bytes // FeatureBank.image_bytes`` images (default budget: half the free
    device memory; never more than the distinct images need).  Yields ``(rows, data)`` per chunk of ``batch_size`` consecutive
    rows, in input order, ``data`` as from ``LoFTR.match_pairs``.  Runs serially on the current stream.  ``stats`` (a dict):
    filled with n_slots, bank_bytes, images_extracted, backbone_calls."""
    for bank, st in _scheduled_chunks("match_pair_list", model, pairs, load, image_hw, budget_bytes, batch_size, extract_batch, stats):
        yield st.rows, match_pairs(model, bank, st.slots0, bank, st.slots1)


def _scheduled_chunks(who, model, pairs, load, image_hw, budget_bytes, batch_size, extract_batch, stats):
    """The schedule of ``plan_pair_list`` carried out on one bank: runs the Extract steps and yields ``(bank, step)`` at every Match
    step (what ``match_pair_list`` and ``refine_pair_list`` share)."""
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"{who}: pairs must be [P, 2], got {p.shape}")
    distinct = len(np.unique(p)) if p.size else 0
    per_image = FeatureBank.image_bytes(model, image_hw)
    if budget_bytes is None:
        budget_bytes = torch.cuda.mem_get_info(_model_device(model))[0] // 2
    n_slots = min(int(budget_bytes) // per_image, max(distinct, 2 * int(batch_size)))
    steps = plan_pair_list(p, n_slots, batch_size, extract_batch)
    bank = FeatureBank(model, n_slots, image_hw)
    bank.EXTRACT_BATCH = max(1, int(extract_batch))
    if stats is not None:
        stats.update(n_slots=n_slots, bank_bytes=n_slots * per_image)
    for st in steps:
        if isinstance(st, Extract):
            batch = load(list(st.images))
            bank.add(batch["image"], mask=batch.get("mask"), scale=batch.get("scale"), slots=st.slots)
        else:
            yield bank, st
    if stats is not None:
        stats.update(images_extracted=bank.images_extracted, backbone_calls=bank.backbone_calls)


def refine_pair_list(model, pairs, pair_offsets, pts0, pts1, load, image_hw, budget_bytes=None, batch_size=8, extract_batch=16, stats=None):
    """``LoFTR.refine_points`` over a whole job list, scheduled like ``match_pair_list`` (the same chunks, the same eviction, one bank).

    ``pairs`` [P, 2] (reference image, query image); ``pair_offsets`` [P+1], a host array that delimits the jobs of each pair in
    ``pts0`` / ``pts1`` [J, 2] (reference point, query point; any device).  Yields ``(job_slice, result)`` per chunk of ``batch_size``
    consecutive pairs, in input order: ``job_slice`` the jobs of the chunk, ``result`` the dict of ``refine_points`` for them with
    ``b_ids`` = the pair's index within the chunk.  ``load``, ``image_hw``, ``budget_bytes``, ``stats`` as for ``match_pair_list``."""
    p = np.asarray(pairs)
    off = np.asarray(pair_offsets).astype(np.int64).reshape(-1)
    if p.ndim != 2 or off.shape[0] != p.shape[0] + 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != pts0.shape[0] or \
            tuple(pts1.shape) != tuple(pts0.shape):
        raise ValueError(f"refine_pair_list: pair_offsets must be [P+1], ascending from 0 to the number of jobs ({tuple(pts0.shape)}, "
                         f"{tuple(pts1.shape)}), got {off.shape} for pairs {p.shape}")
    for bank, st in _scheduled_chunks("refine_pair_list", model, pairs, load, image_hw, budget_bytes, batch_size, extract_batch, stats):
        jobs = slice(int(off[st.rows.start]), int(off[st.rows.stop]))
        b_ids = torch.from_numpy(np.repeat(np.arange(len(st.rows), dtype=np.int64), np.diff(off[st.rows.start:st.rows.stop + 1])))
        yield jobs, refine_points(model, bank, st.slots0, bank, st.slots1, b_ids, pts0[jobs], pts1[jobs])
