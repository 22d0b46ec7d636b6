"""Drop-in ``LoFTR`` matcher whose matching path runs on hand-written HIP kernels (gfx950).

Host-side mirror of the reference interface (zju3dv/LoFTR ``src/loftr/loftr.py``): same
constructor, same ``forward(data)`` that *mutates* the batch dict with the same keys / dtypes,
same sub-module and parameter names (so reference checkpoints load with ``strict=True``), same
exceptions.  Every sub-module after the backbone holds parameters only; its arithmetic is one
call into ``libloftr_hip.so`` (``loftr_amd/ops.py``).  There is no PyTorch fallback: on a box
without the built extension or without a GPU the forward raises.

Scope: forward values, plus the backward of the whole model.  In ``.train()`` mode CoarseMatching
also performs the reference's random sampling / ground-truth padding of the coarse matches
(``coarse_matching.py:200-236``, host-side index arithmetic on the kernels' outputs).  Every node after the backbone is an
autograd node whose forward AND backward are HIP kernels (``loftr_amd/autograd.py``): position encoding, the encoder
layers of both transformers (round 4, ``csrc/encoder_bwd.hip``), CoarseMatching (dual-softmax and Sinkhorn incl.
``bin_score``), FinePreprocess (round 4, ``csrc/fine_bwd.hip``) and FineMatching.  ``LoFTR.full_grads = True``:
``loss.backward()`` fills ``.grad`` of every parameter like the reference's training step (the backbone runs as the
PyTorch module whose convolutions are autograd nodes on the HIP kernels too, ``backbone.Conv2d``; its BatchNorm with batch
statistics and elementwise glue stay PyTorch autograd); ``LoFTR.head_grads = True`` stops at the heads' inputs.
"""
import contextlib
import math
import warnings
import weakref

import torch
import torch.nn as nn

from . import autograd, ops
from .backbone import build_backbone


class PositionEncodingSine(nn.Module):
    """2-D sinusoidal encoding; constant table identical to position_encoding.py:22-35."""

    def __init__(self, d_model, max_shape=(256, 256), temp_bug_fix=True):
        super().__init__()
        ys = torch.arange(1, max_shape[0] + 1, dtype=torch.float32).view(1, -1, 1).expand(1, *max_shape)
        xs = torch.arange(1, max_shape[1] + 1, dtype=torch.float32).view(1, 1, -1).expand(1, *max_shape)
        idx = torch.arange(0, d_model // 2, 2).float()
        if temp_bug_fix:
            freq = torch.exp(idx * (-math.log(10000.0) / (d_model // 2)))
        else:   # the reference's legacy variant: `-log(1e4) / d_model // 2` floors to -1.0 (:28)
            freq = torch.exp(idx * (-math.log(10000.0) / d_model // 2))
        freq = freq[:, None, None]
        pe = torch.zeros((d_model, *max_shape))
        pe[0::4] = torch.sin(xs * freq)
        pe[1::4] = torch.cos(xs * freq)
        pe[2::4] = torch.sin(ys * freq)
        pe[3::4] = torch.cos(ys * freq)
        self.register_buffer("pe", pe.unsqueeze(0), persistent=False)     # [1, C, H, W]

    def forward(self, x):
        """x [N,C,H,W] -> (x + pe) flattened to [N, H*W, C] (fuses loftr.py:58-59's rearrange)."""
        if autograd.wants_grad(x):
            return autograd.pos_encode_flatten(x, self.pe[0])
        return ops.pos_encode_flatten(x, self.pe[0])


class LoFTREncoderLayer(nn.Module):
    """Parameter container + single-layer forward.  transformer.py:7-58."""

    def __init__(self, d_model, nhead, attention="linear"):
        super().__init__()
        if attention != "linear":
            raise NotImplementedError("only attention='linear' is on the HIP path (no shipped config uses 'full')")
        self.dim = d_model // nhead
        self.nhead = nhead
        self.q_proj = nn.Linear(d_model, d_model, bias=False)
        self.k_proj = nn.Linear(d_model, d_model, bias=False)
        self.v_proj = nn.Linear(d_model, d_model, bias=False)
        self.merge = nn.Linear(d_model, d_model, bias=False)
        self.mlp = nn.Sequential(
            nn.Linear(d_model * 2, d_model * 2, bias=False),
            nn.ReLU(True),
            nn.Linear(d_model * 2, d_model, bias=False),
        )
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)

    def weight_tensors(self):
        return {"q_proj": self.q_proj.weight, "k_proj": self.k_proj.weight, "v_proj": self.v_proj.weight,
                "merge": self.merge.weight, "mlp0": self.mlp[0].weight, "mlp2": self.mlp[2].weight,
                "norm1_w": self.norm1.weight, "norm1_b": self.norm1.bias,
                "norm2_w": self.norm2.weight, "norm2_b": self.norm2.bias}

    def weight_struct(self):
        sd = self.weight_tensors()
        for k, v in sd.items():
            if not v.is_contiguous() or v.dtype != torch.float32 or not v.is_cuda:
                raise ops._lib.LoftrHipError(f"{k}: parameters must be contiguous float32 GPU tensors "
                                             f"(got {v.dtype}, {v.device}); the HIP path computes in fp32")
        return ops.layer_weights_struct(sd)

    def forward(self, x, source, x_mask=None, source_mask=None):
        wants = autograd.wants_grad(x, source, *self.parameters())
        if wants and not self.training and autograd.wants_grad(x, source):
            import warnings                                       # (advisor, round 4: no silent graph cut)
            warnings.warn("LoFTREncoderLayer in .eval() mode returns a tensor WITHOUT a graph although its inputs require grad: "
                          "call .train() for the differentiable HIP nodes", stacklevel=2)
        if self.training and wants:      # .eval(): the inference kernels, no graph
            self.weight_struct()                                  # (dtype / device checks)
            return autograd.encoder_layer(x, source, self.weight_tensors(), self.nhead, x_mask, source_mask)
        return ops.encoder_layer(x.contiguous(), source.contiguous(), self.weight_struct(), self.nhead,
                                 x_mask, source_mask)


class LocalFeatureTransformer(nn.Module):
    """transformer.py:61-101.  The layer loop runs inside the C-ABI (one call per transformer)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.d_model = config["d_model"]
        self.nhead = config["nhead"]
        self.layer_names = config["layer_names"]
        self.layers = nn.ModuleList([LoFTREncoderLayer(config["d_model"], config["nhead"], config["attention"])
                                     for _ in range(len(self.layer_names))])
        self._reset_parameters()

    def _reset_parameters(self):
        first = self.layers[0].state_dict() if len(self.layers) else {}
        for p in self.layers[0].parameters() if len(self.layers) else []:
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        # the reference deep-copies ONE initialised layer (transformer.py:71-72) and then re-inits
        # every matrix (:75-78); only the second step matters for the resulting distribution
        for layer in self.layers[1:]:
            for p in layer.parameters():
                if p.dim() > 1:
                    nn.init.xavier_uniform_(p)
        del first

    def forward(self, feat0, feat1, mask0=None, mask1=None, inplace=False, mode=None, skip_padded=False):
        """``inplace`` (not in the reference signature): the caller owns feat0 / feat1 and does not need their
        input values any more; when they are the two halves of one buffer the layers then run on it directly.
        ``mode``: ops.COARSE_MODE for this call ("launches" / "persistent" / "auto"; None = the process default).
        ``skip_padded``: the caller never reads the features of padding tokens (ops.transformer; inference path only)."""
        assert self.d_model == feat0.size(2), "the feature number of src and transformer must be equal"
        for name in self.layer_names:
            if name not in ("self", "cross"):
                raise KeyError
        if not self.training and autograd.wants_grad(feat0, feat1):
            import warnings                                       # (advisor, round 4: no silent graph cut)
            warnings.warn("LocalFeatureTransformer in .eval() mode returns tensors WITHOUT a graph although its inputs require grad: "
                          "call .train() for the differentiable HIP nodes", stacklevel=2)
        if self.training and autograd.wants_grad(feat0, feat1, *self.parameters()):
            # differentiable form: the reference's own layer loop (transformer.py:91-99) over autograd nodes whose forward and
            # backward are the HIP kernels (loftr_amd/autograd.py:_EncoderLayer)
            for layer, name in zip(self.layers, self.layer_names):
                if name == "self":
                    feat0 = layer(feat0, feat0, mask0, mask0)
                    feat1 = layer(feat1, feat1, mask1, mask1)
                else:
                    feat0 = layer(feat0, feat1, mask0, mask1)
                    feat1 = layer(feat1, feat0, mask1, mask0)
            return feat0, feat1
        structs = [layer.weight_struct() for layer in self.layers]
        return ops.transformer(feat0.contiguous(), feat1.contiguous(), structs, self.layer_names, self.nhead,
                               mask0, mask1, inplace=inplace, prepared=self._prepared(structs, feat0.device), mode=mode,
                               skip_padded=skip_padded)

    def _prepared(self, structs, device):
        """The layers' matrices in the library's GEMM operand format, rebuilt only when a weight tensor is modified in
        place (tensor._version), replaced (data_ptr) or moved -- inference weights are constant, so the per-call
        re-encoding (a launch over 11 M weights per transformer) runs once."""
        if self.training or not str(device).startswith("cuda"):
            return None
        mats = [getattr(getattr(layer, n) if "." not in n else layer.mlp[int(n.split(".")[1])], "weight")
                for layer in self.layers for n in ("q_proj", "k_proj", "v_proj", "merge", "mlp.0", "mlp.2")]
        key = tuple((t.data_ptr(), t._version) for t in mats) + (str(device),)
        cached = ops._PREPARED.get(self)                 # module-keyed weak registry (not an attribute: modules stay picklable)
        if cached is None or cached[0] != key or not all(r() is t for r, t in zip(cached[2], mats)):
            cached = (key, ops.transformer_prepare(structs, self.d_model, device), [weakref.ref(t) for t in mats])
            ops._PREPARED[self] = cached
        return cached[1]


def _valid_cells(mask):
    """Cells of the top-left anchored valid rectangle of every sample of a padding mask [N, h, w] (what
    pad_bottom_right produces): tallest column x widest row."""
    return mask.sum(dim=1).amax(dim=-1) * mask.sum(dim=2).amax(dim=-1)


def compute_max_candidates(p_m0, p_m1):
    """Upper bound on the number of coarse matches of a padded batch: per pair the smaller of the two valid areas, summed
    (reference semantics: coarse_matching.py:44-54)."""
    return torch.minimum(_valid_cells(p_m0), _valid_cells(p_m1)).sum()


def _cell_points(ids, width, scale, image_scale, b_ids):
    """Pixel coordinates (x, y) of coarse cell ids on a grid `width` cells wide: cell -> (id mod width, id div width),
    times the coarse stride and, for resized images, the per-image (w, h) ratio of the owning pair."""
    xy = torch.stack((ids.remainder(width), ids.div(width, rounding_mode="floor")), dim=1)
    return xy * (scale if image_scale is None else scale * image_scale[b_ids])


class CoarseMatching(nn.Module):
    """coarse_matching.py:61-261."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.thr = config["thr"]
        self.border_rm = config["border_rm"]
        self.train_coarse_percent = config["train_coarse_percent"]
        self.train_pad_num_gt_min = config["train_pad_num_gt_min"]
        self.match_type = config["match_type"]
        # data['conf_matrix'] is a public output of the reference (:145); writing it costs one
        # L*S*4-byte store per pair.  Set False to elide it (data['conf_matrix'] = None).
        self.materialize_conf = True
        if self.match_type == "dual_softmax":
            self.temperature = config["dsmax_temperature"]
        elif self.match_type == "sinkhorn":
            self.bin_score = nn.Parameter(torch.tensor(config["skh_init_bin_score"], requires_grad=True))
            self.skh_iters = config["skh_iters"]
            self.skh_prefilter = config["skh_prefilter"]
        else:
            raise NotImplementedError()

    def forward(self, feat_c0, feat_c1, data, mask_c0=None, mask_c1=None):
        scale = data["hw0_i"][0] / data["hw0_c"][0]
        kw = dict(thr=self.thr, border_rm=self.border_rm, scale=scale, match_type=self.match_type,
                  mask0=mask_c0, mask1=mask_c1, scale0=data.get("scale0"), scale1=data.get("scale1"))
        if self.match_type == "dual_softmax":
            kw.update(temperature=self.temperature, want_conf=self.materialize_conf)
        else:
            sparse = self.config["sparse_spvs"]          # KeyError with cvpr default_cfg, like the reference (:142)
            kw.update(bin_score=float(self.bin_score.detach()), skh_iters=self.skh_iters,
                      skh_prefilter=self.skh_prefilter and not self.training,      # "if not self.training and ..." (:136)
                      want_assign=bool(sparse))
        hw = (tuple(data["hw0_c"]), tuple(data["hw1_c"]))
        if self.match_type == "dual_softmax" and autograd.wants_grad(feat_c0, feat_c1):
            # conf_matrix with its graph: forward and backward are the HIP kernels (loftr_amd/autograd.py)
            r = autograd.dual_softmax_match(feat_c0, feat_c1, *hw, **dict(kw, want_conf=True))
        elif (self.match_type == "sinkhorn" and not kw["skh_prefilter"] and
              (autograd.wants_grad(feat_c0, feat_c1) or (self.training and autograd.wants_grad(self.bin_score)))):
            r = autograd.sinkhorn_match(feat_c0, feat_c1, self.bin_score, *hw, **{k: v for k, v in kw.items() if k != "bin_score"})
            if not kw["want_assign"]:
                r.pop("conf_matrix_with_bin")
        else:
            if self.match_type == "sinkhorn" and kw["skh_prefilter"] and autograd.wants_grad(feat_c0, feat_c1, self.bin_score):
                # eval-mode prefilter (:136-140) rewrites conf in place inside the kernel: no graph on this path, unlike the
                # reference, which keeps autograd through its in-place writes.  Say so instead of failing later in backward().
                warnings.warn("CoarseMatching: eval-mode skh_prefilter=True returns conf_matrix WITHOUT an autograd graph "
                              "(inputs require grad); use .train() or skh_prefilter=False for a differentiable Sinkhorn head",
                              RuntimeWarning, stacklevel=2)
            r = ops.coarse_match(feat_c0, feat_c1, *hw, **kw)
        if "conf_matrix_with_bin" in r:
            data.update({"conf_matrix_with_bin": r["conf_matrix_with_bin"]})
        data.update({"conf_matrix": r["conf_matrix"]})
        mconf = r["mconf"]
        if self.training:
            data["_match_counts"] = r["counts"]
            return data.update(**self._train_sample(r, data, scale))
        out = {"b_ids": r["b_ids"], "i_ids": r["i_ids"], "j_ids": r["j_ids"]}
        if self.thr >= 0:
            # conf > thr >= 0  =>  mconf != 0 everywhere: the `mconf != 0` filter of :254-258 is a no-op
            out.update({"gt_mask": torch.zeros_like(mconf, dtype=torch.bool), "m_bids": r["b_ids"],
                        "mkpts0_c": r["mkpts0_c"], "mkpts1_c": r["mkpts1_c"], "mconf": mconf})
        else:
            keep = mconf != 0
            out.update({"gt_mask": mconf == 0, "m_bids": r["b_ids"][keep], "mkpts0_c": r["mkpts0_c"][keep],
                        "mkpts1_c": r["mkpts1_c"][keep], "mconf": mconf[keep]})
        data.update(**out)
        data["_match_counts"] = r["counts"]               # [1+N] int32: total, per pair (extra key)


    def _train_sample(self, r, data, scale):
        """Training-mode match list (reference semantics: coarse_matching.py:200-259).  The fine level trains on a fixed
        budget of windows: a share of the candidate cells, filled with the kernels' predictions (subsampled with
        replacement when there are too many) and topped up -- by at least `train_pad_num_gt_min` -- with ground-truth
        matches, which carry mconf = 0 and are dropped again from the coordinate / confidence lists (but NOT from the id
        lists the fine stage gathers with).  The two torch.randint draws happen in the reference's order (predictions,
        then padding) so that a seeded run reproduces its sample."""
        conf = data["conf_matrix"]
        if conf is None:
            raise ops._lib.LoftrHipError("CoarseMatching.train(): materialize_conf must stay True (the losses read conf_matrix)")
        n_batch, n0, n1 = conf.shape
        cells = compute_max_candidates(data["mask0"], data["mask1"]) if "mask0" in data else n_batch * max(n0, n1)
        budget, pad_min = int(cells * self.train_coarse_percent), self.train_pad_num_gt_min
        assert pad_min < budget, "min-num-gt-pad should be less than num-train-matches"
        pred = (r["b_ids"], r["i_ids"], r["j_ids"])
        truth = (data["spv_b_ids"], data["spv_i_ids"], data["spv_j_ids"])
        n_pred, n_truth, dev = pred[0].numel(), truth[0].numel(), r["mconf"].device
        room = budget - pad_min                              # slots the predictions may take
        take = torch.arange(n_pred, device=dev) if n_pred <= room else torch.randint(n_pred, (room,), device=dev)
        fill = torch.randint(n_truth, (max(budget - n_pred, pad_min),), device=dev)
        b_ids, i_ids, j_ids = (torch.cat((p[take], t[fill])) for p, t in zip(pred, truth))
        mconf = torch.cat((r["mconf"][take], r["mconf"].new_zeros(fill.numel())))
        predicted = mconf != 0                               # ground-truth padding is recognised by its zero confidence
        pts0 = _cell_points(i_ids, data["hw0_c"][1], scale, data.get("scale0"), b_ids)
        pts1 = _cell_points(j_ids, data["hw1_c"][1], scale, data.get("scale1"), b_ids)
        return {"b_ids": b_ids, "i_ids": i_ids, "j_ids": j_ids, "gt_mask": ~predicted, "m_bids": b_ids[predicted],
                "mkpts0_c": pts0[predicted], "mkpts1_c": pts1[predicted], "mconf": mconf[predicted]}


class FinePreprocess(nn.Module):
    """fine_preprocess.py:7-59."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.cat_c_feat = config["fine_concat_coarse_feat"]
        self.W = self.config["fine_window_size"]
        d_model_c = self.config["coarse"]["d_model"]
        d_model_f = self.config["fine"]["d_model"]
        self.d_model_f = d_model_f
        self.last_head = None                    # forward_windows: the form its last call took ("windows" / "dense")
        self.last_head_first = None              # forward_windows2: the form the head's FIRST convolution took ("windows" / "dense")
        if self.cat_c_feat:
            self.down_proj = nn.Linear(d_model_c, d_model_f, bias=True)
            self.merge_feat = nn.Linear(2 * d_model_f, d_model_f, bias=True)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.kaiming_normal_(p, mode="fan_out", nonlinearity="relu")

    def _begin(self, data, device):
        """What every form of the forward starts with: sets data["W"]; returns the window geometry (hw0_c, hw1_c, W, stride) the ops
        take, the weight keywords, and the empty result when there is no match (else None)."""
        W = self.W
        stride = data["hw0_f"][0] // data["hw0_c"][0]
        data.update({"W": W})
        empty = None
        if data["b_ids"].shape[0] == 0:
            empty = tuple(torch.empty(0, W ** 2, self.d_model_f, device=device) for _ in range(2))
        kw = {}
        if self.cat_c_feat:
            kw = dict(down_w=self.down_proj.weight, down_b=self.down_proj.bias,
                      merge_w=self.merge_feat.weight, merge_b=self.merge_feat.bias)
        return (tuple(data["hw0_c"]), tuple(data["hw1_c"]), W, stride), kw, empty

    def forward(self, feat_f0, feat_f1, feat_c0, feat_c1, data):
        geo, kw, empty = self._begin(data, feat_f0.device)
        if empty is not None:
            return empty
        wants = autograd.wants_grad(feat_f0, feat_f1, feat_c0, feat_c1, *self.parameters())
        if wants and self.training and not self.cat_c_feat:
            # no silent graph cut (advisor, round 4): the backward of the window gather alone (fine_concat_coarse_feat=False) is not built
            raise ops._lib.LoftrHipError("FinePreprocess: gradients requested with fine_concat_coarse_feat=False, whose backward is not "
                                         "implemented (csrc/fine_bwd.hip covers the reference's default, True)")
        if self.training and self.cat_c_feat and wants:
            return autograd.fine_preprocess(feat_f0, feat_f1, feat_c0, feat_c1, (data["b_ids"], data["i_ids"], data["j_ids"]), geo, **kw)
        return ops.fine_preprocess(feat_f0, feat_f1, feat_c0, feat_c1, data["b_ids"], data["i_ids"], data["j_ids"], *geo, **kw)

    def forward_windows(self, h_sp0, h_sp1, cin, conv, dense_fn, fine_head, feat_c0, feat_c1, data):
        """Inference forward from the INPUTS of the fine head's last convolution `conv` (SP [N, H, W, ceil32(cin)] per image batch): the
        convolution is evaluated at the matched windows only (csrc/window_head.hip), or -- fine_head None and too many windows for that
        to be the cheaper form (ops.window_head_wins) -- densely by `dense_fn(h_sp)` and gathered as in forward.  Bit-identical either
        way (tests/test_hip_window_head.py runs both).  fine_head: None or "windows" (LoFTR.forward does not come here with "dense")."""
        M = data["b_ids"].shape[0]
        dense_pixels = 2 * h_sp0.shape[0] * h_sp0.shape[1] * h_sp0.shape[2]
        windows = fine_head == "windows" or ops.window_head_wins(M, dense_pixels)
        if M == 0 or not windows or not ops.window_head_supported(self.W, cin, conv.out_channels, h_sp0, h_sp1):
            self.last_head = "dense"
            if M == 0:                                      # (forward reads nothing but the device of its maps then)
                return self.forward(h_sp0, h_sp1, feat_c0, feat_c1, data)
            return self.forward(dense_fn(h_sp0), dense_fn(h_sp1), feat_c0, feat_c1, data)
        self.last_head = "windows"
        geo, kw, _ = self._begin(data, h_sp0.device)
        return ops.fine_preprocess_windows(h_sp0, h_sp1, cin, conv, feat_c0, feat_c1, data["b_ids"], data["i_ids"], data["j_ids"], *geo, **kw)

    def forward_windows2(self, t_sp0, t_sp1, cin, head, first_fn, dense_fn, fine_head, feat_c0, feat_c1, data):
        """Inference forward from the INPUTS of the fine head `head` (conv, BN, LeakyReLU, conv; SP [N, H, W, ceil32(cin)] per image
        batch).  Three forms, bit-identical (tests/test_hip_window_head_first.py): both convolutions at the matched windows
        (csrc/window_head_first.hip) while ops.window_head_first_wins says so or fine_head is "windows"; otherwise the first one
        densely by `first_fn(t_sp)` and then forward_windows (the last one at the windows, or densely too)."""
        M = data["b_ids"].shape[0]
        dense_pixels = 2 * t_sp0.shape[0] * t_sp0.shape[1] * t_sp0.shape[2]
        both = (M > 0 and (fine_head == "windows" or ops.window_head_first_wins(M, dense_pixels))
                and ops.window_head_first_supported(self.W, cin, head[0], head[3], t_sp0, t_sp1, M))
        if not both:
            self.last_head_first = "dense"
            if M == 0:                                      # (nothing is read but the device of the maps)
                return self.forward_windows(t_sp0, t_sp1, head[0].out_channels, head[3], dense_fn, fine_head, feat_c0, feat_c1, data)
            stacked = ops.stacked_halves(t_sp0, t_sp1)      # the halves of one backbone batch: one launch
            if stacked is not None:
                h_sp0, h_sp1 = first_fn(stacked).split(t_sp0.shape[0])
            else:
                h_sp0, h_sp1 = first_fn(t_sp0), first_fn(t_sp1)
            return self.forward_windows(h_sp0, h_sp1, head[0].out_channels, head[3], dense_fn, fine_head, feat_c0, feat_c1, data)
        self.last_head = self.last_head_first = "windows"
        geo, kw, _ = self._begin(data, t_sp0.device)
        return ops.fine_preprocess_windows2(t_sp0, t_sp1, cin, head[0], head[1], head[3], feat_c0, feat_c1, data["b_ids"], data["i_ids"],
                                            data["j_ids"], *geo, **kw)

    def forward_gather(self, bank_f0, slot0, bank_f1, slot1, feat_c0, feat_c1, data):
        """Inference forward with the fine maps of pair b read from bank_f0[slot0[b]] / bank_f1[slot1[b]] (LoFTR.match_pairs)."""
        geo, kw, empty = self._begin(data, bank_f0.device)
        if empty is not None:
            return empty
        return ops.fine_preprocess_gather(bank_f0, slot0, bank_f1, slot1, feat_c0, feat_c1, data["b_ids"], data["i_ids"], data["j_ids"],
                                          *geo, **kw)

    def forward_gather_at(self, bank_f0, slot0, bank_f1, slot1, feat_c0, feat_c1, data, c0, c1):
        """forward_gather with the window of match m centred at c0[m] / c1[m] ([M,2] i32 (x, y) in fine pixels) instead of at its
        coarse cell (LoFTR.refine_points); data["i_ids"] / data["j_ids"] are the cells the coarse features are read from."""
        geo, kw, empty = self._begin(data, bank_f0.device)
        if empty is not None:
            return empty
        return ops.fine_preprocess_gather_at(bank_f0, slot0, bank_f1, slot1, feat_c0, feat_c1, data["b_ids"], data["i_ids"], data["j_ids"],
                                             c0, c1, *geo, **kw)


class FineMatching(nn.Module):
    """fine_matching.py:9-74."""

    def forward(self, feat_f0, feat_f1, data):
        M, WW, C = feat_f0.shape
        scale = data["hw0_i"][0] / data["hw0_f"][0]
        if M == 0:
            assert self.training is False, "M is always >0, when training, see coarse_matching.py"
            data.update({"expec_f": torch.empty(0, 3, device=feat_f0.device),
                         "mkpts0_f": data["mkpts0_c"], "mkpts1_f": data["mkpts1_c"]})
            return
        # reference quirk kept: scale1 is applied iff 'scale0' is in the batch (fine_matching.py:68)
        scale1 = data["scale1"] if "scale0" in data else None
        n = len(data["mconf"])
        fine_match = autograd.fine_match if autograd.wants_grad(feat_f0, feat_f1) else ops.fine_match
        if data["mkpts1_c"].shape[0] == M:
            expec, mk1f = fine_match(feat_f0, feat_f1, data["mkpts1_c"], data["b_ids"], scale, scale1)
            mk1f = mk1f[:n]
        else:
            # thr < 0 or .train(): CoarseMatching dropped the `mconf == 0` rows from mkpts*_c (coarse_matching.py:254-258)
            # but not from b_ids, so there are M windows and n < M coarse points.  The reference then adds the
            # refinement of the FIRST n windows to the n kept points (fine_matching.py:69, `[:len(mconf)]`): the
            # kernel computes all M offsets from a zero base (one base point per window, never out of bounds).
            expec, off = fine_match(feat_f0, feat_f1, torch.zeros(M, 2, device=feat_f0.device), data["b_ids"], scale, scale1)
            mk1f = data["mkpts1_c"] + off[:n]
        data.update({"expec_f": expec, "mkpts0_f": data["mkpts0_c"], "mkpts1_f": mk1f})


class LoFTR(nn.Module):
    """loftr.py:12-81."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        # channels-last is MIOpen's fastest fp32 layout on MI355X (-16 % backbone time) and hands the
        # HIP path [.., H, W, C]-ordered maps: the flatten and the fine-window gather then read
        # fully coalesced.  Pure storage-order choice: parameter names / shapes are unchanged.
        self.backbone = build_backbone(config).to(memory_format=torch.channels_last)
        # 'hip': convolutions on the library's implicit-GEMM kernels (backbone.forward_hip); 'torch': MIOpen.
        self.backbone_impl = "hip"
        # With the HIP backbone the FPN top-down (fine) branch runs on a second HIP stream, concurrently with the
        # coarse transformer + coarse matching it does not feed; joined before FinePreprocess.
        self.overlap_fine_branch = True
        self.skip_padded_tiles = True                        # with masks: fully padded 128-token tiles of the coarse level are not computed
        self.coarse_mode = None                              # None: ops.COARSE_MODE ("auto"); "launches" / "persistent" / "auto" for this model
        self.fine_join_late = False                          # True: join the side stream after coarse matching instead of after the coarse transformer (A/B)
        self._side_stream = None
        # None: from 8 pairs on, image0 / image1 batches go through the backbone on two side streams (see run_backbone; measured in the bench
        # step, profiles/r06_coarse_mode_ab.txt: 8 pairs 20.52 -> 20.10 ms, a single pair 4.29 -> 5.34 ms: below 8 pairs the extra launches cost
        # more than the filled tails give); True / False: always / never
        self.backbone_halves = None
        self._half_streams = None
        # The last convolution of the fine head has one consumer in the inference forward, the 5 x 5 windows of FinePreprocess.  None:
        # forward evaluates it at the matched windows only (csrc/window_head.hip) while that is the cheaper form (ops.window_head_wins)
        # and densely otherwise -- and the head's first convolution at the windows' 7 x 7 neighbourhoods only
        # (csrc/window_head_first.hip) while ops.window_head_first_wins; "windows" / "dense": always that form where the window form
        # applies at all (eval mode, HIP backbone, ResNetFPN_8_2, equally sized images, one backbone batch).  Bit-identical results.  run_backbone / match_from_features / match_pairs
        # keep the dense maps.
        self.fine_head = None
        # .train() only: hand the two matching heads their inputs as autograd LEAVES (data['_head_inputs']) and run the heads
        # with a graph, so that LoFTRLoss(...)(data); data['loss'].backward() leaves d loss / d (transformer outputs) in
        # their .grad -- the part of the reference's backward pass this library provides (loftr_amd/autograd.py).
        self.head_grads = False
        # .train() only, round 4: run the WHOLE matcher with a graph -- every node after the backbone is an autograd node whose
        # forward and backward are HIP kernels (loftr_amd/autograd.py: position encoding, encoder layers of both transformers, both
        # matching heads, FinePreprocess, FineMatching); the backbone runs as the PyTorch module with its convolutions as HIP
        # autograd nodes (backbone.Conv2d).  LoFTRLoss(...)(data); data['loss'].backward() then fills .grad of every parameter, as
        # the reference's training step does (src/lightning/lightning_loftr.py:112-133; training.trainval_inference).
        self.full_grads = False
        self.pos_encoding = PositionEncodingSine(config["coarse"]["d_model"],
                                                 temp_bug_fix=config["coarse"]["temp_bug_fix"])
        self.loftr_coarse = LocalFeatureTransformer(config["coarse"])
        self.coarse_matching = CoarseMatching(config["match_coarse"])
        self.fine_preprocess = FinePreprocess(config)
        self.loftr_fine = LocalFeatureTransformer(config["fine"])
        self.fine_matching = FineMatching()

    def _window_head_applies(self, data):
        """forward may hand FinePreprocess the inputs of the fine head's last convolution instead of the fine maps."""
        img0, img1 = data["image0"], data["image1"]
        if (self.fine_head == "dense" or self.training or self.backbone_impl != "hip" or not img0.is_cuda
                or img0.shape[2:] != img1.shape[2:] or not hasattr(self.backbone, "WINDOW_HEAD") or not self.fine_preprocess.cat_c_feat):
            return False
        return img0.shape[0] + img1.shape[0] <= self._backbone_cap(img0)           # (chunked batches: dense)

    def _backbone_cap(self, x):
        """Images of x's size one backbone call takes: the convolution kernels index an activation tensor with 32 bits (conv.hip: images *
        pixels * channels < 2^31 at the widest 1/2-resolution map); larger batches go through in chunks (> 62 pairs at 640 x 480)."""
        return getattr(self, "_backbone_chunk_images", None) or max(1, (2 ** 31 - 1) // ((x.shape[2] // 2) * (x.shape[3] // 2) * 256))

    def run_backbone(self, data, head_input=False):
        """Step 1 of forward (loftr.py:39-54): returns (feat_c0, feat_c1, feat_f0, feat_f1).
        head_input=True (forward only, where _window_head_applies): the last two are the SP inputs of the fine head's last convolution
        (backbone.forward_hip) instead of the fine maps; head_input="t1": the SP inputs of the whole fine head."""
        data.update({"bs": data["image0"].size(0),
                     "hw0_i": data["image0"].shape[2:], "hw1_i": data["image1"].shape[2:]})
        cl = lambda img: img.contiguous(memory_format=torch.channels_last)   # C == 1: a restride, no copy
        use_hip = self.backbone_impl == "hip" and data["image0"].is_cuda and not self.training
        run = self.backbone.forward_hip if use_hip else self.backbone
        self._fine_join = None
        assert not head_input or (use_hip and data["hw0_i"] == data["hw1_i"])
        hkw = dict(head_input=head_input) if head_input else {}
        if data["hw0_i"] == data["hw1_i"]:
            x = cl(torch.cat([data["image0"], data["image1"]], dim=0))
            cap = self._backbone_cap(x)
            if use_hip and x.shape[0] > cap:
                outs = [run(x[i:i + cap]) for i in range(0, x.shape[0], cap)]
                feats_c, feats_f = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
            elif use_hip and self.overlap_fine_branch and (data["bs"] >= 8 if self.backbone_halves is None else self.backbone_halves):
                # The two image sets on TWO side streams (image0 batch, image1 batch -- the halves the outputs are split into anyway): the
                # launches of one half fill the last partly filled round of workgroups of the other's (tools/micro/backbone_halves.py:
                # 14.30 -> 14.00 ms for the 16-image backbone; bit-identical maps), each half's FPN fine branch follows its trunk on the same
                # stream and is joined before FinePreprocess like the single side stream below.
                main = torch.cuda.current_stream(x.device)
                # folded filters made on `main` BEFORE the fork: built inside a half's forward_hip (a fresh model, changed weights) the fold
                # would run on that half's stream while the other half reads the cached buffer unordered after it
                self.backbone.prepare_hip()
                if self._half_streams is None:
                    self._half_streams = [torch.cuda.Stream(device=x.device) for _ in range(2)]
                outs, fines, evs = [], [], []
                for k, st in enumerate(self._half_streams):
                    st.wait_stream(main)
                    xk = data["image0"] if k == 0 else data["image1"]
                    xk.record_stream(st)
                    with torch.cuda.stream(st):
                        fc, fine_fn = run(cl(xk), defer_fine=True, **hkw)
                        ev = torch.cuda.Event(); ev.record(st)
                        ff = fine_fn()
                    outs.append(fc); fines.append(ff); evs.append(ev)
                for k in range(2):
                    main.wait_event(evs[k])                  # the coarse maps; the fine maps are joined later (self._fine_join)
                    outs[k].record_stream(main); fines[k].record_stream(main)
                self._fine_join = list(self._half_streams)
                return outs[0], outs[1], fines[0], fines[1]
            elif use_hip and self.overlap_fine_branch:
                feats_c, fine_fn = run(x, defer_fine=True, **hkw)
                main = torch.cuda.current_stream(x.device)
                if self._side_stream is None:
                    self._side_stream = torch.cuda.Stream(device=x.device)    # (ROCm's priority range is (0, -1): no LOW priority to give it)
                side = self._side_stream
                side.wait_stream(main)                       # the fine branch reads what the trunk produced
                for t in fine_fn.reads:                      # ... and the caching allocator must not recycle those
                    t.record_stream(side)                    #     buffers for this stream while the side stream reads them
                with torch.cuda.stream(side):
                    feats_f = fine_fn()
                feats_f.record_stream(main)                  # allocated on the side stream, consumed on this one
                self._fine_join = side                       # joined in match_from_features before FinePreprocess
            elif head_input:
                feats_c, fine_fn = run(x, defer_fine=True, **hkw)
                feats_f = fine_fn()
            else:
                feats_c, feats_f = run(x)
            (feat_c0, feat_c1), (feat_f0, feat_f1) = feats_c.split(data["bs"]), feats_f.split(data["bs"])
        else:
            (feat_c0, feat_f0), (feat_c1, feat_f1) = run(cl(data["image0"])), run(cl(data["image1"]))
        return feat_c0, feat_c1, feat_f0, feat_f1

    def _join_fine(self, device):
        j = getattr(self, "_fine_join", None)
        if j is not None:
            for st in (j if isinstance(j, list) else [j]):
                torch.cuda.current_stream(device).wait_stream(st)
            self._fine_join = None

    def match_from_features(self, feat_c0, feat_c1, feat_f0, feat_f1, data, head_input=False):
        """Steps 2-5 of forward (loftr.py:51-75): THE hot path.  `data` needs bs, hw0_i, hw1_i.
        head_input=True / "t1" (forward): feat_f0 / feat_f1 are run_backbone(head_input=...)'s SP tensors [N, H, W, Cp]."""
        data.update({"hw0_c": feat_c0.shape[2:], "hw1_c": feat_c1.shape[2:]})
        if head_input:
            data.update({"hw0_f": feat_f0.shape[1:3], "hw1_f": feat_f1.shape[1:3]})
        else:
            data.update({"hw0_f": feat_f0.shape[2:], "hw1_f": feat_f1.shape[2:]})
        # (not with a graph: as_strided's backward only reaches the FIRST half's tensor, the second half's gradient would be dropped)
        both = (ops.stacked_halves(feat_c0, feat_c1)
                if feat_c0.shape == feat_c1.shape and not autograd.wants_grad(feat_c0, feat_c1) else None)
        if both is not None:         # the two coarse maps are halves of one backbone batch: one launch, one buffer
            feat_c0, feat_c1 = self.pos_encoding(both).split(feat_c0.shape[0])
        else:
            feat_c0 = self.pos_encoding(feat_c0)
            feat_c1 = self.pos_encoding(feat_c1)
        if head_input == "t1":
            head = getattr(self.backbone, self.backbone.WINDOW_HEAD)
            fine_pre = lambda c0, c1: self.fine_preprocess.forward_windows2(feat_f0, feat_f1, head[0].in_channels, head, self.backbone.fine_head_first,
                                                                            self.backbone.fine_head_last, self.fine_head, c0, c1, data)
        elif head_input:
            head = getattr(self.backbone, self.backbone.WINDOW_HEAD)
            fine_pre = lambda c0, c1: self.fine_preprocess.forward_windows(feat_f0, feat_f1, head[0].out_channels, head[3], self.backbone.fine_head_last,
                                                                           self.fine_head, c0, c1, data)
        else:
            fine_pre = lambda c0, c1: self.fine_preprocess(feat_f0, feat_f1, c0, c1, data)
        self._match_encoded(feat_c0, feat_c1, data, fine_pre)

    def _match_encoded(self, feat_c0, feat_c1, data, fine_preprocess):
        """Steps 3-5 of forward from the position-encoded coarse features [N, L, C] (shared by match_from_features and match_pairs):
        coarse transformer, coarse matching, fine stage.  fine_preprocess(feat_c0, feat_c1) -> the two window tensors."""
        feat_c0, feat_c1, mask_c0, mask_c1 = self._coarse_transformer(feat_c0, feat_c1, data)
        # Join the side stream (FPN fine branch) HERE, not after coarse matching (self.fine_join_late restores that): the encoder
        # launches leave partly filled rounds that the convolution workgroups use, the score-volume kernels do not -- sharing the
        # GPU only doubled their duration (660 vs 340 us for pass B, profiles/r03_overlap_ab.txt) without shortening the step.
        if not self.fine_join_late:
            self._join_fine(feat_c0.device)
        full = self.training and self.full_grads
        grads = self.training and self.head_grads and not full
        if grads:
            feat_c0, feat_c1 = feat_c0.detach().requires_grad_(True), feat_c1.detach().requires_grad_(True)
            data["_head_inputs"] = {"feat_c0": feat_c0, "feat_c1": feat_c1}
        with torch.enable_grad() if grads else contextlib.nullcontext():
            self.coarse_matching(feat_c0, feat_c1, data, mask_c0=mask_c0, mask_c1=mask_c1)
        self._join_fine(feat_c0.device)                      # fine maps come from the side stream(s)
        if feat_c0.is_cuda:                                  # after the match-count sync: a refused plan / stalled persistent launch raises
            ops.check_transformer_status(feat_c0.device)
        feat_f0_unfold, feat_f1_unfold = fine_preprocess(feat_c0, feat_c1)
        if feat_f0_unfold.size(0) != 0:
            feat_f0_unfold, feat_f1_unfold = self.loftr_fine(feat_f0_unfold, feat_f1_unfold, inplace=True)
        if grads:
            feat_f0_unfold, feat_f1_unfold = feat_f0_unfold.detach().requires_grad_(True), feat_f1_unfold.detach().requires_grad_(True)
            data["_head_inputs"].update({"feat_f0_unfold": feat_f0_unfold, "feat_f1_unfold": feat_f1_unfold})
        with torch.enable_grad() if grads else contextlib.nullcontext():
            self.fine_matching(feat_f0_unfold, feat_f1_unfold, data)

    def _coarse_transformer(self, feat_c0, feat_c1, data):
        """The coarse transformer on the position-encoded coarse features [N, L, C], in place, with the padding masks of `data` (shared by
        _match_encoded and LoFTR.refine_points) -> (feat_c0, feat_c1, mask_c0, mask_c1), the masks flattened or None."""
        mask_c0 = mask_c1 = None
        if "mask0" in data:
            mask_c0, mask_c1 = data["mask0"].flatten(-2), data["mask1"].flatten(-2)
        # The coarse transformer has two forms with the same results to float32 noise (csrc/encoder_fused.hip): ONE persistent launch whose
        # 256 resident workgroups pull the layers' work items from a dependency-ordered queue, or per-call launches.  Alone on the GPU the
        # persistent form takes 3.13 ms against 3.29 (8 pairs, back to back); inside the bench step the variants of the schedule
        # (persistent / launches, fine branch on a side stream, half batches on two streams) all end within 2 % of each other -- the
        # MFMA-dense kernels run at the part's power limit (profiles/r06_coarse_mode_ab.txt, r06_power.txt).  ops.COARSE_MODE "auto" (the
        # default) takes the persistent form from 8 pairs on (profiles/r06_mode_sweep.txt).
        # Padding tokens (MegaDepth batches): nothing below reads their features -- coarse matching fills their scores, the fine stage gathers
        # at matched tokens only -- so the 128-token tiles without a valid token are not computed (self.skip_padded_tiles = False: the
        # reference's per-token mlp result for them; every other token is bit-identical either way).
        feat_c0, feat_c1 = self.loftr_coarse(feat_c0, feat_c1, mask_c0, mask_c1, inplace=True, mode=self.coarse_mode,
                                             skip_padded=self.skip_padded_tiles and mask_c0 is not None)   # fresh pos-encoded copies
        return feat_c0, feat_c1, mask_c0, mask_c1

    def forward(self, data):
        """Updates `data` in place exactly like the reference (loftr.py:29-75).

        data: image0, image1 [N,1,H,W] float; optional mask0/mask1 [N,H/8,W/8] ('0' = padded),
        scale0/scale1 [N,2].  Runs without a graph unless .train() and `full_grads` (see __init__).
        """
        # A graph is built only in .train() mode with `full_grads` AND when the caller's grad mode allows it: a validation pass run under
        # torch.no_grad() with the module still in train mode must not build (and keep) the whole graph (advisor, round 4).
        graph = self.training and self.full_grads and torch.is_grad_enabled()
        with torch.enable_grad() if graph else torch.no_grad():
            return self._forward(data)

    def _forward(self, data):
        dev = data["image0"].device
        if data["image1"].device != dev:
            raise ops._lib.LoftrHipError(f"image0 on {dev} but image1 on {data['image1'].device}")
        if dev.type != "cuda":                       # CPU tensors: the ops raise (no fallback); keep their message
            feat_c0, feat_c1, feat_f0, feat_f1 = self.run_backbone(data)
            return self.match_from_features(feat_c0, feat_c1, feat_f0, feat_f1, data)
        with torch.cuda.device(dev):                 # streams / workspaces / launches all on the tensors' GPU
            # (the side streams stop before the fine head: after coarse matching it runs at the matched windows, or its first
            # convolution densely on this stream -- FinePreprocess.forward_windows2)
            head_input = "t1" if self._window_head_applies(data) else False
            feat_c0, feat_c1, feat_f0, feat_f1 = self.run_backbone(data, head_input=head_input)
            self.match_from_features(feat_c0, feat_c1, feat_f0, feat_f1, data, head_input=head_input)

    def match_pairs(self, bank0, ids0, bank1=None, ids1=None):
        """Match n pairs of images whose backbone maps are in feature banks (loftr_amd/pairs.py: FeatureBank): pair k is
        (bank0[ids0[k]], bank1[ids1[k]]); bank1 defaults to bank0.  Returns the dict forward leaves for image0 = the images of
        ids0 and image1 = the images of ids1, without the images themselves: the same keys, dtypes and order (mask0 / mask1 and
        scale0 / scale1 gathered from the banks when their slots have them), bit for bit with backbone_impl 'hip'.  Inference
        only; runs without a graph."""
        from .pairs import match_pairs
        return match_pairs(self, bank0, ids0, bank1, ids1)

    def refine_points(self, bank0, ids0, bank1, ids1, b_ids, pts0, pts1):
        """Run the fine stage at points the caller names (loftr_amd/pairs.py): n image pairs from feature banks as in
        match_pairs, M point pairs ``pts0`` / ``pts1`` [M,2] in the coordinates forward returns, ``b_ids`` [M] the pair of each, ascending.
        Side 0 is the reference: its point is snapped to the fine grid (at most s/2 per axis, s = image pixels per fine pixel) and
        fixed.  Side 1 is the query: its window is centred at the fine pixel nearest to ``pts1`` and FineMatching refines it from there.
        The coarse transformer runs exactly as in match_pairs (masks from the banks, coarse_mode, skip_padded_tiles, the status check);
        coarse matching does not run.  -> dict: ``pts0`` [M,2] the snapped reference points, ``pts1_start`` [M,2] the snapped query
        points, ``pts1`` [M,2] the refined query points, ``expec_f`` [M,3], ``ok`` [M] u8 (0: a coordinate was not finite; ``pts1`` and
        ``expec_f`` are NaN there).  Called with the rows of a match_pairs result (b_ids, mkpts0_c, mkpts1_c) it returns that result's
        mkpts0_c, mkpts1_c, mkpts1_f and expec_f bit for bit.  Inference only; runs without a graph; ``b_ids`` given on the host is
        checked there, a device tensor costs the readback of one flag before anything is launched."""
        from .pairs import refine_points
        return refine_points(self, bank0, ids0, bank1, ids1, b_ids, pts0, pts1)

    def load_state_dict(self, state_dict, *args, **kwargs):
        for k in list(state_dict.keys()):
            if k.startswith("matcher."):
                state_dict[k.replace("matcher.", "", 1)] = state_dict.pop(k)
        return super().load_state_dict(state_dict, *args, **kwargs)
