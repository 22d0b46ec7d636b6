"""Goldens of the training-side consumers (forward values): the reference's own spvs_coarse / spvs_fine
(src/loftr/utils/supervision.py) and LoFTRLoss (src/losses/loftr_loss.py) on synthetic two-view geometry.

    python tests/golden/make_golden_train.py       # authoring container only (needs /root/reference)

Scene: a plane Z = Z0(x, y) seen by two cameras with a small relative motion; depth1 is the true depth of that
surface from camera 1 (ray / plane intersection), so that the bidirectional warp of spvs_coarse finds mutual nearest
cells; some depth holes (0) exercise the "warped to the corner" edge case.  Case `train_md` adds MegaDepth-style
padding masks and scale0 / scale1."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {"train_sc": dict(N=2, H=96, W=128, masks=False, seed=1),
         "train_md": dict(N=2, H=96, W=96, masks=True, seed=2),
         # corner cases of supervision.py:94-99 / loftr_loss.py:32-36,113-117,138-143: no ground truth at all (depth maps = 0)
         "train_nogt": dict(N=2, H=64, W=64, masks=False, seed=3, no_gt=True)}


def _rot(axis, ang):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def make_inputs(rc):
    rng = np.random.default_rng(rc["seed"])
    N, H, W = rc["N"], rc["H"], rc["W"]
    K0 = np.stack([np.array([[90.0 + 5 * n, 0, W / 2 - 1.5], [0, 92.0, H / 2 + 0.5], [0, 0, 1]]) for n in range(N)]).astype(np.float32)
    K1 = np.stack([np.array([[88.0, 0, W / 2 + 1.0], [0, 91.0 + 3 * n, H / 2 - 1.0], [0, 0, 1]]) for n in range(N)]).astype(np.float32)
    T01, T10, d0s, d1s = [], [], [], []
    for n in range(N):
        R = _rot(rng.standard_normal(3), 0.05 + 0.05 * rng.random())
        t = 0.15 * rng.standard_normal(3)
        T = np.eye(4); T[:3, :3], T[:3, 3] = R, t
        T01.append(T); T10.append(np.linalg.inv(T))
        Z0 = 3.0 + 0.3 * n
        d0 = np.full((H, W), Z0, np.float32)                     # fronto-parallel plane in camera 0
        nrm = R @ np.array([0, 0, 1.0])
        v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        rays = np.linalg.inv(K1[n].astype(np.float64)) @ np.stack([u.ravel(), v.ravel(), np.ones(H * W)])
        d1 = ((Z0 + nrm @ t) / (nrm @ rays)).reshape(H, W).astype(np.float32)
        holes = rng.random((H, W)) < 0.03
        d0[holes] = 0
        d1[rng.random((H, W)) < 0.03] = 0
        d0s.append(d0); d1s.append(d1)
    if rc.get("no_gt"):
        # zero depth alone is not "no ground truth" for the reference: spvs_coarse ignores warp_kpts' valid mask, every cell then
        # warps to the projection of the translation, and one spurious mutual pair appears.  Put that projection far outside
        # the image in both directions: every nearest index is 0 and cell 0 is excluded (supervision.py:76-81).
        d0s = [np.zeros_like(d) for d in d0s]
        d1s = [np.zeros_like(d) for d in d1s]
        for T in T01 + T10:
            T[:3, 3] = (5.0, 0.0, 0.01)
    inp = dict(depth0=np.stack(d0s), depth1=np.stack(d1s), T_0to1=np.stack(T01).astype(np.float32),
               T_1to0=np.stack(T10).astype(np.float32), K0=K0, K1=K1)
    if rc["masks"]:
        h, w = H // 8, W // 8
        m0, m1 = np.zeros((N, h, w), bool), np.zeros((N, h, w), bool)
        m0[0, :9, :], m0[1, :, :10] = True, True
        m1[0, :, :11], m1[1, :10, :] = True, True
        inp.update(mask0=m0, mask1=m1, scale0=np.array([[1.9, 1.9], [1.25, 1.5]], np.float32),
                   scale1=np.array([[1.0, 2.0], [1.6, 1.6]], np.float32))
        # the depth maps / intrinsics live at ORIGINAL resolution = resized * scale: keep it simple and scale K accordingly
        for k, sc in (("K0", inp["scale0"]), ("K1", inp["scale1"])):
            Kk = inp[k].copy(); Kk[:, 0, :] *= sc[:, :1]; Kk[:, 1, :] *= sc[:, 1:]; inp[k] = Kk
        big = lambda d, sc: np.stack([np.kron(d[n], np.ones((2, 2), np.float32)) for n in range(N)])     # 2x depth maps cover scale <= 2
        inp["depth0"], inp["depth1"] = big(inp["depth0"], None), big(inp["depth1"], None)
    return inp


def replay_matcher_outputs(rc, gt_b, gt_i, gt_j):
    """conf_matrix / conf_matrix_with_bin of a case, regenerated from the seed exactly as make() drew them."""
    rng = np.random.default_rng(rc["seed"] + 100)
    N, L = rc["N"], (rc["H"] // 8) * (rc["W"] // 8)
    S = L
    rng.random(len(gt_b)); rng.integers(0, N, 6); rng.integers(1, L, 6); rng.integers(0, S, 6)
    conf = rng.random((N, L, S)).astype(np.float32) ** 4
    conf[gt_b, gt_i, gt_j] = 0.3 + 0.69 * rng.random(len(gt_b)).astype(np.float32)
    conf_bin = rng.random((N, L + 1, S + 1)).astype(np.float32) ** 3
    return conf, conf_bin


def make(name):
    from oracle.ref_shim import import_reference_training
    sup, LoFTRLoss = import_reference_training()
    rc = CASES[name]
    inp = make_inputs(rc)
    N, H, W = rc["N"], rc["H"], rc["W"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    data = {"image0": torch.zeros(N, 1, H, W), "image1": torch.zeros(N, 1, H, W), "dataset_name": ["scannet"] * N,
            "pair_names": [["a"] * N, ["b"] * N], **{k: t(v) for k, v in inp.items()}}
    cfg = {"LOFTR": {"RESOLUTION": (8, 2), "FINE_WINDOW_SIZE": 5}}
    sup.spvs_coarse(data, cfg)
    store = {k: data[k].numpy() for k in ("spv_b_ids", "spv_i_ids", "spv_j_ids", "spv_w_pt0_i", "spv_pt1_i")}
    store["conf_gt_sum"] = data["conf_matrix_gt"].sum((1, 2)).numpy()
    # a plausible matcher output: the GT matches minus a few, plus a few wrong ones; conf / expec_f synthetic
    rng = np.random.default_rng(rc["seed"] + 100)
    L, S = (H // 8) * (W // 8), (H // 8) * (W // 8)
    gt_b, gt_i, gt_j = store["spv_b_ids"], store["spv_i_ids"], store["spv_j_ids"]
    keep = rng.random(len(gt_b)) < 0.8
    b = np.concatenate([gt_b[keep], rng.integers(0, N, 6)]); i = np.concatenate([gt_i[keep], rng.integers(1, L, 6)])
    j = np.concatenate([gt_j[keep], rng.integers(0, S, 6)])
    o = np.lexsort((i, b)); b, i, j = b[o], i[o], j[o]
    data.update(b_ids=t(b), i_ids=t(i), j_ids=t(j))
    sup.spvs_fine(data, cfg)
    store.update(b_ids=b, i_ids=i, j_ids=j, expec_f_gt=data["expec_f_gt"].numpy())
    conf = rng.random((N, L, S)).astype(np.float32) ** 4
    conf[gt_b, gt_i, gt_j] = 0.3 + 0.69 * rng.random(len(gt_b)).astype(np.float32)
    conf_bin = rng.random((N, L + 1, S + 1)).astype(np.float32) ** 3
    expec_f = np.concatenate([data["expec_f_gt"].numpy() + 0.1 * rng.standard_normal((len(b), 2)).astype(np.float32),
                              0.05 + rng.random((len(b), 1)).astype(np.float32)], 1).astype(np.float32)
    store.update(conf_seed=np.int64(rc["seed"] + 100), expec_f=expec_f)
    data.update(conf_matrix=t(conf), conf_matrix_with_bin=t(conf_bin), expec_f=t(expec_f))
    losses = {}
    for tag, (ctype, sparse, mtype, ftype) in {"focal_sparse_ds": ("focal", True, "dual_softmax", "l2_with_std"),
                                                 "focal_sparse_ot": ("focal", True, "sinkhorn", "l2_with_std"),
                                                 "focal_dense_ds": ("focal", False, "dual_softmax", "l2"),
                                                 "ce_dense_ds": ("cross_entropy", False, "dual_softmax", "l2_with_std")}.items():
        lcfg = {"loftr": {"loss": dict(coarse_type=ctype, coarse_weight=1.0, focal_alpha=0.25, focal_gamma=2.0, pos_weight=1.0,
                                       neg_weight=1.0, fine_type=ftype, fine_weight=1.0, fine_correct_thr=1.0),
                          "match_coarse": dict(match_type=mtype, sparse_spvs=sparse)}}
        crit = LoFTRLoss(lcfg).eval()
        d2 = dict(data)
        if ftype == "l2":                   # the reference's plain-l2 path takes [M,2] (loftr_loss.py:110-121)
            d2["expec_f"] = t(expec_f[:, :2].copy())
        crit(d2)
        losses[tag] = {k: float(v) for k, v in d2["loss_scalars"].items()}
    store["losses"] = np.array(json.dumps(losses))
    store["recipe"] = np.array(json.dumps(rc))
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **store)
    print(name, "GT matches", len(gt_b), "predictions", len(b), losses)


# ---- CoarseMatching.train(): random sampling / ground-truth padding (coarse_matching.py:200-259) ------------------
COARSE_TRAIN = {"ctrain_pad": dict(N=2, h=12, w=16, C=256, seed=11, percent=0.4, pad_min=20, masks=False, thr=0.0),      # few predictions: arange + GT padding
                "ctrain_sample": dict(N=2, h=12, w=16, C=256, seed=12, percent=0.12, pad_min=8, masks=True, thr=0.0)}    # more than the budget: sampled


def det_randint(high, size, device=None, **kw):
    """Deterministic stand-in for torch.randint in BOTH implementations (their RNG streams differ by device)."""
    n = size[0]
    return ((torch.arange(n, dtype=torch.int64) * 7919 + 13) % max(int(high), 1)).to(device)


def coarse_train_inputs(rc):
    rng = np.random.default_rng(rc["seed"])
    N, L, C = rc["N"], rc["h"] * rc["w"], rc["C"]
    f0 = rng.standard_normal((N, L, C)).astype(np.float32)
    perm = np.stack([rng.permutation(L) for _ in range(N)])
    f1 = np.stack([f0[n][perm[n]] for n in range(N)]) * 0.9 + 0.45 * rng.standard_normal((N, L, C)).astype(np.float32)
    f0, f1 = f0 * 4, f1.astype(np.float32) * 4           # peaked dual-softmax: a few hundred mutual matches
    G = 60
    spv = dict(spv_b_ids=rng.integers(0, N, G), spv_i_ids=rng.integers(1, L, G), spv_j_ids=rng.integers(0, L, G))
    inp = dict(feat_c0=f0, feat_c1=f1, **spv)
    if rc["masks"]:
        m0, m1 = np.zeros((N, rc["h"], rc["w"]), bool), np.zeros((N, rc["h"], rc["w"]), bool)
        m0[0, :10, :], m0[1, :, :13] = True, True
        m1[0, :, :14], m1[1, :11, :] = True, True
        inp.update(mask0=m0, mask1=m1, scale0=np.array([[1.5, 1.5], [1.0, 2.0]], np.float32), scale1=np.array([[2.0, 1.25], [1.1, 1.1]], np.float32))
    return inp


def coarse_train_config(rc):
    return dict(thr=rc["thr"], border_rm=1, train_coarse_percent=rc["percent"], train_pad_num_gt_min=rc["pad_min"], match_type="dual_softmax",
                dsmax_temperature=0.1, skh_init_bin_score=1.0, skh_iters=3, skh_prefilter=False, sparse_spvs=True)


def make_coarse_train(name):
    from oracle.ref_shim import import_reference
    import_reference()
    import importlib
    cm = importlib.import_module("src.loftr.utils.coarse_matching")
    rc = COARSE_TRAIN[name]
    inp = coarse_train_inputs(rc)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    H, W = rc["h"] * 8, rc["w"] * 8
    data = {"hw0_i": torch.Size([H, W]), "hw1_i": torch.Size([H, W]), "hw0_c": torch.Size([rc["h"], rc["w"]]), "hw1_c": torch.Size([rc["h"], rc["w"]]),
            **{k: t(v) for k, v in inp.items() if not k.startswith("feat")}}
    mod = cm.CoarseMatching(coarse_train_config(rc)).train()
    real = torch.randint
    torch.randint = det_randint
    try:
        m0 = data["mask0"].flatten(-2) if rc["masks"] else None
        m1 = data["mask1"].flatten(-2) if rc["masks"] else None
        with torch.no_grad():
            mod(t(inp["feat_c0"]), t(inp["feat_c1"]), data, mask_c0=m0, mask_c1=m1)
    finally:
        torch.randint = real
    keys = ("b_ids", "i_ids", "j_ids", "gt_mask", "m_bids", "mkpts0_c", "mkpts1_c", "mconf")
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), recipe=np.array(json.dumps(rc)), **{k: data[k].numpy() for k in keys})
    print(name, "fine-level training set", len(data["b_ids"]), "of which predictions", int((~data["gt_mask"]).sum()))


# Intra-op threads of the CPU training steps behind tstep_* / tfull_*.  oneDNN's float32 convolutions split their work by thread count, so the
# backbone's pre-activations move by ~1e-6 from one count to another and a unit within that of zero changes sign; at this count the
# PyTorch-CPU backbone reproduces the recorded forward bit for bit (AVX-512 Xeon and EPYC hosts alike).
GOLDEN_CPU_THREADS = 8


# ---- the whole training-step forward: PL_LoFTR._trainval_inference (lightning_loftr.py:82-93) --------------------------
# compute_supervision_coarse -> matcher(batch) in .train() mode -> compute_supervision_fine -> LoFTRLoss, on images + depth +
# poses; matcher weights seeded like the e2e goldens, torch.randint replaced by det_randint.
STEP_CASES = {"tstep_ds": dict(geometry="train_sc", thr=0.0, percent=0.4, pad_min=20, match_type="dual_softmax"),
              "tstep_ot": dict(geometry="train_sc", thr=0.0, percent=0.4, pad_min=20, match_type="sinkhorn")}
STEP_KEYS = ("spv_b_ids", "spv_i_ids", "spv_j_ids", "b_ids", "i_ids", "j_ids", "gt_mask", "m_bids", "mconf", "mkpts0_c", "mkpts1_c",
             "mkpts0_f", "mkpts1_f", "expec_f", "expec_f_gt")


def step_matcher_cfg(rc):
    from loftr_amd.config import full_default_cfg
    cfg = full_default_cfg()                               # src/config/default.py: temp_bug_fix True, sparse_spvs True
    cfg["match_coarse"].update(thr=rc["thr"], train_coarse_percent=rc["percent"], train_pad_num_gt_min=rc["pad_min"],
                               match_type=rc["match_type"])
    return cfg


def step_loss_cfg(rc):
    return {"loftr": {"loss": dict(coarse_type="focal", coarse_weight=1.0, focal_alpha=0.25, focal_gamma=2.0, pos_weight=1.0, neg_weight=1.0,
                                   fine_type="l2_with_std", fine_weight=1.0, fine_correct_thr=1.0),
                      "match_coarse": dict(match_type=rc["match_type"], sparse_spvs=True)}}


def step_batch(rc):
    """numpy inputs of a training step: images (seeded, correlated) + the two-view geometry of CASES[rc['geometry']]."""
    from loftr_amd.synth import make_images
    geo = CASES[rc["geometry"]]
    inp = make_inputs(geo)
    i0, i1 = make_images(4321, geo["N"], geo["H"], geo["W"])
    return dict(image0=i0, image1=i1, **inp), geo


def make_step(name):
    import copy
    from oracle.ref_shim import import_reference
    from tests.golden.make_golden_e2e import e2e_state_dict
    RefLoFTR, _ = import_reference()
    sup, LoFTRLoss = __import__("oracle.ref_shim", fromlist=["x"]).import_reference_training()
    torch.set_num_threads(GOLDEN_CPU_THREADS)
    rc = STEP_CASES[name]
    batch, geo = step_batch(rc)
    cfg = step_matcher_cfg(rc)
    model = RefLoFTR(copy.deepcopy(cfg))
    model.load_state_dict(e2e_state_dict(model, cfg, 0.3), strict=True)
    model.train()                                          # BatchNorm on batch statistics, CoarseMatching samples / pads
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    data = {"dataset_name": ["scannet"] * geo["N"], "pair_names": [["a"] * geo["N"], ["b"] * geo["N"]], **{k: t(v) for k, v in batch.items()}}
    real = torch.randint
    torch.randint = det_randint
    try:
        with torch.no_grad():
            sup.compute_supervision_coarse(data, {"LOFTR": {"RESOLUTION": (8, 2), "FINE_WINDOW_SIZE": 5}}) if False else sup.spvs_coarse(
                data, {"LOFTR": {"RESOLUTION": (8, 2), "FINE_WINDOW_SIZE": 5}})
            model(data)
            sup.spvs_fine(data, {"LOFTR": {"RESOLUTION": (8, 2), "FINE_WINDOW_SIZE": 5}})
            LoFTRLoss(step_loss_cfg(rc)).train()(data)
    finally:
        torch.randint = real
    store = {k: data[k].numpy() for k in STEP_KEYS}
    store["losses"] = np.array(json.dumps({k: float(v) for k, v in data["loss_scalars"].items()}))
    store["recipe"] = np.array(json.dumps(rc))
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **store)
    print(name, "training set", len(data["b_ids"]), "predictions", int((~data["gt_mask"]).sum()), "GT", len(data["spv_b_ids"]),
          {k: float(v) for k, v in data["loss_scalars"].items()})


# ---- the same step WITH autograd: d loss / d (inputs of the two matching heads) ---------------------------------------------
# lightning_loftr.py:112-133 back-propagates batch['loss'] through the whole network; this library provides the backward of
# the heads only, so the golden keeps the gradients AT the heads' inputs: d loss / d feat_f*_unfold (reached through loss_f
# alone) and, for the coarse features, the part that flows through conf_matrix (their other part -- through FinePreprocess
# and the fine transformer -- has no counterpart here).
GRAD_STEP_CASES = {"tgrad_ds": dict(step="tstep_ds", coarse_gain=0.25, fine_gain=0.25),
                   "tgrad_ot": dict(step="tstep_ot", coarse_gain=1.0, fine_gain=0.25)}     # gain: conf at the ground truth inside the clamp (1e-6, 1 - 1e-6)
GRAD_F1_FULL = 32                 # the LAST windows (the ground-truth padding: the ones with a fine loss) keep d loss / d feat_f1_unfold
                                  # in full; all windows: its per-window norm


def make_step_grads(name):
    import copy
    from oracle.ref_shim import import_reference
    from tests.golden.make_golden_e2e import e2e_state_dict
    RefLoFTR, _ = import_reference()
    sup, LoFTRLoss = __import__("oracle.ref_shim", fromlist=["x"]).import_reference_training()
    torch.set_num_threads(GOLDEN_CPU_THREADS)
    gc = GRAD_STEP_CASES[name]
    rc = STEP_CASES[gc["step"]]
    batch, geo = step_batch(rc)
    cfg = step_matcher_cfg(rc)
    model = RefLoFTR(copy.deepcopy(cfg))
    model.load_state_dict(e2e_state_dict(model, cfg, 0.3, gc["coarse_gain"], gc["fine_gain"]), strict=True)
    model.train()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    data = {"dataset_name": ["scannet"] * geo["N"], "pair_names": [["a"] * geo["N"], ["b"] * geo["N"]], **{k: t(v) for k, v in batch.items()}}
    seen = {}

    def tap(module, key):
        inner = module.forward

        def forward(a, b, *args, **kw):
            a.retain_grad(); b.retain_grad()
            seen[key] = (a, b)
            return inner(a, b, *args, **kw)
        module.forward = forward
    tap(model.coarse_matching, "coarse")
    tap(model.fine_matching, "fine")
    real = torch.randint
    torch.randint = det_randint
    try:
        C = {"LOFTR": {"RESOLUTION": (8, 2), "FINE_WINDOW_SIZE": 5}}
        with torch.no_grad():
            sup.spvs_coarse(data, C)
        model(data)
        with torch.no_grad():
            sup.spvs_fine(data, C)
        ot = rc["match_type"] == "sinkhorn"
        ckey = "conf_matrix_with_bin" if ot else "conf_matrix"          # the tensor the coarse loss reads (loftr_loss.py:174-177)
        data[ckey].retain_grad(); data["expec_f"].retain_grad()
        LoFTRLoss(step_loss_cfg(rc)).train()(data)
    finally:
        torch.randint = real
    data["loss"].backward()
    # Round 4: the gradient of EVERY parameter of the reference's training step (lightning_loftr.py:112-133 back-propagates batch['loss'] into
    # the whole matcher) -> tests/golden/tfull_*.npz, as digests (make_golden_layer_grad.digest: vectors whole; matrices / filters as a
    # strided sub-matrix plus all row and column sums of their 2-D view).
    from tests.golden.make_golden_layer_grad import digest
    full = dict(recipe=np.array(json.dumps(dict(rc, **gc))), losses=np.array(json.dumps({k: float(v) for k, v in data["loss_scalars"].items()})))
    for pname, prm in model.named_parameters():
        gnp = (prm.grad if prm.grad is not None else torch.zeros_like(prm)).numpy()
        full.update(digest("grad/" + pname, gnp.reshape(gnp.shape[0], -1) if gnp.ndim > 2 else gnp))
    # ... and the same step in float64 (same seeds, same sampled matches): |fp32 - fp64| per tensor is the reference's OWN rounding noise, the
    # yardstick the test holds the HIP path to (some gradients -- BatchNorm shifts, the fine-level q / k projections behind the attention
    # normaliser -- are sums with heavy cancellation: 1e-3 relative is not what float32 autograd itself delivers there).
    m64 = RefLoFTR(copy.deepcopy(cfg))
    m64.load_state_dict(e2e_state_dict(m64, cfg, 0.3, gc["coarse_gain"], gc["fine_gain"]), strict=True)
    m64 = m64.double().train()
    d64 = {"dataset_name": ["scannet"] * geo["N"], "pair_names": [["a"] * geo["N"], ["b"] * geo["N"]],
           **{k: (t(v).double() if t(v).is_floating_point() else t(v)) for k, v in batch.items()}}
    torch.randint = det_randint
    try:
        with torch.no_grad():
            sup.spvs_coarse(d64, C)
        m64(d64)
        with torch.no_grad():
            sup.spvs_fine(d64, C)
        LoFTRLoss(step_loss_cfg(rc)).train()(d64)
    finally:
        torch.randint = real
    same = all(torch.equal(d64[k], data[k]) for k in ("b_ids", "i_ids", "j_ids"))
    d64["loss"].backward()
    noise = {}
    for (pname, prm), (_, p64) in zip(model.named_parameters(), m64.named_parameters()):
        a = (prm.grad if prm.grad is not None else torch.zeros_like(prm)).double()
        b_ = p64.grad if p64.grad is not None else torch.zeros_like(p64)
        noise[pname] = float((a - b_).abs().max() / max(float(b_.abs().max()), 1e-300))
        g64 = b_.numpy()
        # (round 5) the float64 gradients themselves, same digest: what an arithmetic that is INDEPENDENT of the reference's float32
        # kernels is to be measured against -- its distance to this, next to the reference's own (noise), not its distance to one float32 sample
        full.update(digest("grad64/" + pname, g64.reshape(g64.shape[0], -1) if g64.ndim > 2 else g64))
    full["ref_noise"] = np.array(json.dumps(noise))
    full["ref64_same_matches"] = np.array(same)
    print("reference fp32 vs fp64 (same match set: %s): worst relative gradient deviations" % same,
          sorted(noise.items(), key=lambda kv: -kv[1])[:6])
    np.savez_compressed(os.path.join(HERE, name.replace("tgrad", "tfull") + ".npz"), **full)
    print(name.replace("tgrad", "tfull"), "%d parameter tensors, %.0f kB" % (len(list(model.parameters())),
          os.path.getsize(os.path.join(HERE, name.replace("tgrad", "tfull") + ".npz")) / 1e3))
    # d loss / d conf_matrix and d loss / d expec_f are now known.  The heads' OWN backward, cut from the rest of the graph
    # (the final feat_*1 of a transformer is computed from the final feat_*0, so feat_*0.grad of the full graph also contains
    # the transformer's share): re-run each head on detached copies of its inputs and back-propagate the node gradient.
    fc0, fc1 = (x.detach().requires_grad_(True) for x in seen["coarse"])
    ff0, ff1 = (x.detach().requires_grad_(True) for x in seen["fine"])
    scratch = {k: data[k] for k in ("hw0_c", "hw1_c", "hw0_i", "hw1_i") }
    model.coarse_matching.eval()                                       # same conf_matrix (:105-119), no sampling
    extra = {}
    if ot:
        model.coarse_matching.bin_score.grad = None
    model.coarse_matching(fc0, fc1, scratch)
    assert torch.equal(scratch[ckey].detach(), data[ckey].detach())
    scratch[ckey].backward(data[ckey].grad)
    g_c0, g_c1 = fc0.grad, fc1.grad
    if ot:
        extra["grad_bin_score"] = np.float64(model.coarse_matching.bin_score.grad)
    scratch = {k: data[k] for k in ("hw0_i", "hw0_f", "mkpts0_c", "mkpts1_c", "mconf", "b_ids")}
    model.fine_matching(ff0, ff1, scratch)
    assert torch.equal(scratch["expec_f"].detach(), data["expec_f"].detach())
    scratch["expec_f"].backward(data["expec_f"].grad)
    WW = ff0.shape[1]
    off_centre = ff0.grad.clone(); off_centre[:, WW // 2] = 0
    assert float(off_centre.abs().max()) == 0                     # feat_f0 is read at the centre only (fine_matching.py:43)
    gb, gi, gj = (data[k].numpy() for k in ("spv_b_ids", "spv_i_ids", "spv_j_ids"))
    print("conf at the ground truth:", np.sort(data["conf_matrix"].detach().numpy()[gb, gi, gj])[[0, len(gb) // 2, -1]])
    store = dict(recipe=np.array(json.dumps(dict(rc, **gc))), **extra, b_ids=data["b_ids"].numpy(), i_ids=data["i_ids"].numpy(), j_ids=data["j_ids"].numpy(),
                 expec_f=data["expec_f"].detach().numpy(), expec_f_gt=data["expec_f_gt"].numpy(), grad_expec=data["expec_f"].grad.numpy(), grad_feat_c0=g_c0.numpy(), grad_feat_c1=g_c1.numpy(),
                 grad_feat_f0_centre=ff0.grad[:, WW // 2].numpy(), grad_feat_f1_tail=ff1.grad[-GRAD_F1_FULL:].numpy(),
                 grad_feat_f1_norm=ff1.grad.flatten(1).norm(dim=1).numpy(),
                 losses=np.array(json.dumps({k: float(v) for k, v in data["loss_scalars"].items()})))
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **store)
    print(name, "windows", len(data["b_ids"]), {k: float(np.abs(v).max()) for k, v in store.items() if k.startswith("grad_")},
          json.loads(str(store["losses"])))


if __name__ == "__main__":
    for nm in sys.argv[1:] or list(CASES) + list(COARSE_TRAIN) + list(STEP_CASES) + list(GRAD_STEP_CASES):
        (make if nm in CASES else make_coarse_train if nm in COARSE_TRAIN else make_step if nm in STEP_CASES else make_step_grads)(nm)
