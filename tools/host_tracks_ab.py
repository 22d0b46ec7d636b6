#!/usr/bin/env python
"""Are the host routines of the reconstruction chain the same functions in two builds of libloftr_hip.so, bit for bit?

    python tools/host_tracks_ab.py OLD.so NEW.so

The GPU tests of the atlas, the triangulation, the bundle adjustment, the registration and the model lookup compare the kernels with the
host routines, and kernels and host routines share their per-item steps (csrc/*_core.h, csrc/tracks_core.h), so a change that moves both
sides together is invisible to those tests.  This tool calls loftr_atlas_host, loftr_triangulate_tracks_host, loftr_bundle_adjust_host,
loftr_register_corr_host, loftr_model_cells_host and loftr_model_lookup_host of the two libraries with identical inputs and requires the
same status and byte-equal outputs.  The outputs are filled with a pattern before each call, so that what a call leaves unwritten
compares too.  Inputs: the cases of tests/_atlas_cases.py, _triangulation_cases.py, _bundle_cases.py, _registration_cases.py and
_model_lookup_cases.py at the sizes the GPU tests use, and for every track table one input per way of raising an error bit (first offset,
last offset, a descending pair, an image id of -1 and of n, a cam_obs entry out of range, in the wrong image, out of order).
Runs on the CPU; exit status 0 when every call is equal."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _atlas_cases as AC                                                              # noqa: E402
import _bundle_cases as BC                                                             # noqa: E402
import _model_lookup_cases as MC                                                       # noqa: E402
import _model_lookup_oracle as MO                                                      # noqa: E402
import _registration_cases as RC                                                       # noqa: E402
import _registration_oracle as RO                                                      # noqa: E402
import _triangulation_cases as TC                                                      # noqa: E402
from loftr_amd import _lib                                                             # noqa: E402
from loftr_amd.atlas import _grid                                                      # noqa: E402

NAMES = ("loftr_atlas_host", "loftr_triangulate_tracks_host", "loftr_bundle_adjust_host", "loftr_register_corr_host", "loftr_model_cells_host",
         "loftr_model_lookup_host")
ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def load(path):
    lib = C.CDLL(os.path.abspath(path))
    for name in NAMES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def outputs(*specs):
    """Output arrays (shape, dtype) pre-filled with a pattern."""
    return [np.frombuffer(b"\x5a" * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape).copy() for shape, dt in specs]


CALLS = [0]


def result(status, out):
    CALLS[0] += 1
    return bytes([status & 255]) + b"".join(a.tobytes() for a in out)


def atlas(lib, a):
    k0, k1, conf, rows, mask, row_images, n_images, gh, gw, inv, min_track_len = a
    M, R = len(conf), len(row_images)
    Kb = max(1, min(2 * M, n_images * gh * gw))
    out = outputs((n_images + 1, np.int64), ((Kb, 2), np.float32), (Kb, np.float32), (Kb, np.int32), (R + 1, np.int64), ((max(M, 1), 2), np.int32),
                  (max(M, 1), np.float32), (Kb, np.int32), (Kb, np.int32), (Kb, np.uint8), (16, np.int64))
    st = _lib.AtlasOut(*[ptr(x) for x in out])
    return result(lib.loftr_atlas_host(ptr(k0), ptr(k1), ptr(conf), ptr(rows), ptr(mask), M, ptr(row_images), R, n_images, gh, gw, inv,
                                       min_track_len, C.byref(st)), out)


def triangulate(lib, a):
    offsets, image, xy, K, T, thresh, cos_min = a
    nt, N = len(offsets) - 1, len(image)
    out = outputs(((nt, 3), np.float32), (nt, np.int32), (nt, np.float32), (nt, np.float32), (nt, np.uint8), (N, np.uint8), (8, np.int64))
    return result(lib.loftr_triangulate_tracks_host(ptr(offsets), nt, ptr(image), ptr(xy), N, ptr(K), ptr(T), len(K), thresh, cos_min,
                                                    *[ptr(x) for x in out]), out)


def bundle(lib, a):
    offsets, image, xy, mask, xyz, K, T, fixed, cam_offsets, cam_obs, huber, max_iters = a
    nt, N, n = len(offsets) - 1, len(image), len(K)
    out = outputs(((n, 4, 4), np.float64), ((nt, 3), np.float32), (N, np.uint8), (n, np.uint8), (nt, np.uint8), (16, np.int64))
    return result(lib.loftr_bundle_adjust_host(ptr(offsets), nt, ptr(image), ptr(xy), ptr(mask), N, ptr(xyz), ptr(K), ptr(T), ptr(fixed), n,
                                               ptr(cam_offsets), ptr(cam_obs), huber, max_iters, 30, 1e-2, 1e-9, *[ptr(x) for x in out]), out)


def register(lib, a):
    offsets, image, xy, xyz, status, posed, cam_offsets, cam_obs, min_corr = a
    nt, N, n = len(offsets) - 1, len(image), len(posed)
    out = outputs((n, np.int32), (n, np.int32), (n, np.int32), (n + 1, np.int64), ((N, 3), np.float32), ((N, 2), np.float32), (N, np.int64),
                  (N, np.int32), (8, np.int64))
    return result(lib.loftr_register_corr_host(ptr(offsets), nt, ptr(image), ptr(xy), N, ptr(xyz), ptr(status), ptr(posed), n, ptr(cam_offsets),
                                               ptr(cam_obs), min_corr, *[ptr(x) for x in out]), out)


def model(lib, a):
    """loftr_model_cells_host, then loftr_model_lookup_host on the cells it wrote."""
    kp_offsets, keypoints, kp_point, xyz, gh, gw, inv, kd, kq, conf, rows, mask, row_db, row_query, Q = a
    K, P, M, R = len(kp_point), len(xyz), len(conf), len(row_db)
    cell, status = outputs((K, np.int32), (1, np.int32))
    first = result(lib.loftr_model_cells_host(ptr(kp_offsets), len(kp_offsets) - 1, ptr(keypoints), ptr(kp_point), K, P, gh, gw, inv, ptr(cell),
                                              ptr(status)), [cell, status])
    out = outputs(((max(M, 1), 3), np.float32), ((max(M, 1), 2), np.float32), (max(M, 1), np.int64), (max(M, 1), np.int32), (max(M, 1), np.int32),
                  (max(M, 1), np.float32), (Q + 1, np.int64), (M, np.uint8), (16, np.int64))
    md = _lib.Model(ptr(kp_offsets), ptr(cell), ptr(kp_point), ptr(xyz), K, P, len(kp_offsets) - 1, gh, gw, inv)
    st = _lib.ModelLookupOut(*[ptr(x) for x in out])
    return first + result(lib.loftr_model_lookup_host(C.byref(md), ptr(kd), ptr(kq), ptr(conf), ptr(rows), ptr(mask), M, ptr(row_db),
                                                      ptr(row_query), R, Q, C.byref(st)), out)


RUN = {"atlas": atlas, "triangulate": triangulate, "bundle": bundle, "register": register, "model": model}


def corruptions(t, groups):
    """(name, table) per way of raising an error bit; t: dict with offsets, obs_image and, when `groups`, cam_offsets / cam_obs."""
    n, N = (len(t["cam_offsets"]) - 1) if groups else int(t["obs_image"].max()) + 1, len(t["obs_image"])
    edits = [("first offset", "offsets", 0, 1), ("last offset", "offsets", -1, N + 1), ("descending pair", "offsets", 2, int(t["offsets"][3]) + 1),
             ("image -1", "obs_image", N // 2, -1), ("image n", "obs_image", N // 2, n)]
    if groups:
        obs, off = t["cam_obs"], t["cam_offsets"]
        i = next(i for i in range(n - 1) if off[i + 1] - off[i] >= 2 and off[i + 2] > off[i + 1])      # an image with two slots and a successor
        edits += [("cam_obs out of range", "cam_obs", int(off[i]), N), ("cam_obs in the wrong image", "cam_obs", int(off[i]), int(obs[off[i + 1]])),
                  ("cam_obs out of order", "cam_obs", int(off[i]), int(obs[off[i] + 1]))]
    for name, key, idx, val in edits:
        c = dict(t)
        c[key] = t[key].copy()
        c[key][idx] = val
        yield name, c


def cases():
    """(kind, label, arguments) of every call."""
    f32, f64 = (lambda a: np.ascontiguousarray(a, np.float32)), (lambda a: np.ascontiguousarray(a, np.float64))
    # ---- atlas: every case as one add of all its rows, at the cell sizes and track lengths of the tests
    for name, (n_images, hw, rows), cells in (("random", AC.random_case(), (2.0, 0.5, 16.0)), ("invalid", AC.invalid_case()[:3], (2.0,)),
                                              ("tracks", AC.track_case()[:3], (2.0,)), ("stress", AC.stress_case(), (2.0,))):
        ids, k0, k1, conf, bids, mask = AC.chunks(rows, len(rows))[0]
        for cell_px in cells:
            inv, gh, gw = _grid(hw, cell_px)
            for min_track_len in (2, 3):
                yield "atlas", (name, cell_px, min_track_len), (f32(k0), f32(k1), f32(conf), bids.astype(np.int32),
                                                                None if mask is None else mask.astype(np.uint8), ids.astype(np.int32), n_images,
                                                                int(gh), int(gw), float(inv), min_track_len)
    # ---- triangulation
    def tri(s):
        return (s["offsets"], s["obs_image"], s["obs_xy"], f64(s["K"]), f64(s["T"]), TC.THRESH_PX, TC.COS_MIN)
    scene = TC.scene()
    yield "triangulate", ("scene",), tri(scene)
    yield "triangulate", ("hand",), tri(TC.hand_cases()[0])
    for n_tracks in (1, 3, 37, 101):
        yield "triangulate", ("scene", n_tracks), tri(TC.scene(seed=4, n_tracks=n_tracks))
    for name, c in corruptions(scene, False):
        yield "triangulate", ("scene", name), tri(c)
    # ---- bundle adjustment
    def ba(s, huber=0.0, max_iters=30, **edit):
        s = dict(s, **edit)
        n = len(s["K"])
        cam_offsets, cam_obs = edit.get("cam_offsets"), edit.get("cam_obs")
        if cam_offsets is None:
            cam_offsets, cam_obs = RO.groups(s["obs_image"], n)
        return (s["offsets"], s["obs_image"], s["obs_xy"], s["obs_mask"].astype(np.uint8), s["xyz"], f64(s["K"]), f64(s["T_cam_from_world"]),
                s["fixed"].astype(np.uint8), cam_offsets, cam_obs, huber, max_iters)
    yield "bundle", ("scene_a",), ba(BC.scene_a())
    yield "bundle", ("scene_b",), ba(BC.scene_b())
    yield "bundle", ("scene_huber",), ba(BC.scene_huber(), 2.0, 40)
    yield "bundle", ("hand",), ba(BC.hand_problem()[0])
    yield "bundle", ("exact",), ba(BC.exact_problem())
    for slots in (63, 64, 65, 129):
        yield "bundle", ("all_see_all", slots), ba(BC.all_see_all(3, slots), max_iters=8)
    for n_free in (1, 63, 64, 65):
        yield "bundle", ("spread", n_free), ba(BC.spread(n_free, max(40, 2 * n_free)), max_iters=8)
    for n_tracks in (1, 3, 37, 257, 4096, 4097):
        yield "bundle", ("spread 2", n_tracks), ba(BC.spread(2, n_tracks), max_iters=6)
    a = BC.scene_a()
    grouped = dict(a, **dict(zip(("cam_offsets", "cam_obs"), RO.groups(a["obs_image"], len(a["K"])))))
    for name, c in corruptions(grouped, True):
        yield "bundle", ("scene_a", name), ba(a, max_iters=4, **{k: c[k] for k in ("offsets", "obs_image", "cam_offsets", "cam_obs")})
    # ---- registration
    reg = lambda c: tuple(RC.args(c))
    for name, c in sorted(RC.edge_cases().items()) + sorted(RC.scene_cases().items()):
        yield "register", (name,), reg(c)
    for name, c, _ in RC.bad_inputs():
        yield "register", (name,), reg(c)
    for k in (0, 1, 63, 64, 65, 129, 4097):
        yield "register", ("list", k), reg(RC.list_case(k))
    for n in (1, 63, 64, 65, 255, 256, 257, 4097):
        yield "register", ("images", n), reg(RC.images_case(n))
    for T in (1, 3, 257, 4097):
        yield "register", ("random", T), reg(RC.random_case(50 + T, 7, T, 9))
    yield "register", ("700 images",), reg(RC.random_case(61, 700, 3000, 12, min_corr=30))
    yield "register", ("long track",), reg(RC.long_track())
    s = RC.scene_cases()["scene_a_min4"]
    for name, c in corruptions(s, True):
        yield "register", ("scene_a", name), reg(c)
    # ---- model cells and lookup
    def lookup(case):
        m, q = case["model"], case["q"]
        inv, gh, gw = MO.grid(m["image_hw"], m["cell_px"])
        return (m["kp_offsets"], m["keypoints"], m["kp_point"], m["xyz"], int(gh), int(gw), float(inv), q["kpts_db"], q["kpts_q"], q["conf"], q["rows"],
                q["mask"], q["row_db"], q["row_query"], q["Q"])
    rnd = MC.random_case()
    named = [("random", rnd), ("hand", MC.hand_case()[0]), ("edge", MC.edge_case()[0]), ("same key", MC.same_key_case(4096)),
             ("query bits", MC.key_bits_case("query")), ("point bits", MC.key_bits_case("point")), ("tiled", MC.tiled(rnd, 256 * 1024 + 1))]
    named += [(f"prefix {M}", MC.prefix(rnd, M)) for M in (0, 1, 63, 64, 65, 257, 1025)]
    named += [(f"Q = {Q}", MC.empty_queries_case(Q)) for Q in (1, 3, 1025)]
    for name, case in named:
        yield "model", (name,), lookup(case)


def main(old_path, new_path):
    old, new = load(old_path), load(new_path)
    if old._handle == new._handle:
        sys.exit("the two paths name one library")
    total, bad = {}, []
    for kind, label, args in cases():
        total[kind] = total.get(kind, 0) + 1
        if RUN[kind](old, args) != RUN[kind](new, args):
            bad.append((kind, label))
    n = sum(total.values())
    for kind, label in bad[:20]:
        print("DIFFERENT", kind, label)
    print(f"{'FAIL' if bad else 'PASS'}: {n - len(bad)} of {n} cases byte-equal, {CALLS[0] // 2} host calls per library ("
          + ", ".join(f"{k} {v}" for k, v in sorted(total.items())) + ")")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
