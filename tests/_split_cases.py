"""Inputs shared by the track-splitting tests (tests/test_split.py and tests/test_split_abi.py on the CPU, tests/test_hip_split.py on the
GPU): hand cases with their expected result written out, seeded random graphs, the sizes the kernels' block and wave edges need, and a
noisy synthetic pair list whose atlas has inconsistent tracks."""
import functools

import numpy as np

import _triangulation_cases as TC

OUT = ("track_id_new", "track_len_new", "edge_state", "round_accepted", "counts")


def case(edges, kp_image, track_id, track_ok, n_images, min_track_len=2, max_rounds=32):
    """-> the arguments of ops.split_tracks_host; edges: [(u, v, conf)]."""
    e = np.array([(u, v) for u, v, _ in edges], np.int32).reshape(-1, 2)
    c = np.array([w for _, _, w in edges], np.float32)
    return (e, c, np.array(kp_image, np.int32), np.array(track_id, np.int32), np.array(track_ok, np.uint8), n_images, min_track_len, max_rounds)


def counts(n_tracks=0, errors=0, ignored=0, internal=0, conflict=0, open_=0, bad_tracks=0, bad_kp=0, rescued=0, rounds=0, largest=0):
    return [n_tracks, errors, ignored, internal, conflict, open_, bad_tracks, bad_kp, rescued, rounds, largest, 0, 0, 0, 0, 0]


def expect(track_id_new, track_len, edge_state, round_accepted, max_rounds, **c):
    acc = list(round_accepted) + [0] * (max_rounds - len(round_accepted))
    return dict(track_id_new=list(track_id_new), track_len_new=list(track_len) + [0] * (len(track_id_new) - len(track_len)),
                edge_state=list(edge_state), round_accepted=acc, counts=counts(**c))


# image A = 0, B = 1: a row (A, B) reaches A in keypoint 0, its reversed row comes back to A in the neighbouring keypoint 1
MINIMAL = [(0, 2, 0.9), (2, 1, 0.6)]
# keypoints 0, 1 in image 0, 2 in image 1, 3 in image 2; the chain 0 - 2 - 3 - 1 comes back to image 0
TIES = [(0, 2, 0.5), (2, 3, 0.5), (3, 1, 0.5)]
# 11 keypoints: 0 and 1 in image 0, k >= 2 in image k - 1; the chain 0 - 2 - 3 - ... - 10 with descending confidences, then 10 - 1
CHAIN_IMAGES = [0, 0] + list(range(1, 10))
CHAIN = [(0, 2, 0.95)] + [(k, k + 1, 0.95 - 0.05 * (k - 1)) for k in range(2, 10)] + [(10, 1, 0.3)]
# images 0: k0..3, 1: k4..8, 2: k9..13.  t0 = {0,4,9} ok, t1 = {1,2,5} not, t2 = {3,6} ok, t3 = {7,10,11} not, t4 = {8,12} ok, 13 loose
MIXED_IMAGES = [0] * 4 + [1] * 5 + [2] * 5
MIXED_TRACKS = [0, 1, 1, 2, 0, 1, 2, 3, 4, 0, 3, 3, 4, -1]
MIXED = [(0, 4, 0.9), (4, 9, 0.9), (1, 5, 0.8), (5, 2, 0.7), (3, 6, 0.6), (7, 10, 0.5), (7, 11, 0.5), (8, 12, 0.4), (6, 8, 0.3), (13, 12, 0.2)]


def hand():
    """-> [(name, arguments, expected outputs as lists)]"""
    out = []
    add = lambda name, args, **kw: out.append((name, args, expect(max_rounds=args[7], **kw)))
    # the stronger edge wins; the other keypoint of image A ends -1
    add("minimal", case(MINIMAL, [0, 0, 1], [0, 0, 0], [0], 2), track_id_new=[0, -1, 0], track_len=[2], edge_state=[1, 2], round_accepted=[1],
        n_tracks=1, internal=1, conflict=1, bad_tracks=1, bad_kp=3, rescued=2, rounds=1, largest=2)
    add("minimal_weaker_first", case(MINIMAL[::-1], [0, 0, 1], [0, 0, 0], [0], 2), track_id_new=[0, -1, 0], track_len=[2], edge_state=[2, 1],
        round_accepted=[1], n_tracks=1, internal=1, conflict=1, bad_tracks=1, bad_kp=3, rescued=2, rounds=1, largest=2)
    add("minimal_len3", case(MINIMAL, [0, 0, 1], [0, 0, 0], [0], 2, min_track_len=3), track_id_new=[-1, -1, -1], track_len=[], edge_state=[1, 2],
        round_accepted=[1], internal=1, conflict=1, bad_tracks=1, bad_kp=3, rounds=1, largest=2)
    add("minimal_len1", case(MINIMAL, [0, 0, 1], [0, 0, 0], [0], 2, min_track_len=1), track_id_new=[0, 1, 0], track_len=[2, 1], edge_state=[1, 2],
        round_accepted=[1], n_tracks=2, internal=1, conflict=1, bad_tracks=1, bad_kp=3, rescued=3, rounds=1, largest=2)
    add("minimal_no_rounds", case(MINIMAL, [0, 0, 1], [0, 0, 0], [0], 2, max_rounds=0), track_id_new=[-1, -1, -1], track_len=[], edge_state=[3, 3],
        round_accepted=[], open_=2, bad_tracks=1, bad_kp=3, largest=1)
    add("minimal_marked_consistent", case(MINIMAL, [0, 0, 1], [0, 0, 0], [1], 2), track_id_new=[0, 0, 0], track_len=[3], edge_state=[0, 0],
        round_accepted=[], n_tracks=1, ignored=2)
    # equal confidences: ties go to the lower edge
    add("ties", case(TIES, [0, 0, 1, 2], [0, 0, 0, 0], [0], 3), track_id_new=[0, -1, 0, 0], track_len=[3], edge_state=[1, 1, 2], round_accepted=[1, 1],
        n_tracks=1, internal=2, conflict=1, bad_tracks=1, bad_kp=4, rescued=3, rounds=2, largest=3)
    # a duplicated row: the second copy of the winning edge becomes internal one round later
    add("duplicate", case([MINIMAL[0], MINIMAL[0], MINIMAL[1]], [0, 0, 1], [0, 0, 0], [0], 2), track_id_new=[0, -1, 0], track_len=[2],
        edge_state=[1, 1, 2], round_accepted=[1], n_tracks=1, internal=2, conflict=1, bad_tracks=1, bad_kp=3, rescued=2, rounds=1, largest=2)
    # descending confidences merge one edge per round
    chain_ids = lambda n: [0, -1] + [0] * n + [-1] * (9 - n)
    add("chain", case(CHAIN, CHAIN_IMAGES, [0] * 11, [0], 10), track_id_new=chain_ids(9), track_len=[10], edge_state=[1] * 9 + [2],
        round_accepted=[1] * 9, n_tracks=1, internal=9, conflict=1, bad_tracks=1, bad_kp=11, rescued=10, rounds=9, largest=10)
    add("chain_3_rounds", case(CHAIN, CHAIN_IMAGES, [0] * 11, [0], 10, max_rounds=3), track_id_new=chain_ids(3), track_len=[4],
        edge_state=[1] * 3 + [3] * 7, round_accepted=[1] * 3, n_tracks=1, internal=3, open_=7, bad_tracks=1, bad_kp=11, rescued=4, rounds=3, largest=4)
    add("chain_1_round", case(CHAIN, CHAIN_IMAGES, [0] * 11, [0], 10, max_rounds=1), track_id_new=chain_ids(1), track_len=[2],
        edge_state=[1] + [3] * 9, round_accepted=[1], n_tracks=1, internal=1, open_=9, bad_tracks=1, bad_kp=11, rescued=2, rounds=1, largest=2)
    add("chain_no_rounds", case(CHAIN, CHAIN_IMAGES, [0] * 11, [0], 10, max_rounds=0), track_id_new=[-1] * 11, track_len=[], edge_state=[3] * 10,
        round_accepted=[], open_=10, bad_tracks=1, bad_kp=11, largest=1)
    # two inconsistent components next to three consistent tracks, a loose keypoint and edges that span two tracks
    add("mixed", case(MIXED, MIXED_IMAGES, MIXED_TRACKS, [1, 0, 1, 0, 1], 3), track_id_new=[0, 1, -1, 2, 0, 1, 2, 3, 4, 0, 3, -1, 4, -1],
        track_len=[3, 2, 2, 2, 2], edge_state=[0, 0, 1, 2, 0, 1, 2, 0, 0, 0], round_accepted=[2], n_tracks=5, ignored=6, internal=2, conflict=2,
        bad_tracks=2, bad_kp=6, rescued=4, rounds=1, largest=2)
    add("mixed_len3", case(MIXED, MIXED_IMAGES, MIXED_TRACKS, [1, 0, 1, 0, 1], 3, min_track_len=3), track_id_new=[0] + [-1] * 3 + [0] + [-1] * 4 + [0] + [-1] * 4,
        track_len=[3], edge_state=[0, 0, 1, 2, 0, 1, 2, 0, 0, 0], round_accepted=[2], n_tracks=1, ignored=6, internal=2, conflict=2, bad_tracks=2,
        bad_kp=6, rounds=1, largest=2)
    # nothing to do
    add("no_edges", case([], [0, 0, 1], [0, 0, 0], [0], 2), track_id_new=[-1] * 3, track_len=[], edge_state=[], round_accepted=[], bad_tracks=1, bad_kp=3,
        largest=1)
    add("no_tracks", case([(0, 1, 0.5)], [0, 1], [-1, -1], [], 2), track_id_new=[-1, -1], track_len=[], edge_state=[0], round_accepted=[], ignored=1)
    add("nothing", case([], [], [], [], 0), track_id_new=[], track_len=[], edge_state=[], round_accepted=[])
    add("self_edge", case([(0, 0, 0.5), (0, 1, 0.4)], [0, 1], [0, 0], [0], 2), track_id_new=[0, 0], track_len=[2], edge_state=[1, 1], round_accepted=[1],
        n_tracks=1, internal=2, bad_tracks=1, bad_kp=2, rescued=2, rounds=1, largest=2)
    return out


def errors():
    """-> [(name, arguments, the bits of counts[1])]: every bit the entry points can be given, alone and together.  Bit 16 (a member
    list longer than n_images) cannot be reached through an entry point: the lists are the routine's own."""
    good = dict(edges=MINIMAL, kp_image=[0, 0, 1], track_id=[0, 0, 0], track_ok=[0], n_images=2)
    mk = lambda **over: case(**{**good, **over})
    nan, inf = float("nan"), float("inf")
    return [("edge_high", mk(edges=[(0, 3, 0.9), (2, 1, 0.6)]), 1), ("edge_negative", mk(edges=[(0, 2, 0.9), (-1, 1, 0.6)]), 1),
            ("track_high", mk(track_id=[0, 1, 0]), 2), ("track_low", mk(track_id=[0, -2, 0]), 2), ("image_high", mk(kp_image=[0, 0, 2]), 2),
            ("image_negative", mk(kp_image=[-1, 0, 1]), 2), ("descends", mk(kp_image=[0, 1, 0]), 4), ("conf_nan", mk(edges=[(0, 2, nan), (2, 1, 0.6)]), 8),
            ("conf_inf", mk(edges=[(0, 2, 0.9), (2, 1, inf)]), 8), ("conf_negative", mk(edges=[(0, 2, -0.1), (2, 1, 0.6)]), 8),
            ("all", mk(edges=[(0, 7, nan), (2, 1, 0.6)], kp_image=[1, 0, 5], track_id=[0, 9, 0]), 15),
            ("edges_without_keypoints", case([(0, 0, 0.5)], [], [], [], 0), 1)]


@functools.lru_cache(maxsize=None)
def random_graph(seed, K=400, E=260, n_images=12, flip=0.15, loose=0.05):
    """A random match graph over K keypoints in n_images images: confidences from three values (ties everywhere), tracks = the connected
    components of at least 2 keypoints, track_ok = the truth with a share `flip` of the flags inverted, a share `loose` of the keypoints
    torn out of their track (their edges then span two tracks or leave every track), some duplicate edges and self edges."""
    rng = np.random.default_rng(seed)
    kp_image = np.sort(rng.integers(0, n_images, K)).astype(np.int32)
    u = rng.integers(0, K, E)
    v = np.clip(u + rng.integers(-40, 41, E), 0, K - 1) if seed % 2 else rng.integers(0, K, E)
    edges = np.stack([u, v], 1).astype(np.int32)
    edges[E // 2:E // 2 + 10] = edges[:10]                                                # duplicates
    conf = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), E)
    parent = list(range(K))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges.tolist():
        ra, rb = find(a), find(b)
        parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(k) for k in range(K)])
    ids = {}
    for r in sorted(set(root.tolist())):
        if (root == r).sum() >= 2:
            ids[r] = len(ids)
    track_id = np.array([ids.get(r, -1) for r in root.tolist()], np.int32)
    T = len(ids)
    track_ok = np.ones(T, np.uint8)
    for r, t in ids.items():
        ims = kp_image[root == r]
        track_ok[t] = len(set(ims.tolist())) == len(ims)
    track_ok ^= (rng.random(T) < flip).astype(np.uint8)
    torn = rng.random(K) < loose
    track_id[torn] = np.where(rng.random(int(torn.sum())) < 0.5, -1, rng.integers(0, max(T, 1), int(torn.sum()))).astype(np.int32)
    if T == 0:
        track_id[:] = -1
    return edges, conf, kp_image, track_id, track_ok, n_images


def random_args(seed, min_track_len=2, max_rounds=32, **kw):
    return (*random_graph(seed, **kw), min_track_len, max_rounds)


def one_component(members, extra_edges=0, seed=0):
    """One inconsistent track whose grown list reaches `members` keypoints: keypoint k in image k for k < members, plus one second
    keypoint in the last image that makes the track inconsistent.  A chain with random confidences above 0.5, `extra_edges` random
    weaker edges among the chain's keypoints, and the second keypoint hanging on keypoint 0 (on itself when members = 1) by the weakest
    edge: every chain edge is accepted before it, so the list reaches all `members` images and that edge conflicts.
    n_images = members."""
    rng = np.random.default_rng(seed)
    kp_image = list(range(members)) + [members - 1]
    edges = [(k, k + 1, 0.5 + 0.4 * rng.random()) for k in range(members - 1)]
    edges.append((0 if members > 1 else members, members, 0.05))
    for _ in range(extra_edges):
        edges.append((int(rng.integers(0, members)), int(rng.integers(0, members)), float(rng.choice([0.2, 0.3, 0.4]))))
    return case(edges, kp_image, [0] * (members + 1), [0], members)


def sized(E, K, seed=1):
    """A random graph of exactly E edges over K keypoints in 12 images, every track marked inconsistent."""
    rng = np.random.default_rng(seed + 7 * E + K)
    kp_image = np.sort(rng.integers(0, 12, K)).astype(np.int32)
    u = rng.integers(0, K, E)
    edges = np.stack([u, np.clip(u + rng.integers(-30, 31, E), 0, K - 1)], 1).astype(np.int32).reshape(-1, 2)
    conf = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), E)
    T = max(K // 50, 1)
    track_id = (np.arange(K) * T // K).astype(np.int32)                                  # contiguous blocks of keypoints: every edge inside or across
    return edges, conf, kp_image, track_id, np.zeros(T, np.uint8), 12, 2, 32


# ---- a noisy pair list whose atlas has inconsistent tracks ---------------------------------------------------------------------------
HW, CELL = (480.0, 640.0), 2.0


@functools.lru_cache(maxsize=None)
def noisy_scene(seed=11, n_cams=8, n_points=300, noise_px=0.5, keep=0.7, window=None):
    """Cameras and points as in _triangulation_cases.sfm_scene, but `n_cams` cameras on a 6-unit baseline (f = 500, 640 x 480 images),
    `n_points` points, every pair of images (or the pairs (i, i+1 .. i+window)) a row that observes a share `keep` of the co-visible
    points with independent Gaussian noise of `noise_px` on both sides, NOT snapped to the cells: a point reaches an image in
    neighbouring cells through different rows, so inconsistent components occur.
    -> dict(K, T, X, rows = [(a, b, k0 [M,2] f32, k1 [M,2] f32, conf [M] f32, point [M] i64)])."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-3.0, 3.0, n_cams)
    cams = [TC.camera(500.0, (x, rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)), TC.rotation(rng.standard_normal(3), rng.uniform(0, 5)))
            for x in xs]
    K, T = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    X = rng.uniform([-2.5, -1.5, 5], [2.5, 1.5, 8], (n_points, 3))
    px = np.stack([[TC.project(K[i], T[i], x) for x in X] for i in range(n_cams)])       # [n, P, 2]
    inside = (px[..., 0] > 2) & (px[..., 0] < HW[1] - 2) & (px[..., 1] > 2) & (px[..., 1] < HW[0] - 2)
    rows = []
    for a in range(n_cams):
        for b in range(a + 1, n_cams if window is None else min(n_cams, a + window + 1)):
            seen = np.nonzero(inside[a] & inside[b] & (rng.random(n_points) < keep))[0]
            k0 = (px[a, seen] + noise_px * rng.standard_normal((len(seen), 2))).astype(np.float32)
            k1 = (px[b, seen] + noise_px * rng.standard_normal((len(seen), 2))).astype(np.float32)
            rows.append((a, b, k0, k1, rng.uniform(0.5, 1.0, len(seen)).astype(np.float32), seen))
    return dict(K=K, T=T, X=X, rows=rows, n=n_cams)


def run_atlas(device, **kw):
    """KeypointAtlas over noisy_scene(**kw) on `device` -> SfmResult."""
    import torch
    from loftr_amd import KeypointAtlas
    s = noisy_scene(**kw)
    atlas = KeypointAtlas(s["n"], HW, CELL, device=device)
    dev = torch.device(device)
    for a, b, k0, k1, c, _ in s["rows"]:
        data = {"mkpts0_f": torch.from_numpy(k0).to(dev), "mkpts1_f": torch.from_numpy(k1).to(dev), "mconf": torch.from_numpy(c).to(dev),
                "m_bids": torch.zeros(len(c), dtype=torch.int64, device=dev)}
        atlas.add(np.array([[a, b]]), data)
    return atlas.finalize()
