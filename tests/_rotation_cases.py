"""Seeded synthetic view graphs for the rotation-averaging tests (tests/test_rotation.py, tests/test_hip_rotation.py): images with random
rotations, pairs (i, j) with j - i <= win plus random chords, per-axis Gaussian noise on every relative rotation, and planted edges
whose rotation is replaced by a random one.  Every scene carries its own distinct edge weights; a test about duplicates or ties sets
others."""
import math

import numpy as np


def rot_from_quat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def random_rotation(rng):
    q = rng.normal(size=4)
    return rot_from_quat(q / np.linalg.norm(q))


def small_rotation(rng, sigma_deg):
    """exp of a vector with independent N(0, sigma) components (degrees per axis)."""
    v = rng.normal(size=3) * math.radians(sigma_deg)
    a = float(np.linalg.norm(v))
    if a == 0.0:
        return np.eye(3)
    ax = v / a
    return rot_from_quat(np.concatenate([[math.cos(a / 2)], ax * math.sin(a / 2)]))


def angle_deg(R):
    """Rotation angle of R [..., 3, 3], degrees, from the chord |R - I|_F."""
    chord = np.linalg.norm((R - np.eye(3)).reshape(*R.shape[:-2], 9), axis=-1)
    return np.degrees(2.0 * np.arcsin(np.clip(chord / (2.0 * math.sqrt(2.0)), 0.0, 1.0)))


class Scene:
    """edge_image [E,2] i32, edge_R [E,3,3] f64 (x_b = R x_a), edge_weight [E] i32 (distinct), n, R_gt [n,3,3], planted [E] bool."""

    def __init__(self, name, edge_image, edge_R, edge_weight, n, R_gt, planted):
        self.name, self.edge_image, self.edge_R, self.edge_weight, self.n, self.R_gt, self.planted = \
            name, edge_image, edge_R, edge_weight, n, R_gt, planted

    @property
    def args(self):
        return self.edge_image, self.edge_R, self.edge_weight, self.n


def make_scene(name, n, win, seed, chords=0, noise_deg=0.5, planted=0.0):
    """n images, the pairs (i, j) with 0 < j - i <= win and `chords` random further pairs; `planted`: the share of edges (a count when
    >= 1) replaced by random rotations; weights: a permutation of 100 .. 100 + E - 1, so planted edges weigh as the good ones do."""
    rng = np.random.default_rng(seed)
    R_gt = np.stack([random_rotation(rng) for _ in range(n)]) if n else np.zeros((0, 3, 3))
    pairs = [(i, j) for i in range(n) for j in range(i + 1, min(n, i + win + 1))]
    have = set(pairs)
    while chords > 0 and n > win + 2:
        i, j = sorted(rng.choice(n, size=2, replace=False).tolist())
        if (i, j) not in have:
            have.add((i, j))
            pairs.append((i, j))
            chords -= 1
    E = len(pairs)
    edge_image = np.array(pairs, np.int32).reshape(-1, 2)
    edge_R = np.zeros((E, 3, 3))
    for e, (a, b) in enumerate(pairs):
        edge_R[e] = small_rotation(rng, noise_deg) @ R_gt[b] @ R_gt[a].T if noise_deg > 0 else R_gt[b] @ R_gt[a].T
    k = int(planted) if planted >= 1 else int(round(planted * E))
    mask = np.zeros(E, bool)
    if k:
        mask[rng.choice(E, size=k, replace=False)] = True
        for e in np.nonzero(mask)[0]:
            edge_R[e] = random_rotation(rng)
    weight = (rng.permutation(E) + 100).astype(np.int32)
    return Scene(name, edge_image, edge_R, weight, n, R_gt, mask)


# ---- the named scenes --------------------------------------------------------------------------------------------------------------
# planted outliers: between 5 and 64 images; chosen with the oracle alone (tests/test_rotation.py checks the margins again): every good
# edge ends below half of max_err_deg = 10 and every planted edge above twice it
OUTLIER_SCENES = (
    dict(name="outliers_5", n=5, win=4, seed=11, planted=2),
    dict(name="outliers_12", n=12, win=3, seed=12, chords=4, planted=0.12),
    dict(name="outliers_24", n=24, win=3, seed=13, chords=8, planted=0.15),
    dict(name="outliers_40", n=40, win=4, seed=14, chords=10, planted=0.2),
    dict(name="outliers_64", n=64, win=3, seed=15, chords=20, planted=0.1),
)
# averaging against chaining: noisy, nothing planted; the oracle shows at least a factor 2 between the tree's error and the average's
CHAIN_SCENES = (
    dict(name="chain_12", n=12, win=3, seed=30, noise_deg=1.0),
    dict(name="chain_30", n=30, win=4, seed=25, noise_deg=1.0),
    dict(name="chain_64", n=64, win=4, seed=23, chords=10, noise_deg=1.0),
)


def outlier_scenes():
    return [make_scene(**kw) for kw in OUTLIER_SCENES]


def chain_scenes():
    return [make_scene(**kw) for kw in CHAIN_SCENES]


def hub_scene(spokes=70, seed=31):
    """Image 0 joined to `spokes` images that are also chained: a neighbour list longer than a 64-lane step."""
    rng = np.random.default_rng(seed)
    n = spokes + 1
    R_gt = np.stack([random_rotation(rng) for _ in range(n)])
    pairs = [(0, j) for j in range(1, n)] + [(j, j + 1) for j in range(1, n - 1)]
    edge_R = np.stack([small_rotation(rng, 0.5) @ R_gt[b] @ R_gt[a].T for a, b in pairs])
    planted = np.zeros(len(pairs), bool)
    planted[[5, 40, 100]] = True
    for e in np.nonzero(planted)[0]:
        edge_R[e] = random_rotation(rng)
    weight = (rng.permutation(len(pairs)) + 100).astype(np.int32)
    return Scene("hub_70", np.array(pairs, np.int32), edge_R, weight, n, R_gt, planted)


def two_components(seed=41):
    """Images 0 .. 9 and 10 .. 15 with no edge between them; the first holds the heavier edges, so the root lies there."""
    a, b = make_scene("a", 10, 3, seed), make_scene("b", 6, 2, seed + 1)
    edge_image = np.concatenate([a.edge_image, b.edge_image + 10]).astype(np.int32)
    weight = np.concatenate([a.edge_weight + 1000, b.edge_weight]).astype(np.int32)
    return Scene("two_components", edge_image, np.concatenate([a.edge_R, b.edge_R]), weight, 16, np.concatenate([a.R_gt, b.R_gt]),
                 np.concatenate([a.planted, b.planted]))


def with_duplicates(scene, seed=51):
    """Every fourth edge once more, stored the other way round with fresh noise and a weight above or below the first one's in turn."""
    rng = np.random.default_rng(seed)
    idx = np.arange(0, scene.edge_image.shape[0], 4)
    im = scene.edge_image[idx][:, ::-1]
    R = np.stack([(small_rotation(rng, 0.3) @ scene.R_gt[b] @ scene.R_gt[a].T).T for a, b in scene.edge_image[idx]])
    w = scene.edge_weight[idx] + np.where(np.arange(idx.size) % 2 == 0, 1000, -50).astype(np.int32)
    return Scene(scene.name + "_dup", np.concatenate([scene.edge_image, im]).astype(np.int32), np.concatenate([scene.edge_R, R]),
                 np.concatenate([scene.edge_weight, w]).astype(np.int32), scene.n, scene.R_gt,
                 np.concatenate([scene.planted, np.zeros(idx.size, bool)])), idx


# ---- the arguments of the ops layer ------------------------------------------------------------------------------------------------
def ops_args(scene, root=-1, cycle_deg=5.0, loss_deg=5.0, max_err_deg=10.0, max_iters=20, pcg_iters=30, pcg_tol=1e-4, step_tol_deg=1e-3):
    """The numpy arguments of ops.rotation_averaging_host for a scene: the adjacency and edge_use by rotations.view_graph, the angles
    converted as average_rotations converts them."""
    import torch
    from loftr_amd import rotations
    im = np.ascontiguousarray(scene.edge_image, np.int32).reshape(-1, 2)
    R, w = np.ascontiguousarray(scene.edge_R, np.float64).reshape(-1, 3, 3), np.ascontiguousarray(scene.edge_weight, np.int32)
    adj_offsets, adj_edge, use = (t.numpy() for t in rotations.view_graph(torch.from_numpy(im), torch.from_numpy(R), torch.from_numpy(w), scene.n))
    return [im, R, w, adj_offsets, adj_edge, use, scene.n, root, math.cos(math.radians(cycle_deg) / 2), 2 * math.sin(math.radians(loss_deg) / 2),
            2 * math.sin(math.radians(max_err_deg) / 2), math.radians(step_tol_deg), max_iters, pcg_iters, pcg_tol]


def error_cases():
    """-> [(name, ops arguments, the bit of counts[1] that must be set)]: every bit the entry points can be given."""
    base = with_duplicates(make_scene("err", 9, 3, 61))[0]
    out = []
    a = ops_args(base)
    a[0] = a[0].copy(); a[0][4, 1] = base.n
    out.append(("image_outside", a, 1))
    a = ops_args(base)
    a[0] = a[0].copy(); a[0][3, 0] = -1
    out.append(("image_negative", a, 1))
    a = ops_args(base)
    a[0] = a[0].copy(); a[0][2, 1] = a[0][2, 0]
    out.append(("self_edge", a, 2))
    a = ops_args(base)
    a[4] = a[4].copy(); a[4][[0, 1]] = a[4][[1, 0]]
    out.append(("neighbours_descend", a, 4))
    a = ops_args(base)
    a[4] = a[4].copy(); a[4][5] = a[0].shape[0]
    out.append(("slot_outside", a, 4))
    a = ops_args(base)
    a[3] = a[3].copy(); a[3][3] += 1
    out.append(("offsets_shifted", a, 4))
    a = ops_args(base)
    a[3] = a[3].copy(); a[3][-1] -= 1
    out.append(("offsets_end", a, 4))
    a = ops_args(base)
    a[5] = np.ones_like(a[5])
    out.append(("two_used_edges", a, 4))
    a = ops_args(base, root=base.n)
    out.append(("root_outside", a, 8))
    a = ops_args(base, root=-2)
    out.append(("root_below", a, 8))
    return out


# ---- a pair list with one wrongly matched row -----------------------------------------------------------------------------------------
FALSE_ROW, FALSE_POINTS = 4, 40


def false_row_atlas(device, bad_row=FALSE_ROW, deg=25.0):
    """The atlas of _triangulation_cases.sfm_scene() (5 images, every pair a row, 60 points) with row `bad_row` replaced by matches of the
    first FALSE_POINTS points regenerated from a false pose of its second image, the true one turned by `deg` about the optical axis: the
    matches are coherent with a wrong geometry, so the five-point model of the row has many inliers; the tracks of the other points
    never meet the row.  -> (SfmResult on `device`, the scene)."""
    import torch
    import _triangulation_cases as TC
    from loftr_amd import KeypointAtlas
    s = TC.sfm_scene()
    atlas = KeypointAtlas(5, TC.SFM_HW, TC.SFM_CELL, device=device)
    dev = torch.device(device)
    for r, (a, b, k0, k1, c) in enumerate(s["rows"]):
        if r == bad_row:
            T = s["T"][b].copy()
            T[:3] = TC.rotation((0.0, 0.0, 1.0), deg) @ T[:3]
            p = np.stack([TC.project(s["K"][b], T, x) for x in s["X"]])
            assert (p > 0).all() and (p[:, 0] < TC.SFM_HW[1]).all() and (p[:, 1] < TC.SFM_HW[0]).all()
            k1 = (np.floor(p / TC.SFM_CELL) * TC.SFM_CELL + TC.SFM_CELL / 2).astype(np.float32)
            k0, k1, c = k0[:FALSE_POINTS], k1[:FALSE_POINTS], c[:FALSE_POINTS]
        data = {"mkpts0_f": torch.from_numpy(k0).to(dev), "mkpts1_f": torch.from_numpy(k1).to(dev), "mconf": torch.from_numpy(c).to(dev),
                "m_bids": torch.zeros(len(c), dtype=torch.int64, device=dev)}
        atlas.add(np.array([[a, b]]), data)
    return atlas.finalize(), s
