"""Writes tests/golden/pair_lists.npz: the image structure of the reference's two 1500-pair test lists (no images, no poses).

    python tests/golden/make_pair_lists.py [REFERENCE_ROOT]

Per list an int32 [1500, 2] of image indices renumbered in first-use order (row order, image0 before image1) and the number of
distinct images.  Images are identified as the reference's datasets identify them:
  * scannet: (scene, sub-scene, frame) of assets/scannet_test_1500/test.npz['name'] (src/datasets/scannet.py:69-75);
  * megadepth: image_paths[i] of the five scene-info files of assets/megadepth_test_1500_scene_info, in the order their list file
    gives (src/datasets/megadepth.py: pair_infos -> image_paths).
Only run where the reference is; the tests read the .npz alone (tests/test_pairs_plan.py, tools/micro/pairs_bench.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def renumber(keys0, keys1):
    ids, out = {}, np.zeros((len(keys0), 2), np.int32)
    for r, (a, b) in enumerate(zip(keys0, keys1)):
        out[r, 0] = ids.setdefault(a, len(ids))
        out[r, 1] = ids.setdefault(b, len(ids))
    return out, len(ids)


def scannet(root):
    names = np.load(os.path.join(root, "assets", "scannet_test_1500", "test.npz"))["name"]
    k = lambda s, sub, f: (int(s), int(sub), int(f))
    return renumber([k(n[0], n[1], n[2]) for n in names], [k(n[0], n[1], n[3]) for n in names])


def megadepth(root):
    d = os.path.join(root, "assets", "megadepth_test_1500_scene_info")
    scenes = [s.strip() for s in open(os.path.join(d, "megadepth_test_1500.txt")).read().split() if s.strip()]
    k0, k1 = [], []
    for s in scenes:
        info = np.load(os.path.join(d, s + ".npz"), allow_pickle=True)
        paths = info["image_paths"]
        for (i0, i1), *_ in info["pair_infos"]:
            k0.append(str(paths[i0])); k1.append(str(paths[i1]))
    return renumber(k0, k1)


def main(root):
    arrays = {}
    for name, fn in (("scannet", scannet), ("megadepth", megadepth)):
        pairs, n = fn(root)
        arrays[name + "_pairs"], arrays[name + "_images"] = pairs, np.int32(n)
        print(f"{name}: {len(pairs)} pairs over {n} distinct images ({2 * len(pairs) / n:.2f} uses per image)")
    np.savez_compressed(os.path.join(HERE, "pair_lists.npz"), **arrays)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
