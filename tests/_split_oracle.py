"""Track splitting in Python dicts and sets: an independent statement of the rule that shares no code with
csrc/split_core.h.  A component is a set of keypoints, disjointness is a set intersection of image sets, the best word of a component
is a max over tuples.  ``rng``: a numpy Generator; every phase of every round then visits its edges in a fresh random order, which
must not change anything."""
import numpy as np

IGNORED, INTERNAL, CONFLICT, OPEN = 0, 1, 2, 3
NAMES = ("n_tracks", "error_bits", "n_ignored", "n_internal", "n_conflict", "n_open", "n_inconsistent_tracks", "n_inconsistent_keypoints",
         "n_rescued", "n_rounds", "largest_component")


def error_bits(edge_kp, edge_conf, kp_image, track_id, T, n_images):
    K = len(kp_image)
    bits = 0
    if any(not 0 <= int(k) < K for k in np.asarray(edge_kp).reshape(-1)):
        bits |= 1
    if any(not -1 <= int(t) < T for t in track_id) or any(not 0 <= int(i) < n_images for i in kp_image):
        bits |= 2
    if any(int(kp_image[k - 1]) > int(kp_image[k]) for k in range(1, K)):
        bits |= 4
    if any(not (np.isfinite(c) and c >= 0) for c in np.asarray(edge_conf, np.float32)):
        bits |= 8
    return bits


def split(edge_kp, edge_conf, kp_image, track_id, track_ok, n_images, min_track_len=2, max_rounds=32, rng=None):
    edge_kp = np.asarray(edge_kp, np.int64).reshape(-1, 2)
    conf = np.asarray(edge_conf, np.float32)
    E, K, T = len(edge_kp), len(kp_image), len(track_ok)
    out = {"track_id_new": np.zeros(K, np.int32), "track_len_new": np.zeros(K, np.int32), "edge_state": np.zeros(E, np.uint8),
           "round_accepted": np.zeros(max_rounds, np.int32), "counts": np.zeros(16, np.int64)}
    bits = error_bits(edge_kp, conf, kp_image, track_id, T, n_images)
    if bits:
        out["counts"][1] = bits
        return out
    visit = (lambda: range(E)) if rng is None else (lambda: [int(e) for e in rng.permutation(E)])
    free = [int(track_id[k]) >= 0 and not track_ok[int(track_id[k])] for k in range(K)]
    members = {}                                                          # label -> set of keypoints
    label = {}                                                            # keypoint -> label
    frozen = {}                                                           # track -> its keypoints
    for k in range(K):
        if int(track_id[k]) >= 0 and not free[k]:
            frozen.setdefault(int(track_id[k]), set()).add(k)
    for ks in frozen.values():
        members[min(ks)] = ks
        label.update({k: min(ks) for k in ks})
    for k in range(K):
        if free[k]:
            members[k], label[k] = {k}, k
    state = {}
    for e, (u, v) in enumerate(edge_kp.tolist()):
        state[e] = OPEN if int(track_id[u]) == int(track_id[v]) and free[u] else IGNORED
    word = lambda e: (float(conf[e]) + 0.0, -e)                           # (-0.0 + 0.0 is +0.0)
    images = lambda l: {int(kp_image[k]) for k in members[l]}
    for r in range(max_rounds):
        best, candidates = {}, set()
        for e in visit():                                                 # propose
            if state[e] != OPEN:
                continue
            a, b = (label[k] for k in edge_kp[e].tolist())
            if a == b:
                state[e] = INTERNAL
            elif images(a) & images(b):
                state[e] = CONFLICT
            else:
                candidates.add(e)
                for l in (a, b):
                    best[l] = max(best.get(l, word(e)), word(e))
        accepted = []
        for e in visit():                                                 # accept
            if e in candidates and all(best[label[k]] == word(e) for k in edge_kp[e].tolist()):
                accepted.append(e)
        for e in accepted:                                                # merge
            a, b = sorted(label[k] for k in edge_kp[e].tolist())
            members[a] |= members.pop(b)
            label.update({k: a for k in members[a]})
            state[e] = INTERNAL
        out["round_accepted"][r] = len(accepted)
        if not accepted:
            break
    number = {}
    for l in sorted(members):
        if len(members[l]) >= min_track_len:
            number[l] = len(number)
            out["track_len_new"][number[l]] = len(members[l])
    for k in range(K):
        out["track_id_new"][k] = number.get(label.get(k, -1), -1)
    for e in range(E):
        out["edge_state"][e] = state[e]
    c = out["counts"]
    c[0] = len(number)
    for s in (IGNORED, INTERNAL, CONFLICT, OPEN):
        c[2 + s] = sum(1 for e in range(E) if state[e] == s)
    c[6] = sum(1 for t in range(T) if not track_ok[t])
    c[7] = sum(free)
    c[8] = sum(1 for k in range(K) if free[k] and out["track_id_new"][k] >= 0)
    c[9] = int((out["round_accepted"] > 0).sum())
    c[10] = max([len(members[l]) for l in members if free[l]], default=0)
    return out
