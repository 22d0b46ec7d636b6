"""Inputs of the undistortion tests (tests/test_undistort.py on the CPU, tests/test_hip_undistort.py on the GPU)."""
import numpy as np

KS = (-0.3, -0.12, 0.0, 0.08, 0.5)


def cameras():
    """One camera per coefficient of KS (with a skew), then one with fx = 0."""
    K = np.zeros((len(KS) + 1, 3, 3))
    for i in range(len(K)):
        K[i] = [[500.0 + 20 * i, 0.5 * i, 320.0 + i], [0.0, 510.0 - 10 * i, 240.0 - i], [0.0, 0.0, 1.0]]
    K[-1, 0, 0] = 0.0
    return K, np.array(KS + (0.05,))


def monotone_radius(k, margin=0.9):
    """The largest undistorted radius used with k: inside the monotone range 1 + 3 k r^2 > 0 for a barrel k (with a margin), 1.6 else."""
    return min(1.6, margin / np.sqrt(-3.0 * k)) if k < 0 else 1.6


def batch(M, seed=3):
    """M distorted pixels over the cameras above: most inside the monotone range of their camera; every seventh beyond the fold of a
    barrel coefficient, every eleventh NaN or infinite, every thirteenth in the camera with fx = 0.  -> xy [M,2] f32, image [M] i32,
    K [n,3,3] f64, radial [n] f64."""
    rng = np.random.default_rng(seed + M)
    K, k = cameras()
    image = rng.integers(0, len(KS), M).astype(np.int32)
    xy = np.zeros((M, 2), np.float32)
    for p in range(M):
        i = image[p]
        r = rng.uniform(0, monotone_radius(k[i]))
        if p % 7 == 3:                                                   # far beyond the fold of k = -0.3: r_d > max r (1 + k r^2) = 0.70
            i = image[p] = 0
            r = rng.uniform(1.5, 3.0)
        ang = rng.uniform(0, 2 * np.pi)
        x = r * np.array([np.cos(ang), np.sin(ang)])
        xd = x * (1 + k[i] * r * r) if p % 7 != 3 else x                 # (beyond the fold the pixel itself is placed at radius r)
        xy[p] = K[i][:2, :2] @ xd + K[i][:2, 2]
        if p % 11 == 5:
            xy[p, p % 2] = (np.nan, np.inf, -np.inf)[p % 3]
        if p % 13 == 6:
            image[p] = len(KS)
    return xy, image, K, k
