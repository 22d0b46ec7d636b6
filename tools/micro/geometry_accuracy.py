#!/usr/bin/env python
"""Accuracy of the host homography / fundamental-matrix estimator on the noisy scenes of tests/test_geometry.py, against the oracle's
normalised least-squares fit on the true inliers (tests/_geometry_oracle.py).  One line per scene: estimator's error, oracle's error,
ratio.  Homography: mean corner error on the 640 x 480 frame (px); fundamental: RMS Sampson distance of the true inliers (px).

    python tools/micro/geometry_accuracy.py > profiles/geometry_accuracy.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_geometry as T                                               # noqa: E402


def main():
    print("# model n outliers thresh_px conf | estimator oracle ratio   (0.5 px noise on both images, seed 0, scene seed 100 + n + 10 * outliers)")
    for model in T.MODELS:
        for n in (300, 2000):
            for o in (0.0, 0.4):
                err, ref = T.accuracy_ratio(model, n, o, seed=100 + n + int(10 * o))
                print(f"{model:12s} {n:5d} {o:.1f} {T.THR[model]:.1f} 0.999 | {err:.4f} {ref:.4f} {err / ref:.3f}")


if __name__ == "__main__":
    main()
