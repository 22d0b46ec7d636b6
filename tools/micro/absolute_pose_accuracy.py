#!/usr/bin/env python
"""Accuracy of the host absolute-pose estimator (loftr_estimate_absolute_pose) on the noisy scenes of tests/test_absolute_pose.py,
against the oracle's Levenberg-Marquardt fit on the true inliers (tests/_absolute_pose_oracle.py).  Metric: the RMS distance, over the
true inliers, between a pose's projections and the noise-free true projections (px).  One line per configuration: the range of
estimator / oracle over --scenes scenes, and the rotation / camera-centre errors of the worst scene.  CPU only.

    python tools/micro/absolute_pose_accuracy.py [--scenes 25] [--thresh 3.0] > profiles/absolute_pose_accuracy.txt"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from loftr_amd import evaluation as EV                                  # noqa: E402
import _absolute_pose_oracle as O                                       # noqa: E402


def rms_to_clean(sc, R, t):
    inl = ~sc["is_outlier"]
    return float(np.sqrt(np.mean(np.sum((O.project(sc["K"], R, t, sc["X"][inl])[0] - sc["clean"][inl]) ** 2, axis=1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=25)
    ap.add_argument("--thresh", type=float, default=3.0)
    a = ap.parse_args()
    print(f"# n outliers scene thresh_px conf | ratio min median max | worst scene: estimator px, oracle px, R err deg, centre err   "
          f"(0.5 px noise, {a.scenes} scenes each, estimator seed = scene index)")
    total = []
    for n in (300, 2000):
        for o in (0.0, 0.4):
            for planar in (False, True):
                rng = np.random.default_rng(100 + n + int(10 * o) + planar)
                rows = []
                for s in range(a.scenes):
                    sc = O.make_scene(rng, n, 0.5, o, planar, a.thresh)
                    R, t, mask = EV.estimate_absolute_pose_native(sc["X"], sc["kpts"], sc["K"], a.thresh, 0.999, s)
                    inl = ~sc["is_outlier"]
                    Ro, to = O.fit_pose(sc["K"], sc["X"][inl], sc["kpts"][inl], sc["R"], sc["t"])
                    e, r = rms_to_clean(sc, R, t), rms_to_clean(sc, Ro, to)
                    rows.append((e / r, e, r, O.rotation_error_deg(R, sc["R"]), float(np.linalg.norm(R.T @ t - sc["R"].T @ sc["t"]))))
                rows.sort()
                ratios = [x[0] for x in rows]
                total += ratios
                w = rows[-1]
                print(f"{n:5d} {o:.1f} {'planar ' if planar else 'general'} {a.thresh:.1f} 0.999 | {ratios[0]:.4f} {np.median(ratios):.4f} {ratios[-1]:.4f} | "
                      f"{w[1]:.4f} {w[2]:.4f} {w[3]:.5f} {w[4]:.5f}")
    print(f"# all {len(total)} scenes: ratio {min(total):.4f} .. {max(total):.4f}")


if __name__ == "__main__":
    main()
