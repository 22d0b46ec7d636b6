"""Ground-truth figures of the track triangulation on the seeded test scene (host routine; no GPU needed): the share of tracks whose
final inlier mask equals the true inlier set and the worst RMS ratio against the oracle's Gauss-Newton optimum -- what
tests/test_triangulation.py::test_result_against_ground_truth asserts.

    python tools/micro/triangulation_accuracy.py > profiles/triangulation_accuracy.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _triangulation_cases as TC                                   # noqa: E402
from loftr_amd import triangulate_tracks                            # noqa: E402

if __name__ == "__main__":
    s = TC.scene()
    got = triangulate_tracks(s["offsets"], s["obs_image"], s["obs_xy"], s["K"], s["T"], TC.THRESH_PX, TC.MIN_ANGLE_DEG).to_host()
    print(TC.accuracy_report(TC.ground_truth_figures(s, got)))
    print("statuses:", {k: v for k, v in got["stats"].items()})
