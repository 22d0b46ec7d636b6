"""Writes profiles/position_accuracy.txt: the host routine of global positioning against the numpy oracle of
tests/_position_oracle.py and against ground truth, on the scenes of tests/test_position.py.  The constants MEASURED_* of that test are
read off this file.

    python tools/position_accuracy.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _position_cases as PC      # noqa: E402
import _position_oracle as PO     # noqa: E402
from loftr_amd import positions   # noqa: E402


def main():
    scenes = [PC.small(), PC.ring(), PC.line(), PC.exact("ring"), PC.exact("line")] + PC.further_cases()
    lines = ["global positioning: host routine (loftr_global_positions_host) against the numpy oracle and ground truth",
             "d_*: largest distance to the oracle's conjugate-gradient leg; err_*: largest centre error after a similarity (Umeyama)",
             f"{'scene':<16} {'trials':>6} {'pcg':>5} {'d_centres':>10} {'d_xyz':>10} {'d_depth':>10} {'err_host':>10} {'err_pcg':>10} {'err_dense':>10}"]
    worst = np.zeros(3)
    for sc in scenes:
        got = positions.global_positions(*sc.args).to_host()
        want, dense = PO.positions(*sc.args, solver="pcg"), PO.positions(*sc.args, solver="dense")
        m, a = got["cam_state"] > 0, got["point_active"]
        d = np.array([np.abs(got["centres"][m] - want["centres"][m]).max(), np.abs(got["xyz"][a] - want["xyz"][a]).max(),
                      np.abs(got["depth_scale"] - want["depth_scale"]).max()])
        worst = np.maximum(worst, d)
        idx = np.nonzero(m)[0]
        err = [PO.align_error(r["centres"][idx], sc.c_gt[idx]) for r in (got, want, dense)]
        lines.append(f"{sc.name:<16} {got['stats']['n_trials']:>6} {got['stats']['n_pcg_iters']:>5} {d[0]:>10.3e} {d[1]:>10.3e} {d[2]:>10.3e} "
                     f"{err[0]:>10.3e} {err[1]:>10.3e} {err[2]:>10.3e}")
    lines.append(f"largest: d_centres {worst[0]:.3e}, d_xyz {worst[1]:.3e}, d_depth {worst[2]:.3e}")
    lines.append("ring / line: 0.5 px noise at f = 500, 0.5 degrees on the rotations, 7 % gross outliers (one per track at most); the ring has "
                 "radius 6, the line spans 6")
    path = os.path.join(ROOT, "profiles", "position_accuracy.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
