"""Writes profiles/calibration_accuracy.txt: the host routine of view-graph calibration against the numpy oracle of
tests/_calibration_oracle.py and against ground truth, on the scenes of tests/_calibration_cases.py, and the end-to-end chain on the
atlas scene against the yardstick run with the true intrinsics.  The constants MEASURED_* of tests/test_calibration.py are read off
this file.

    python tools/calibration_accuracy.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _calibration_cases as CC      # noqa: E402
import _calibration_oracle as CO     # noqa: E402
from loftr_amd import ops_calib      # noqa: E402


def main():
    lines = ["view-graph calibration: host routine (loftr_calibrate_view_graph_host) against the numpy oracle and ground truth",
             "d_*: largest distance to the oracle's conjugate-gradient leg (pcg) and to its dense leg; err_*: largest relative focal error",
             f"{'scene':<16} {'E':>4} {'trials':>6} {'pcg':>4} {'d_scale_pcg':>11} {'d_resid_pcg':>11} {'d_scale_dns':>11} {'d_resid_dns':>11} "
             f"{'err_start':>9} {'err_host':>9} {'err_dense':>9} {'good_max':>9} {'false_min':>9}"]
    worst = np.zeros(4)
    scenes = [("small", CC.small())] + [(name, CC.ring(**kw)) for name, kw in CC.GENERAL + CC.PLANTED + CC.SHARED]
    for name, sc in scenes:
        a = CC.raw_args(sc)
        G = len(a[6]) - 1
        got = ops_calib.calibrate_view_graph_host(*a)
        legs = [CO.calibrate(a[0], a[1], a[2], a[3], a[4], a[5], G, solver=s) for s in ("pcg", "dense")]
        d = np.array([np.abs(got[k] - leg[k]).max() for leg in legs for k in ("focal_scale", "edge_resid")])
        worst = np.maximum(worst, d)
        err = [np.abs(x / sc.f_true - 1).max() for x in (sc.f0, got["focal"], legs[1]["focal"])]
        r = got["edge_resid"]
        lines.append(f"{name:<16} {len(a[0]):>4} {got['counts'][0]:>6} {got['counts'][3]:>4} {d[0]:>11.3e} {d[1]:>11.3e} {d[2]:>11.3e} {d[3]:>11.3e} "
                     f"{err[0]:>9.4f} {err[1]:>9.4f} {err[2]:>9.4f} {r[~sc.planted].max():>9.4f} "
                     f"{(r[sc.planted].min() if sc.planted.any() else float('nan')):>9.4f}")
    lines.append(f"largest: d_scale_pcg {worst[0]:.3e}, d_resid_pcg {worst[1]:.3e}, d_scale_dense {worst[2]:.3e}, d_resid_dense {worst[3]:.3e}")
    lines.append("scenes: 0.3 to 1 px noise, 40 or 80 points per edge, focals 600 to 1100 at 1000 x 750 pixels, start 1.2 * 1000 for every image; "
                 "a quarter of the edges of the *_false scenes are random rank-2 matrices")
    lines.append("")
    lines.append("degenerate ring (every camera looks at the origin), starts 10 % off: largest relative focal error")
    lines.append(f"{'seed':<6} {'start':>8} {'prior 1e-3':>11} {'prior 0':>9}")
    for seed in CC.DEGENERATE_SEEDS:
        sc = CC.ring(seed, n=12, k=3, noise=0.5, degenerate=True, start=0.1)
        a = CC.raw_args(sc)
        e = [np.abs(ops_calib.calibrate_view_graph_host(*a, prior_weight=pw)["focal"] / sc.f_true - 1).max() for pw in (1e-3, 0.0)]
        lines.append(f"{seed:<6} {np.abs(sc.f0 / sc.f_true - 1).max():>8.4f} {e[0]:>11.4f} {e[1]:>9.4f}")
    lines.append("")
    lines.append("end to end on the atlas scene (8 images, 220 points, 2 px cells, 24 rows; CPU chain): SfmResult.reconstruct_uncalibrated() against")
    lines.append("the yardstick SfmResult.reconstruct(K_true, ba={'refine_focal': True}) on the same atlas; focal: largest relative error of the")
    lines.append("final K; centre: largest centre error after a similarity (ring of radius 6)")
    from loftr_amd import evaluation
    sfm, sc = CC.atlas_scene("cpu")
    cal = sfm.calibrate()
    rec, ref = sfm.reconstruct_uncalibrated(), sfm.reconstruct(sc.K_true, ba={"refine_focal": True})
    e0 = np.median(evaluation.focal_errors(np.full(sc.n, 1.2 * CC.W), sc.K_true))
    e1 = evaluation.focal_errors(cal.focal, sc.K_true)
    (fu, cu), (fy, cy) = CC.reconstruction_errors(rec, sc), CC.reconstruction_errors(ref, sc)
    lines.append(f"tracks {sfm.track_len.numel()}, posed {int(rec.posed.sum())} / {int(ref.posed.sum())}; median focal error: start {e0:.4f}, "
                 f"after calibration alone {np.median(e1):.4f} (largest {e1.max():.4f})")
    lines.append(f"uncalibrated: focal {fu:.3e}, centre {cu:.3e};  yardstick: focal {fy:.3e}, centre {cy:.3e}")
    lines.append(f"excess over the yardstick: focal {fu - fy:.3e}, centre {cu - cy:.3e}")
    lines.append("margin asserted by the tests: focal excess <= 2e-3, centre excess <= 2.5e-3.  Reason: both runs end in the same bundle")
    lines.append("adjustment over the same tracks and differ only in the start values of the focals (about 1 % off against exact), so they stop")
    lines.append("on ftol at neighbouring points of one basin.  The margins are a third (focal) and a tenth (centre) of the yardstick's OWN error")
    lines.append("above, which the 2 px cells cause, and ten times the measured focal excess.  The scene is one where the yardstick run converges")
    lines.append("and poses all 8 images.")
    path = os.path.join(ROOT, "profiles", "calibration_accuracy.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
