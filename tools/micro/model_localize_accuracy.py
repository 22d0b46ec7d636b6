"""Per-query accuracy of the localisation against the triangulated model on the seeded test scene (host routines; no GPU needed): the
pose errors against the same estimator fed the ground-truth points -- what
tests/test_model_lookup.py::test_scene_poses_are_within_twice_the_ground_truth_baseline asserts.

    python tools/micro/model_localize_accuracy.py > profiles/model_localize_accuracy.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _model_lookup_cases as MC                                    # noqa: E402

if __name__ == "__main__":
    model, _, pts = MC.build_model("cpu")
    res = MC.localize_scene(model).solve(MC.query_scene()["K"], thresh_px=3.0, conf=0.999, seed=0)
    print(MC.accuracy_report(MC.accuracy_figures(res, MC.run_oracle(MC.scene_as_case(model)))))
    print("triangulation:", pts.stats)
    print("lookup:", res.stats)
