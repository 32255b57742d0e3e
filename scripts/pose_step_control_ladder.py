"""The perturbation ladder of the pose phase's step control (tests/test_gpu_pose_step_control.py): translation sigma 5 mm x 2^rung,
rotation sigma 2 mrad x 2^rung on small_scene(5 keyframes, seed 21).  Per rung: every keyframe's cost before the pose phase, after the
plain phase and after the controlled one.  Writes profiles/pose_step_control_ladder.json; the test reads the first rung at which the
plain phase raises some keyframe's cost from it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.test_gpu_pose_step_control import CONTROL, LADDER, LADDER_RUNGS, ladder_rung   # noqa: E402


def main():
    rungs = [ladder_rung(r) for r in range(LADDER_RUNGS)]
    raised = [row["rung"] for row in rungs if row["plain_raised"]]
    table = dict(scene="tests.common.small_scene(num_keyframes=5, seed=21)", control=list(CONTROL), lambda_initial=1e-3,
                 first_raised_rung=min(raised) if raised else None, rungs=rungs)
    out = sys.argv[1] if len(sys.argv) > 1 else LADDER
    with open(out, "w") as f:
        json.dump(table, f, indent=1)
    for row in rungs:
        print(row["rung"], "plain raised", row["plain_raised"], "controlled rejected", row["controlled_rejected"])


if __name__ == "__main__":
    main()
