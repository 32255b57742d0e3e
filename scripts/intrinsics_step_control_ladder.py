#!/usr/bin/env python3
"""The ladder of the intrinsics step's control on the CPU: the oracle (orc_intrinsics_accumulate, orc_evaluate_cost) and the binary32 model
of the damped step, both through tests/intrinsics_step_control.py (ladder_profile).  Depth and colour intrinsics, both residual types.

  table     per scene and step of the PLAIN sequence (every step applied): the cost before, and the cost of the damped step at every
            rung 0, 0.25, 1, 4, 10, 16, 64, 100, 256 from that state; `kind` by the default ladder's four rungs (0, 1, 4, 16):
            "falls" (the plain step lowers the cost), "R" (it raises it and a rung lowers it), "H" (no rung lowers it)
  sequences per scene and choice of ladder: eight controlled steps from the scene's first state, lambda carried over; per step the
            accepted rung (or null), the trials and the cost after; `final` the cost the sequence ends at
  search    the states "R" and "H" found over the scenes of tests/two_cameras.py and the seeds of tests.common.small_scene
            (tests/test_cpu_intrinsics_step_control.py asserts the two it uses; rises below 1e-6 relative are within the noise of the
            binary32 terms and are listed with their margins for that reason)

Writes profiles/intrinsics_step_control_ladder.json."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import intrinsics_step_control as isc   # noqa: E402


def main():
    out = isc.ladder_profile()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "intrinsics_step_control_ladder.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    for name, final in out["plain_final"].items():
        print(name, "plain after 8 steps", final, {label: s["final"] for label, s in out["sequences"][name].items()})


if __name__ == "__main__":
    main()
