"""bench.py --dump-outputs on the GPU: two runs with the same arguments time exactly --steps iterations each and write the same
outputs of the timed region, bit for bit (the scene is seeded; the sums of the backend have a defined order)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_runs_dump_the_same_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dumped = []
    for run in ("a", "b"):
        proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--keyframes", "12",
                               "--surfels", "100000", "--no-cpu-baseline", "--no-extras", "--dump-outputs", str(tmp_path / run)],
                              capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert proc.returncode == 0, proc.stderr[-3000:]
        lines = [l for l in proc.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, proc.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 4 and out["launch_window"]["iterations_timed"] == 4
        assert out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] - 1e3) < 1e-6 * 1e3
        files = sorted(os.listdir(tmp_path / run))
        assert "keyframe_poses.npy" in files and "surfel_positions.npy" in files
        dumped.append({f[:-4]: np.load(tmp_path / run / f) for f in files})
    a, b = dumped
    assert a.keys() == b.keys()
    assert a["keyframe_poses"].shape == (12, 7) and a["surfel_positions"].shape[0] == out["config"]["surfels"]
    for name in a:
        assert a[name].dtype in (np.float32, np.float64) and a[name].shape == b[name].shape, name
        assert a[name].tobytes() == b[name].tobytes(), name
