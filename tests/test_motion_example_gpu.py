"""examples/grasp_and_pull.py at a small size: the held end follows the tool, the tissue pulls back on it, and let go it springs back."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grasp_and_pull_example(gpu, tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "grasp_and_pull.py"), "--n", "7", "--steps", "8", "--free", "8", "--out", str(tmp_path)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "grasp and pull ok" in out.stdout
    line = [w for w in out.stdout.splitlines() if w.startswith("RESULT ")][0]
    r = {k: float(x) for k, x in (w.split("=") for w in line.split()[1:])}
    print(line)
    assert r["held"] == 16 and r["builds"] == 1 and r["fixed_after"] == 48
    assert r["follow"] <= 1e-12           # the held nodes are where the tool is
    assert r["fx"] < 0                    # pulled along +x, the tissue pulls the tool back
    assert r["end_held"] > 0.0149 and r["end_free"] < r["end_held"]   # dragged 0.15 cells; released, the end is on its way back
    for name in ("before", "held", "after"):
        text = (tmp_path / (name + ".obj")).read_text().splitlines()
        assert sum(w.startswith("v ") for w in text) == 7 * 16 - 5 * 4 and sum(w.startswith("f ") for w in text) == 2 * (2 * 9 + 4 * 6 * 3)
