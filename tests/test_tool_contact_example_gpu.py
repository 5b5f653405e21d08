"""examples/tool_pushes.py at a small size: the beam carries the lowered tool (its depth stays below the tool's travel, the tissue pushes
the tool up) and holds it back while it is dragged."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tool_pushes_example(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tool_pushes.py"), "--n", "8", "--lower", "15", "--drag", "10"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tool pushes ok" in out.stdout
    line = [w for w in out.stdout.splitlines() if w.startswith("RESULT ")][0]
    r = {k: float(x) for k, x in (w.split("=") for w in line.split()[1:])}
    print(out.stdout)
    assert r["contacts"] > 0 and 0 < r["depth"] < r["travel"]
    assert r["fy_pressed"] > 0 and r["fx_dragged"] < 0
    assert r["sag"] < 0 < r["along"]       # pressed down, and taken along by the friction
