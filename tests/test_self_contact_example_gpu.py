"""examples/cut_slab_rests.py at a small size: with self-collision the slab's lowest node ends above the stump's top minus one cell,
without it the slab sinks through and ends below that."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cut_slab_rests_example(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cut_slab_rests.py"), "--n", "5", "--steps", "50"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cut slab rests ok" in out.stdout
    line = [w for w in out.stdout.splitlines() if w.startswith("RESULT ")][0]
    r = {k: float(x) for k, x in (w.split("=") for w in line.split()[1:])}
    print(line)
    assert r["contacts"] > 0
    assert r["with"] > -r["cell"]       # carried by the stump
    assert r["without"] < -r["cell"]    # nothing carries it
