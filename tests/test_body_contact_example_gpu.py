"""examples/parts_collide.py on its small beam: without the contact call the detached piece falls through the beam by the free-fall
distance, with it the piece ends above the beam's top."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parts_collide_example(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "parts_collide.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "parts collide ok" in out.stdout
    line = [w for w in out.stdout.splitlines() if w.startswith("RESULT ")][0]
    r = {k: float(x) for k, x in (w.split("=") for w in line.split()[1:])}
    print(line)
    assert r["contacts"] > 0 and r["fall"] > 2 * r["start"]
    # without contact: below the beam's top, and by the free-fall distance below where it started.  The figure is the mean of the nodes,
    # not the centre of mass, which is what falls by exactly that distance: the two differ by the deformation of the piece under a load
    # that is uniform per node and not per mass, a few per cent of a cell here against a fall of many cells -- 2 % of the fall allowed
    assert r["without"] < 0 and abs((r["start"] - r["without"]) - r["fall"]) <= 0.02 * r["fall"]
    # with contact: above the beam's top, and not higher than it started
    assert 0 < r["with"] <= r["start"] + 1e-9
