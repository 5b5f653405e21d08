"""examples/enclosing_surface.py runs: every drawn vertex is outside the tets, and the search went through the centre grid."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_example_enclosing_surface(gpu):
    env = {k: v for k, v in os.environ.items() if k not in ("FEMBRAIN_EMBED_CLOSEST", "FEMBRAIN_EMBED_RING_BUDGET")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "enclosing_surface.py")], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "enclosing surface ok" in out.stdout
    n_vertices = int(out.stdout.split(" drawn vertices")[0].split()[-1])
    n_outside = int(out.stdout.split(" outside the tets")[0].split()[-1])
    assert n_vertices == n_outside >= 8192
    assert "closest centres by ring" in out.stdout and " 1 centre grid(s) built" in out.stdout
    per_point = float(out.stdout.split(" per point (a scan")[0].split()[-1])
    n_tets = int(out.stdout.split(" tets;")[0].split()[-1])
    assert per_point < n_tets / 2  # (with the points the ring left to the scan, a fifth of them on the CPU, at n_tets each)
