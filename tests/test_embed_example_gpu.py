"""examples/embedded_surface.py runs, and the two files it writes hold the drawn surface: the polygonizer's vertex and triangle counts."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_example_embedded_surface(gpu, tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "embedded_surface.py"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "embedded surface ok" in out.stdout
    n_vertices = int(out.stdout.split(" drawn vertices")[0].split()[-1])
    n_triangles = int(out.stdout.split(" triangles bound")[0].split()[-1])
    assert n_vertices > 1000
    for stem in ("before", "after"):
        lines = open(str(tmp_path / (stem + ".obj"))).read().splitlines()
        assert sum(ln.startswith("v ") for ln in lines) == sum(ln.startswith("vn ") for ln in lines) == n_vertices
        assert sum(ln.startswith("f ") for ln in lines) == n_triangles
