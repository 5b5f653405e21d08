"""examples/detach_part.py runs and prints its closing line."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_detach_part_example(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "detach_part.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "detach part ok" in out.stdout
