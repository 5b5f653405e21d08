"""examples/probe_contact.py runs: the box misses, then touches, the set only grows, the BOTTOM face presses and stays after the mouse-up."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_example_probe_contact(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "probe_contact.py"), "12", "5"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "probe contact ok" in out.stdout
    frames = re.findall(r"frame (\d+): (\w+), (\d+) touched \((\d+) new\), face (\w+)", out.stdout)
    assert [int(f[0]) for f in frames] == list(range(5))
    assert frames[0][1:] == ("miss", "0", "0", "none") and frames[1][1] == "set" and int(frames[1][2]) == int(frames[1][3]) == 6 * 6
    assert all(f[4] == "BOTTOM" for f in frames[1:])
    assert "0 touched, face kept BOTTOM" in out.stdout
    assert re.search(r"volume before \d\.\d+ after \d\.\d+", out.stdout)
