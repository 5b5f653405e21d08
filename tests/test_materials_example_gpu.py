"""examples/tumor_inclusion.py runs (documentation that must not rot): a stiff inclusion stepped, cut through, materials read back."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_tumor_inclusion_example_runs(gpu):
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "examples", "tumor_inclusion.py"), "--n", "8"], text=True)
    assert "of them tumour" in out and "pieces added" in out and "3 steps after the cut" in out
    cut = [ln for ln in out.splitlines() if ln.startswith("pieces whose centroid")][0].replace(",", " ").split()
    assert int(cut[-1]) > 0   # the blade went through the inclusion: there are tumour pieces
