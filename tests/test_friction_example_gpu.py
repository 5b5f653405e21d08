"""examples/friction_holds.py: a block pushed sideways on another glides like a free body without friction, is held with a friction
coefficient above the load ratio and slides, slower, with one below it.

The bounds come from a rigid-block model of the same steps (a point mass under the sideways load and the regularised friction of its
weight, implicit Euler), which gives 0.10 of the frictionless drift for mu = 0.5 and 0.65 for mu = 0.05; they are not a measurement.
The factor of about 3 on the first and the +-0.25 on the second cover the fluctuating normal force and the blocks' deformation.
Measured on an MI355X: 0.968 of the free sideways fall with mu = 0, then 0.119 and 0.629 of that run's drift."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_friction_holds_example(gpu):
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "examples", "friction_holds.py")], text=True, cwd=ROOT)
    print(out)
    m = re.search(r"^RESULT free=(\S+) mu0=(\S+) mu05=(\S+) mu005=(\S+)$", out, re.M)
    assert m, out
    free, mu0, mu05, mu005 = (float(x) for x in m.groups())
    dt, steps = 0.01, 40
    assert abs(free - 38.4 / 27.0 * dt * dt * steps * (steps + 1) / 2) < 1e-12   # F_x / m dt^2 k (k + 1) / 2: 38.4 N on 27 kg
    print("fractions of the free sideways fall: mu=0 %.4f, mu=0.5 %.4f of the mu=0 run, mu=0.05 %.4f of the mu=0 run" % (mu0 / free, mu05 / mu0, mu005 / mu0))
    assert abs(mu0 - free) <= 0.05 * free
    assert 0.0 <= mu05 <= 0.3 * mu0
    assert 0.4 * mu0 <= mu005 <= 0.9 * mu0
    assert "friction holds ok" in out
