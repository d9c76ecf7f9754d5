"""examples/anymal_forward_simulation.cpp end to end on the GPU: OCPSolver in closed loop against Robot::forwardDynamics / stepForwardEuler."""
import math
import os
import re
import subprocess

import pytest

from helpers import ANYMAL_URDF, ROOT

pytestmark = pytest.mark.gpu


def test_anymal_forward_simulation_example():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "anymal_forward_simulation"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(ROOT, "examples", "anymal_forward_simulation"), ANYMAL_URDF, "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    rows = re.findall(r"step (\d+): base height = (\S+) quaternion norm = (\S+) max \|a\| = (\S+) fz = (\S+) (\S+) (\S+) (\S+)", r.stdout)
    assert [int(x[0]) for x in rows] == list(range(5)), r.stdout
    for row in rows:
        vals = [float(x) for x in row[1:]]
        assert all(math.isfinite(x) for x in vals), row
        assert abs(vals[1] - 1.0) <= 1e-15, row                # quaternion norm
        assert 0.3 < vals[0] < 0.7, row                        # a standing ANYmal stays standing over five steps
        assert all(x > 0 for x in vals[3:]), row               # and its feet push
