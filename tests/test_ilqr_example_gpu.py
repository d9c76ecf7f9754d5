"""examples/anymal_ilqr.cpp on the GPU: 256 standing ANYmal plants, started off the pose and under pushed-off solver torques, improved by ten calls of
idocp_rbd_ilqr_iterate_device.  It builds, exits 0, plants accept a step in the first iteration, and the mean cost after the last iteration is below
the one after the first."""
import os
import re
import subprocess

import pytest

from helpers import ANYMAL_URDF, ROOT

pytestmark = pytest.mark.gpu


def test_anymal_ilqr_example():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "anymal_ilqr"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(ROOT, "examples", "anymal_ilqr"), ANYMAL_URDF], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    print(r.stdout)
    rows = re.findall(r"iteration (\d+): mean cost = (\S+)  accepted = (\d+)  mean alpha = (\S+)  max \|e0\| = (\S+)", r.stdout)
    assert [int(x[0]) for x in rows] == list(range(10)), r.stdout
    cost = [float(x[1]) for x in rows]
    assert int(rows[0][2]) > 0, rows[0]
    assert cost[-1] < cost[0], cost
