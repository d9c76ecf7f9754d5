"""examples/anymal_ilqr_full_cost.cpp on the GPU: 256 perturbed standing ANYmal plants under the ANYmal workload's own cost (a_weight and f_weight
set, u_weight = 0), improved by idocp_rbd_ilqr_iterate_gn_device.  It builds, exits 0, prints the mean cost before and after its iterations, and the
mean cost after is below the mean cost before (no factor is fixed in advance; observed 1.633e2 before, 1.084e1 after); the mean cost of an
iteration never lies above the one before it."""
import os
import re
import subprocess

import pytest

from helpers import ANYMAL_URDF, ROOT

pytestmark = pytest.mark.gpu


def test_anymal_ilqr_full_cost_example():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "anymal_ilqr_full_cost"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(ROOT, "examples", "anymal_ilqr_full_cost"), ANYMAL_URDF], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    print(r.stdout)
    assert "256 plants" in r.stdout and "32 residual rows per stage" in r.stdout
    before = float(re.search(r"mean cost before = (\S+)", r.stdout).group(1))
    after = float(re.search(r"mean cost after = (\S+)", r.stdout).group(1))
    rows = re.findall(r"iteration (\d+): mean cost = (\S+)  accepted = (\d+)", r.stdout)
    assert [int(x[0]) for x in rows] == list(range(5)), r.stdout
    print("mean cost before %.6e, after %.6e" % (before, after))
    assert after < before, (before, after)
    cost = [before] + [float(x[1]) for x in rows]
    assert all(b <= a for a, b in zip(cost[:-1], cost[1:])), cost      # (a rejected plant keeps its cost, so the mean never rises)
    assert int(rows[0][2]) > 0, rows[0]
