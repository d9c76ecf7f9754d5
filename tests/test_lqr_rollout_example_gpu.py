"""examples/anymal_lqr_rollout.cpp on the GPU: the solver's torques rolled out on the nominal plant, linearised, turned into LQR gains about that
rollout by idocp_rbd_lqr_backward, and 256 perturbed plants run without gains, with the solver's Riccati gains and with the LQR gains.  It builds,
exits 0 and prints finite numbers (no ranking of the three is asserted); with zero perturbation the LQR-gain run reproduces the open-loop
trajectory bit for bit, because K 0 adds nothing."""
import math
import os
import re
import subprocess

import pytest

from helpers import ANYMAL_URDF, ROOT

pytestmark = pytest.mark.gpu

RUNS = ("no gains", "solver's Riccati gains", "LQR gains about the rollout")


def run(perturbation):
    r = subprocess.run([os.path.join(ROOT, "examples", "anymal_lqr_rollout"), ANYMAL_URDF, "10", perturbation], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    print(r.stdout)
    rows = {name: re.search(re.escape(name) + r": mean final distance = (\S+), plants lost = (\d+)", r.stdout) for name in RUNS}
    off = re.search(r"LQR run against the nominal rollout: max difference = (\S+)", r.stdout)
    assert all(rows.values()) and off, r.stdout
    return {name: (float(m.group(1)), int(m.group(2))) for name, m in rows.items()}, float(off.group(1))


def test_anymal_lqr_rollout_example():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "anymal_lqr_rollout"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rows, off = run("0.02")
    assert all(math.isfinite(mean) and mean > 0.0 and 0 <= lost < 256 for mean, lost in rows.values()), rows
    assert math.isfinite(off) and off > 0.0
    rows, off = run("0")
    assert off == 0.0, off
    assert rows["LQR gains about the rollout"] == (0.0, 0) and rows["no gains"] == (0.0, 0), rows
