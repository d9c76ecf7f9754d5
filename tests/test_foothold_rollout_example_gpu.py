"""examples/anymal_foothold_rollout.cpp on the GPU: the trotting solver's torques and gains rolled out closed loop on 256 perturbed plants over the first
lift-off and touchdown, with latched footholds and with the nominal's footholds.  It exits 0 and prints, for both runs, a finite touchdown spread, mean
tangential force and final distance over the plants that stayed finite, and their number; which
run does better is reported (README), not asserted.  Two solver iterations keep the case to seconds."""
import math
import os
import re
import subprocess

import pytest

from helpers import ANYMAL_URDF, ROOT

pytestmark = pytest.mark.gpu


def test_anymal_foothold_rollout_example():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "anymal_foothold_rollout"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(ROOT, "examples", "anymal_foothold_rollout"), ANYMAL_URDF, "22", "0.001", "2"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    print(r.stdout)
    head = re.search(r"first lift-off at step (\d+), first touchdown at step (\d+)", r.stdout)
    assert head and 0 < int(head.group(1)) < int(head.group(2)) < 22, r.stdout
    rows = re.findall(r"(latched|nominal) footholds: finite plants = (\d+)\s+touchdown spread = (\S+) m\s+mean tangential force = (\S+) N\s+mean final \|x \(-\) x_ref\| = (\S+)", r.stdout)
    assert [row[0] for row in rows] == ["latched", "nominal"], r.stdout
    assert all(math.isfinite(float(x)) for row in rows for x in row[1:]), r.stdout
    assert all(0 < int(row[1]) <= 256 for row in rows), r.stdout
    assert float(rows[0][2]) > 1e-6 and float(rows[1][2]) < 1e-12, r.stdout      # (per-plant points spread; the forced points are one point)
