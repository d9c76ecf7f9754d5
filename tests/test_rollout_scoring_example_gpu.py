"""examples/anymal_rollout_scoring.cpp on the GPU: the converged standing policy on 256 perturbed plants with and without its gains, every plant scored by
idocp_rbd_score_rollout_device on the arrays the rollout left in device memory.  The numbers are finite and the gains pay: the mean cost with them is
below the mean cost without."""
import math
import os
import re
import subprocess

import pytest

from helpers import ANYMAL_URDF, ROOT

pytestmark = pytest.mark.gpu


def test_anymal_rollout_scoring_example():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "anymal_rollout_scoring"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(ROOT, "examples", "anymal_rollout_scoring"), ANYMAL_URDF], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    print(r.stdout)
    line = r"%s\s+cost mean = (\S+) worst = (\S+)\s+violation mean = (\S+) worst = (\S+)"
    closed, opened = re.search(line % "with gains:", r.stdout), re.search(line % "without gains:", r.stdout)
    assert closed and opened, r.stdout
    numbers = [float(x) for m in (closed, opened) for x in m.groups()]
    assert all(math.isfinite(x) and x >= 0.0 for x in numbers), r.stdout
    assert numbers[0] < numbers[4] and numbers[1] < numbers[5], r.stdout      # mean and worst cost: with gains below without
