"""examples/anymal_ilqr_constrained.cpp on the GPU: 256 perturbed standing ANYmal plants under the ANYmal workload's cost, the joint limits, a
friction cone with a small coefficient and a tight acceleration box, improved by idocp_rbd_ilqr_iterate_penalty_device with mu raised per
iteration and, from the same start, by idocp_rbd_ilqr_iterate_gn_device.  It builds, exits 0, and prints for both runs the mean cost, the mean
sq_violation and the mean L1 violation before and after, with the plants that are not finite counted; both runs start from the same three
means, and the penalty run ends with a smaller mean sq_violation than it started with (no factor fixed).  How the two runs end is printed, not
asserted: with the example's defaults (mu 10 raised by 4 per iteration, five iterations) the cost-only run ends LOWER on an MI355X -- mean cost
163.3 -> 27.61 under the penalty and -> 10.84 without, mean sq_violation 5357 -> 1472 under the penalty and -> 1252 without, mean L1 violation
135.5 -> 74.1 and -> 47.7, no plant failing in either run.  Why the penalty run is behind here has not been looked into.  A finding, recorded in DESIGN.md as well."""
import os
import re
import subprocess

import pytest

from helpers import ANYMAL_URDF, ROOT

pytestmark = pytest.mark.gpu

LINE = r"  %s: mean cost = (\S+)  mean sq_violation = (\S+)  mean L1 violation = (\S+)  \(over (\d+) plants, (\d+) not finite\)"


def test_anymal_ilqr_constrained_example():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "anymal_ilqr_constrained"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(ROOT, "examples", "anymal_ilqr_constrained"), ANYMAL_URDF], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "256 plants" in r.stdout and "32 cost rows and 32 constraint rows per stage" in r.stdout
    before = [[float(x) for x in m] for m in re.findall(LINE % "before", r.stdout)]
    after = [[float(x) for x in m] for m in re.findall(LINE % "after", r.stdout)]
    assert len(before) == 2 and len(after) == 2 and before[0] == before[1], r.stdout
    assert before[0][1] > 0 and before[0][3] + before[0][4] == 256
    print("penalty run: sq_violation %.6e -> %.6e; cost-only run: -> %.6e" % (before[0][1], after[0][1], after[1][1]))
    assert after[0][1] < before[0][1], (before, after)
