"""examples/anymal_ilqr_al.cpp on the GPU: the 256 plants of anymal_ilqr_constrained.cpp improved three ways from the same start -- the cost alone,
the penalty with that example's mu schedule, AL at the schedule's first mu held fixed with a multiplier update every second iteration.  It builds,
exits 0 and prints finite figures for all three runs; the three runs start from the same figures.  How the runs end is printed, not asserted; the
figures of one run on an MI355X are in DESIGN.md section 6."""
import math
import os
import re
import subprocess

import pytest

from helpers import ANYMAL_URDF, ROOT

pytestmark = pytest.mark.gpu

LINE = r"  (cost|penalty|AL) %s: mean cost = (\S+)  mean sq_violation = (\S+)  largest infeasibility = (\S+)  \(over (\d+) plants, (\d+) failed\)"


def test_anymal_ilqr_al_example():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "anymal_ilqr_al"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(ROOT, "examples", "anymal_ilqr_al"), ANYMAL_URDF], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "256 plants" in r.stdout and "68 multiplier rows" in r.stdout and r.stdout.count("(multipliers updated)") == 2
    before, after = re.findall(LINE % "before", r.stdout), re.findall(LINE % "after", r.stdout)
    assert [m[0] for m in before] == [m[0] for m in after] == ["cost", "penalty", "AL"], r.stdout
    figures = lambda m: [float(x) for x in m[1:4]]      # noqa: E731
    assert figures(before[0]) == figures(before[1]) == figures(before[2]) and figures(before[0])[1] > 0
    for m in before + after:
        assert all(math.isfinite(x) for x in figures(m)) and int(m[4]) + int(m[5]) == 256, m
