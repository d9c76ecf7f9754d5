"""examples/anymal_sampling_refinement.cpp on the GPU: a torque sequence pushed off the converged solution by 2 N m on every joint, repaired by six
iterations of perturb / rollout / score / weights / weighted mean on device arrays.  It exits 0, every printed number is finite, and the nominal's cost
after the last iteration is below its cost before the first.  The run is deterministic (fixed seed, fixed order of summation).  The example's defaults
are what is tested: 256 plants, 10 steps, sigma = 1 N m on every joint, temperature = 2 (the scores of the first iteration lie hundreds apart, so the
first updates follow the best sample; as the scores close up several samples share the weight)."""
import math
import os
import re
import subprocess

import pytest

from helpers import ANYMAL_URDF, ROOT

pytestmark = pytest.mark.gpu


def test_anymal_sampling_refinement_example():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "anymal_sampling_refinement"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(ROOT, "examples", "anymal_sampling_refinement"), ANYMAL_URDF], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    print(r.stdout)
    rows = re.findall(r"iteration (\d+): nominal cost = (\S+)\s+s_min = (\S+)\s+effective samples = (\S+)\s+finite = (\d+)", r.stdout)
    final = re.search(r"final: nominal cost = (\S+)", r.stdout)
    assert len(rows) == 6 and final, r.stdout
    numbers = [float(x) for row in rows for x in row[1:]] + [float(final.group(1))]
    assert all(math.isfinite(x) for x in numbers), r.stdout
    assert all(int(row[4]) == 256 and float(row[3]) >= 1.0 for row in rows), r.stdout
    assert float(final.group(1)) < float(rows[0][1]), r.stdout      # the nominal's cost: after the last iteration below before the first
