"""examples/anymal_rollout_linearisation.cpp on the GPU: the standing policy rolled out on a few perturbed plants, linearised with
idocp_rbd_linearize_rollout, the products of A (open loop) and of A + B K (closed loop), and the gap between a re-rollout from x_0 (+) (+-eps) d
under the same torques and the linear prediction.  It exits 0 and prints finite numbers; the gap is of second order in eps, so it falls by about
100 when eps falls 10 times: asserted as a factor between 30 and 300."""
import math
import os
import re
import subprocess

import pytest

from helpers import ANYMAL_URDF, ROOT

pytestmark = pytest.mark.gpu


def test_anymal_rollout_linearisation_example():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "anymal_rollout_linearisation"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(ROOT, "examples", "anymal_rollout_linearisation"), ANYMAL_URDF, "10", "0.02", "1e-3"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    print(r.stdout)
    norm_open = re.search(r"open loop:\s+max \|prod A\|_inf = (\S+)", r.stdout)
    norm_closed = re.search(r"closed loop: max \|prod \(A \+ B K\)\|_inf = (\S+)", r.stdout)
    gaps = re.findall(r"gap of the linear prediction at eps = (\S+): (\S+)", r.stdout)
    assert norm_open and norm_closed and len(gaps) == 2, r.stdout
    numbers = [float(norm_open.group(1)), float(norm_closed.group(1))] + [float(x) for g in gaps for x in g]
    assert all(math.isfinite(x) for x in numbers), r.stdout
    assert float(norm_open.group(1)) > 0.0 and float(norm_closed.group(1)) > 0.0
    assert abs(float(gaps[0][0]) / float(gaps[1][0]) - 10.0) < 1e-6, r.stdout      # eps fell 10 times
    ratio = float(gaps[0][1]) / float(gaps[1][1])
    assert 30.0 < ratio < 300.0, (ratio, r.stdout)
