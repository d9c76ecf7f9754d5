"""The three linearisations with rows -- idocp_rbd_linearize_rollout_cost, _penalty, _al -- run ONE check sequence, ONE device body and ONE host
staging list (rbd_capi.hip: linearizeRowsDevice, linearizeRowsHost); this file pins the collapses that body rests on where the neighbouring files
do not.  They hold the penalty call to the cost call on an objective WITH constraints (the cost rows, A, B), the AL call with lambda = NULL to the
penalty call, and the two forms of each call to one another, all at n = 5, steps = 4 (n = 70 for the cost call) WITHOUT a touchdown in the penalty
and AL forms.  New here, every comparison on tobytes():
  (a) on an objective created WITHOUT constraints the penalty call returns the arrays it shares with the cost call (A, B, G, rho, lx, lu), its rows
      being the cost rows alone;
  (b) the AL call with lambda_traj = NULL returns the penalty call's arrays, with a touchdown impulse in the schedule;
  (c) host form and device form of each of the three return the same arrays, the penalty and AL forms with the touchdown, the AL form under
      non-zero multipliers.
Shapes: chain2 with n = 5, steps = 2; ANYmal with n = 3 (odd: the pass chunk is even), steps = 2, two active contacts then four (so the
touchdown of the other two lies in front of step 1), the linearised cone."""
import functools

import numpy as np
import pytest

import rbd_al as AL
import rbd_forward as F
import rbd_gauss_newton as GN
import rbd_penalty as PN
import rbd_score as RS
from rbd_batch import Rbd
from test_rbd_gauss_newton_host import full_cost
from test_rbd_ilqr_gpu import start
from test_rbd_penalty_gpu import median_bounds

pytestmark = pytest.mark.gpu

STEPS, MU, T0 = 2, 25.0, 0.0
CASES = [("chain2", 5, None), ("anymal", 3, "linearized")]
SHARED = ("A_traj", "B_traj", "G_traj", "rho_traj", "lx_traj", "lu_traj")


@functools.lru_cache(maxsize=None)
def case(which, n, cone):
    """(model with limits, model dict, cost, constraints, active, pts, ts, dt, the rollout q, v, u, multipliers); bounds at the medians of the
    rollout as in test_rbd_penalty_gpu.py, so that constraint rows are active"""
    m, M, _, active, pts, dt, ts, (q0, v0, u) = start(which, n, STEPS)
    rng = np.random.default_rng([53, len(which), n])
    cost = full_cost(m, rng)
    if which == "anymal":
        active = ((0, 1, 1, 0), (1, 1, 1, 1))
    else:
        u = rng.uniform(-3, 3, u.shape)
    r = Rbd(m)
    q, v, a, f = F.rollout(r, q0, v0, u, active, ts, dt, pts, impulse=True)
    r.close()
    assert np.isfinite(q).all() and np.isfinite(v).all()
    mm, cons = median_bounds(m, M, q[:STEPS], v[:STEPS], u, a, f, None)
    if cone:      # (the friction coefficient at the median force ratio of the ACTIVE contacts: a lifted foot has no force)
        ff = np.asarray(f).reshape(-1, 3)
        ff = ff[ff[:, 2] > 0]
        cons.mu = float(np.median(np.hypot(ff[:, 0], ff[:, 1]) / ff[:, 2]))
        cons.linearized_friction_cone = 1
    lam = rng.uniform(0.0, 2.0, (STEPS, n, AL.multiplier_rows(mm, M, cons)))
    return mm, M, cost, cons, active, pts, ts, dt, (q, v, u), lam


def calls(r, o, cons, which, n, cone, device):
    """the three calls on one objective: {entry: {name: array}}"""
    mm, M, cost, _, active, pts, ts, dt, (q, v, u), lam = case(which, n, cone)
    return {
        "cost": GN.linearize_cost(r, M, o, q, v, u, active, ts, dt, pts, impulse=True, device=device),
        "penalty": PN.linearize_penalty(r, M, cons, o, MU, q, v, u, active, ts, dt, pts, impulse=True, device=device),
        "al_null": AL.linearize_al(r, M, cons, o, MU, None, q, v, u, active, ts, dt, pts, impulse=True, device=device),
        "al": AL.linearize_al(r, M, cons, o, MU, lam if cons is not None else None, q, v, u, active, ts, dt, pts, impulse=True, device=device),
    }


def same_bytes(x, y):
    return x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("which,n,cone", CASES)
def test_the_forms_collapse_onto_one_another(which, n, cone):
    mm, M, cost, cons, active, pts, ts, dt, (q, v, u), lam = case(which, n, cone)
    r = Rbd(mm)
    bare = RS.Objective(r, cost, None, T0, dt, STEPS)
    full = RS.Objective(r, cost, cons, T0, dt, STEPS)
    assert r.lib.idocp_rbd_objective_constraint_rows(bare.h) == 0 and r.lib.idocp_rbd_objective_constraint_rows(full.h) > 0
    host_bare, host_full = calls(r, bare, None, which, n, cone, False), calls(r, full, cons, which, n, cone, False)
    dev_bare, dev_full = calls(r, bare, None, which, n, cone, True), calls(r, full, cons, which, n, cone, True)
    if which == "anymal":      # (the schedule does carry a touchdown, and A_traj[0] its E)
        plain = GN.linearize_cost(r, M, bare, q, v, u, active, ts, dt, pts, impulse=False, want=("A_traj",))
        assert not same_bytes(plain["A_traj"][0], host_bare["cost"]["A_traj"][0]) and same_bytes(plain["A_traj"][1], host_bare["cost"]["A_traj"][1])
    # (a) without constraints: the penalty call's shared arrays are the cost call's (and so are the AL call's)
    for entry in ("penalty", "al_null"):
        for name in SHARED:
            assert same_bytes(host_bare[entry][name], host_bare["cost"][name]), (entry, name)
    # (b) lambda_traj = NULL: the penalty call's arrays; the multipliers do move the constraint rows
    for name in PN.OUTPUTS:
        assert same_bytes(host_full["al_null"][name], host_full["penalty"][name]), name
    assert not same_bytes(host_full["al"]["rho_traj"], host_full["penalty"]["rho_traj"])
    # (c) host form and device form: the same arrays, on both objectives
    for host, dev in ((host_bare, dev_bare), (host_full, dev_full)):
        for entry in host:
            for name in host[entry]:
                assert np.isfinite(host[entry][name]).all(), (entry, name)
                assert same_bytes(host[entry][name], dev[entry][name]), (entry, name)
    bare.close()
    full.close()
    r.close()
