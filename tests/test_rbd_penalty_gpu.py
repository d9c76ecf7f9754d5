"""idocp_rbd_linearize_rollout_penalty and idocp_rbd_score_penalty on the GPU (the penalty form of rbd_residual_kernel.hip, rbd_penalty_kernel.hip) at
n = 5, steps = 4: ANYmal under both cone kinds and the chain of 2 joints.  The upper bound of every quantity sits at the MEDIAN of its rolled-out
values (q_max, a_max; v_max and u_max at the median of the magnitudes), the lower bound of q and a at the lower quartile, and the friction
coefficient at the median of the tangential-to-normal force ratio, so every enabled kind has active and inactive rows -- asserted first.
G, rho, D, lx, lu against the numpy referee of rbd_penalty.py (held to central differences by test_rbd_penalty_host.py) at the 1e-11 of
test_rbd_gauss_newton_gpu.py; the cost rows and A, B bit for bit the cost call's; mu = 0 equal to the cost call; a sample's bits whatever n and the
outputs asked for; a NaN that stays in its sample's slice; the refusals.  sq_violation against the referee at 1e-11, one call against two
accumulated windows bit for bit, independent of n."""
import functools
import math

import numpy as np
import pytest

import rbd_forward as F
import rbd_gauss_newton as GN
import rbd_gradients as G
import rbd_penalty as PN
import rbd_score as RS
from idocp_amd import capi
from rbd_batch import E_ARG, Rbd
from test_rbd_gauss_newton_host import full_cost
from test_rbd_gradients_gpu import BAR
from test_rbd_ilqr_gpu import start

pytestmark = pytest.mark.gpu

N, STEPS, MU, T0 = 5, 4, 25.0, 0.0
CASES = [("anymal", "linearized"), ("anymal", "nonlinear"), ("chain2", None)]


def same(x, y):
    return np.array_equal(x, y, equal_nan=True)


def median_bounds(m, M, q, v, u, a, f, cone):
    """(model with limits, constraints) for the rolled-out values q [.., nq], ...: see the head of the file"""
    nu, nv, nq = m.nu, m.nv, m.nq
    mm = capi.Model.from_buffer_copy(m)
    cons = capi.Constraints()
    cons.joint_position_limits = cons.joint_velocity_limits = cons.joint_torque_limits = 1
    cons.joint_acceleration_lower_limit = cons.joint_acceleration_upper_limit = 1
    flat = lambda x, w: np.asarray(x).reshape(-1, x.shape[-1])[:, x.shape[-1] - w:]      # noqa: E731
    qj, vj, uj, aj = flat(q, nu), flat(v, nu), flat(u, nu), flat(a, nu)
    mm.q_min[:nu], mm.q_max[:nu] = np.percentile(qj, 25, axis=0), np.median(qj, axis=0)
    mm.v_max[:nu], mm.u_max[:nu] = np.median(np.abs(vj), axis=0), np.median(np.abs(uj), axis=0)
    cons.a_min[:nu], cons.a_max[:nu] = np.percentile(aj, 25, axis=0), np.median(aj, axis=0)
    if cone:
        ff = np.asarray(f).reshape(-1, 3)
        cons.mu = float(np.median(np.hypot(ff[:, 0], ff[:, 1]) / ff[:, 2]))
        cons.linearized_friction_cone, cons.friction_cone = int(cone == "linearized"), int(cone == "nonlinear")
    return mm, cons


@functools.lru_cache(maxsize=None)
def case(which, cone, push=False):
    """(model with limits, model dict, cost, constraints, tables, active, pts, ts, dt, the rollout q, v, u, a, f).  push: sample 0 of ANYmal takes 15
    times its torques, so that a pinned foot PULLS on the ground (an active -fz row) -- the data of the linearisation and score tests; the
    iteration tests keep the configuration without it"""
    m, M, _, active, pts, dt, ts, (q0, v0, u) = start(which, N, STEPS)
    rng = np.random.default_rng([41, len(which)])
    cost = full_cost(m, rng)
    if which != "anymal":
        u = rng.uniform(-3, 3, u.shape)
    elif push:
        u = u.copy()
        u[:, 0] *= 15.0
    r = Rbd(m)
    q, v, a, f = F.rollout(r, q0, v0, u, active, ts, dt, pts)
    r.close()
    mm, cons = median_bounds(m, M, q[:STEPS], v[:STEPS], u, a, f, cone)
    return mm, M, cost, cons, RS.reference_tables(M, cost, T0, dt, STEPS), active, pts, ts, dt, (q, v, u, a, f)


@functools.lru_cache(maxsize=None)
def referee(which, cone):
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone, True)
    return PN.reference_penalty_linearization_batch(mm, M, cost, cons, MU, tables, dt, q, v, u, active, pts, ts)


def run(r, o, which, cone, n=N, mu=MU, **kw):
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone, True)
    c = lambda x: None if x is None else np.ascontiguousarray(x[:, :n])      # noqa: E731
    return PN.linearize_penalty(r, M, cons, o, mu, c(q), c(v), c(u), active, ts, dt, c(pts), **kw)


@pytest.mark.parametrize("which,cone", CASES)
def test_rows_diagonal_and_gradients(which, cone):
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone, True)
    nv, nu, nx = mm.nv, mm.nu, 2 * mm.nv
    ref = referee(which, cone)
    r = Rbd(mm)
    o = RS.Objective(r, cost, cons, T0, dt, STEPS)
    R, Rc = r.lib.idocp_rbd_objective_residual_rows(o.h), r.lib.idocp_rbd_objective_constraint_rows(o.h)
    assert Rc == PN.constraint_rows(mm, M, cons) == {"linearized": 32, "nonlinear": 20, None: 4}[cone]
    bare = RS.Objective(r, cost, None, T0, dt, STEPS)
    assert r.lib.idocp_rbd_objective_constraint_rows(bare.h) == 0
    # 0. every enabled kind has an active and an inactive row in the data
    sig, Dr = ref["rho_traj"][:, :, R:], ref["D_traj"]
    kinds = {"a": sig[:, :, :nu], "q": Dr[:, :, nv - nu:nv], "v": Dr[:, :, nx - nu:nx], "u": Dr[:, :, nx:]}
    if cone:
        ncone = PN.cone_count(cons)
        cones = sig[:, :, nu:nu + 4 * ncone].reshape(STEPS, N, 4, ncone)
        kinds.update(cone0=cones[..., 0], cone_tangential=cones[..., 1:])      # (cone0: -fz > 0, a foot pulling on the ground)
    for name, x in kinds.items():
        assert (x != 0).any() and (x == 0).any(), (which, cone, name)
    # 1. against the referee
    out = run(r, o, which, cone)
    for name in ("G_traj", "rho_traj", "D_traj", "lx_traj", "lu_traj"):
        dist = G.distance(out[name], ref[name])
        print("%s %s %s: %.2e (bar %.0e)" % (which, cone, name, dist, BAR))
        assert dist <= BAR, (which, cone, name, dist)
    assert ((out["G_traj"][:, :, R:] != 0).any(axis=3) == (ref["G_traj"][:, :, R:] != 0).any(axis=3)).all()      # (the same rows are active)
    assert same(out["D_traj"], ref["D_traj"])
    # 2. the cost rows and A, B: the bits of the cost call
    costs = GN.linearize_cost(r, M, o, q, v, u, active, ts, dt, pts)
    assert same(out["A_traj"], costs["A_traj"]) and same(out["B_traj"], costs["B_traj"])
    assert same(out["G_traj"][:, :, :R], costs["G_traj"]) and same(out["rho_traj"][:, :, :R], costs["rho_traj"])
    assert G.distance(out["lu_traj"], costs["lu_traj"]) > 1e-3      # (the penalty is not small)
    # 3. mu = 0: zero rows, zero D, the cost call's gradients
    zero = run(r, o, which, cone, mu=0.0)
    assert (zero["G_traj"][:, :, R:] == 0).all() and (zero["rho_traj"][:, :, R:] == 0).all() and (zero["D_traj"] == 0).all()
    assert np.array_equal(zero["lx_traj"], costs["lx_traj"]) and np.array_equal(zero["lu_traj"], costs["lu_traj"])
    # ... and no row switched on
    off = capi.Constraints()
    oo = RS.Objective(r, cost, off, T0, dt, STEPS)
    none = PN.linearize_penalty(r, M, off, oo, MU, q, v, u, active, ts, dt, pts)
    Ro = r.lib.idocp_rbd_objective_constraint_rows(oo.h)
    assert Ro == (nu + 3) // 4 * 4 and (none["G_traj"][:, :, R:] == 0).all() and (none["D_traj"] == 0).all()
    assert np.array_equal(none["lx_traj"], costs["lx_traj"]) and np.array_equal(none["lu_traj"], costs["lu_traj"])
    # 4. a sample's bits whatever n, the outputs asked for and the form of the call
    one = run(r, o, which, cone, n=1)
    for name in PN.OUTPUTS:
        assert same(out[name][:, :1], one[name]), name
    for want in (("G_traj",), ("D_traj",), ("lx_traj", "rho_traj"), ("lu_traj", "A_traj")):
        part = run(r, o, which, cone, want=want)
        for name in want:
            assert same(part[name], out[name]), (want, name)
    dev = run(r, o, which, cone, device=True)
    for name in PN.OUTPUTS:
        assert same(dev[name], out[name]), name
    for x in (o, bare, oo):
        x.close()
    r.close()


@pytest.mark.parametrize("which,cone", [("anymal", "linearized"), ("chain2", None)])
def test_a_nan_stays_in_its_sample(which, cone):
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone, True)
    r = Rbd(mm)
    o = RS.Objective(r, cost, cons, T0, dt, STEPS)
    clean = run(r, o, which, cone)
    bad = q.copy()
    bad[2, 3, mm.nq - 1] = np.nan
    got = PN.linearize_penalty(r, M, cons, o, MU, bad, v, u, active, ts, dt, pts)
    for name in PN.OUTPUTS:
        want = clean[name].copy()
        want[2, 3] = np.nan
        assert same(got[name], want), name
    o.close()
    r.close()


def test_refusals():
    which, cone = "anymal", "linearized"
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone, True)
    r = Rbd(mm)
    o = RS.Objective(r, cost, cons, T0, dt, STEPS)
    sh = PN.output_shapes(mm, M, cons, STEPS, N)
    ok = {k: np.zeros(sh[k]) for k in PN.OUTPUTS}

    def refused(rc, who, text):
        assert rc == E_ARG and capi.last_error().startswith(who + ": ") and text in capi.last_error(), (rc, capi.last_error(), who, text)

    who = "idocp_rbd_linearize_rollout_penalty"
    call = lambda r_=r, o_=o, mu=MU: PN.linearize_penalty_raw(r_, o_, N, STEPS, active, ts, dt, u, pts, q, v, PN.penalty_struct(**ok), mu, False)      # noqa: E731
    assert call() == 0
    refused(call(mu=-1.0), who, "mu must be finite and non-negative")
    refused(call(mu=math.nan), who, "mu must be finite and non-negative")
    r2 = Rbd(mm)
    refused(call(r_=r2), who, "the objective was created on another handle")
    r2.close()
    crossed = capi.Constraints.from_buffer_copy(cons)
    crossed.a_min[3], crossed.a_max[3] = 1.0, -1.0
    oc = RS.Objective(r, cost, crossed, T0, dt, STEPS)
    refused(call(o_=oc), who, "the pair (a_min, a_max) of actuated joint 3 has lo > hi")
    sq = np.zeros(N)
    refused(PN.score_penalty_raw(r, oc, N, 0, STEPS, active, 0, q, v, u, a, f, sq), "idocp_rbd_score_penalty", "the pair (a_min, a_max) of actuated joint 3 has lo > hi")
    refused(PN.score_penalty_raw(r, o, N, 0, STEPS, active, 0, q, v, u, None, f, sq), "idocp_rbd_score_penalty", "a_traj is NULL")
    refused(PN.score_penalty_raw(r, o, N, 0, STEPS, active, 0, q, v, u, a, None, sq), "idocp_rbd_score_penalty", "f_traj is NULL")
    oc.close()
    o.close()
    r.close()


@pytest.mark.parametrize("which,cone", CASES)
def test_score_penalty(which, cone):
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone, True)
    r = Rbd(mm)
    o = RS.Objective(r, cost, cons, T0, dt, STEPS)
    sq = PN.score_penalty(r, o, q[:STEPS], v[:STEPS], u, a, f, active)
    want = referee(which, cone)["sq_violation"]
    rel = np.abs(sq - want).max() / np.abs(want).max()
    print("%s %s: sq_violation %s, |gpu - referee| / |referee| %.2e (bar 1e-11)" % (which, cone, sq, rel))
    assert (want > 0).all() and rel <= 1e-11
    # the squares are not the score's L1 violation, and both see the same rows
    _, l1, _ = RS.score(r, o, q, v, u, a, f, active, terminal=True, want_stage=False)
    assert (l1 > 0).all() and not np.allclose(l1, sq)
    # a synthetic force that pulls on the ground (fz < 0) on every other contact: against the rows of the score referee
    if cone:
        pull = f.copy()
        pull[:, :, ::2, 2] = -np.abs(pull[:, :, ::2, 2]) - 1.0
        got = PN.score_penalty(r, o, q[:STEPS], v[:STEPS], u, a, pull, active)
        want_pull = np.array([dt * 0.5 * math.fsum(max(0.0, g) ** 2 for k in range(STEPS)
                                                   for g in RS.constraint_rows(mm, cons, q[k, i], v[k, i], u[k, i], a[k, i], pull[k, i], list(active[k])))
                              for i in range(N)])
        rel = np.abs(got - want_pull).max() / np.abs(want_pull).max()
        print("%s %s: pulling feet, sq_violation %s, |gpu - rows of the score referee| %.2e (bar 1e-11)" % (which, cone, got, rel))
        assert not same(got, sq) and rel <= 1e-11
    # one call against two accumulated windows, and against n = 1
    first = PN.score_penalty(r, o, q[:3], v[:3], u[:3], a[:3], None if f is None else f[:3], None if active is None else active[:3])
    both = PN.score_penalty(r, o, q[3:STEPS], v[3:STEPS], u[3:], a[3:], None if f is None else f[3:], None if active is None else active[3:], first_step=3,
                            accumulate=first)
    assert same(both, sq) and not same(first, sq)
    one = PN.score_penalty(r, o, q[:STEPS, 2:3], v[:STEPS, 2:3], u[:, 2:3], a[:, 2:3], None if f is None else f[:, 2:3], active)
    assert same(one, sq[2:3])
    # a NaN stays in its sample
    bad = a.copy()
    bad[1, 4, mm.nv - 1] = np.nan
    got = PN.score_penalty(r, o, q[:STEPS], v[:STEPS], u, bad, f, active)
    assert np.isnan(got[4]) and same(got[:4], sq[:4])
    o.close()
    r.close()
