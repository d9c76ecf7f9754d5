"""The condensed LQR stage the kernels leave on the device -- idocp_ocp_get_lqr_stage after idocp_ocp_launch_kernel ids 0 and 1 (the tangent RNEA and
ocp_condense_kernel: cost and barrier assembly, the state-equation rows on SE(3), and the back half of the condensation behind MJtJinv) -- against the
INDEPENDENT stage Lagrangian of ocp_lqr_cases.py, without the oracle in between: the upper triangle of Qxx (the block below it is written by the sweep),
Qxu, Quu, A, B, lx, lu, Fx, quantity by quantity at ocp_stage_cases.BAR = 1e-11 under helpers.rel_err.  test_ocp_lqr_stage_host.py runs the same cases on
the oracle, holds the referee to itself and shows that the cases see single-term errors.

What is reached: all 16 contact sets uniform over a three-stage horizon (ocp_lqr_cases: why three), batch 3, on ANYmal in the specialised and, through
IDOCP_GENERAL_AXES, the general leg sweep and on other_quadruped(1) -- OcpLaunch::condense with DIMF = 12 and general, condenseMixed with the plain 6 class
and the flight class; two problems per set (six joint limits + linearised cone + trotting reference | nonlinear cone + both acceleration limits +
time-varying reference) in two barrier states each (right after init_constraints with rows 1e-3 inside and beyond their bounds | after one
update_solution, the iterate set again); the grid stages of the event chain of ocp_stage_cases (stage 0 on the EVENTS class; time steps and chain neighbours
differ); one handle whose three instances hold DIFFERENT inputs, each held to its own answer; the terminal stage through P[N], s[N] of idocp_ocp_get_riccati.
The slack and the dual of every row are read from the handle under test (get_constraint_data): they are state, not arithmetic of the stage.  The impulse, aux
and lift positions cannot be reached through idocp_ocp_get_lqr_stage and are out of scope.

Instances that hold equal inputs agree bit for bit; a failure names the case, the instance, the stage, the quantity and the worst row; the worst distance
per quantity is printed (-s)."""
import ctypes as C

import numpy as np
import pytest

import ocp_lqr_cases as L
import ocp_stage_cases as S
import rbd_cases as RC
from helpers import HipOCP, P, arr
from idocp_amd import capi

pytestmark = pytest.mark.gpu
SWEEPS = (("anymal", "xyy"), ("anymal", "general"), (1, "general"))
SWEEP_IDS = ["%s-%s" % x for x in SWEEPS]
STATES = ("init", "updated")


def solver(monkeypatch, m, sweep, cost, cons, T, N, events=0):
    if sweep == "general" and m.nv == 18:
        monkeypatch.setenv("IDOCP_GENERAL_AXES", "1")      # (read when the handle is created)
    return HipOCP(m, cost, cons, T, N, batch=L.BATCH, max_num_impulse=events)


def set_stages(g, s, n):
    for name in L.SET_FIELDS:
        x = L.stage_arrays(s, name, n)
        capi.check(g.lib.idocp_ocp_set_solution_stages(g.h, name.encode(), len(x), P(arr(x))), "set " + name)


def set_chain(g, s, n):
    for name in L.SET_FIELDS + ("xi",):      # (xi back to zero: ocp_lqr_cases, out of scope)
        k = n if name in ("q", "v", "lmd", "gmm") else n - 1
        capi.check(g.lib.idocp_ocp_set_solution_chain(g.h, name.encode(), k, P(arr(np.asarray(s[name][:k]).reshape(k, -1)))), "set %s along the chain" % name)


def linearise(g, q0, v0):
    """idocp_ocp_launch_kernel ids 0 and 1 at the initial state q0, v0 ([nq] for every instance, or [batch][nq])"""
    lib, bufs = capi.lib(), []
    for x, dim in ((q0, g.nq), (v0, g.nv)):
        x, d = g._bc(x, dim), C.c_void_p()
        capi.check(lib.idocp_device_alloc(C.byref(d), x.nbytes))
        capi.check(lib.idocp_device_upload(d, x.ctypes.data, x.nbytes))
        bufs.append(d)
    try:
        for kid in (0, 1):
            capi.check(lib.idocp_ocp_launch_kernel(g.h, kid, *bufs), "launch_kernel %d" % kid)
        capi.check(lib.idocp_ocp_synchronize(g.h), "synchronize")
    finally:
        for d in bufs:
            lib.idocp_device_free(d)


def prepare(g, s, t0, state, setter, n):
    setter(g, s, n)
    g.init_constraints(t0)
    if state == "updated":
        assert g.update(t0, s["q_init"], s["v_init"]) == 0, capi.lib().idocp_last_error()
        setter(g, s, n)
    linearise(g, s["q_init"], s["v_init"])


def same_bits(a, b):
    return all(np.array_equal(np.triu(x) if k == 0 else x, np.triu(y) if k == 0 else y) for k, (x, y) in enumerate(zip(a, b)))


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("kind", L.PROBLEMS)
@pytest.mark.parametrize("mask", RC.ALL_MASKS, ids=RC.mask_id)
@pytest.mark.parametrize("which,sweep", SWEEPS, ids=SWEEP_IDS)
def test_uniform_contact_sets(monkeypatch, which, sweep, mask, kind, state):
    m, M, s = L.iterate(which)
    cost, cons = L.problem(m, kind)
    g = solver(monkeypatch, m, sweep, cost, cons, L.N * L.DT, L.N)
    g.set_contact_status(mask, s["pts"])
    prepare(g, s, L.T0, state, set_stages, L.N)
    recs = L.rigid_body(which, mask)
    data = [g.constraint_data(b) for b in range(L.BATCH)]
    label = "%s %s %s %s %s" % (which, sweep, RC.mask_id(mask), kind, state)
    if state == "init":      # the handle's barrier state is the one the iterate was built for (near and bumped rows, family by family)
        L.check_barrier_construction(cons, m.nu, mask, *data[0])
    worst, first = {}, None
    for b, (slack, dual) in enumerate(data):
        assert np.array_equal(slack, data[0][0]) and np.array_equal(dual, data[0][1]), "%s: the barrier state of instance %d differs from instance 0" % (label, b)
        got = [g.lqr_stage(i, b) for i in range(L.N)]
        if first is None:
            first = got
            refs = [L.lqr_stage(m, M, cost, cons, recs[i], L.uniform_stage(s, i, mask), slack[i], dual[i]) for i in range(L.N)]
        for i in range(L.N):
            where = "%s, instance %d, stage %d" % (label, b, i)
            L.hold(L.distances(got[i], refs[i]), where, worst)
            assert same_bits(got[i], first[i]), where + ": differs from instance 0 on the same inputs"
    print("%s: %s" % (label, L.summary(worst)))


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("kind", L.PROBLEMS)
@pytest.mark.parametrize("which,sweep", SWEEPS, ids=SWEEP_IDS)
def test_event_chain_grid_stages(monkeypatch, which, sweep, kind, state):
    """OcpLaunch::condenseMixed on the chain with every node kind: the grid stages (stage 0 carries the switching constraint: the EVENTS class)"""
    m, M, s = L.chain_iterate(which)
    cost, cons = L.problem(m, kind, L.CHAIN_T0)
    g = solver(monkeypatch, m, sweep, cost, cons, S.CHAIN_T, S.CHAIN_N, S.CHAIN_EVENTS)
    S.build_chain(g, which)
    g.set_solution("q", s["q"][0]); g.set_solution("v", s["v"][0])
    g.init_constraints(L.CHAIN_T0)
    chain = g.chain(L.CHAIN_T0)
    times = g.chain_times(L.CHAIN_T0)
    assert [(c["kind"], c["dimf"]) for c in chain[:-1]] == [(k, S.dimf_of(mk)) for k, mk in S.FORWARD_CHAIN] and chain[-1]["kind"] == "terminal"
    assert chain[0]["sw_dimi"] == 6
    prepare(g, s, L.CHAIN_T0, state, set_chain, len(chain))
    recs = L.rigid_body(which, None, True)
    assert len({round(chain[p]["dt"], 12) for p in recs}) > 1
    data = [g.constraint_data(b) for b in range(L.BATCH)]
    worst, first = {}, {}
    for b, (slack, dual) in enumerate(data):
        assert np.array_equal(slack, data[0][0]) and np.array_equal(dual, data[0][1])
        for p, rec in recs.items():
            c, i = chain[p], chain[p]["index"]
            where = "%s %s chain %s %s, instance %d, position %d (stage %d)" % (which, sweep, kind, state, b, p, i)
            got = g.lqr_stage(c["slot"], b)
            if b == 0:
                st = dict(dt=c["dt"], t=times[p], level=i, mask=S.FORWARD_CHAIN[p][1], q=s["q"][p], v=s["v"][p], a=s["a"][p], f=s["f"][p], u=s["u"][p], beta=s["beta"][p],
                          mu=s["mu"][p], q_next=s["q"][p + 1], v_next=s["v"][p + 1], q_prev=s["q"][p - 1] if p else s["q_init"], lmd=s["lmd"][p], gmm=s["gmm"][p],
                          lmd_next=s["lmd"][p + 1], gmm_next=s["gmm"][p + 1])
                first[p] = (got, L.lqr_stage(m, M, cost, cons, rec, st, slack[i], dual[i]))
            L.hold(L.distances(got, first[p][1]), where, worst)
            assert same_bits(got, first[p][0]), where + ": differs from instance 0 on the same inputs"
    print("%s %s chain %s %s: %s" % (which, sweep, kind, state, L.summary(worst)))


@pytest.mark.parametrize("which,sweep", SWEEPS, ids=SWEEP_IDS)
def test_instances_with_different_inputs(monkeypatch, which, sweep):
    """idocp_ocp_set_solution_batch for q, v, a, u (every stage of instance b holds sample b) and a different (q, v) per instance at the launch: each
    instance is held to ITS OWN referee answer -- an instance that read its neighbour's iterate or record would not be.  What this case cannot see:
    the setter gives an instance ONE q for all its stages, so q+ = q and the SE(3) blocks of the state equation are trivial here but for the q- term
    of stage 0 (they are held by the other tests); and the v of the launch enters no quantity of this record (Fv- contributes -gmm only), so of the
    per-instance initial state only q is observed."""
    mask, kind = (1, 1, 0, 1), "limits"
    m, M, s = L.iterate(which)
    cost, cons = L.problem(m, kind)
    g = solver(monkeypatch, m, sweep, cost, cons, L.N * L.DT, L.N)
    g.set_contact_status(mask, s["pts"])
    set_stages(g, s, L.N)
    for name in ("q", "v", "a", "u"):
        g.set_solution_batch(name, np.asarray(s[name][:L.BATCH]))
    g.init_constraints(L.T0)
    q0 = np.array([s["q"][(b + 1) % L.BATCH] for b in range(L.BATCH)])
    q0[0] = s["q_init"]
    v0 = np.array([s["v"][(b + 2) % L.BATCH] for b in range(L.BATCH)])
    linearise(g, q0, v0)
    worst = {}
    for b in range(L.BATCH):
        slack, dual = g.constraint_data(b)
        for i in range(L.N):
            st = L.uniform_stage(s, i, mask)
            st.update(q=s["q"][b], v=s["v"][b], a=s["a"][b], u=s["u"][b], q_next=s["q"][b], v_next=s["v"][b], q_prev=s["q"][b] if i else q0[b])
            rec = S.referee_record(M, st["q"], st["v"], st["a"], st["f"], st["u"], s["pts"], L.DT, mask, "stage")
            ref = L.lqr_stage(m, M, cost, cons, rec, st, slack[i], dual[i])
            L.hold(L.distances(g.lqr_stage(i, b), ref), "%s %s per-instance inputs, instance %d, stage %d" % (which, sweep, b, i), worst)
    print("%s %s per-instance inputs: %s" % (which, sweep, L.summary(worst)))


@pytest.mark.parametrize("kind", L.PROBLEMS)
@pytest.mark.parametrize("which,sweep", SWEEPS, ids=SWEEP_IDS)
def test_terminal_stage(monkeypatch, which, sweep, kind):
    """After a full idocp_ocp_compute_direction P[N] is the terminal cost's Gauss-Newton Hessian (its qq and vv blocks) and s[N] MINUS its gradient, the
    costate terms included (ocp_riccati_kernel.hip, terminal stage: `s = -lx`; riccati_recursion_solver.cpp:53-56)"""
    m, M, s = L.iterate(which)
    cost, cons = L.problem(m, kind)
    g = solver(monkeypatch, m, sweep, cost, cons, L.N * L.DT, L.N)
    g.set_contact_status((1, 0, 1, 1), s["pts"])
    set_stages(g, s, L.N)
    g.init_constraints(L.T0)
    rc = g.lib.idocp_ocp_compute_direction(g.h, L.T0, P(g._bc(s["q_init"], g.nq)), P(g._bc(s["v_init"], g.nv)))
    assert rc == 0, capi.lib().idocp_last_error()
    for b in range(L.BATCH):
        Pm, sv, _, _ = g.riccati(b)
        L.hold_terminal(which, kind, Pm[L.N], sv[L.N], "%s %s %s, instance %d" % (which, sweep, kind, b))
