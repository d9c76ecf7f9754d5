"""The stage terms with frame Jacobians of their own as the kernels leave them on the device -- the ext record of ocp_ext_kernel read with
idocp_ocp_get_ext_terms at EVERY chain position (frame heights, ContactDistance rows and weights, task rows and weights, the gradient share, cost, violation,
KKT error), what ocp_ext_hessian_kernel and the condensation add of it to the condensed stage (idocp_ocp_get_lqr_stage) and to the terminal record (P[N],
s[N] of idocp_ocp_get_riccati), and the slack and dual ocp_ext_init_kernel leaves -- against the INDEPENDENT referee of ocp_ext_cases.py, without the oracle
in between, quantity by quantity at ocp_stage_cases.BAR = 1e-11 under helpers.rel_err.  test_ocp_ext_terms_host.py holds the referee to itself, runs the
oracle's condensed stage on the same cases and shows that the cases see single-term errors.

What is reached: LeggedDims<4, 3> (the only instantiation of the three kernels) on ANYmal in the specialised and the general leg sweep and on
other_quadruped(1); the problems "task" (all four component slots: 6D time-varying on the base, 3D thigh, 6D shank, 3D foot), "task2" (two components,
the unused slots exactly zero) and "distance" (masks all down, one up, diagonal pair, three up, flight); node kinds grid, impulse (task_weighti), aux, lift
and terminal on the event chain of ocp_stage_cases, ParNMPC's stages with its last one (stage and terminal weight together) and the refusal of its
placeholder; the barrier states right after init_constraints and after one update; one handle whose instances hold different configurations; instances with
equal inputs agree bit for bit; the condensed stage and P[N], s[N] on all three problems ("distance" too: Jc^T w Jc and the rows' share of lq are in the
record, observed Qxx 3.8e-13, lx 3.0e-15); the fixed-base terminal form (taskSpaceColumn, dev_task.hpp) on UnOCPSolver: iiwa14 and chains of 2 and 8
joints, 3D and 6D, the frame on the last and on a middle joint.  ParNMPC runs "distance" too (rows on stage 1 and on the last stage, observed lq 3.3e-15).  Not reached: the stage form of the
fixed-base cost (ocp_ext_cases: why).

A failure names case, instance, position, quantity and worst row; the worst distance per quantity is printed (-s)."""
import ctypes as C

import numpy as np
import pytest

import ocp_ext_cases as X
import ocp_lqr_cases as L
import ocp_stage_cases as S
import rbd_cases as RC
from helpers import HipOCP, HipParNMPC, HipUnOCP, P
from idocp_amd import capi
from test_ocp_lqr_stage_gpu import SWEEPS, SWEEP_IDS, STATES, linearise, set_chain, set_stages, solver

TASK_MASK, hold_terminal = X.TASK_MASK, X.hold_terminal

pytestmark = pytest.mark.gpu


def cases():
    return [(kind, TASK_MASK) for kind in ("task", "task2")] + [("distance", mask) for mask in X.DISTANCE_MASKS]


CASE_IDS = ["%s-%s" % (k, RC.mask_id(mk)) for k, mk in cases()]


def set_refs(g, which, kind, t0):
    """the poses of the time-varying first component at the times the handle reports (idocp_ocp_get_chain_times -> idocp_ocp_set_task_refs)"""
    times = g.chain_times(t0)
    if kind == "task":
        pose = X.task_pose(which, kind, t0)
        g.set_task_refs(t0, np.array([pose(t) for t in times]))
    return times


def cd_rows(g, cons, nu, b):
    """slack and dual [N][4] of the ContactDistance rows of instance b (zeros without the constraint)"""
    if not cons.contact_distance:
        return np.zeros((g.N, 4)), np.zeros((g.N, 4))
    at = L.families(cons, nu)[0]["cd"]
    slack, dual = g.constraint_data(b)
    return slack[:, at], dual[:, at]


def hold_records(g, label, M, cost, cons, nodes, qs, pose, rows, worst, stage_of=None):
    """every node of every instance against the referee (computed once: the instances hold equal inputs), and bit for bit against instance 0"""
    first = {}
    for b in range(g.batch):
        slack, dual = rows(b)
        for p, node in enumerate(nodes):
            where = "%s, instance %d, position %d (%s)" % (label, b, p, node["kind"])
            got = X.device_record(g, b, p)
            if b == 0:
                i = stage_of(p) if stage_of else p
                on = node["kind"] == "stage" and i < len(slack)
                first[p] = (got, X.ext_record(M, cost, cons, node, qs[p], slack[i] if on else None, dual[i] if on else None, pose=pose))
            X.hold(X.distances(got, first[p][1]), where, worst)
            assert all(np.array_equal(got[k], first[p][0][k]) for k in X.QUANTITIES), where + ": differs from instance 0 on the same inputs"
    return first


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("kind,mask", cases(), ids=CASE_IDS)
@pytest.mark.parametrize("which,sweep", SWEEPS, ids=SWEEP_IDS)
def test_uniform_handle(monkeypatch, which, sweep, kind, mask, state):
    """the ext record of the N grid stages and the terminal node, the condensed stage and P[N], s[N] ("task", "task2"), the rows init_constraints leaves"""
    m, M, s = X.iterate(which, kind)
    cost, cons = X.problem(m, M, which, kind)
    g = solver(monkeypatch, m, sweep, cost, cons, L.N * L.DT, L.N)
    g.set_contact_status(mask, s["pts"])
    set_refs(g, which, kind, L.T0)
    set_stages(g, s, L.N)
    g.init_constraints(L.T0)
    label = "%s %s %s %s %s" % (which, sweep, kind, RC.mask_id(mask), state)
    if kind == "distance" and state == "init":      # ocp_ext_init_kernel: s = the height pushed up to the barrier, dual = barrier / s, from level 2 on
        sl, du = cd_rows(g, cons, m.nu, 0)
        ref = np.array([X.init_slack_dual(z, cons.barrier) for z in RC.feet(M, s["q"][2])[:, 2]])
        assert not sl[:2].any() and not du[:2].any(), label
        # (the dual against barrier / the handle's OWN slack: that is the rule, and a bumped slack of 1e-4 turns the 2e-15 the height is rounded by into
        #  1e-11 of barrier / s -- held against the referee's slack the rule would be charged with the rounding of the kinematics)
        X.hold({"slack": S.worst_row(sl[2], ref[:, 0]), "dual": S.worst_row(du[2], cons.barrier / sl[2])}, label + ", init_constraints")
        assert L.BAR < cons.barrier and cons.barrier <= sl[2][1] < 2 * cons.barrier, sl[2]      # the foot below the ground was bumped
    if state == "updated":
        assert g.update(L.T0, s["q_init"], s["v_init"]) == 0, capi.lib().idocp_last_error()
        set_stages(g, s, L.N)
    linearise(g, s["q_init"], s["v_init"])
    pose, nodes, worst = X.task_pose(which, kind, L.T0), X.uniform_nodes(mask), {}
    first = hold_records(g, label, M, cost, cons, nodes, s["q"], pose, lambda b: cd_rows(g, cons, m.nu, b), worst)
    if kind == "distance" and all(mask):      # every row idles: exactly zero
        assert all(not first[p][0][k].any() for p in first for k in ("Jc", "w", "lq")), label
    if kind == "task2":
        assert all(not first[p][0]["JJ"][12:].any() and not first[p][0]["tw"][12:].any() for p in first), label + ": unused slots"
    print("%s: %s" % (label, X.summary(worst)))
    # ---- the terms are ADDED into the records: the condensed grid stages, then P[N], s[N] after a full direction
    recs, worst = X.rigid_body(which, kind, tuple(mask)), {}
    slack, dual = g.constraint_data(0)
    for i in range(L.N):
        ref = L.lqr_stage(m, M, cost, cons, recs[i], L.uniform_stage(s, i, mask), slack[i], dual[i], ext=first[i][1])
        for b in range(L.BATCH):
            L.hold(L.distances(g.lqr_stage(i, b), ref), "%s, instance %d, condensed stage %d" % (label, b, i), worst)
    print("%s condensed: %s" % (label, L.summary(worst)))
    if state == "init":
        rc = g.lib.idocp_ocp_compute_direction(g.h, L.T0, P(g._bc(s["q_init"], g.nq)), P(g._bc(s["v_init"], g.nv)))
        assert rc == 0, capi.lib().idocp_last_error()
        for b in range(L.BATCH):
            Pm, sv, _, _ = g.riccati(b)
            hold_terminal(which, kind, Pm[L.N], sv[L.N], "%s, instance %d" % (label, b))


@pytest.mark.parametrize("kind", X.PROBLEMS)
@pytest.mark.parametrize("which,sweep", SWEEPS, ids=SWEEP_IDS)
def test_event_chain(monkeypatch, which, sweep, kind):
    """every node kind: grid, impulse (its own weights, no dt), aux, lift (regular stages, constraint level 0: no ContactDistance rows) and terminal"""
    m, M, s = X.iterate(which, kind, True)
    cost, cons = X.problem(m, M, which, kind, L.CHAIN_T0)
    g = solver(monkeypatch, m, sweep, cost, cons, S.CHAIN_T, S.CHAIN_N, S.CHAIN_EVENTS)
    S.build_chain(g, which)
    times = set_refs(g, which, kind, L.CHAIN_T0)
    g.set_solution("q", s["q"][0]); g.set_solution("v", s["v"][0])
    g.init_constraints(L.CHAIN_T0)
    chain = g.chain(L.CHAIN_T0)
    assert [c["kind"] for c in chain] == [k for k, _ in S.FORWARD_CHAIN] + ["terminal"]
    set_chain(g, s, len(chain))
    g.init_constraints(L.CHAIN_T0)
    linearise(g, s["q_init"], s["v_init"])
    nodes, worst = X.chain_nodes(chain, times), {}
    label = "%s %s chain %s" % (which, sweep, kind)
    first = hold_records(g, label, M, cost, cons, nodes, s["q"], X.task_pose(which, kind, L.CHAIN_T0), lambda b: cd_rows(g, cons, m.nu, b), worst,
                         stage_of=lambda p: chain[p]["index"])
    if kind == "distance":
        live = [p for p in first if first[p][0]["w"].any()]
        assert live == [p for p, c in enumerate(chain) if c["kind"] == "stage" and c["index"] >= 2 and not all(nodes[p]["mask"])] and live, live
    print("%s: %s" % (label, X.summary(worst)))


@pytest.mark.parametrize("kind", X.PROBLEMS)
@pytest.mark.parametrize("which", S.MODELS, ids=str)
def test_parnmpc_handle(which, kind):
    """ParNMPC's stages: stage i at t + (i + 1) dt, the last one with dt w + w_f in the weights and dt w alone in `cost`; the placeholder is refused"""
    m, M, s = X.iterate(which, kind)
    t0 = L.T0 - L.DT      # (stage i then sits at ocp_lqr_cases' time of stage i)
    cost, cons = X.problem(m, M, which, kind, t0)
    g = HipParNMPC(m, cost, cons, L.N * L.DT, L.N, batch=L.BATCH)
    g.set_contact_status(TASK_MASK, s["pts"])
    times = set_refs(g, which, kind, t0)
    assert len(times) == L.N + 1 and np.allclose(times[:L.N], t0 + L.DT * np.arange(1, L.N + 1), atol=1e-12), times
    for name in L.SET_FIELDS:
        g.set_stage_values(name, L.stage_arrays(s, name)[:L.N])
    g.init_constraints(t0)
    lib, bufs = capi.lib(), []
    for x, dim in ((s["q_init"], g.nq), (s["v_init"], g.nv)):
        x, d = g._bc(x, dim), C.c_void_p()
        capi.check(lib.idocp_device_alloc(C.byref(d), x.nbytes))
        capi.check(lib.idocp_device_upload(d, x.ctypes.data, x.nbytes))
        bufs.append(d)
    try:
        for phase in (0, 1):
            capi.check(lib.idocp_parnmpc_launch_phase(g.h, phase, *bufs), "launch_phase %d" % phase)
        capi.check(lib.idocp_ocp_synchronize(g.h), "synchronize")
    finally:
        for d in bufs:
            lib.idocp_device_free(d)
    nodes, worst = X.uniform_nodes(TASK_MASK, t0, backward=True), {}
    label = "%s parnmpc %s" % (which, kind)
    first = hold_records(g, label, M, cost, cons, nodes, s["q"], X.task_pose(which, kind, t0), lambda b: cd_rows(g, cons, m.nu, b), worst)
    if kind == "distance":      # the rows live from level 2 on: ParNMPC's stage 1 (its iterate is not posed over the ground) and its last stage (posed)
        assert [p for p in first if first[p][0]["w"].any()] == [1, 2] and first[2][0]["violation"][0] > 0.5 * L.DT * 0.02, label
    else:
        assert S.worst_row(first[L.N - 1][0]["tw"], first[L.N - 2][0]["tw"])[0] > 1000 * L.BAR      # the last stage carries w_f
    one = np.zeros(g.nv)      # every array is nullable on its own: one quantity alone
    capi.check(lib.idocp_ocp_get_ext_terms(g.h, 0, L.N - 1, None, None, None, None, None, P(one), None, None, None), "get_ext_terms, lq alone")
    assert np.array_equal(one, first[L.N - 1][0]["lq"]), label
    print("%s: %s" % (label, X.summary(worst)))
    for (b, p), text in (((0, -1), b"position"), ((L.BATCH, 0), b"instance"), ((0, L.N), b"placeholder")):
        assert lib.idocp_ocp_get_ext_terms(g.h, b, p, *[None] * 9) == -1 and text in lib.idocp_last_error(), (b, p, lib.idocp_last_error())


def test_handle_without_ext_record_is_refused():
    m, _, s = L.iterate("anymal")
    cost, cons = L.problem(m, "limits")
    g = HipOCP(m, cost, cons, L.N * L.DT, L.N, batch=1)
    assert g.lib.idocp_ocp_get_ext_terms(g.h, 0, 0, *[None] * 9) == -1 and b"no ext record" in g.lib.idocp_last_error()


@pytest.mark.parametrize("which,sweep", SWEEPS, ids=SWEEP_IDS)
def test_instances_with_different_inputs(monkeypatch, which, sweep):
    """idocp_ocp_set_solution_batch for q: every stage of instance b holds configuration b; each instance is held to ITS OWN answer"""
    kind, mask = "task", TASK_MASK
    m, M, s = X.iterate(which, kind)
    cost, cons = X.problem(m, M, which, kind)
    g = solver(monkeypatch, m, sweep, cost, cons, L.N * L.DT, L.N)
    g.set_contact_status(mask, s["pts"])
    set_refs(g, which, kind, L.T0)
    set_stages(g, s, L.N)
    g.set_solution_batch("q", np.asarray(s["q"][:L.BATCH]))
    g.init_constraints(L.T0)
    linearise(g, s["q_init"], s["v_init"])
    pose, worst = X.task_pose(which, kind, L.T0), {}
    for b in range(L.BATCH):
        for p, node in enumerate(X.uniform_nodes(mask)):
            ref = X.ext_record(M, cost, cons, node, s["q"][b], pose=pose)
            X.hold(X.distances(X.device_record(g, b, p), ref), "%s %s per-instance inputs, instance %d, position %d" % (which, sweep, b, p), worst)
    print("%s %s per-instance inputs: %s" % (which, sweep, X.summary(worst)))


@pytest.mark.parametrize("arm,dim,where", X.FIXED_CASES, ids=X.FIXED_IDS)
def test_fixed_base_terminal_stage(arm, dim, where):
    """taskSpaceColumn (dev_task.hpp) on UnOCPSolver: P[N], s[N] of idocp_unocp_get_riccati against the terminal weights plus JJ^T W_f JJ and
    JJ^T W_f diff; the frame on the last joint and on a middle one (the columns behind it exactly zero)"""
    m, M, cost, cons, joint, it = X.fixed_case(arm, dim, where)
    g = HipUnOCP(m, cost, cons, L.N * L.DT, L.N, batch=L.BATCH)
    for name in ("q", "v"):
        g.set_solution(name, it[name])
    g.launch(0, it["q"], it["v"])
    g.launch(1, it["q"], it["v"])
    first = None
    for b in range(L.BATCH):
        Pm, sv, _, _ = g.riccati(b)
        X.hold_fixed_terminal(arm, dim, where, Pm[L.N], sv[L.N], "fixed base %s %dD %s, instance %d" % (arm, dim, where, b))
        first = first or (Pm[L.N], sv[L.N])
        assert np.array_equal(Pm[L.N], first[0]) and np.array_equal(sv[L.N], first[1]), "instance %d differs from instance 0 on the same inputs" % b
