"""The cases of test_ocp_lqr_stage_gpu.py with the ORACLE in the kernels' place (no GPU): the condensed LQR stage of oracle::OCPSolver
(OracleOCP.stage(0, ...) then lqr_stage(i)) against the independent stage Lagrangian of ocp_lqr_cases.py, quantity by quantity at
ocp_stage_cases.BAR = 1e-11 under helpers.rel_err; the referee against itself (float64 against long double, and the error estimate of its
differenced SE(3) Jacobians) within a quarter of that bar; and the SENSITIVITY of the cases: every single-term mutation of the referee listed
in ocp_lqr_cases.MUTATIONS must move the oracle-referee distance to at least 1000 x the bar on at least one case -- the evidence that the
cases can see the errors they are meant for.

Observed (printed with -s): the oracle at most 1.2e-12 from the referee (Quu; Qxx, Qxu 1.1e-12), the referee 3.9e-13 from itself, the error estimate
of the differenced Jacobians 1.2e-17; the weakest mutation (J of the configuration difference) moves the referee 5.2e-5.  DESIGN.md section 6b has the row."""
import numpy as np
import pytest

import ocp_lqr_cases as L
import ocp_stage_cases as S
import rbd_cases as RC
from helpers import OracleOCP, P, arr

MODELS = S.MODELS
STATES = ("init", "updated")
ORACLE_FIELDS = tuple(f for f in L.SET_FIELDS if f != "nu_passive")      # (no setter on the oracle; nu_passive cannot enter a condensed stage)


def set_slot(o, slot, name, value):
    import ctypes as C
    o.lib.oracle_ocp_set_stage.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_double)]
    assert o.lib.oracle_ocp_set_stage(o.h, slot, name.encode(), P(arr(np.asarray(value).reshape(-1)))) == 0, name


def set_iterate(o, s, slots):
    """slots: [(slot, index into the iterate's arrays, terminal?)]"""
    for slot, p, terminal in slots:
        for name in ORACLE_FIELDS + (("xi",) if "xi" in s else ()):
            if not terminal or name in ("q", "v", "lmd", "gmm"):
                set_slot(o, slot, name, s[name][p])


def oracle_uniform(which, kind, mask, state):
    """(oracle handle linearised at the iterate, slack, dual) of a uniform case"""
    m, _, s = L.iterate(which)
    cost, cons = L.problem(m, kind)
    o = OracleOCP(m, cost, cons, L.N * L.DT, L.N)
    o.set_contact_status(mask, s["pts"])
    slots = [(i, i, i == L.N) for i in range(L.N + 1)]
    set_iterate(o, s, slots)
    o.init_constraints(L.T0)
    if state == "updated":
        assert o.update(L.T0, s["q_init"], s["v_init"]) == 0
        set_iterate(o, s, slots)
    assert o.stage(0, L.T0, s["q_init"], s["v_init"]) == 0
    return (m, cost, cons, o) + o.constraint_data()


def referee_uniform(which, kind, mask, slack, dual, T=L.LD, mutate=None, stages=range(L.N)):
    m, M, s = L.iterate(which)
    cost, cons = L.problem(m, kind)
    recs = L.rigid_body(which, mask)
    return [L.lqr_stage(m, M, cost, cons, recs[i], L.uniform_stage(s, i, mask), slack[i], dual[i], T, mutate) for i in stages]


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("kind", L.PROBLEMS)
@pytest.mark.parametrize("mask", RC.ALL_MASKS, ids=RC.mask_id)
@pytest.mark.parametrize("which", MODELS, ids=str)
def test_uniform_contact_sets(which, mask, kind, state):
    """all 16 contact sets on two models, both problems, both barrier states: the oracle within the bar, the referee within a quarter of it of itself"""
    m, cost, cons, o, slack, dual = oracle_uniform(which, kind, mask, state)
    if state == "init":      # the barrier state is the one the iterate was built for: near and bumped rows family by family, z / s over six decades
        L.check_barrier_construction(cons, m.nu, mask, slack, dual)
    else:                    # after the update the duality s z - eps of the rows is no longer zero
        live = slack[L.N - 1] > 0
        assert np.abs(slack[L.N - 1][live] * dual[L.N - 1][live] - cons.barrier).max() > 1e-6
    refs = referee_uniform(which, kind, mask, slack, dual)
    refs64 = referee_uniform(which, kind, mask, slack, dual, np.float64)
    worst = {}
    label = "%s %s %s %s" % (which, RC.mask_id(mask), kind, state)
    for i in range(L.N):
        L.check_referee(refs64[i], refs[i], "%s stage %d" % (label, i))
        L.hold(L.distances(o.lqr_stage(i), refs[i]), "%s, stage %d" % (label, i), worst)
    print("oracle %s: %s" % (label, L.summary(worst)))


def oracle_chain(which, kind, state):
    m, _, s = L.chain_iterate(which)
    cost, cons = L.problem(m, kind, L.CHAIN_T0)
    o = OracleOCP(m, cost, cons, S.CHAIN_T, S.CHAIN_N, max_num_impulse=S.CHAIN_EVENTS)
    S.build_chain(o, which)
    o.set_solution("q", s["q"][0]); o.set_solution("v", s["v"][0])
    o.init_constraints(L.CHAIN_T0)
    chain = o.chain(L.CHAIN_T0)
    assert [c["kind"] for c in chain[:-1]] == [k for k, _ in S.FORWARD_CHAIN] and chain[-1]["kind"] == "terminal"
    slots = [(c["slot"], p, c["kind"] == "terminal") for p, c in enumerate(chain)]
    set_iterate(o, s, slots)
    o.init_constraints(L.CHAIN_T0)
    if state == "updated":
        assert o.update(L.CHAIN_T0, s["q_init"], s["v_init"]) == 0
        set_iterate(o, s, slots)
    assert o.stage(0, L.CHAIN_T0, s["q_init"], s["v_init"]) == 0
    return (m, cost, cons, o, chain) + o.constraint_data()


def chain_stage(s, chain, p):
    """st of ocp_lqr_cases.lqr_stage for the grid stage at chain position p: its chain neighbours, its own time step and time"""
    c, mask = chain[p], S.FORWARD_CHAIN[p][1]
    return dict(dt=c["dt"], t=c["t"], level=c["index"], mask=mask, q=s["q"][p], v=s["v"][p], a=s["a"][p], f=s["f"][p], u=s["u"][p], beta=s["beta"][p], mu=s["mu"][p],
                q_next=s["q"][p + 1], v_next=s["v"][p + 1], q_prev=s["q"][p - 1] if p else s["q_init"], lmd=s["lmd"][p], gmm=s["gmm"][p],
                lmd_next=s["lmd"][p + 1], gmm_next=s["gmm"][p + 1])


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("kind", L.PROBLEMS)
@pytest.mark.parametrize("which", MODELS, ids=str)
def test_event_chain_grid_stages(which, kind, state):
    """the grid stages of the event chain of ocp_stage_cases: their time steps and chain neighbours (impulse, aux, lift) differ from the uniform case"""
    m, cost, cons, o, chain, slack, dual = oracle_chain(which, kind, state)
    _, M, s = L.chain_iterate(which)
    recs = L.rigid_body(which, None, True)
    assert len({round(chain[p]["dt"], 12) for p in recs}) > 1
    worst = {}
    for p, rec in recs.items():
        i = chain[p]["index"]
        st = chain_stage(s, chain, p)
        ref, ref64 = (L.lqr_stage(m, M, cost, cons, rec, st, slack[i], dual[i], T) for T in (L.LD, np.float64))
        label = "%s chain %s %s, position %d (stage %d)" % (which, kind, state, p, i)
        L.check_referee(ref64, ref, label)
        L.hold(L.distances(o.lqr_stage(chain[p]["slot"]), ref), label, worst)
    print("oracle %s chain %s %s: %s" % (which, kind, state, L.summary(worst)))


@pytest.mark.parametrize("kind", L.PROBLEMS)
@pytest.mark.parametrize("which", MODELS, ids=str)
def test_terminal_stage(which, kind):
    """P[N] = the terminal cost's Gauss-Newton Hessian (its qq and vv blocks) and s[N] = MINUS its gradient (ocp_riccati_kernel.hip: `s = -lx` of the
    terminal stage; riccati_recursion_solver.cpp:53-56), after a full direction"""
    mask = (1, 0, 1, 1)
    m, cost, cons, o, slack, dual = oracle_uniform(which, kind, mask, "init")
    assert o.stage(1, L.T0, L.iterate(which)[2]["q_init"], L.iterate(which)[2]["v_init"]) == 0
    Pm, sv, _, _ = o.riccati()
    L.hold_terminal(which, kind, Pm[L.N], sv[L.N], "oracle %s %s" % (which, kind))


SENSITIVITY_CASES = [("anymal", (1, 1, 1, 1), "limits", "init"), ("anymal", (1, 0, 0, 1), "accel", "init"), (1, (0, 1, 1, 1), "accel", "updated"),
                     ("anymal", (0, 0, 1, 0), "limits", "updated")]


@pytest.fixture(scope="module")
def oracle_cases():
    out = []
    for which, mask, kind, state in SENSITIVITY_CASES:
        m, cost, cons, o, slack, dual = oracle_uniform(which, kind, mask, state)
        out.append((which, mask, kind, slack, dual, [o.lqr_stage(i) for i in range(L.N)]))
    return out


@pytest.mark.parametrize("mutation", L.MUTATIONS)
def test_sensitivity_to_single_term_mutations(oracle_cases, mutation):
    """a referee with ONE term wrong is at least 1000 x the bar from the oracle on at least one case (and the unmutated one within the bar on all:
    test_uniform_contact_sets): a kernel with that term wrong cannot pass the GPU test"""
    worst, where = 0.0, None
    for which, mask, kind, slack, dual, got in oracle_cases:
        refs = referee_uniform(which, kind, mask, slack, dual, np.float64, mutation)
        for i in range(L.N):
            for name, (d, _) in L.distances(got[i], refs[i]).items():
                if d > worst:
                    worst, where = d, (which, RC.mask_id(mask), kind, i, name)
    print("mutation %s: distance %.1e at %s" % (mutation, worst, where))
    assert worst >= 1000 * L.BAR, (mutation, worst)
