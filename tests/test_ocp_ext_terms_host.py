"""The cases of test_ocp_ext_terms_gpu.py without a GPU: the referee of ocp_ext_cases.py (task-space components, ContactDistance rows) against itself --
float64 against long double within a quarter of ocp_stage_cases.BAR = 1e-11, the error estimate of its differenced Jlog6 likewise --; the ORACLE's condensed
stage and terminal stage (oracle::OCPSolver, lqr_stage / riccati) against ocp_lqr_cases.lqr_stage / terminal_stage with the referee's ext terms added, at the
bar; the evidence that the cases tell the LOCAL row of ContactDistance from the derivative of the world height; and the SENSITIVITY of the cases: every
single-term mutation of ocp_ext_cases.MUTATIONS moves a quantity of the record at least 1000 x the bar away from the ORACLE's record on at least one node
(the kernels are held to the unmutated referee within the bar, so a kernel with that term wrong cannot pass the GPU test).

The oracle's UN-CONDENSED read (oracle_ocp_get_ext_terms / oracle_parnmpc_get_ext_terms: z, Jc, w, JJ, tw, lq, cost, violation, kkt_error of one chain
position, row by row) is held per node at the bar on the same cases: the uniform handles of OCPSolver (all three problems, the five masks of "distance") and
of ParNMPCSolver (its last stage with stage and terminal weight together), and every node of the event chain (grid, impulse, aux, lift, terminal), where the
referee is also held to itself.  The mutations are measured against the oracle's records, not against the unmutated referee.  The slack and dual of the
ContactDistance rows are the oracle's own (state).  Its fixed-base solver (oracle::UnOCPSolver on ocp_ext_cases.FIXED_CASES) is held through P[N], s[N].

Observed (printed with -s): the referee at most 3.0e-13 from itself (the terminal stage with the task terms; the record 1.2e-13, JJ), the error estimate of the
differenced Jlog6 at most 5.8e-16; the oracle's condensed stage at most 4.5e-14 from the referee (A), its terminal stage 3.7e-15; the local and the world row
differ by 0.43 .. 1.7 on the cases; the oracle's un-condensed records at most 1.5e-15 (JJ) from the referee on every node of the uniform, ParNMPC and event-chain cases; the weakest
mutation (reference at the previous stage's time) is 2.2e-1 from the oracle.  On the MI355X
(test_ocp_ext_terms_gpu.py): the ext record at most 3.5e-15 (lq; JJ 1.4e-15), the condensed stage 2.6e-14 (Qxx), P[N] 2.6e-15, s[N] 2.0e-16.  DESIGN.md
section 6b has the row."""
import functools

import numpy as np
import pytest

import ocp_ext_cases as X
import ocp_lqr_cases as L
import ocp_stage_cases as S
import rbd_cases as RC
from helpers import OracleOCP, OracleParNMPC, OracleUnOCP
from test_ocp_lqr_stage_host import set_iterate

MODELS = S.MODELS
TASK_MASK, hold_terminal = X.TASK_MASK, X.hold_terminal


def init_rows(M, node, q, eps):
    """slack and dual of the four ContactDistance rows right after init_constraints, by the rule (ocp_ext_cases.init_slack_dual)"""
    z = RC.feet(M, q)[:, 2]
    return tuple(np.array(x) for x in zip(*[X.init_slack_dual(zc, eps) for zc in z]))


def uniform_records(which, kind, mask, backward, T, mutate=None):
    m, M, s = X.iterate(which, kind)
    cost, cons = X.problem(m, M, which, kind)
    pose = X.task_pose(which, kind, X.T0)
    out = []
    for i, node in enumerate(X.uniform_nodes(mask, backward=backward)):
        slack, dual = init_rows(M, node, s["q"][i], cons.barrier)
        out.append(X.ext_record(M, cost, cons, node, s["q"][i], slack, dual, T, mutate, pose))
    return out


def cases():
    out = [(kind, TASK_MASK, backward) for kind in ("task", "task2") for backward in (False, True)]
    return out + [("distance", mask, False) for mask in X.DISTANCE_MASKS]


CASE_IDS = ["%s-%s-%s" % (k, RC.mask_id(mk), "parnmpc" if b else "ocp") for k, mk, b in cases()]


@pytest.mark.parametrize("kind,mask,backward", cases(), ids=CASE_IDS)
@pytest.mark.parametrize("which", MODELS, ids=str)
def test_referee_against_itself(which, kind, mask, backward):
    refs, refs64 = (uniform_records(which, kind, mask, backward, T) for T in (L.LD, np.float64))
    for i, (r64, r) in enumerate(zip(refs64, refs)):
        X.check_referee(r64, r, "%s %s %s node %d" % (which, kind, RC.mask_id(mask), i))
        for a in r["angles"]:      # the logarithm stays away from 0 (Jlog6 far from I) and from pi
            assert 0.2 < a < 2.6, (i, r["angles"])      # (ocp_ext_cases._reference_for_all)
    if kind == "task2":      # the two unused slots
        assert all(not r["JJ"][12:].any() and not r["tw"][12:].any() for r in refs)
    if kind == "distance":
        live = refs[2]
        assert not any(r["Jc"].any() or r["w"].any() or r["z"].any() for r in refs[:2] + refs[3:]), "rows before level 2 or on the terminal node"
        assert np.abs(live["z"][:3] - np.array(X.FOOT_HEIGHTS)).max() < 1e-11
        if all(mask):
            assert not live["Jc"].any() and not live["w"].any() and not live["lq"].any() and live["z"].all()
        else:
            up = [c for c in range(4) if not mask[c]]
            assert all(live["w"][c] > 0 for c in up) and not any(live["w"][c] for c in range(4) if mask[c])
            if 1 in up:
                assert live["violation"][0] > 0.5 * X.DT * 0.02      # the foot below the ground: a bumped slack, a non-zero residual
            if 0 in up:
                assert live["w"][0] > 0.9 * X.DT * 1e-4 / 1e-6       # z / s = eps / s^2 with s = 1e-3


@pytest.mark.parametrize("which", MODELS, ids=str)
def test_local_and_world_rows_differ(which):
    """the convention the referee follows (row 2 of the LOCAL Jacobian) is far from the derivative of the world height on the cases"""
    for mask in X.DISTANCE_MASKS[1:]:
        live = uniform_records(which, "distance", mask, False, np.float64)[2]
        for c in range(4):
            if not mask[c]:
                gap = np.abs(live["Jc"][c] - live["Jc_world"][c]).max()
                print("%s %s foot %d: local and world row differ by %.2e" % (which, RC.mask_id(mask), c, gap))
                assert gap > 1e6 * X.BAR, (mask, c, gap)


ORACLE_CASES = [(kind, TASK_MASK, backward) for kind in ("task", "task2") for backward in (False, True)] \
    + [("distance", mask, False) for mask in X.DISTANCE_MASKS] + [("distance", TASK_MASK, True)]
ORACLE_IDS = ["%s-%s-%s" % (k, RC.mask_id(mk), "parnmpc" if b else "ocp") for k, mk, b in ORACLE_CASES]


@functools.lru_cache(maxsize=None)
def oracle_uniform(which, kind, mask, backward):
    """[(node, q, the oracle's un-condensed record)] of the uniform handle of a case right after init_constraints"""
    m, M, s = X.iterate(which, kind)
    t0 = L.T0 - L.DT if backward else L.T0      # (ParNMPC's stage i then sits at ocp_lqr_cases' time of stage i)
    cost, cons = X.problem(m, M, which, kind, t0)
    o = (OracleParNMPC if backward else OracleOCP)(m, cost, cons, L.N * L.DT, L.N)
    o.set_contact_status(mask, s["pts"])
    nodes = X.uniform_nodes(mask, t0, backward=backward)
    if kind == "task":
        times = [n["t"] for n in nodes]
        o.set_task_refs(times, np.array([X.task_pose(which, kind, t0)(t) for t in times]))
    if backward:
        for name in ("q", "v", "a"):
            o.set_stage_values(name, L.stage_arrays(s, name)[:L.N])
    else:
        set_iterate(o, s, [(i, i, i == L.N) for i in range(L.N + 1)])
    o.init_constraints(t0)
    return [(node, s["q"][p], X.oracle_record(o, backward, p)) for p, node in enumerate(nodes)], t0


@functools.lru_cache(maxsize=None)
def oracle_event_chain(which, kind):
    """the same along the event chain of ocp_stage_cases (oracle::OCPSolver)"""
    m, M, s = X.iterate(which, kind, True)
    cost, cons = X.problem(m, M, which, kind, L.CHAIN_T0)
    o = OracleOCP(m, cost, cons, S.CHAIN_T, S.CHAIN_N, max_num_impulse=S.CHAIN_EVENTS)
    S.build_chain(o, which)
    o.set_solution("q", s["q"][0]); o.set_solution("v", s["v"][0])
    o.init_constraints(L.CHAIN_T0)
    chain = o.chain(L.CHAIN_T0)
    assert [c["kind"] for c in chain[:-1]] == [k for k, _ in S.FORWARD_CHAIN] and chain[-1]["kind"] == "terminal"
    times = [c["t"] for c in chain]
    if kind == "task":
        o.set_task_refs(times, np.array([X.task_pose(which, kind, L.CHAIN_T0)(t) for t in times]))
    set_iterate(o, s, [(c["slot"], p, c["kind"] == "terminal") for p, c in enumerate(chain)])
    o.init_constraints(L.CHAIN_T0)
    return [(node, s["q"][p], X.oracle_record(o, False, p)) for p, node in enumerate(X.chain_nodes(chain, times))], L.CHAIN_T0


def referee_of(which, kind, t0, node, q, rec, T=L.LD, mutate=None):
    m, M, _ = X.iterate(which, kind)
    cost, cons = X.problem(m, M, which, kind, t0)
    return X.ext_record(M, cost, cons, node, q, rec["slack"], rec["dual"], T, mutate, X.task_pose(which, kind, t0))


@pytest.mark.parametrize("kind,mask,backward", ORACLE_CASES, ids=ORACLE_IDS)
@pytest.mark.parametrize("which", MODELS, ids=str)
def test_oracle_records_of_the_uniform_handles(which, kind, mask, backward):
    """the oracle's un-condensed record of every node against the referee at the bar (OCPSolver: N grid stages and the terminal node; ParNMPCSolver: N stages)"""
    records, t0 = oracle_uniform(which, kind, mask, backward)
    worst, label = {}, "oracle %s %s %s %s" % (which, kind, RC.mask_id(mask), "parnmpc" if backward else "ocp")
    for p, (node, q, rec) in enumerate(records):
        X.hold(X.distances(rec, referee_of(which, kind, t0, node, q, rec)), "%s, position %d (%s)" % (label, p, node["kind"]), worst)
    if kind == "distance" and not all(mask):
        assert [p for p, (_, _, rec) in enumerate(records) if rec["w"].any()] == ([1, 2] if backward else [2]), label
    print("%s: %s" % (label, X.summary(worst)))


@pytest.mark.parametrize("kind", X.PROBLEMS)
@pytest.mark.parametrize("which", MODELS, ids=str)
def test_oracle_records_of_the_event_chain(which, kind):
    """every node kind (grid, impulse with its own weights, aux and lift at constraint level 0, terminal): the referee against itself, the oracle at the bar"""
    records, t0 = oracle_event_chain(which, kind)
    worst, label = {}, "oracle %s chain %s" % (which, kind)
    assert {node["kind"] for node, _, _ in records} == {"stage", "impulse", "aux", "lift", "terminal"}
    for p, (node, q, rec) in enumerate(records):
        ref = referee_of(which, kind, t0, node, q, rec)
        X.check_referee(referee_of(which, kind, t0, node, q, rec, np.float64), ref, "%s node %d" % (label, p))
        X.hold(X.distances(rec, ref), "%s, position %d (%s)" % (label, p, node["kind"]), worst)
    print("%s: %s" % (label, X.summary(worst)))


@pytest.mark.parametrize("mutation", X.MUTATIONS)
def test_sensitivity_to_single_term_mutations(mutation):
    """against the ORACLE's records: a referee with one term wrong is at least 1000 x the bar away from the second implementation on some node"""
    worst, where = 0.0, None
    for which in MODELS:
        sets = [((kind, RC.mask_id(mask), backward), kind) + oracle_uniform(which, kind, mask, backward) for kind, mask, backward in ORACLE_CASES]
        sets += [((kind, "chain", False), kind) + oracle_event_chain(which, kind) for kind in X.PROBLEMS]
        for tag, kind, records, t0 in sets:
            for p, (node, q, rec) in enumerate(records):
                for name, (d, _) in X.distances(referee_of(which, kind, t0, node, q, rec, np.float64, mutation), rec).items():
                    if d > worst:
                        worst, where = d, (which,) + tag + (p, name)
    print("mutation %s: distance %.1e from the oracle at %s" % (mutation, worst, where))
    assert worst >= 1000 * X.BAR, (mutation, worst)


def oracle_task(which, kind, mask):
    m, M, s = X.iterate(which, kind)
    cost, cons = X.problem(m, M, which, kind)
    o = OracleOCP(m, cost, cons, L.N * L.DT, L.N)
    o.set_contact_status(mask, s["pts"])
    if kind == "task":
        times = L.T0 + L.DT * np.arange(L.N + 1)
        o.set_task_refs(times, np.array([X.task_pose(which, kind, L.T0)(t) for t in times]))
    set_iterate(o, s, [(i, i, i == L.N) for i in range(L.N + 1)])
    o.init_constraints(L.T0)
    assert o.stage(0, L.T0, s["q_init"], s["v_init"]) == 0
    return (m, M, s, cost, cons, o) + o.constraint_data()


@pytest.mark.parametrize("kind", ("task", "task2"))
@pytest.mark.parametrize("which", MODELS, ids=str)
def test_oracle_condensed_and_terminal_stage(which, kind):
    """the terms are really ADDED into the stage: the oracle's condensed grid stages and P[N], s[N] against the stage Lagrangian with the referee's ext terms"""
    m, M, s, cost, cons, o, slack, dual = oracle_task(which, kind, TASK_MASK)
    pose = X.task_pose(which, kind, L.T0)
    nodes = X.uniform_nodes(TASK_MASK)
    recs = L.rigid_body(which, TASK_MASK)
    worst = {}
    for i in range(L.N):
        ext = X.ext_record(M, cost, cons, nodes[i], s["q"][i], pose=pose)
        ref = L.lqr_stage(m, M, cost, cons, recs[i], L.uniform_stage(s, i, TASK_MASK), slack[i], dual[i], ext=ext)
        bare = L.lqr_stage(m, M, cost, cons, recs[i], L.uniform_stage(s, i, TASK_MASK), slack[i], dual[i])
        assert S.worst_row(bare["lx"], ref["lx"])[0] > 1000 * L.BAR and S.worst_row(bare["Qxx"], ref["Qxx"])[0] > 1000 * L.BAR
        L.hold(L.distances(o.lqr_stage(i), ref), "oracle %s %s, stage %d" % (which, kind, i), worst)
    print("oracle %s %s: %s" % (which, kind, L.summary(worst)))
    assert o.stage(1, L.T0, s["q_init"], s["v_init"]) == 0
    Pm, sv, _, _ = o.riccati()
    hold_terminal(which, kind, Pm[L.N], sv[L.N], "oracle %s %s" % (which, kind))


@pytest.mark.parametrize("arm,dim,where", X.FIXED_CASES, ids=X.FIXED_IDS)
def test_oracle_fixed_base_terminal_stage(arm, dim, where):
    """the fixed-base cost (oracle::UnOCPSolver): P[N], s[N] against the terminal weights plus JJ^T W_f JJ and JJ^T W_f diff of the referee"""
    m, M, cost, cons, joint, it = X.fixed_case(arm, dim, where)
    o = OracleUnOCP(m, cost, cons, L.N * L.DT, L.N)
    for name in ("q", "v"):
        o.set_solution(name, it[name])
    assert o.stage(0, 0.0, it["q"], it["v"]) == 0 and o.stage(1, 0.0, it["q"], it["v"]) == 0
    Pm, sv, _, _ = o.riccati()
    X.hold_fixed_terminal(arm, dim, where, Pm[L.N], sv[L.N], "oracle fixed base %s %dD %s" % (arm, dim, where))
