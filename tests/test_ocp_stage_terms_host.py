"""The comparison of test_ocp_stage_terms_gpu.py with the ORACLE in the kernels' place (no GPU): the un-condensed stage data of
oracle::OCPSolver / ParNMPCSolver (oracle_ocp_get_uncondensed: M, J, [dID; dC]/d(q, v), [ID - S^T u; C] of a chain position, captured in
front of the condensation) against the independent numpy model of ocp_stage_cases.py, term by term and as the record a float64
implementation forms from them -- on every case of the GPU test: all 16 contact sets on two models with distinct iterates per stage,
an event chain with every node kind in both discretisations (the backward-Euler impulse stage included: the oracle keeps its whole
un-condensed system), the hard states.  This checks the case module and the node-kind conventions it states before any kernel is
asked, and extends the oracle's own pin (test_independent_rbd_host.py: four feet, one partial set, its rigid-body entry points) to the
solver's stage assembly on the same classes.

The referee against itself, on every case and over EVERY compared quantity: the distance between its float64 and its long double route
(the inverse of K = [M J^T; J 0], the two products, and every term taken back out of them) and cond(K) are printed (-s) and each held
to a quarter of the bar the quantity is held to.  Observed: self-distance at most 1.1e-12 (dID/dq taken back out; the products 2.4e-14),
cond(K) at most 4.9e3, straight legs, half turns and the stiff Baumgarte step included -- no state needed softening; the oracle at most
8.6e-13 from the referee (dID/dq).  One handle, `stiff` at the Baumgarte step 1e-3, holds dID/dq, dID/dv and ID - S^T u at
ocp_stage_cases.STIFF_BAR = eps nv / step^2 = 4e-9 instead of 1e-11 (the rounding of the float64 record itself; referee against itself
3.4e-10 there, oracle 3e-10) and everything else at 1e-11; the tests assert that no other case has a bar other than 1e-11."""
import ctypes as C

import numpy as np
import pytest

import ocp_stage_cases as S
import rbd_cases as RC
from helpers import NODE_KINDS, OracleOCP, OracleParNMPC, P, anymal_problem, arr

FIELDS = ("q", "v", "a", "f", "u")


def fetch(o, backward, pos, name, shape=None):
    fn = o.lib.oracle_parnmpc_get_uncondensed if backward else o.lib.oracle_ocp_get_uncondensed
    fn.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_double)]
    n = fn(o.h, pos, name.encode(), None)
    assert n >= 0, name
    out = np.zeros(max(n, 1))
    fn(o.h, pos, name.encode(), P(out))
    return out[:n] if shape is None else out[:n].reshape(shape, order="F")


def oracle_record(o, backward, pos):
    """(kind, active mask, dimf, record) of a chain position: the record a float64 implementation forms from the oracle's un-condensed data"""
    meta = fetch(o, backward, pos, "meta")
    assert meta[0] == 1.0, "no un-condensed record at chain position %d" % pos
    nv, nf = o.nv, int(meta[2])
    M, J = fetch(o, backward, pos, "M", (nv, nv)), fetch(o, backward, pos, "J", (nf, nv))
    K = np.block([[M, J.T], [J, np.zeros((nf, nf))]])
    rec = S.record_of(K, fetch(o, backward, pos, "dIDCdqv", (nv + nf, 2 * nv)), fetch(o, backward, pos, "IDC"))
    kind = NODE_KINDS[int(meta[1])]
    if backward and kind == "terminal":
        kind = "stage"      # (the last backward-Euler stage is a TerminalParNMPC: a regular stage with the terminal cost on top)
    return kind, tuple((int(meta[7]) >> c) & 1 for c in range(4)), nf, rec


def keep_uncondensed(o, backward):
    fn = o.lib.oracle_parnmpc_keep_uncondensed if backward else o.lib.oracle_ocp_keep_uncondensed
    fn.argtypes = [C.c_void_p, C.c_int]
    fn(o.h, 1)


def set_slot(o, backward, slot, name, value):
    fn = o.lib.oracle_parnmpc_set_stage if backward else o.lib.oracle_ocp_set_stage
    fn.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_double)]
    assert fn(o.h, slot, name.encode(), P(arr(value))) == 0, name


def linearise(o, backward, q0, v0):
    keep_uncondensed(o, backward)
    if backward:
        o.lib.oracle_parnmpc_compute_direction.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        assert o.lib.oracle_parnmpc_compute_direction(o.h, 0.0, P(arr(q0)), P(arr(v0))) == 0
    else:
        assert o.stage(0, 0.0, q0, v0) == 0      # (linearizeOCP alone: the records are captured in front of the condensation)


def oracle_solver(m, backward, T, N, events=0):
    cost, cons = anymal_problem(m, trotting_ref=False)
    return (OracleParNMPC if backward else OracleOCP)(m, cost, cons, T, N, max_num_impulse=events)


def two_stage_oracle(m, backward, time_step, mask, s):
    """the oracle's records of a two-stage handle with the per-stage inputs s (ocp_stage_cases.uniform_inputs)"""
    o = oracle_solver(m, backward, S.N_UNIFORM * time_step, S.N_UNIFORM)
    o.set_contact_status(mask, s["pts"])
    for name in ("q", "v"):
        o.set_solution(name, s[name][0])
    o.init(0.0) if backward else o.init_constraints(0.0)
    for i in range(S.N_UNIFORM):
        for name in FIELDS:
            set_slot(o, backward, i, name, np.asarray(s[name][i]).reshape(-1))
    linearise(o, backward, s["q"][0], s["v"][0])
    return [oracle_record(o, backward, i) for i in range(S.N_UNIFORM)]


def hold_records(records, refs, nv, kinds_masks, label, worst, stiff=False):
    # every quantity of every record at the bar of the layer; only the one named stiff handle holds three terms at their own stated bar
    assert all({name for name, bar in ref["bars"].items() if bar != S.BAR} == (set(S.STIFF_TERMS) if stiff else set()) for ref in refs), label
    for p, ((kind, mask, dimf, rec), ref, (want_kind, want_mask)) in enumerate(zip(records, refs, kinds_masks)):
        assert (kind, mask, dimf) == (want_kind, tuple(want_mask), ref["dimf"]), (label, p, kind, mask, dimf)
        S.hold(S.distances(rec, ref, nv), "%s, position %d (%s, contacts %s)" % (label, p, kind, RC.mask_id(mask)), ref["bars"], worst)


UNIFORM = [(mask, False) for mask in RC.ALL_MASKS] + [(mask, True) for mask in S.BACKWARD_MASKS]


@pytest.mark.parametrize("mask,backward", UNIFORM, ids=lambda x: RC.mask_id(x) if isinstance(x, tuple) else ("backward" if x else "forward"))
@pytest.mark.parametrize("which", S.MODELS, ids=str)
def test_uniform_contact_sets(which, mask, backward):
    m, _, s = S.uniform_inputs(which)
    refs = S.uniform_reference(which, mask)
    S.check_referee(refs, "%s %s" % (which, RC.mask_id(mask)))
    worst = {}
    hold_records(two_stage_oracle(m, backward, S.TS, mask, s), refs, m.nv, [("stage", mask)] * S.N_UNIFORM, "%s uniform" % which, worst)
    print("oracle %s, %s %s: %s" % ("backward" if backward else "forward", which, RC.mask_id(mask), S.summary(worst)))


@pytest.mark.parametrize("backward", (False, True), ids=("forward", "backward"))
@pytest.mark.parametrize("which", S.MODELS, ids=str)
def test_event_chain(which, backward):
    m, _, s = S.chain_inputs(which)
    want = S.BACKWARD_CHAIN if backward else S.FORWARD_CHAIN
    o = oracle_solver(m, backward, S.CHAIN_T, S.CHAIN_N, S.CHAIN_EVENTS)
    S.build_chain(o, which)
    for name in ("q", "v"):
        o.set_solution(name, s[name][0])
    o.init(0.0) if backward else o.init_constraints(0.0)
    chain = o.chain(0.0)[:len(want)]      # (forward: without the terminal stage; backward: the last stage reads "terminal" and has dynamics)
    assert [c["kind"] for c in chain[:-1]] == [k for k, _ in want[:-1]] and chain[-1]["kind"] in (want[-1][0], "terminal")
    assert [c["dimf"] for c in chain] == [S.dimf_of(mask) for _, mask in want]
    for p, c in enumerate(chain):
        for name in FIELDS:
            if name != "u" or c["kind"] != "impulse":
                set_slot(o, backward, c["slot"], name, np.asarray(s[name][p]).reshape(-1))
    linearise(o, backward, s["q"][0], s["v"][0])
    refs = S.chain_reference(which, backward)
    S.check_referee(refs, "%s chain, %s" % (which, "backward" if backward else "forward"))
    worst = {}
    hold_records([oracle_record(o, backward, p) for p in range(len(chain))], refs, m.nv, want, "%s chain" % which, worst)
    print("oracle %s chain, %s: %s" % ("backward" if backward else "forward", which, S.summary(worst)))


@pytest.mark.parametrize("mask", RC.HARD_MASKS, ids=RC.mask_id)
@pytest.mark.parametrize("pair", S.HARD_PAIRS, ids="-".join)
def test_hard_states(pair, mask):
    m = S.hard_state(pair[0])[0]
    states = [S.hard_state(name)[2] for name in pair]
    s = {name: [x[name] for x in states] for name in FIELDS}
    s["pts"] = states[0]["pts"]
    refs = S.hard_reference(pair, mask)
    S.check_referee(refs, "%s %s" % ("-".join(pair), RC.mask_id(mask)))
    worst = {}
    hold_records(two_stage_oracle(m, False, S.hard_time_step(pair), mask, s), refs, m.nv, [("stage", mask)] * 2, "-".join(pair), worst, stiff=pair == S.STIFF_PAIR)
    print("oracle %s %s: %s" % ("-".join(pair), RC.mask_id(mask), S.summary(worst)))
