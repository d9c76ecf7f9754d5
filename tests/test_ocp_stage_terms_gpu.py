"""The stage kernels of OCPSolver / ParNMPCSolver against the INDEPENDENT rigid-body model, term by term, without the oracle in between:
the record ocp_condense_kernel leaves of every stage -- MJtJinv, MJtJinv [dID; dC]/d(q, v), MJtJinv [ID - S^T u; C], read at every chain
position of every instance with idocp_ocp_get_contact_dynamics_chain after one idocp_ocp_compute_direction -- against the numpy
Newton-Euler model with complex-step derivatives and a long double inverse (ocp_stage_cases.py, which also states the conventions of the
node kinds and where they were read).  One inverse of the device's MJtJinv gives M and J back, two products dID/d(q, v), dC/d(q, v),
ID - S^T u and C: a failure names the term and the packed row.  test_ocp_stage_terms_host.py runs the same cases on the oracle.

What is reached (ocp_condense_kernel<D, RESIDUAL, DIMF, BWD, MERIT, XYY, EVENTS> and the nominal sweeps / impulse kernels in front of it).
Which launch a forward-Euler handle takes is decided by launchCondenseO (ocp_capi.hip): OcpLaunch::condense on an event-free chain with
all feet down, or when no stage falls into the all-feet, half, event-half or flight class; OcpLaunch::condenseMixed otherwise, the terminal
stage on its general instantiation.
* one contact set on the whole horizon, all 16 sets, two stages with distinct (q, v, a, f, u), batch 3, on ANYmal in the specialised (XYY)
  and, through IDOCP_GENERAL_AXES, the general leg sweep and on other_quadruped(1), which only the general sweep takes:
  dimf 12 -> condense, DIMF = 12;  dimf 9 and 3 -> condense, the general DIMF = -1;  dimf 6 -> condenseMixed, the plain DIMF = 6 class;
  dimf 0 -> condenseMixed, the flight class DIMF = 0 with its narrow LDS layout (the only place the flight class is reached);
* an event chain with grid, impulse, aux and lift nodes, phases of dimf 6 -> 12 -> 9 -> 3 and a two-foot impulse while two feet stand
  -> condenseMixed: stage 0 carries the switching constraint (asserted) and the impulse has two feet, both the EVENTS class DIMF = 6;
  stage 1 the plain DIMF = 6; the aux stage and the grid stage behind it DIMF = 12; the lifts and the nine-row stage the general one;
* the backward-Euler form (HipParNMPC): every regular stage on the general BWD instantiation, on four contact sets and on the same event
  chain through the ParNMPC event kernels.  Its IMPULSE stage keeps no such record (ocp_stage_cases.py: parnmpc_event_kernels.hip leaves
  Minv and Minv ImD only, no contact rows and no derivative product): that kind is left out of the record comparison; the two quantities it
  does leave are held to the referee;
* the eight hard states of rbd_cases on five two-stage handles (a handle has one Baumgarte step: `stiff` and `rest` fill a handle each)
  and the position in the batch (bit for bit).

Every instance of a handle holds the SAME inputs here (idocp_ocp_set_solution_stages / _chain write to all instances) and the instances
must agree bit for bit: that catches a dependence on the position in the batch, not an instance that reads another instance's iterate or
record.  Per-instance inputs are held by test_ocp_gpu.py::test_batch_instances_and_ragged_sizes (direction against the oracle).

Bar: helpers.rel_err < 1e-11 for every product and every term, the block of K = MJtJinv^-1 that must vanish included.  On ONE handle,
`stiff` at the Baumgarte step 1e-3, dID/dq, dID/dv and ID - S^T u are held at ocp_stage_cases.STIFF_BAR = eps nv / step^2 = 4e-9 instead:
the record's entries grow with 1 / step^2 and its rounding to float64 alone costs that much of the terms taken back out of it (the
referee's own float64 record: 3.4e-10); its products, M, J, dC/d(q, v), C stay at 1e-11, and no other case has another bar (asserted).
Observed on one MI355X: products 6.1e-14, terms 1.5e-12 (dID/dv; dID/dq 6.3e-13), vanishing block 7.8e-14, backward impulse
Minv 1.9e-15; on the stiff handle dID/dq 6.8e-10, dID/dv 9.9e-12, ID - S^T u 6.5e-12.  DESIGN.md (section 6b) has the table row."""
import numpy as np
import pytest

import ocp_stage_cases as S
import rbd_cases as RC
from helpers import HipOCP, HipParNMPC, P, anymal_problem, arr
from idocp_amd import capi

pytestmark = pytest.mark.gpu
FIELDS = ("q", "v", "a", "f", "u")
# (model, leg sweep): ANYmal qualifies for the specialised sweep and runs the general one under IDOCP_GENERAL_AXES; another quadruped only the general
SWEEPS = (("anymal", "xyy"), ("anymal", "general"), (1, "general"))
SWEEP_IDS = ["%s-%s" % x for x in SWEEPS]
UNIFORM = [(mask, False) for mask in RC.ALL_MASKS] + [(mask, True) for mask in S.BACKWARD_MASKS]
form_id = lambda x: RC.mask_id(x) if isinstance(x, tuple) else ("backward" if x else "forward")      # noqa: E731


def solver(monkeypatch, m, sweep, backward, T, N, batch, events=0):
    if sweep == "general" and m.nv == 18:
        monkeypatch.setenv("IDOCP_GENERAL_AXES", "1")      # (read when the handle is created; a model off ANYmal's pattern runs the general sweep anyway)
    cost, cons = anymal_problem(m, trotting_ref=False)
    return (HipParNMPC if backward else HipOCP)(m, cost, cons, T, N, batch=batch, max_num_impulse=events)


def direction(g, backward, q0, v0):
    fn = g.lib.idocp_parnmpc_compute_direction if backward else g.lib.idocp_ocp_compute_direction
    rc = fn(g.h, 0.0, P(g._bc(q0, g.nq)), P(g._bc(v0, g.nv)))      # (linearises at the iterate and does not integrate)
    assert rc == 0, capi.lib().idocp_last_error()


def records(g, positions):
    """[instance][position] -> (dimf, MJ, MJD, MJIDC)"""
    return [[S.device_record(g, b, p) for p in positions] for b in range(g.batch)]


def same_bits(a, b, lead=None):
    """two records bit for bit; lead = nv: only the leading nv x nv block of MJtJinv and the leading nv entries of MJtJinv IDC (all that a
    backward-Euler impulse stage writes)"""
    if lead is not None:
        return a[0] == b[0] and np.array_equal(a[1][:lead, :lead], b[1][:lead, :lead]) and np.array_equal(a[3][:lead], b[3][:lead])
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def two_stage_records(monkeypatch, m, sweep, backward, time_step, mask, s, batch):
    """the records of both stages of every instance of a two-stage handle with the per-stage inputs s (ocp_stage_cases.uniform_inputs)"""
    n = S.N_UNIFORM
    g = solver(monkeypatch, m, sweep, backward, n * time_step, n, batch)
    g.set_contact_status(mask, s["pts"])
    for name in FIELDS:
        k = n if backward or name not in ("q", "v") else min(n + 1, len(s[name]))      # (forward Euler: q and v of the terminal stage too)
        capi.check(g.lib.idocp_ocp_set_solution_stages(g.h, name.encode(), k, P(arr(np.asarray(s[name][:k]).reshape(k, -1)))), "set " + name)
    g.init(0.0) if backward else g.init_constraints(0.0)
    direction(g, backward, s["q"][0], s["v"][0])
    return records(g, range(n))


def hold_all(recs, refs, nv, label, worst, stiff=False):
    """every instance's records against the referee's (dimf asserted), and the instances against each other bit for bit (they hold the same inputs)"""
    assert stiff or all(set(ref["bars"].values()) == {S.BAR} for ref in refs), label
    for b, inst in enumerate(recs):
        for p, (rec, ref) in enumerate(zip(inst, refs)):
            where = "%s, instance %d, position %d" % (label, b, p)
            assert rec[0] == ref["dimf"], (where, rec[0], ref["dimf"])
            S.hold(S.distances(rec[1:], ref, nv), where, ref["bars"], worst)
            assert same_bits(rec, recs[0][p]), where + ": differs from instance 0 on the same inputs"


@pytest.mark.parametrize("mask,backward", UNIFORM, ids=form_id)
@pytest.mark.parametrize("which,sweep", SWEEPS, ids=SWEEP_IDS)
def test_uniform_contact_sets(monkeypatch, which, sweep, mask, backward):
    """One contact set on the whole horizon, every set (which launch and class each takes: module docstring); batch 3 (the last workgroup of the
    nominal sweeps is not full), distinct iterates on the two stages, u != 0, forces on every foot, points some centimetres off the feet"""
    m, _, s = S.uniform_inputs(which)
    refs = S.uniform_reference(which, mask)
    worst = {}
    recs = two_stage_records(monkeypatch, m, sweep, backward, S.TS, mask, s, S.BATCH)
    hold_all(recs, refs, m.nv, "%s %s uniform %s" % (which, sweep, RC.mask_id(mask)), worst)
    print("%s uniform, %s %s, dimf %d: %s" % ("backward" if backward else "forward", which, sweep, S.dimf_of(mask), S.summary(worst)))


def chain_records(monkeypatch, which, sweep, backward, batch):
    m, _, s = S.chain_inputs(which)
    want = S.BACKWARD_CHAIN if backward else S.FORWARD_CHAIN
    g = solver(monkeypatch, m, sweep, backward, S.CHAIN_T, S.CHAIN_N, batch, S.CHAIN_EVENTS)
    S.build_chain(g, which)
    for name in ("q", "v"):
        g.set_solution(name, s[name][0])
    g.init(0.0) if backward else g.init_constraints(0.0)
    chain = [c for c in g.chain(0.0) if c["kind"] != "terminal"]      # (the terminal stage / the placeholder behind a backward-Euler chain: no dynamics)
    # the case must not degenerate: every node kind, the contact counts of the phases, the two-foot impulse
    assert [(c["kind"], c["dimf"]) for c in chain] == [(kind, S.dimf_of(mask)) for kind, mask in want]
    assert backward or chain[0]["sw_dimi"] == 6      # (forward Euler: the stage two steps ahead of the impulse carries its switching constraint)
    n = len(chain)
    for name in FIELDS:
        capi.check(g.lib.idocp_ocp_set_solution_chain(g.h, name.encode(), n, P(arr(np.asarray(s[name][:n]).reshape(n, -1)))), "set %s along the chain" % name)
    direction(g, backward, s["q"][0], s["v"][0])
    return m, want, records(g, range(n))


@pytest.mark.parametrize("backward", (False, True), ids=("forward", "backward"))
@pytest.mark.parametrize("which,sweep", SWEEPS, ids=SWEEP_IDS)
def test_event_chain(monkeypatch, which, sweep, backward):
    """OcpLaunch::condenseMixed (forward) / the BWD instantiation and parnmpc_event_kernels.hip (backward) on a chain with every node kind.
    Backward Euler: the impulse position keeps Minv and Minv ImD only (module docstring) -- those two are held, the record is not."""
    m, want, recs = chain_records(monkeypatch, which, sweep, backward, S.BATCH)
    refs = S.chain_reference(which, backward)
    nv = m.nv
    worst = {kind: {} for kind in ("stage", "impulse", "aux", "lift")}
    for b, inst in enumerate(recs):
        for p, (rec, ref, (kind, mask)) in enumerate(zip(inst, refs, want)):
            where = "%s %s chain, instance %d, position %d (%s, contacts %s)" % (which, sweep, b, p, kind, RC.mask_id(mask))
            assert rec[0] == ref["dimf"], (where, rec[0], ref["dimf"])
            if backward and kind == "impulse":
                Minv, MinvImD = S.backward_impulse_record(ref)
                S.hold({"Minv": S.worst_row(rec[1][:nv, :nv], Minv), "Minv ImD": S.worst_row(rec[3][:nv], MinvImD)}, where, {"Minv": S.BAR, "Minv ImD": S.BAR}, worst[kind])
            else:
                S.hold(S.distances(rec[1:], ref, nv), where, ref["bars"], worst[kind])
            assert same_bits(rec, recs[0][p], nv if backward and kind == "impulse" else None), where + ": differs from instance 0 on the same inputs"
    for kind, w in worst.items():
        print("%s chain, %s %s, %s: %s" % ("backward" if backward else "forward", which, sweep, kind,
                                        S.summary(w) if "MJtJinv" in w else "  ".join("%s %.1e" % x for x in w.items())))


@pytest.mark.parametrize("mask", RC.HARD_MASKS, ids=RC.mask_id)
@pytest.mark.parametrize("pair", S.HARD_PAIRS, ids="-".join)
@pytest.mark.parametrize("sweep", ("xyy", "general"))
def test_hard_states(monkeypatch, sweep, pair, mask):
    """straight legs, +-pi, quaternion w = 0 and w < 0, v x 20, Baumgarte step 1e-3 (T = N 1e-3), points 0.5 m off, rest: one state per stage"""
    m = S.hard_state(pair[0])[0]
    states = [S.hard_state(name)[2] for name in pair]
    s = {name: [x[name] for x in states] for name in FIELDS}
    s["pts"] = states[0]["pts"]
    worst = {}
    recs = two_stage_records(monkeypatch, m, sweep, False, S.hard_time_step(pair), mask, s, S.BATCH)
    hold_all(recs, S.hard_reference(pair, mask), m.nv, "%s %s %s" % ("-".join(pair), sweep, RC.mask_id(mask)), worst, stiff=pair == S.STIFF_PAIR)
    print("hard %s, %s, %s: %s" % ("-".join(pair), sweep, RC.mask_id(mask), S.summary(worst)))


@pytest.mark.parametrize("backward", (False, True), ids=("forward", "backward"))
def test_position_in_the_batch(monkeypatch, backward):
    """batch 5, instances 1 to 4 holding copies of instance 0's inputs: every record of every position agrees bit for bit, on the uniform
    launch (dimf 12, 9, 3) and on the event chain"""
    m, _, s = S.uniform_inputs("anymal")
    for mask in RC.HARD_MASKS:
        recs = two_stage_records(monkeypatch, m, "xyy", backward, S.TS, mask, s, 5)
        assert len(recs) == 5
        for b in range(1, 5):
            for p in range(S.N_UNIFORM):
                assert same_bits(recs[b][p], recs[0][p]), (RC.mask_id(mask), b, p)
    _, want, recs = chain_records(monkeypatch, "anymal", "xyy", backward, 5)
    for b in range(1, 5):
        for p, (kind, _) in enumerate(want):
            assert same_bits(recs[b][p], recs[0][p], m.nv if backward and kind == "impulse" else None), ("chain", b, p)
