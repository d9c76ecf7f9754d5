"""The condensation + expansion layer against an INDEPENDENT answer: tests/golden/kkt_anymal.json holds the Newton direction of a small hybrid
ANYmal problem (2-contact stages with a switching constraint, an impulse stage, an aux stage, 4-contact stages, a lift stage, the terminal stage)
obtained by tests/golden/gen_golden_kkt.py from ONE DENSE SOLVE of the un-condensed KKT system of the whole horizon in all variables
(q v a f u | lmd gmm beta mu xi) -- no MJtJinv, no condensed Hessians, no Riccati recursion, no expansion formulas.

* CPU: the oracle's condense -> Riccati -> expand direction (contact_dynamics.hxx:105-190, impulse_dynamics_forward_euler.hxx:59-142,
  riccati_recursion_solver.cpp:48-251) equals it field by field and node by node to 1e-9;
* CPU: the fixture is what the generator produces today from the oracle's un-condensed stage data (it cannot go stale silently);
* GPU (-m gpu): the HIP direction through the C ABI equals it to 1e-9.

One entry of the fixture is NOT the Newton step, on purpose: on a stage that carries a switching constraint the reference forms [dbeta; dmu]
without the Phia^T dxi term (contact_dynamics.hxx:171-190); the generator follows the reference there, by a dense solve of the two stationarity
rows concerned, and records how far that is from the Newton value (`dense_system.newton_minus_reference_dbeta_on_switching_stages`)."""
import functools
import json
import os
import sys

import numpy as np
import pytest

from helpers import GOLDEN, HipOCP, HipParNMPC, HipUnOCP, HipUnParNMPC, OracleOCP, OracleParNMPC, OracleUnOCP, OracleUnParNMPC

sys.path.insert(0, GOLDEN)
import gen_golden_kkt as G      # noqa: E402
import gen_golden_kkt_iiwa14 as GI      # noqa: E402
import gen_golden_kkt_parnmpc as GP      # noqa: E402
import gen_golden_kkt_parnmpc_events as GE      # noqa: E402
import gen_golden_kkt_parnmpc_iiwa14 as GA      # noqa: E402

TOL = 1e-9


def fixture():
    with open(os.path.join(GOLDEN, "kkt_anymal.json")) as f:
        return json.load(f)


def second_iteration(Solver, spec, **kw):
    o, qm, vm = G.build(spec, Solver, **kw)
    M = len(o.chain(0.0))
    assert o.update(0.0, qm, vm) == 0
    assert o.update(0.0, qm, vm) == 0
    return o, M


def compare(got, ref, what):
    table = []
    for f in G.FIELDS:
        want = np.array(ref["direction"][f])
        have = got[f]
        assert have.shape == want.shape, (f, have.shape, want.shape)
        for p in range(want.shape[0]):
            scale = max(1.0, np.max(np.abs(want[p])))
            table.append((np.max(np.abs(have[p] - want[p])) / scale, f, p))
    worst = max(table)
    print("%s: worst field / node %s at chain position %d: %.2e" % (what, worst[1], worst[2], worst[0]))
    assert worst[0] < TOL, "%s differs from the dense Newton direction: %s at chain position %d by %.3e" % (what, worst[1], worst[2], worst[0])


def test_the_chain_has_every_node_kind():
    ref = fixture()
    kinds = [c["kind"] for c in ref["chain"]]
    assert set(kinds) == {"stage", "impulse", "aux", "lift", "terminal"}
    assert {c["dimf"] for c in ref["chain"] if c["kind"] == "stage"} == {6, 12}
    assert any(c["sw_event"] >= 0 for c in ref["chain"])
    assert ref["dense_system"]["max_abs_residual"] < 1e-12
    # the reference's dual direction on the switching stage is far from the Newton value: the test below would see the difference
    assert ref["dense_system"]["newton_minus_reference_dbeta_on_switching_stages"] > 1.0


def test_oracle_direction_is_the_dense_newton_direction():
    ref = fixture()
    o, M = second_iteration(OracleOCP, ref["spec"])
    assert [c["kind"] for c in o.chain(0.0)] == [c["kind"] for c in ref["chain"]]
    compare({f: o.get_chain(f, M) for f in G.FIELDS}, ref, "oracle")


def test_fixture_is_what_the_generator_produces():
    import ctypes as C
    ref = fixture()
    assert ref["spec"] == G.problem_spec()
    o, qm, vm = G.build(ref["spec"], OracleOCP)
    M = len(o.chain(0.0))
    assert o.update(0.0, qm, vm) == 0
    o.lib.oracle_ocp_keep_uncondensed.argtypes = [C.c_void_p, C.c_int]
    o.lib.oracle_ocp_keep_uncondensed(o.h, 1)
    assert o.update(0.0, qm, vm) == 0
    dense, _, info = G.dense_direction(o, M, o.get_chain("dq", M)[0], o.get_chain("dv", M)[0])
    assert info["unknowns"] == ref["dense_system"]["unknowns"]
    compare(dense, ref, "regenerated dense solve")


@pytest.mark.gpu
def test_hip_direction_is_the_dense_newton_direction():
    ref = fixture()
    g, M = second_iteration(HipOCP, ref["spec"], batch=2)
    assert [c["kind"] for c in g.chain(0.0)] == [c["kind"] for c in ref["chain"]]
    for inst in (0, 1):
        compare({f: g.get_chain(f, M, inst) for f in G.FIELDS}, ref, "HIP (instance %d)" % inst)


# ---- the fixed-base path: tests/golden/kkt_iiwa14.json (gen_golden_kkt_iiwa14.py) ----
# One dense un-condensed solve, three condensations held to it: the oracle's OCPSolver on the arm (a eliminated through M^-1, Riccati on u), the oracle's
# UnOCPSolver (u eliminated through u = ID(q, v, a), Riccati on a: unconstrained_dynamics.hxx:55-106, split_unriccati_factorizer.hxx) and the HIP kernels.

def fixture_arm():
    with open(os.path.join(GOLDEN, "kkt_iiwa14.json")) as f:
        return json.load(f)


def compare_arm(got, ref, what):
    worst = (-1.0, "", -1)
    for f in GI.FIELDS:
        want = np.array(ref["direction"][f])
        have = got[f]
        n = have.shape[0]                                  # (the stage-only fields stop in front of the terminal stage)
        assert n in (want.shape[0], want.shape[0] - 1) and have.shape[1] == want.shape[1], (f, have.shape, want.shape)
        for p in range(n):
            e = np.max(np.abs(have[p] - want[p])) / max(1.0, np.max(np.abs(want[p])))
            worst = max(worst, (e, f, p))
    print("%s: worst field / stage %s at stage %s: %.2e" % (what, worst[1], worst[2], worst[0]))
    assert worst[0] < TOL, "%s differs from the dense Newton direction: %s at stage %s by %.3e" % (what, worst[1], worst[2], worst[0])


def second_iteration_arm(Solver, spec, **kw):
    o, qm, vm = GI.build(spec, Solver, **kw)
    assert o.update(0.0, qm, vm) == 0
    assert o.update(0.0, qm, vm) == 0
    return o


def test_arm_fixture_is_what_the_generator_produces():
    import ctypes as C
    ref = fixture_arm()
    assert ref["spec"] == GI.problem_spec()
    o, qm, vm = GI.build(ref["spec"], OracleOCP)
    assert o.update(0.0, qm, vm) == 0
    o.lib.oracle_ocp_keep_uncondensed.argtypes = [C.c_void_p, C.c_int]
    o.lib.oracle_ocp_keep_uncondensed(o.h, 1)
    assert o.update(0.0, qm, vm) == 0
    dense, _, info = GI.dense_direction(o, ref["spec"]["N"] + 1, o.get("dq")[0], o.get("dv")[0])
    assert info["unknowns"] == ref["dense_system"]["unknowns"] and ref["dense_system"]["max_abs_residual"] < 1e-13
    compare_arm(dense, ref, "regenerated dense solve")
    assert (G.NV, G.NU, G.NX) == (18, 12, 36)               # (the arm's dimensions did not leak into the ANYmal generator)


def test_both_oracle_condensations_of_the_arm_are_the_dense_newton_direction():
    ref = fixture_arm()
    o = second_iteration_arm(OracleOCP, ref["spec"])
    compare_arm({f: o.get(f) for f in GI.FIELDS}, ref, "oracle OCPSolver on the arm")
    u = second_iteration_arm(OracleUnOCP, ref["spec"])
    compare_arm({f: u.direction(f) for f in GI.FIELDS}, ref, "oracle UnOCPSolver")


@pytest.mark.gpu
def test_hip_fixed_base_direction_is_the_dense_newton_direction():
    ref = fixture_arm()
    g = second_iteration_arm(HipUnOCP, ref["spec"], batch=2)
    for inst in (0, 1):
        compare_arm({f: g.direction(f, inst) for f in GI.FIELDS}, ref, "HIP UnOCP kernels (instance %d)" % inst)


# ---- the fixed-base path on chains that are NOT iiwa14: the dense answer computed at test time ----
# The committed fixture covers seven +z joints.  The same dense un-condensed solve on a two-joint and an eight-joint random chain (arbitrary unit axes and
# joint rpy; the smallest and the largest UnLaunch<nv>, the two-round linearisation form at eight) and on the committed six-joint arm, from the oracle's
# un-condensed stage data of a problem built like GI.problem_spec().  The rigid-body terms those stage data consist of are held on these chains by
# tests/test_independent_rbd_host.py, so the answer shares neither a condensation nor a rigid-body formula with what it checks.

OTHER_CHAINS = {"random2": (2, 1), "arm6": (6, None), "random8": (8, 1)}


def other_chain_model(which):
    """a fresh struct every time: GI.problem / unocp_problem write the torque limits into it"""
    import tempfile
    from arm_chains import arm6_model, random_arm
    nv, seed = OTHER_CHAINS[which]
    if seed is None:
        return arm6_model()
    with tempfile.TemporaryDirectory() as d:
        return random_arm(nv, seed, d)


@functools.lru_cache(maxsize=None)
def dense_direction_of_chain(which):
    import ctypes as C
    nv = OTHER_CHAINS[which][0]
    spec = GI.problem_spec(nv, seed=7007 + nv)
    assert spec["N"] == 6
    o, qm, vm = GI.build(spec, OracleOCP, model=other_chain_model(which))
    assert o.update(0.0, qm, vm) == 0
    o.lib.oracle_ocp_keep_uncondensed.argtypes = [C.c_void_p, C.c_int]
    o.lib.oracle_ocp_keep_uncondensed(o.h, 1)
    assert o.update(0.0, qm, vm) == 0
    dense, _, info = GI.dense_direction(o, spec["N"] + 1, o.get("dq")[0], o.get("dv")[0], nv=nv)
    assert info["max_abs_residual"] < 1e-12 and info["unknowns"] == (spec["N"] + 1) * 4 * nv + spec["N"] * 3 * nv, info
    assert (G.NV, G.NU, G.NX) == (18, 12, 36)
    return spec, {"direction": dense}


@pytest.mark.parametrize("which", list(OTHER_CHAINS))
def test_both_oracle_condensations_of_other_chains_are_the_dense_newton_direction(which):
    spec, ref = dense_direction_of_chain(which)
    o = second_iteration_arm(OracleOCP, spec, model=other_chain_model(which))
    compare_arm({f: o.get(f) for f in GI.FIELDS}, ref, "oracle OCPSolver on %s" % which)
    u = second_iteration_arm(OracleUnOCP, spec, model=other_chain_model(which))
    compare_arm({f: u.direction(f) for f in GI.FIELDS}, ref, "oracle UnOCPSolver on %s" % which)


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(OTHER_CHAINS))
def test_hip_fixed_base_direction_on_other_chains_is_the_dense_newton_direction(which):
    spec, ref = dense_direction_of_chain(which)
    g = second_iteration_arm(HipUnOCP, spec, model=other_chain_model(which), batch=2)
    for inst in (0, 1):
        compare_arm({f: g.direction(f, inst) for f in GI.FIELDS}, ref, "HIP UnOCP kernels on %s (instance %d)" % (which, inst))


# ---- the ParNMPC stage: tests/golden/kkt_parnmpc.json (gen_golden_kkt_parnmpc.py) ----
# The coarse update of ParNMPCSolver is the Newton step of ONE backward-Euler stage; on a horizon of one stage it is the whole iteration.  The dense solve of that
# stage's un-condensed system against the condensed route: backward-Euler contact-dynamics condensation + the block-wise KKT inverse
# (split_parnmpc.hxx, split_kkt_matrix_inverter.hxx:56-197) -- four feet, two feet, none.

def fixture_parnmpc():
    with open(os.path.join(GOLDEN, "kkt_parnmpc.json")) as f:
        return json.load(f)


def compare_stage(have, ref_case, what):
    worst = (-1.0, "")
    for f in GP.FIELDS:
        want = np.array(ref_case["direction"][f])
        assert have[f].shape == want.shape, (f, have[f].shape, want.shape)
        worst = max(worst, (np.max(np.abs(have[f] - want)) / max(1.0, np.max(np.abs(want))), f))
    print("%s: worst field %s: %.2e" % (what, worst[1], worst[0]))
    assert worst[0] < TOL, "%s differs from the dense stage-wise Newton step: %s by %.3e" % (what, worst[1], worst[0])


def test_parnmpc_stage_fixture_is_what_the_generator_produces_and_the_oracle_condensation_equals_it():
    import ctypes as C
    ref = fixture_parnmpc()
    assert ref["spec"] == GP.problem_spec() and {k: v["active"] for k, v in ref["cases"].items()} == GP.CASES
    assert {v["dense_system"]["dimf"] for v in ref["cases"].values()} == {0, 6, 12}
    for name, case in ref["cases"].items():
        o, qm, vm = GP.run(ref["spec"], case["active"], OracleParNMPC)
        o.lib.oracle_parnmpc_keep_uncondensed.argtypes = [C.c_void_p, C.c_int]
        o.lib.oracle_parnmpc_keep_uncondensed(o.h, 1)
        assert o.update(0.0, qm, vm) == 0
        dense, info = GP.dense_stage_step(o)
        assert info["unknowns"] == case["dense_system"]["unknowns"]
        compare_stage(dense, case, "regenerated dense solve (%s)" % name)
        compare_stage({f: o.get(f)[0] for f in GP.FIELDS}, case, "oracle ParNMPCSolver (%s)" % name)


@pytest.mark.gpu
def test_hip_parnmpc_stage_is_the_dense_stage_wise_newton_step():
    ref = fixture_parnmpc()
    for name, case in ref["cases"].items():
        g, qm, vm = GP.run(ref["spec"], case["active"], HipParNMPC, batch=2)
        assert g.update(0.0, qm, vm) == 0
        for inst in (0, 1):
            compare_stage({f: g.get(f, inst)[0] for f in GP.FIELDS}, case, "HIP ParNMPC kernels (%s, instance %d)" % (name, inst))


# ---- the ParNMPC stages of a horizon with events: tests/golden/kkt_parnmpc_events.json (gen_golden_kkt_parnmpc_events.py) ----
# The coarse iterate of EVERY chain position (regular, aux with 3 / 6 / 12 switching rows, impulse with as many, lift, terminal; aux_mat of the stage behind,
# the state of the stage in front) from dense solves of the stages' un-condensed systems, against the condensed route: backward-Euler condensation of the
# contact / impulse dynamics, the premultiplied base rows, the block-wise KKT inverses (split_kkt_matrix_inverter.hxx:44-166,
# impulse_split_kkt_matrix_inverter.hxx:34-80).

def fixture_parnmpc_events():
    with open(os.path.join(GOLDEN, "kkt_parnmpc_events.json")) as f:
        return json.load(f)


def compare_chain(have, case, what, tol=TOL):
    worst = (-1.0, "", -1)
    for f in GE.FIELDS:
        want = np.array(case["iterate"][f])
        assert have[f].shape == want.shape, (f, have[f].shape, want.shape)
        for p in range(want.shape[0]):
            worst = max(worst, (np.max(np.abs(have[f][p] - want[p])) / max(1.0, np.max(np.abs(want[p]))), f, p))
    print("%s: worst field %s at chain position %d (%s): %.2e" % (what, worst[1], worst[2], case["stages"][worst[2]]["chain_kind"], worst[0]))
    assert worst[0] < tol, "%s differs from the dense stage-wise Newton steps: %s at chain position %d by %.3e" % (what, worst[1], worst[2], worst[0])


def test_parnmpc_event_chain_fixture_is_what_the_generator_produces_and_the_oracle_condensation_equals_it():
    ref = fixture_parnmpc_events()
    assert ref["spec"] == GE.problem_spec() and set(ref["cases"]) == set(GE.CASES)
    kinds, rows = set(), set()
    md = GE.model_dict()
    for name, case in ref["cases"].items():
        o, qm, vm = GE.build(ref["spec"], name, OracleParNMPC)
        GE.prepare(o, qm, vm)
        dense, infos = GE.coarse_iterates(o, md, qm)
        assert [i["chain_kind"] for i in infos] == [i["chain_kind"] for i in case["stages"]]
        compare_chain(dense, case, "regenerated dense solves (%s)" % name)
        compare_chain({f: o.get_chain(f, len(infos)) for f in GE.FIELDS}, case, "oracle ParNMPCSolver, coarse update (%s)" % name)
        kinds |= {i["chain_kind"] for i in infos}
        rows |= {i["switching_rows"] for i in infos if i["switching_rows"]}
    assert kinds == {"stage", "aux", "impulse", "lift", "terminal"} and rows == {3, 6, 12}


@pytest.mark.gpu
def test_hip_parnmpc_coarse_update_along_an_event_chain_is_the_dense_stage_wise_newton_step():
    import ctypes as C
    from idocp_amd import capi
    from helpers import P, arr
    ref = fixture_parnmpc_events()
    for name, case in ref["cases"].items():
        g, qm, vm = GE.build(ref["spec"], name, HipParNMPC, batch=2)
        assert g.update(0.0, qm, vm) == 0
        dq, dv = C.c_void_p(), C.c_void_p()
        capi.check(g.lib.idocp_parnmpc_prev_state(g.h, C.byref(dq), C.byref(dv)), "prev_state")
        qb, vb = arr(np.tile(qm, (2, 1))), arr(np.tile(vm, (2, 1)))
        capi.check(g.lib.idocp_device_upload(dq, qb.ctypes.data, qb.nbytes), "upload q")
        capi.check(g.lib.idocp_device_upload(dv, vb.ctypes.data, vb.nbytes), "upload v")
        capi.check(g.lib.idocp_parnmpc_discretize(g.h, 0.0), "discretize")
        for ph in (0, 1, 2):                                  # tangent RNEA, backward-Euler condensation, KKT inverse + coarse update
            capi.check(g.lib.idocp_parnmpc_launch_phase(g.h, ph, dq, dv), "phase %d" % ph)
        capi.check(g.lib.idocp_ocp_synchronize(g.h), "synchronize")
        M = len(case["stages"])
        for inst in (0, 1):
            raw = {}
            for f, dim in (("lmd", 18), ("gmm", 18), ("u", 12), ("q", 19), ("v", 18), ("xi", 12)):
                out = np.zeros((M + 1, dim))
                capi.check(g.lib.idocp_parnmpc_get_new_solution_chain(g.h, f.encode(), inst, P(out)), "get_new_solution_chain " + f)
                raw[f] = out[:M]
            # the fixture's layout: f / mu of an impulse stage in the slots of their contacts, the untouched ones as the iterate has them
            cur_f, cur_mu = g.get_chain("f", M + 1, inst)[:M], g.get_chain("mu", M + 1, inst)[:M]
            have = {"new_lmd": raw["lmd"], "new_gmm": raw["gmm"], "new_q": raw["q"], "new_v": raw["v"], "new_u": raw["u"].copy(),
                    "new_xi": np.zeros((M, 12)), "new_f": cur_f.copy(), "new_mu": cur_mu.copy()}
            for p, st in enumerate(case["stages"]):
                if st["impulse"]:
                    n = st["dimf"]
                    landing = [c for c in range(4) if np.any(np.array(case["iterate"]["new_f"][p]).reshape(4, 3)[c] != cur_f[p].reshape(4, 3)[c])]
                    assert 3 * len(landing) == n, (name, p, landing, n)
                    rows = [3 * c + k for c in landing for k in range(3)]
                    have["new_f"][p][rows], have["new_mu"][p][rows] = raw["u"][p][:n], raw["xi"][p][:n]
                    have["new_u"][p] = 0.0
                elif st["switching_rows"]:
                    have["new_xi"][p][:st["switching_rows"]] = raw["xi"][p][:st["switching_rows"]]
            compare_chain(have, case, "HIP ParNMPC kernels, coarse update (%s, instance %d)" % (name, inst))


# ---- a WHOLE ParNMPC iteration against one dense solve over the horizon ----
# The backward correction is block back-substitution with the pivots K_i + aux_mat_{i+1}; it solves the horizon's Newton system with aux_old - aux_new added to
# every stage's state block (gen_golden_kkt_parnmpc_events.py dense_iteration).  Exact on the arm (kkt_parnmpc_iiwa14.json); to first order in the base's step on
# ANYmal (kkt_parnmpc_events.json "whole_iteration": compared near the solution, relative to each field's magnitude).

def fixture_parnmpc_arm():
    with open(os.path.join(GOLDEN, "kkt_parnmpc_iiwa14.json")) as f:
        return json.load(f)


def compare_arm_iteration(have, ref, what):
    worst = (-1.0, "")
    for f in GA.FIELDS:
        want = np.array(ref["direction"][f])
        assert have[f].shape == want.shape, (f, have[f].shape, want.shape)
        worst = max(worst, (np.max(np.abs(have[f] - want)) / max(1.0, np.max(np.abs(want))), f))
    print("%s: worst field %s: %.2e" % (what, worst[1], worst[0]))
    assert worst[0] < TOL, "%s differs from the dense solve of the whole iteration: %s by %.3e" % (what, worst[1], worst[0])


def direction_of_iteration(Solver, build, spec, number, **kw):
    """the direction of iteration `number` (1-based): that many updates, the last one's direction"""
    o, qm, vm = build(spec, Solver, **kw)
    for _ in range(number):
        assert o.update(0.0, qm, vm) == 0
    return o


def test_whole_parnmpc_iteration_on_the_arm_is_the_dense_solve():
    ref = fixture_parnmpc_arm()
    assert ref["spec"] == GA.problem_spec() and ref["iterations_before"] == GA.ITERATIONS_BEFORE
    o, qm, vm = GA.build(ref["spec"], OracleParNMPC)
    for _ in range(GA.ITERATIONS_BEFORE - 1):
        assert o.update(0.0, qm, vm) == 0
    dense, info = GA.dense_direction(o, qm, vm)
    assert info["unknowns"] == ref["dense_system"]["unknowns"] and (GE.NV, GE.NU) == (18, 12)
    compare_arm_iteration(dense, ref, "regenerated dense solve")
    GE.finish(o)
    compare_arm_iteration({f: o.get(f) for f in GA.FIELDS}, ref, "oracle ParNMPCSolver on the arm, taken through the sweeps")
    n = GA.ITERATIONS_BEFORE + 1
    o = direction_of_iteration(OracleParNMPC, GA.build, ref["spec"], n)
    compare_arm_iteration({f: o.get(f) for f in GA.FIELDS}, ref, "oracle ParNMPCSolver on the arm, updateSolution")
    u = direction_of_iteration(OracleUnParNMPC, GA.build, ref["spec"], n)
    compare_arm_iteration({f: u.get(f) for f in GA.FIELDS}, ref, "oracle UnParNMPCSolver")


@pytest.mark.gpu
def test_hip_whole_unparnmpc_iteration_is_the_dense_solve():
    ref = fixture_parnmpc_arm()
    g = direction_of_iteration(HipUnParNMPC, GA.build, ref["spec"], GA.ITERATIONS_BEFORE + 1, batch=2)
    for inst in (0, 1):
        compare_arm_iteration({f: g.get(f, inst) for f in GA.FIELDS}, ref, "HIP UnParNMPC kernels (instance %d)" % inst)


# the whole iteration on the two-joint and the eight-joint chain, the dense answer computed at test time (GA.dense_direction with the chain's nv)

@functools.lru_cache(maxsize=None)
def dense_iteration_of_chain(which):
    nv = OTHER_CHAINS[which][0]
    spec = GA.problem_spec(nv, seed=2718 + nv)
    o, qm, vm = GA.build(spec, OracleParNMPC, model=other_chain_model(which))
    for _ in range(GA.ITERATIONS_BEFORE - 1):
        assert o.update(0.0, qm, vm) == 0
    dense, info = GA.dense_direction(o, qm, vm, nv=nv)
    assert info["max_abs_residual"] < 1e-12 and info["unknowns"] == spec["N"] * 7 * nv and (GE.NV, GE.NU) == (18, 12), info
    return spec, {"direction": dense}


@pytest.mark.parametrize("which", ["random2", "random8"])
def test_whole_unparnmpc_iteration_on_other_chains_is_the_dense_solve(which):
    spec, ref = dense_iteration_of_chain(which)
    u = direction_of_iteration(OracleUnParNMPC, functools.partial(GA.build, model=other_chain_model(which)), spec, GA.ITERATIONS_BEFORE + 1)
    compare_arm_iteration({f: u.get(f) for f in GA.FIELDS}, ref, "oracle UnParNMPCSolver on %s" % which)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["random2", "random8"])
def test_hip_whole_unparnmpc_iteration_on_other_chains_is_the_dense_solve(which):
    spec, ref = dense_iteration_of_chain(which)
    g = direction_of_iteration(HipUnParNMPC, functools.partial(GA.build, model=other_chain_model(which)), spec, GA.ITERATIONS_BEFORE + 1, batch=2)
    for inst in (0, 1):
        compare_arm_iteration({f: g.get(f, inst) for f in GA.FIELDS}, ref, "HIP UnParNMPC kernels on %s (instance %d)" % (which, inst))


def compare_whole_iteration(o, M, case, what, bar):
    worst = (-1.0, "")
    for f in GE.DIRECTION:
        want = np.array(case["direction"][f])
        have = o.get_chain(f, M)
        if np.max(np.abs(want)) > 0:
            worst = max(worst, (np.max(np.abs(have - want)) / np.max(np.abs(want)), f))
    print("%s: worst field %s: %.2e of its magnitude (base step %.1e)" % (what, worst[1], worst[0], case["info"]["base_step"]))
    assert worst[0] < bar, "%s differs from the dense solve of the whole iteration: %s by %.3e of its magnitude" % (what, worst[1], worst[0])


def test_whole_parnmpc_iteration_on_anymal_is_the_dense_solve_to_first_order_in_the_base_step():
    ref = fixture_parnmpc_events()
    md = GE.model_dict()
    assert set(ref["whole_iteration"]) == set(GE.WHOLE_CASES)
    for name, case in ref["whole_iteration"].items():
        info = case["info"]
        assert info["after_iterations"] == GE.WHOLE_AFTER[name]
        # the distance falls with the base's step: what is left of it is the composition of the sweeps' corrections on SE(3), not a formula
        far = info["one_iteration_in"]
        assert info["worst_relative_mismatch"] < 1e-5 and info["base_step"] < 1e-5 and far["base_step"] > 1e-2
        assert info["worst_relative_mismatch"] / info["base_step"] < 20 * max(1.0, far["worst_relative_mismatch"] / far["base_step"])
        o, whole, winfo = GE.whole_iteration(ref["spec"], name, OracleParNMPC, md, GE.WHOLE_AFTER[name])
        M = len(o.chain(0.0))
        assert winfo["unknowns"] == info["unknowns"]
        for f in GE.DIRECTION:
            want = np.array(case["direction"][f])
            assert np.max(np.abs(whole[f] - want)) <= 1e-7 * max(np.max(np.abs(want)), 1e-300), (name, f)      # (the regenerated dense solve)
        compare_whole_iteration(o, M, case, "oracle ParNMPCSolver, whole iteration (%s)" % name, 1e-5)


# (No HIP twin of the ANYmal test: near the solution, where the comparison has to be made, the direction is 1e-6 of the iterate and two FP64 evaluation orders ten
# iterations apart differ by more than this identity's slack.  The kernels are held to the restatement on every iteration of such runs at 1e-10 of the
# ITERATE (tests/test_parnmpc_hybrid_gpu.py), the restatement to the dense solve here; on the arm, where the identity is exact, the HIP kernels are compared directly.)
