"""The yardstick of the rollout scoring without a GPU.

1. The numpy referee of tests/rbd_score.py against the oracle: an OCPSolver of the oracle with N = steps, T = steps dt, a uniform contact status and
   every constraint component off is handed a random trajectory stage by stage (oracle_ocp_set_stage), and OCPSolver::costAndViolation(alpha = 0)
   -- the sum the line search evaluates -- must equal the referee's cost with the terminal term, for the constant, the trotting and the time-varying
   reference.  The referee's reference tables are held to oracle_ocp_q_ref on the way.  This passes with or without the scoring calls: it
   validates what test_rbd_score_gpu.py measures against.
2. The host-side planning (idocp_amd/csrc/rbd_objective.hpp) as a stand-alone program under the address and undefined-behaviour sanitizers
   (tests/cpp/rbd_objective_plan.cpp): the tables against closed forms, every refusal, the per-step masks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import independent_rbd as IR
import rbd_policy as RP
import rbd_score as RS
from helpers import ROOT, OracleOCP, P, anymal_contact_points, anymal_model, anymal_problem, arr, running_problem
from idocp_amd import capi
from rbd_batch import random_samples

STEPS = 3


def problem(kind):
    """(cost, constraints with every component off, t0, dt): the stage times cross the period boundary of the trotting reference and the end of the
    time-varying window"""
    m = anymal_model()
    if kind == "time_varying":
        cost, cons = running_problem(m, steps=1)
        cost.tv_t_begin, cost.tv_t_end = 1.0, 1.1
        cost.v_ref[5] = 0.7                                # (the reference turns as well)
        t0, dt = 0.96, 0.05                                # 0.96 before, 1.01 and 1.06 inside, 1.11 beyond
    else:
        cost, cons = anymal_problem(m, trotting_ref=kind == "trotting")
        t0, dt = 0.9, 0.06                                 # trotting: t_start 0.5, t_period 0.5 -- 0.9, 0.96 in the first period, 1.02, 1.08 in the second
    cost.set("u_weight", np.linspace(0.01, 0.02, m.nu)).set("u_ref", np.linspace(-1.0, 1.0, m.nu))
    cons = capi.Constraints()
    capi.lib().idocp_constraints_init(C.byref(cons))
    for name in ("joint_position_limits", "joint_velocity_limits", "joint_torque_limits", "linearized_friction_cone", "linearized_impulse_friction_cone",
                 "friction_cone", "impulse_friction_cone", "joint_acceleration_lower_limit", "joint_acceleration_upper_limit", "contact_distance"):
        setattr(cons, name, 0)
    return m, cost, cons, t0, dt


@pytest.mark.parametrize("mask", [(1, 1, 1, 1), (1, 0, 0, 1)], ids=["all_feet", "two_feet"])
@pytest.mark.parametrize("kind", ["constant", "trotting", "time_varying"])
def test_referee_cost_equals_the_oracles_line_search_cost(kind, mask):
    m, cost, cons, t0, dt = problem(kind)
    M = IR.model_from_struct(m)
    rng = np.random.default_rng([11, len(kind), sum(mask)])
    q_ref0 = np.array(cost.q_ref[:m.nq])
    q = RP.perturbed_configurations(M, rng, np.repeat(q_ref0[None], STEPS + 1, axis=0), angle=1.5)
    _, v, a, f, _ = random_samples(rng, STEPS + 1)
    u = rng.uniform(-20, 20, (STEPS, m.nu))
    o = OracleOCP(m, cost, cons, STEPS * dt, STEPS)
    o.set_contact_status(mask, anymal_contact_points(m))
    chain = o.chain(t0)                                    # (discretises at t0: the stage times are t0 + k dt)
    assert [c["kind"] for c in chain] == ["stage"] * STEPS + ["terminal"]
    assert np.allclose([c["t"] for c in chain], [t0 + k * dt for k in range(STEPS + 1)], rtol=0, atol=1e-15)
    o.lib.oracle_ocp_set_stage.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_double)]
    for k, c in enumerate(chain):
        fields = (("q", q[k]), ("v", v[k])) + ((("a", a[k]), ("u", u[k]), ("f", f[k])) if k < STEPS else ())
        for name, x in fields:
            assert o.lib.oracle_ocp_set_stage(o.h, c["slot"], name.encode(), P(arr(x))) == 0, name
    # the referee's reference tables against the oracle's q_ref(t)
    tables = RS.reference_tables(M, cost, t0, dt, STEPS)
    for k, c in enumerate(chain):
        qr = np.zeros(m.nq)
        o.lib.oracle_ocp_q_ref(o.h, C.c_double(c["t"]), P(qr))
        assert np.abs(RP.same_rotation(tables[0][k], qr) - qr).max() < 1e-14, (kind, k)
    if kind != "constant":
        assert np.abs(tables[0][1:] - q_ref0).max() > 1e-3       # (the reference moves)
    out = np.zeros(2)
    o.lib.oracle_ocp_cost_and_violation.argtypes = [C.c_void_p, C.c_double, capi.c_double_p]
    assert o.lib.oracle_ocp_cost_and_violation(o.h, 0.0, P(out)) == 0
    got, _, stage = RS.reference_score(m, M, cost, None, tables, dt, q, v, u, a[:STEPS], f[:STEPS], [mask] * STEPS, terminal=True)
    err = abs(got - out[0]) / max(1.0, abs(out[0]))
    print("%s %s: oracle %.15g, referee %.15g, %.2e; stage costs %s" % (kind, mask, out[0], got, err, stage))
    assert err < 1e-13, (got, out[0])
    assert stage[-1] > 0 and (stage[:-1] > 0).all()


def test_objective_planning_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "rbd_objective_plan")
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "idocp_amd/csrc"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests/cpp/rbd_objective_plan.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rbd objective plan: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_objective_without_a_device_is_refused_not_faked():
    """no CPU fallback: without a GPU there is no handle, hence no objective; the argument errors that need no handle are reported"""
    lib = capi.lib()
    out = C.c_void_p()
    m, cost, cons, t0, dt = problem("constant")
    assert lib.idocp_rbd_objective_create(None, C.byref(cost), C.byref(cons), t0, dt, STEPS, C.byref(out)) == -1
    assert b"idocp_rbd_objective_create: null handle or out" in lib.idocp_last_error()
    assert lib.idocp_rbd_objective_get_reference(None, 0, None, None) == -1
    assert lib.idocp_rbd_objective_reference_device(None, None, None) == -1
    assert lib.idocp_rbd_score_rollout(None, None, 1, 0, 1, None, 0, 0, None) == -1
    assert b"idocp_rbd_score_rollout: null handle, objective or io" in lib.idocp_last_error()
    lib.idocp_rbd_objective_destroy(None)
