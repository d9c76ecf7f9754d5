"""The yardstick of the cost gradients and of the iLQR line-search step without a GPU.

(a) The numpy referee of tests/rbd_gradients.py against central differences of rbd_score.reference_score along idocp_model_integrate_configuration (q),
    and along v and u: an independent check, the referee's Jlog6 never enters the differences.  ANYmal with the base turned 0.3 .. 1 rad and
    shifted against the reference (Jlog6 is far from the identity there: leaving it out moves a base row by about half the angle, relatively), one
    sample ON the reference (the small-angle branch: finite, zero on the q rows), chains of 2 and 8 joints.
(b) The host-only planner of idocp_amd/csrc/rbd_objective.hpp as a stand-alone program under the address and undefined-behaviour sanitizers
    (tests/cpp/rbd_gradient_plan.cpp): every refusal with its code and text, the weight tables.
(c) The numpy referee of accept and of step torques on hand-made cases.
This passes or fails with the referee and the planner alone; test_rbd_gradients_gpu.py and test_rbd_ilqr_gpu.py hold the kernels to them."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import independent_rbd as IR
import rbd_gradients as G
import rbd_score as RS
from helpers import ROOT, anymal_model, anymal_problem
from idocp_amd import capi

STEPS, DT = 2, 0.02
H = float(np.finfo(np.float64).eps) ** (1.0 / 3.0)      # the step of central differences
# The largest relative error measured over the cases below is 1.3e-9 (the chain of 8 joints: the roundoff eps |cost| / h of its larger total cost;
# ANYmal's base rows, the only ones that are not quadratic, stay at 6e-11, the chain of 2 joints at 2e-10).  Ten times the measured value, and
# far below the 1e-6 any correct referee meets:
FD_BAR = 1.3e-8


def gradient_cost(m, rng=None, trotting=False):
    """a cost the gradients take: a_weight = f_weight = 0, every other weight and reference non-trivial"""
    if m.ncontacts:
        cost, _ = anymal_problem(m, trotting_ref=trotting)
        cost.set("u_weight", np.linspace(0.01, 0.02, m.nu)).set("u_ref", np.linspace(-1.0, 1.0, m.nu))
        cost.set("v_ref", np.linspace(-0.2, 0.3, m.nv))
    else:
        cost = capi.Cost()
        cost.set("q_ref", rng.uniform(-1, 1, m.nv)).set("v_ref", rng.uniform(-1, 1, m.nv)).set("u_ref", rng.uniform(-1, 1, m.nv))
        for name in ("q_weight", "v_weight", "u_weight", "qf_weight", "vf_weight"):
            cost.set(name, rng.uniform(0.1, 10, m.nv))
    cost.set("a_weight", np.zeros(m.nv))
    for c in range(4):
        for x in range(3):
            cost.f_weight[c][x] = 0.0
    return cost


def turned(M, rng, q_ref, lo, hi):
    """q_ref (+) d with a base rotation of lo .. hi rad, a shift of up to 0.3 m and joints moved by up to 0.5 rad"""
    d = rng.uniform(-0.5, 0.5, M["nv"])
    if M.get("floating"):
        ax = rng.normal(size=3)
        d[:3], d[3:6] = rng.uniform(-0.3, 0.3, 3), ax / np.linalg.norm(ax) * rng.uniform(lo, hi)
    return G.RBD.integrate(M, q_ref, d)


@functools.lru_cache(maxsize=None)
def fd_case(which):
    """(model, model dict, cost, tables, q [STEPS + 1][nq], v, u [STEPS][nu]) of one sample"""
    rng = np.random.default_rng([5, len(which)])
    if which.startswith("chain"):
        m, M = IR.chain(int(which[5:]), 1)
        cost = gradient_cost(m, rng)
    else:
        m = anymal_model()
        M = IR.model_from_struct(m)
        cost = gradient_cost(m)
    tables = RS.reference_tables(M, cost, 0.3, DT, STEPS)
    if which == "anymal_on_reference":
        q = tables[0].copy()
    else:
        q = np.array([turned(M, rng, tables[0][k], 0.3, 1.0) for k in range(STEPS + 1)])
    return m, M, cost, tables, q, rng.uniform(-1, 1, (STEPS + 1, m.nv)), rng.uniform(-12, 12, (STEPS, m.nu))


def central_differences(m, M, cost, tables, q, v, u):
    """(lx, lu) of the total cost with the terminal term by central differences of rbd_score.reference_score"""
    lib = capi.lib()

    def integrate(qq, d, length):
        out = np.zeros(m.nq)
        capi.check(lib.idocp_model_integrate_configuration(C.byref(m), np.ascontiguousarray(qq).ctypes.data, np.ascontiguousarray(d).ctypes.data, length, out.ctypes.data), "integrate")
        return out

    def total(qq, vv, uu):
        return RS.reference_score(m, M, cost, None, tables, DT, qq, vv, uu, terminal=True)[0]

    lx, lu = np.zeros((STEPS + 1, 2 * m.nv)), np.zeros((STEPS, m.nu))
    for k in range(STEPS + 1):
        for r in range(m.nv):
            e = np.zeros(m.nv)
            e[r] = 1.0
            pair = []
            for sgn in (1.0, -1.0):
                qq = q.copy()
                qq[k] = integrate(q[k], e, sgn * H)
                pair.append(total(qq, v, u))
            lx[k, r] = (pair[0] - pair[1]) / (2 * H)
            vp, vm = v.copy(), v.copy()
            vp[k, r] += H
            vm[k, r] -= H
            lx[k, m.nv + r] = (total(q, vp, u) - total(q, vm, u)) / (2 * H)
        if k < STEPS:
            for j in range(m.nu):
                up, um = u.copy(), u.copy()
                up[k, j] += H
                um[k, j] -= H
                lu[k, j] = (total(q, v, up) - total(q, v, um)) / (2 * H)
    return lx, lu


@pytest.mark.parametrize("which", ["anymal", "anymal_on_reference", "chain2", "chain8"])
def test_referee_against_central_differences(which):
    m, M, cost, tables, q, v, u = fd_case(which)
    lx, lu = G.reference_gradients(m, M, cost, tables, DT, q, v, u, terminal=True)
    fx, fu = central_differences(m, M, cost, tables, q, v, u)
    assert np.isfinite(lx).all() and np.isfinite(lu).all()
    for k in range(STEPS + 1):
        dq, dv = G.distance(fx[k, :m.nv], lx[k, :m.nv]), G.distance(fx[k, m.nv:], lx[k, m.nv:])
        du = G.distance(fu[k], lu[k]) if k < STEPS else 0.0
        print("%s slice %d: |central differences - referee| q rows %.2e, v rows %.2e, u %.2e (bar %.1e)" % (which, k, dq, dv, du, FD_BAR))
        assert max(dq, dv, du) < FD_BAR, (which, k, dq, dv, du)      # measured: 1.3e-9 at most (see FD_BAR)
    assert FD_BAR < 1e-6
    if which == "anymal_on_reference":
        assert (lx[:, :m.nv] == 0.0).all()                                # e = 0 exactly: the small-angle branch of Jlog6, finite
    if which == "anymal":
        # the bar has teeth: with J = I on the base rows the referee would miss it by orders of magnitude
        W = np.array(cost.q_weight[:m.nv])
        e = G.RBD.difference(M, tables[0][0], q[0])
        without = DT * (W * e)
        assert G.distance(without[:6], lx[0, :6]) > 1e3 * FD_BAR, G.distance(without[:6], lx[0, :6])


def test_gradient_planning_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "rbd_gradient_plan")
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "idocp_amd/csrc"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests/cpp/rbd_gradient_plan.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rbd gradient plan: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ------------------------------------------------------------------ (c) accept and step torques, by hand

CONSTS = dict(penalty=2.0, armijo=0.5, shrink=0.5, alpha_min=0.2)
CASES = ("accepted", "armijo", "nan_trial", "done", "alpha_min")


def hand_made(nq=3, nu=2, steps=2):
    """five samples, one per case of CASES; every array distinct so that a wrong copy shows"""
    n = len(CASES)
    rng = np.random.default_rng(99)
    s = {"q_traj": rng.normal(size=(steps + 1, n, nq)), "v_traj": rng.normal(size=(steps + 1, n, nu)), "u_traj": rng.normal(size=(steps, n, nu)),
         "a_traj": rng.normal(size=(steps, n, nu)), "f_traj": None,
         "trial_q": rng.normal(size=(steps + 1, n, nq)), "trial_v": rng.normal(size=(steps + 1, n, nu)), "trial_u": rng.normal(size=(steps, n, nu)),
         "trial_a": rng.normal(size=(steps, n, nu)), "trial_f": None}
    #                 accepted           armijo                 nan_trial  done   alpha_min
    s["cost"] = np.array([10.0, 10.0, 10.0, 10.0, 10.0])
    s["violation"] = np.array([1.0, 1.0, 1.0, 1.0, 1.0])                       # merit 12
    s["trial_cost"] = np.array([9.0, 11.5, np.nan, 1.0, 13.0])
    s["trial_violation"] = np.array([1.2, 0.2, 0.0, 0.0, 0.0])                 # trial merit 11.4, 11.9, nan, 1, 13
    s["expected"] = np.array([[-2.0, 0.5]] * n)                                # alpha = 1: merit + 0.5 (-2 + 0.5) = 11.25; alpha = 0.3: 12 - 0.2775
    s["alpha"] = np.array([0.5, 1.0, 1.0, 1.0, 0.3])                           # sample 0: 12 + 0.5 (-1 + 0.125) = 11.5625 >= 11.4
    s["done"] = np.array([0, 0, 0, 1, 0], dtype=np.int32)
    s["alpha_accepted"] = np.array([0.0, 0.0, 0.0, 0.25, 0.0])
    return s


def test_accept_referee_on_hand_made_cases():
    s = hand_made()
    new = G.reference_accept(s, CONSTS)
    i = {name: k for k, name in enumerate(CASES)}
    assert list(new["done"]) == [1, 0, 0, 1, 0]
    assert list(new["alpha"]) == [0.5, 0.5, 0.5, 1.0, 0.0]                   # 0.3 * 0.5 = 0.15 < alpha_min: 0
    assert list(new["alpha_accepted"]) == [0.5, 0.0, 0.0, 0.25, 0.0]
    assert list(new["cost"]) == [9.0, 10.0, 10.0, 10.0, 10.0] and list(new["violation"]) == [1.2, 1.0, 1.0, 1.0, 1.0]
    for cur, tri in (("q_traj", "trial_q"), ("v_traj", "trial_v"), ("u_traj", "trial_u"), ("a_traj", "trial_a")):
        assert np.array_equal(new[cur][:, i["accepted"]], s[tri][:, i["accepted"]]), cur
        for name in CASES[1:]:
            assert np.array_equal(new[cur][:, i[name]], s[cur][:, i[name]]), (cur, name)
    assert new["f_traj"] is None
    # the inputs are untouched, the trial arrays too
    assert np.array_equal(hand_made()["q_traj"], s["q_traj"]) and np.array_equal(new["trial_q"], s["trial_q"])
    # on the Armijo bound exactly: accepted (<=)
    s2 = hand_made()
    s2["trial_cost"][1], s2["trial_violation"][1] = 11.25, 0.0
    assert G.reference_accept(s2, CONSTS)["done"][1] == 1
    # a NaN in expected rejects
    s3 = hand_made()
    s3["expected"][0] = np.nan
    assert G.reference_accept(s3, CONSTS)["done"][0] == 0


def test_step_torques_referee():
    u = np.array([[[1.0, -0.0], [2.0, 3.0], [4.0, 5.0]]])
    k = np.array([[[0.5, 7.0], [np.nan, np.inf], [1.0, -1.0]]])
    out = G.reference_step_torques(u, k, np.array([0.25, 0.0, 1.0]))
    assert np.array_equal(out[0, 0], [1.125, 1.75]) and np.array_equal(out[0, 2], [5.0, 4.0])
    assert out[0, 1].tobytes() == u[0, 1].tobytes()                            # alpha = 0: u itself, whatever k holds
    zero = G.reference_step_torques(u, np.ones_like(u), np.zeros(3))
    assert zero.tobytes() == u.tobytes()                                      # (-0.0 keeps its sign)


def test_without_a_device_the_calls_are_refused_not_faked():
    lib = capi.lib()
    assert lib.idocp_rbd_objective_gradients(None, None, 1, 0, 1, 0, None) == -1
    assert b"idocp_rbd_objective_gradients: null handle, objective or io" in lib.idocp_last_error()
    assert lib.idocp_rbd_objective_get_lqr_weights(None, None, None, None) == -1
    assert lib.idocp_rbd_objective_lqr_weights_device(None, None, None, None) == -1
    assert lib.idocp_rbd_ilqr_step_torques(None, 1, 1, None, None, None, None) == -1
    assert lib.idocp_rbd_ilqr_accept(None, 1, 1, None) == -1
    assert lib.idocp_rbd_ilqr_iterate(None, None, 1, 1, None, 0.0, 0.01, None, None, 0) == -1
    assert b"idocp_rbd_ilqr_iterate: null handle, objective or io" in lib.idocp_last_error()
    assert lib.idocp_rbd_ilqr_workspace_bytes(None, 1, 1) == 0
