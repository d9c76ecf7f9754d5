"""The yardstick of the Gauss-Newton residual rows (idocp_rbd_linearize_rollout_cost, idocp_rbd_lqr_backward_gn) without a GPU.

(a) The numpy referee of tests/rbd_gauss_newton.py -- the diagonal gradient plus G^T rho -- against central differences of the numpy stage cost: the
    numpy forward dynamics (rbd_forward.reference), then the cost formula of rbd_score.reference_score, along idocp_model_integrate_configuration
    (q) and along v and u.  The step and the bar are those of test_rbd_gradients_host.py.  ANYmal under its workload's own cost (a_weight and
    f_weight set, u_weight zero) with one foot in the air, chains of 2 and 8 joints under a random a_weight.
(b) 1/2 sum |rho|^2 against the numpy score: the score under the full cost minus the score with a_weight and f_weight zeroed.
(c) The backward pass with G^T G against a dense solve of the whole KKT system with the dense stage Hessian inserted, at the bar of
    test_rbd_lqr_host.py; its float64 form against its long-double form on the inputs test_rbd_lqr_gn_gpu.py uses.
(d) The library exports the calls, capi mirrors the structure, and without a device the calls refuse."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import independent_rbd as IR
import rbd_cases as RC
import rbd_forward as F
import rbd_gauss_newton as GN
import rbd_lqr as L
import rbd_score as RS
from helpers import ROOT, anymal_model, anymal_problem
from idocp_amd import capi
from test_rbd_gradients_host import FD_BAR, H, gradient_cost
from test_rbd_lqr_host import CONDITIONING_BAR, KKT_BAR

DT, T0 = 0.01, 0.3


def full_cost(m, rng=None):
    """a cost with a_weight (and on the quadruped f_weight) set: the ANYmal workload's own, or a random one on a chain"""
    if m.ncontacts:
        return anymal_problem(m, trotting_ref=False)[0]
    cost = gradient_cost(m, rng)
    cost.set("a_weight", rng.uniform(0.01, 0.1, m.nv))
    return cost


def without_rows(cost):
    bare = capi.Cost.from_buffer_copy(cost)
    bare.set("a_weight", np.zeros(len(bare.a_weight)))
    for c in range(4):
        for x in range(3):
            bare.f_weight[c][x] = 0.0
    return bare


@functools.lru_cache(maxsize=None)
def fd_case(which):
    """(model, model dict, cost, tables, q [2][nq], v [2][nv], u [1][nu], active, pts, time step) of one sample, one step and the terminal slice"""
    rng = np.random.default_rng([7, len(which)])
    if which == "anymal":
        m, M, (q, v, _, _, pts, u) = RC.quadruped("anymal")
        cost = full_cost(m)
        q, v, u = np.array([q[0], q[1]]), 0.3 * np.array([v[0], v[1]]), 0.25 * u[:1]
        active, pts, ts = ((1, 0, 1, 1),), pts[:1], RC.TS
    else:
        m, M = IR.chain(int(which[5:]), 1)
        cost = full_cost(m, rng)
        q, v, u = rng.uniform(-1, 1, (2, m.nv)), rng.uniform(-1, 1, (2, m.nv)), rng.uniform(-5, 5, (1, m.nu))
        active, pts, ts = None, None, None
    return m, M, cost, RS.reference_tables(M, cost, T0, DT, 1), q, v, u, active, pts, ts


_SOLVED = {}


def numpy_cost(m, M, cost, tables, q, v, u, active, pts, ts):
    """the total cost of the slices: the numpy forward dynamics at every stage slice, then the formula of the score"""
    nc = GN.contacts_of(m, M)

    def solve(k):      # (remembered: a perturbed terminal slice leaves the stage slices as they were)
        key = (id(M), q[k].tobytes(), v[k].tobytes(), u[k].tobytes())
        if key not in _SOLVED:
            _SOLVED[key] = F.reference(M, q[k], v[k], u[k], active[k] if nc else [], pts[k] if nc else None, ts)
        return _SOLVED[key]

    sol = [solve(k) for k in range(len(u))]
    a = np.array([s[0] for s in sol])
    f = np.array([s[1] for s in sol]) if nc else None
    return RS.reference_score(m, M, cost, None, tables, DT, q, v, u, a, f, active, terminal=True)[0]


def central_differences(m, M, cost, tables, q, v, u, active, pts, ts):
    lib = capi.lib()

    def integrate(qq, d, length):
        out = np.zeros(m.nq)
        capi.check(lib.idocp_model_integrate_configuration(C.byref(m), np.ascontiguousarray(qq).ctypes.data, np.ascontiguousarray(d).ctypes.data, length, out.ctypes.data), "integrate")
        return out

    total = lambda qq, vv, uu: numpy_cost(m, M, cost, tables, qq, vv, uu, active, pts, ts)      # noqa: E731
    steps = len(u)
    lx, lu = np.zeros((steps + 1, 2 * m.nv)), np.zeros((steps, m.nu))
    for k in range(steps + 1):
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
        if k < steps:
            for j in range(m.nu):
                up, um = u.copy(), u.copy()
                up[k, j] += H
                um[k, j] -= H
                lu[k, j] = (total(q, v, up) - total(q, v, um)) / (2 * H)
    return lx, lu


@pytest.mark.parametrize("which", ["anymal", "chain2", "chain8"])
def test_full_gradient_against_central_differences(which):
    """Observed with the step H = eps^(1/3) of test_rbd_gradients_host.py: ANYmal 2.3e-10 (lu; lx 9.6e-11, its force rows included), the chain of 2
    joints 4.9e-12, the chain of 8 joints 1.6e-10; the bar is that test's FD_BAR = 1.3e-8, and the force rows meet it at that step."""
    m, M, cost, tables, q, v, u, active, pts, ts = fd_case(which)
    ref = GN.reference_cost_linearization(m, M, cost, tables, DT, q, v, u, active, pts, ts)
    fx, fu = central_differences(m, M, cost, tables, q, v, u, active, pts, ts)
    assert np.isfinite(ref["lx_traj"]).all() and np.isfinite(ref["lu_traj"]).all()
    dx, du = GN.GR.distance(fx, ref["lx_traj"]), GN.GR.distance(fu, ref["lu_traj"])
    print("%s: |central differences - referee| lx %.2e, lu %.2e (bar %.1e)" % (which, dx, du, FD_BAR))
    assert max(dx, du) < FD_BAR, (which, dx, du)
    # the rows carry weight: without G^T rho the gradient misses the bar by orders of magnitude
    bare = GN.GR.reference_gradients(m, M, cost, tables, DT, q, v, u, terminal=True)
    assert GN.GR.distance(bare[1], ref["lu_traj"]) > 1e3 * FD_BAR
    if which == "anymal":
        R = GN.residual_rows(m.nv, 4)
        assert R == 32 and (ref["G_traj"][0, m.nv + 3:m.nv + 6] == 0).all() and (ref["rho_traj"][0, m.nv + 3:m.nv + 6] == 0).all()      # the lifted foot
        assert (ref["G_traj"][0, m.nv + 12:] == 0).all() and np.abs(ref["G_traj"][0, m.nv:m.nv + 3]).max() > 0


@pytest.mark.parametrize("which", ["anymal", "chain8"])
def test_half_the_squared_rows_is_the_score_of_the_two_terms(which):
    m, M, cost, tables, q, v, u, active, pts, ts = fd_case(which)
    ref = GN.reference_cost_linearization(m, M, cost, tables, DT, q, v, u, active, pts, ts)
    full = numpy_cost(m, M, cost, tables, q, v, u, active, pts, ts)
    bare = numpy_cost(m, M, without_rows(cost), tables, q, v, u, active, pts, ts)
    half = 0.5 * float(np.sum(ref["rho_traj"] ** 2))
    print("%s: 1/2 |rho|^2 = %.15g, score difference %.15g" % (which, half, full - bare))
    assert half > 1e-6 and abs(half - (full - bare)) <= 1e-12 * max(1.0, abs(full))      # (a difference of two sums of |full|: a few ulps of it)


@pytest.mark.parametrize("nx,nu,rows", [(36, 12, 32), (4, 2, 4)])
def test_referee_against_a_dense_kkt_solve(nx, nu, rows):
    steps = 5
    rng = np.random.default_rng(2025 + nx)
    c = GN.random_case_gn(rng, nx, nu, steps, 1, rows)
    A, B, lx, lu, Gt = c["A"][:, 0], c["B"][:, 0], c["lx"][:, 0], c["lu"][:, 0], c["G"][:, 0]
    x0, reg = rng.normal(size=nx), 0.25
    for refined in (False, True):
        ref = GN.referee_gn(A, B, c["wx"], c["wu"], c["wxf"], lx, lu, reg, Gt, refined=refined)
        du_dense, cost_dense = GN.dense_kkt_gn(A, B, c["wx"], c["wu"], c["wxf"], lx, lu, reg, Gt, x0)
        du, _ = L.closed_loop(A, B, ref["K_traj"], ref["k_traj"], x0)
        cost = 0.5 * x0 @ ref["P0"] @ x0 + ref["p0"] @ x0 + ref["expected"][0] + ref["expected"][1]
        d_u, d_c = L.distance(du, du_dense), abs(cost - cost_dense) / max(1.0, abs(cost_dense))
        print("(%d, %d, %d) refined %d: closed loop against the dense du %.2e, cost %.15g against %.15g (%.2e)" % (nx, nu, rows, refined, d_u, cost, cost_dense, d_c))
        assert d_u <= KKT_BAR and d_c <= KKT_BAR, (d_u, d_c)
    # G matters: the diagonal referee on the same case is far from the dense answer
    plain = L.referee(A, B, c["wx"], c["wu"], c["wxf"], lx, lu, reg)
    assert L.distance(L.closed_loop(A, B, plain["K_traj"], plain["k_traj"], x0)[0], du_dense) > 1e-3


@pytest.mark.parametrize("nx,nu,rows,steps", [(36, 12, 32, 3), (36, 12, 4, 3), (16, 8, 8, 3), (4, 2, 4, 3)])
def test_float64_referee_sits_on_the_long_double_one(nx, nu, rows, steps):
    """the inputs of test_rbd_lqr_gn_gpu.py: G at the scale of B needs no scaling down, float64 and long double differ by less than a tenth of the bar"""
    c = GN.random_case_gn(np.random.default_rng(11 + nx + rows), nx, nu, steps, 2, rows)
    plain, refined = GN.referee_gn_batch(c, 0.1), GN.referee_gn_batch(c, 0.1, refined=True)
    for name in ("K_traj", "k_traj", "P0", "p0", "expected"):
        d = L.distance(plain[name], refined[name])
        print("(%d, %d, %d) %s: float64 against long double %.2e" % (nx, nu, rows, name, d))
        assert d < CONDITIONING_BAR and d < 0.1 * L.FLOOR, (name, d)


def test_symbols_and_structure():
    lib = capi.lib()
    for name in ("idocp_rbd_linearize_rollout_cost", "idocp_rbd_lqr_backward_gn", "idocp_rbd_ilqr_iterate_gn"):
        assert hasattr(lib, name) and hasattr(lib, name + "_device"), name
    header = open(os.path.join(ROOT, "include", "idocp_hip.h")).read()
    body = re.search(r"typedef struct idocp_rbd_cost_linearization_io \{(.*?)\} idocp_rbd_cost_linearization_io_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [x.strip(" *") for x in re.sub(r"^(const\s+)?(double|int)\s*", "", decl).split(",")]
    assert fields == [name for name, _ in capi.RbdCostLinearizationIO._fields_], fields


def test_without_a_device_the_calls_are_refused_not_faked():
    lib = capi.lib()
    assert lib.idocp_rbd_linearize_rollout_cost(None, None, 1, 1, None, 0.0, 0.01, None, None, None, None, None, 0) == -1
    assert b"idocp_rbd_linearize_rollout_cost: null handle" in lib.idocp_last_error()
    assert lib.idocp_rbd_lqr_backward_gn(None, 1, 1, None, 4, None) == -1
    assert b"idocp_rbd_lqr_backward_gn: null handle or io" in lib.idocp_last_error()
    assert lib.idocp_rbd_ilqr_iterate_gn(None, None, 1, 1, None, 0.0, 0.01, None, None, 0) == -1
    assert b"idocp_rbd_ilqr_iterate_gn: null handle, objective or io" in lib.idocp_last_error()
    assert lib.idocp_rbd_ilqr_gn_workspace_bytes(None, 1, 1) == 0 and lib.idocp_rbd_objective_residual_rows(None) == 0
