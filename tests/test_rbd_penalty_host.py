"""The yardstick of the constraint penalty (idocp_rbd_score_penalty, idocp_rbd_linearize_rollout_penalty) without a GPU.

(a) The numpy referee of tests/rbd_penalty.py -- the cost gradient plus Gc^T sigma plus the diagonal terms -- against central differences of its
    own one-stage merit in (dq, dv, du): the numpy forward dynamics, the cost formula of rbd_score.reference_score and mu dt / 2 sum max(0, g)^2
    over the rows of rbd_score.constraint_rows.  Three steps, H1 = 2e-4, H1 / 2 and H1 / 8, all above the step at which rounding takes over
    (eps^(1/3) = 6e-6): the error of a central difference is c H^2 there, so it must fall by 4 per halving; the test asks for 3 from H1 to
    H1 / 2 and for 3 again from H1 / 2 to H1 / 8.  Bounds sit beside the nominal values so that every kind has active rows, none within 1e-2 of
    its kink; the friction coefficient sits in the widest gap between the tangential-to-normal ratios.
    Measured (|central differences - referee| relative to the gradient's largest entry, at H1, H1 / 2, H1 / 4, H1 / 8):
      ANYmal, linearized cone  2.77e-03  9.18e-04  1.64e-04  4.00e-09   (ratios 3.02, 5.59, 4.1e4)
      ANYmal, FrictionCone     3.50e-05  8.70e-06  2.16e-06  6.37e-07   (ratios 4.02, 4.03, 3.39)
      chain2                   1.61e-07  4.02e-08  (H1, H1 / 2: ratio 4.00)
    The linearized cone's slow fall at the larger steps is a force row crossing its kink INSIDE the step (df/dq is of the order 1e3, so a step
    of 2e-4 moves a force row by 0.2 while the guard keeps rows only 1e-2 away; the squared hinge is only once differentiable): once the step
    is below the distance to the kink, at H1 / 8, the error collapses by four orders to 4.0e-09.  A wrong term in the referee would leave a
    floor; there is none down to 4e-09.
(b) sq_violation of the referee against the rows of the score referee: for one sample the rows with g > 0 are the same numbers, and
    sum dt h^2 / 2 recomputed with math.fsum is the referee's.
(c) The library exports the calls and capi mirrors the structure."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import rbd_forward as F
import rbd_gauss_newton as GN
import rbd_penalty as PN
import rbd_score as RS
from idocp_amd import capi
from test_rbd_gauss_newton_host import DT, fd_case

MU = 40.0
H1 = 2e-4


def bounds_beside(m, M, q, v, u, a, f, cone, mask):
    """(model with limits, constraints): every third joint violates the upper side by 0.1 .. 0.3, every third the lower side, the rest is inside; the
    friction coefficient at the median of the tangential-to-normal ratios of the active contacts"""
    nu, nv, nq = m.nu, m.nv, m.nq
    mm = capi.Model.from_buffer_copy(m)
    cons = capi.Constraints()
    cons.joint_position_limits = cons.joint_velocity_limits = cons.joint_torque_limits = 1
    cons.joint_acceleration_lower_limit = cons.joint_acceleration_upper_limit = 1
    side = np.arange(nu) % 3      # 0: above hi, 1: below lo, 2: inside
    off = 0.1 + 0.1 * (np.arange(nu) % 3)

    def box(x):
        lo = np.where(side == 1, x + off, x - 1.0)
        hi = np.where(side == 0, x - off, x + 1.0)
        return lo, np.maximum(hi, lo)

    lo, hi = box(q[nq - nu:])
    mm.q_min[:nu], mm.q_max[:nu] = lo, hi
    for name, x in (("v_max", v[nv - nu:]), ("u_max", u)):      # symmetric boxes: |x| - off on the violated joints, |x| + 1 inside
        getattr(mm, name)[:nu] = np.where(side == 2, np.abs(x) + 1.0, np.maximum(np.abs(x) - off, 0.0))
    lo, hi = box(a[nv - nu:])
    cons.a_min[:nu], cons.a_max[:nu] = lo, hi
    if cone and f is not None:
        on = [c for c in range(len(mask)) if mask[c]]
        if cone == "linearized":      # (one ratio per row pair: the x rows and the y rows of every active contact)
            ratios = sorted(abs(f[c][x]) * math.sqrt(2.0) / f[c][2] for c in on for x in (0, 1))
        else:
            ratios = sorted(math.hypot(f[c][0], f[c][1]) / f[c][2] for c in on)
        # between two neighbouring ratios, in the widest gap that leaves rows on either side: no row sits near its kink
        gaps = [(ratios[i + 1] - ratios[i], i) for i in range(len(ratios) - 1)]
        i = max(gaps)[1]
        cons.mu = 0.5 * (ratios[i] + ratios[i + 1])
        cons.linearized_friction_cone = int(cone == "linearized")
        cons.friction_cone = int(cone == "nonlinear")
    return mm, cons


@functools.lru_cache(maxsize=None)
def penalty_case(which, cone):
    m, M, cost, tables, q, v, u, active, pts, ts = fd_case(which)
    nc = GN.contacts_of(m, M)
    a, f = F.reference(M, q[0], v[0], u[0], active[0] if nc else [], pts[0] if nc else None, ts)[:2]
    mm, cons = bounds_beside(m, M, q[0], v[0], u[0], np.asarray(a), np.asarray(f) if nc else None, cone, active[0] if nc else [])
    return mm, M, cost, cons, tables, q, v, u, active, pts, ts


def stage_merit(mm, M, cost, cons, tables, q, v, u, active, pts, ts):
    """cost + MU sq_violation of the ONE stage slice, from the numpy forward dynamics and the formulas of the score referee"""
    nc = GN.contacts_of(mm, M)
    a, f = F.reference(M, q, v, u, active[0] if nc else [], pts[0] if nc else None, ts)[:2]
    a, f = np.asarray(a), (np.asarray(f) if nc else None)
    cost_k = RS.reference_score(mm, M, cost, None, tables, DT, q[None], v[None], u[None], a[None], f[None] if nc else None, active)[0]
    rows = RS.constraint_rows(mm, cons, q, v, u, a, f if nc else np.zeros((0, 3)), list(active[0]) if nc else [])
    return cost_k + MU * DT * 0.5 * math.fsum(max(0.0, g) ** 2 for g in rows), rows


def central_differences(mm, M, cost, cons, tables, q, v, u, active, pts, ts, h):
    lib = capi.lib()

    def integrate(qq, d, length):
        out = np.zeros(mm.nq)
        capi.check(lib.idocp_model_integrate_configuration(C.byref(mm), np.ascontiguousarray(qq).ctypes.data, np.ascontiguousarray(d).ctypes.data, length, out.ctypes.data), "integrate")
        return out

    merit = lambda qq, vv, uu: stage_merit(mm, M, cost, cons, tables, qq, vv, uu, active, pts, ts)[0]      # noqa: E731
    g = np.zeros(2 * mm.nv + mm.nu)
    for r in range(mm.nv):
        e = np.zeros(mm.nv)
        e[r] = 1.0
        g[r] = (merit(integrate(q, e, h), v, u) - merit(integrate(q, e, -h), v, u)) / (2 * h)
        g[mm.nv + r] = (merit(q, v + h * e, u) - merit(q, v - h * e, u)) / (2 * h)
    for j in range(mm.nu):
        e = np.zeros(mm.nu)
        e[j] = 1.0
        g[2 * mm.nv + j] = (merit(q, v, u + h * e) - merit(q, v, u - h * e)) / (2 * h)
    return g


CASES = [("anymal", "linearized"), ("anymal", "nonlinear"), ("chain2", None)]


@pytest.mark.parametrize("which,cone", CASES)
def test_merit_gradient_against_central_differences_falls_as_second_order(which, cone):
    mm, M, cost, cons, tables, q, v, u, active, pts, ts = penalty_case(which, cone)
    ref = PN.reference_penalty_linearization(mm, M, cost, cons, MU, tables, DT, q, v, u, active, pts, ts)
    grad = np.concatenate([ref["lx_traj"][0], ref["lu_traj"][0]])
    bare = GN.reference_cost_linearization(mm, M, cost, tables, DT, q, v, u, active, pts, ts)
    assert np.abs(grad - np.concatenate([bare["lx_traj"][0], bare["lu_traj"][0]])).max() > 1e-2 * np.abs(grad).max()      # (the penalty carries weight)
    rows = stage_merit(mm, M, cost, cons, tables, q[0], v[0], u[0], active, pts, ts)[1]
    assert min(abs(g) for g in rows) > 1e-2      # (no row near its kink: the merit is smooth over both steps)
    err = []
    for h in (H1, H1 / 2, H1 / 8):
        fd = central_differences(mm, M, cost, cons, tables, q[0], v[0], u[0], active, pts, ts, h)
        err.append(np.abs(fd - grad).max() / np.abs(grad).max())
    print("%s %s: |central differences - referee| / |gradient| at H = %.0e, H / 2, H / 8: %s, ratios %s" % (
        which, cone, H1, " ".join("%.2e" % e for e in err), " ".join("%.2f" % (a / b) for a, b in zip(err[:-1], err[1:]))))
    assert err[1] <= err[0] / 3 and err[2] <= err[1] / 3, (which, cone, err)


@pytest.mark.parametrize("which,cone", CASES)
def test_sq_violation_is_the_score_referees_rows_squared(which, cone):
    mm, M, cost, cons, tables, q, v, u, active, pts, ts = penalty_case(which, cone)
    nc = GN.contacts_of(mm, M)
    p = PN.reference_penalty_rows(mm, M, cons, MU, DT, q[0], v[0], u[0], active[0] if nc else None, pts[0] if nc else None, ts)
    rows = stage_merit(mm, M, cost, cons, tables, q[0], v[0], u[0], active, pts, ts)[1]
    positive = sorted(g for g in rows if g > 0)
    assert len(positive) >= 4 and len(positive) < len(rows)
    assert len(p["h"]) == len(positive) and np.allclose(sorted(p["h"]), positive, rtol=1e-9, atol=0)      # (two forward solves: the refined one and the plain one)
    again = DT * 0.5 * math.fsum(h * h for h in p["h"])
    assert again == p["sq"] and p["sq"] > 0
    # sigma, D and the gradient are those of 1/2 |sigma|^2 + the boxes: |sigma|^2 / 2 + the diagonal share is mu sq
    nu = mm.nu
    diag = sum(x * x for x in p["gdiag"]) / (2 * DT * MU)      # (dt mu b)^2 / (2 dt mu) = dt mu b^2 / 2
    assert abs(0.5 * float(p["sigma"] @ p["sigma"]) + diag - MU * p["sq"]) <= 1e-12 * MU * p["sq"]
    assert PN.constraint_rows(mm, M, cons) == {("anymal", "linearized"): 32, ("anymal", "nonlinear"): 20, ("chain2", None): 4}[(which, cone)]
    assert (p["D"][:mm.nv - nu] == 0).all() and set(np.unique(p["D"])) <= {0.0, DT * MU} and (p["D"] == DT * MU).any()


def test_the_library_exports_the_calls_and_capi_mirrors_the_structure():
    lib = capi.lib()
    for name in ("idocp_rbd_objective_constraint_rows", "idocp_rbd_score_penalty", "idocp_rbd_linearize_rollout_penalty", "idocp_rbd_lqr_backward_gn_diag",
                 "idocp_rbd_ilqr_iterate_penalty"):
        assert hasattr(lib, name) and (name.endswith("_rows") or hasattr(lib, name + "_device")), name
    assert hasattr(lib, "idocp_rbd_ilqr_penalty_workspace_bytes")
    assert lib.idocp_rbd_objective_constraint_rows(None) == 0 and lib.idocp_rbd_ilqr_penalty_workspace_bytes(None, None, 4, 4) == 0
    assert C.sizeof(capi.RbdPenaltyLinearizationIO) == 7 * C.sizeof(C.c_void_p)
