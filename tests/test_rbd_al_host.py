"""The yardstick of the augmented Lagrangian (idocp_rbd_score_al, idocp_rbd_multiplier_update, idocp_rbd_linearize_rollout_al) without a GPU: the
numpy referee of tests/rbd_al.py on the one-stage cases of test_rbd_penalty_host.py, multipliers drawn with the correct signs (a third zero, a
third small, a third large enough to switch on a row that its value alone leaves off).

(a) lambda = 0: the referee IS the penalty referee (np.array_equal on every output).
(b) The referee's merit gradient against central differences of cost + mu sq_shifted, on the step ladder H1, H1 / 2, H1 / 8 and the bar of
    test_rbd_penalty_host.py (a fall by 3 per halving, twice), with its guard on the SHIFTED rows: none within 1e-2 of its kink.
(c) The multiplier identity: the AL gradient at (trajectory, lambda) equals the cost gradient plus sum_k dt (dg/dz)^T lambda+, the gradient of the
    Lagrangian at the updated multipliers.
(d) lambda+ has the right sign on every one-sided row and is 0 on the rows whose shifted value is inactive.
(e) A numpy AL loop against the pure penalty at the same mu on the chain of 2 joints.
(f) The library exports the calls."""
import math

import numpy as np
import pytest

import rbd_al as AL
import rbd_fd_derivatives as D
import rbd_forward as F
import rbd_gauss_newton as GN
import rbd_penalty as PN
import rbd_score as RS
from idocp_amd import capi
from test_rbd_gauss_newton_host import DT
from test_rbd_penalty_host import CASES, H1, MU, central_differences, penalty_case


def unshifted_rows(mm, M, cons, q, v, u, active, pts, ts):
    nc = GN.contacts_of(mm, M)
    a, f = F.reference(M, q, v, u, active[0] if nc else [], pts[0] if nc else None, ts)[:2]
    return AL.al_rows(mm, M, cons, MU, None, q, v, u, np.asarray(a), np.asarray(f) if nc else None, list(active[0]) if nc else [])


def multipliers(which, cone):
    """lambda [1][L] of the case: the first seed whose shifted rows all keep 1e-2 from their kinks (the guard of test_rbd_penalty_host.py)"""
    mm, M, cost, cons, tables, q, v, u, active, pts, ts = penalty_case(which, cone)
    base = unshifted_rows(mm, M, cons, q[0], v[0], u[0], active, pts, ts)
    nc = GN.contacts_of(mm, M)
    a, f = F.reference(M, q[0], v[0], u[0], active[0] if nc else [], pts[0] if nc else None, ts)[:2]
    for seed in range(50):
        lam = AL.draw_multipliers(np.random.default_rng([seed, len(which)]), mm, M, cons, MU, (1,), base["unshifted"][None])
        lam = np.where(base["read"], lam, 0.0)
        mask = list(active[0]) if nc else []
        rows = AL.al_rows(mm, M, cons, MU, lam[0], q[0], v[0], u[0], np.asarray(a), np.asarray(f) if nc else None, mask)
        off = np.where(np.arange(len(lam[0])) >= 4 * mm.nu, base["unshifted"] <= 0, base["unshifted"] == 0) & base["read"]
        switched_on, still_off = (off & (rows["shifted"] != 0)).any(), (rows["shifted"][rows["read"]] == 0).any()
        if (not off.any() or (switched_on and still_off)) and min(kink_distances(mm, M, cons, lam[0], q[0], v[0], u[0], np.asarray(a), np.asarray(f) if nc else None, mask)) > 1e-2:
            return lam
    raise AssertionError("no seed keeps the shifted rows off their kinks with a row switched on and a row left off")


def kink_distances(mm, M, cons, lam, q, v, u, a, f, mask):
    """distance of every read row's shifted value to its kink(s): y to lo and hi of an enabled side, g~ to 0"""
    nu, nv, nq = mm.nu, mm.nv, mm.nq
    rows = AL.al_rows(mm, M, cons, MU, lam, q, v, u, a, f, mask)
    lim = lambda name: np.array(getattr(mm, name)[:nu])      # noqa: E731
    boxes = ((q[nq - nu:], lim("q_min"), lim("q_max")), (v[nv - nu:], -lim("v_max"), lim("v_max")), (u, -lim("u_max"), lim("u_max")),
             (a[nv - nu:], np.array(cons.a_min[:nu]), np.array(cons.a_max[:nu])))
    out = []
    for kind, (x, lo, hi) in enumerate(boxes):
        for j in range(nu):
            y = x[j] + lam[kind * nu + j] / MU
            out += [abs(y - lo[j]), abs(y - hi[j])]
    for row in rows["dg"]:
        out.append(abs(rows["unshifted"][row] + lam[row] / MU))
    return out


def shifted_merit(mm, M, cost, cons, tables, lam, q, v, u, active, pts, ts):
    """cost + MU sq_shifted of the ONE stage slice, from the numpy forward dynamics, the score referee's cost and the shifted rows"""
    nc = GN.contacts_of(mm, M)
    a, f = F.reference(M, q, v, u, active[0] if nc else [], pts[0] if nc else None, ts)[:2]
    a, f = np.asarray(a), (np.asarray(f) if nc else None)
    cost_k = RS.reference_score(mm, M, cost, None, tables, DT, q[None], v[None], u[None], a[None], f[None] if nc else None, active)[0]
    rows = AL.al_rows(mm, M, cons, MU, lam, q, v, u, a, f, list(active[0]) if nc else [])
    return cost_k + MU * DT * 0.5 * math.fsum(x * x for x in rows["shifted"])


@pytest.mark.parametrize("which,cone", CASES)
def test_zero_multipliers_are_the_penalty_referee(which, cone):
    mm, M, cost, cons, tables, q, v, u, active, pts, ts = penalty_case(which, cone)
    pen = PN.reference_penalty_linearization(mm, M, cost, cons, MU, tables, DT, q, v, u, active, pts, ts)
    L = AL.multiplier_rows(mm, M, cons)
    assert L == {("anymal", "linearized"): 68, ("anymal", "nonlinear"): 56, ("chain2", None): 8}[(which, cone)] and L % 2 == 0
    for lam in (None, np.zeros((1, L))):
        al = AL.reference_al_linearization(mm, M, cost, cons, MU, lam, tables, DT, q, v, u, active, pts, ts)
        for name in ("rho_traj", "G_traj", "D_traj", "lx_traj", "lu_traj"):
            assert np.array_equal(al[name], pen[name]), name
        assert al["sq_shifted"] == pen["sq_violation"]


@pytest.mark.parametrize("which,cone", CASES)
def test_merit_gradient_against_central_differences_falls_as_second_order(which, cone):
    """Measured (|central differences - referee| relative to the gradient's largest entry, at H1, H1 / 2, H1 / 8):
      ANYmal, linearized cone  2.92e-04  7.35e-05  2.63e-09   (ratios 3.97, 2.8e4: below the distance to the nearest kink the error collapses)
      ANYmal, FrictionCone     4.07e-05  1.02e-05  6.53e-07   (ratios 4.00, 15.6)
      chain2                   2.01e-08  5.02e-09  3.19e-10   (ratios 4.00, 15.8)"""
    mm, M, cost, cons, tables, q, v, u, active, pts, ts = penalty_case(which, cone)
    lam = multipliers(which, cone)
    ref = AL.reference_al_linearization(mm, M, cost, cons, MU, lam, tables, DT, q, v, u, active, pts, ts)
    grad = np.concatenate([ref["lx_traj"][0], ref["lu_traj"][0]])
    pen = PN.reference_penalty_linearization(mm, M, cost, cons, MU, tables, DT, q, v, u, active, pts, ts)
    assert np.abs(grad - np.concatenate([pen["lx_traj"][0], pen["lu_traj"][0]])).max() > 1e-2 * np.abs(grad).max()      # (the multipliers carry weight)
    # a row that its value alone leaves off is switched on by its multiplier
    rows = AL.reference_al_rows(mm, M, cons, MU, lam[0], DT, q[0], v[0], u[0], None if active is None else active[0], None if pts is None else pts[0], ts)["rows"]
    cone_rows = np.arange(len(lam[0])) >= 4 * mm.nu
    off = np.where(cone_rows, rows["unshifted"] <= 0, rows["unshifted"] == 0) & rows["read"]
    assert not off.any() or ((off & (rows["shifted"] != 0)).any() and (rows["shifted"][rows["read"]] == 0).any())      # (chain2: no row is off)
    merit = lambda mm_, M_, cost_, cons_, tables_, qq, vv, uu, active_, pts_, ts_: (shifted_merit(mm_, M_, cost_, cons_, tables_, lam[0], qq, vv, uu, active_, pts_, ts_), None)      # noqa: E731
    import test_rbd_penalty_host as TP
    keep = TP.stage_merit
    TP.stage_merit = merit      # (central_differences of that file differentiates the module's stage_merit)
    try:
        err = []
        for h in (H1, H1 / 2, H1 / 8):
            fd = central_differences(mm, M, cost, cons, tables, q[0], v[0], u[0], active, pts, ts, h)
            err.append(np.abs(fd - grad).max() / np.abs(grad).max())
    finally:
        TP.stage_merit = keep
    print("%s %s: |central differences - referee| / |gradient| at H = %.0e, H / 2, H / 8: %s, ratios %s" % (
        which, cone, H1, " ".join("%.2e" % e for e in err), " ".join("%.2f" % (a / b) for a, b in zip(err[:-1], err[1:]))))
    assert err[1] <= err[0] / 3 and err[2] <= err[1] / 3, (which, cone, err)


@pytest.mark.parametrize("which,cone", CASES)
def test_the_gradient_is_the_lagrangians_at_the_updated_multipliers_and_the_signs(which, cone):
    mm, M, cost, cons, tables, q, v, u, active, pts, ts = penalty_case(which, cone)
    lam = multipliers(which, cone)
    ref = AL.reference_al_linearization(mm, M, cost, cons, MU, lam, tables, DT, q, v, u, active, pts, ts)
    rows = AL.reference_al_rows(mm, M, cons, MU, lam[0], DT, q[0], v[0], u[0], None if active is None else active[0], None if pts is None else pts[0], ts)["rows"]
    plus = MU * rows["shifted"]
    grad = np.concatenate([ref["lx_traj"][0], ref["lu_traj"][0]])
    lagrangian = np.concatenate([ref["cost_lx"][0], ref["cost_lu"][0]]) + DT * ref["J"][0].T @ plus
    dist = np.abs(grad - lagrangian).max() / np.abs(grad).max()
    print("%s %s: |AL gradient - (cost gradient + dt J^T lambda+)| / |gradient| = %.2e" % (which, cone, dist))
    assert dist <= 1e-12      # (the same products in another order: s (s h) against dt (mu h))
    # the signs: cone rows and upper sides >= 0, lower sides <= 0, and 0 exactly where the shifted value is inactive
    nu = mm.nu
    assert (plus[4 * nu:] >= 0).all()
    assert ((plus != 0) == (rows["shifted"] != 0)).all() and (plus[~rows["read"]] == 0).all()
    assert (np.sign(plus[:4 * nu]) == np.sign(rows["shifted"][:4 * nu])).all()
    only_upper = capi.Constraints.from_buffer_copy(cons)
    only_upper.joint_acceleration_lower_limit = 0
    r2 = AL.reference_al_rows(mm, M, only_upper, MU, np.abs(lam[0]), DT, q[0], v[0], u[0], None if active is None else active[0], None if pts is None else pts[0], ts)["rows"]
    assert (r2["shifted"][3 * nu:4 * nu] >= 0).all() and (r2["shifted"][3 * nu:4 * nu] > 0).any()


# ---- (e) the numpy AL loop

def chain_rollout(M, q0, v0, u, dt, K=None, kff=None, alpha=0.0, ref=None):
    q, v, us, acc = [np.array(q0)], [np.array(v0)], [], []
    for k in range(len(u)):
        uk = np.array(u[k])
        if K is not None:
            uk = uk + alpha * kff[k] + K[k] @ np.concatenate([q[k] - ref[0][k], v[k] - ref[1][k]])
        a = np.asarray(F.reference(M, q[k], v[k], uk, [], None, None)[0])
        us.append(uk); acc.append(a)
        q.append(q[k] + dt * v[k]); v.append(v[k] + dt * a)
    return np.array(q), np.array(v), np.array(us), np.array(acc)


def al_loop(mm, M, cost, cons, tables, dt, q0, v0, u0, mu, passes, update_every):
    """`passes` backward passes at fixed mu; update_every = 0: the pure penalty (lambda stays 0).  Returns the final infeasibility."""
    from test_rbd_ilqr_gn_gpu import numpy_weights
    steps, L = len(u0), AL.multiplier_rows(mm, M, cons)
    wx, wu, wxf = numpy_weights(mm, cost, dt)
    q, v, u, a = chain_rollout(M, q0, v0, u0, dt)
    lam = np.zeros((steps, L))

    def merit(q, v, u, a):
        c = RS.reference_score(mm, M, cost, None, tables, dt, q, v, u, a, None, None, terminal=True)[0]
        return c + mu * AL.reference_score_update(mm, M, cons, mu, dt, lam, q[:steps], v[:steps], u, a, None, None)["sq_shifted"]

    for it in range(passes):
        lin = AL.reference_al_linearization(mm, M, cost, cons, mu, lam, tables, dt, q, v, u)
        AB = [D.reference(M, q[k], v[k], u[k], [], None, None, dt) for k in range(steps)]
        lqr = PN.referee_gn_diag(np.array([d["A"] for d in AB]), np.array([d["B"] for d in AB]), wx, wu, wxf, lin["lx_traj"], lin["lu_traj"], 1e-6,
                                 lin["G_traj"], lin["D_traj"])
        now, alpha = merit(q, v, u, a), 1.0
        while alpha >= 1e-3:
            trial = chain_rollout(M, q[0], v[0], u, dt, lqr["K_traj"], lqr["k_traj"], alpha, (q, v))
            if merit(*trial) < now:
                q, v, u, a = trial
                break
            alpha *= 0.5
        if update_every and (it + 1) % update_every == 0:
            lam = AL.reference_score_update(mm, M, cons, mu, dt, lam, q[:steps], v[:steps], u, a, None, None)["lambda_plus"]
    return AL.reference_score_update(mm, M, cons, mu, dt, lam, q[:steps], v[:steps], u, a, None, None)["infeasibility"]


def test_multiplier_rounds_end_more_feasible_than_the_penalty_at_the_same_mu():
    """chain2, n = 1, 4 steps, mu = 5 fixed, 8 backward passes each: the pure penalty against AL with a multiplier update after every second
    pass.  Measured (infeasibility = the largest unshifted row at the end): penalty 7.1404e-01, AL 2.7336e-01.  The bounds sit at the medians
    of the first rollout, so the FIXED initial state violates its own rows: 0.2731 is the floor no torque sequence gets under, and AL is on it
    after 8 passes (12 or 16 passes: 2.7307e-01).  The budget was chosen on the CPU: at mu = 20 and 100 the penalty alone is already at the floor
    (2.6757e-01 and 2.7195e-01 against AL's 2.7307e-01 -- on an infeasible problem the penalty trades the floor row against the others) and
    the comparison shows nothing; the moderate mu is where multipliers pay."""
    import independent_rbd as IR
    from test_rbd_gauss_newton_host import full_cost
    from test_rbd_penalty_gpu import median_bounds
    steps, dt, mu = 4, 0.01, 5.0
    m, M = IR.chain(2, 1)
    rng = np.random.default_rng(5)
    cost = full_cost(m, rng)
    q0, v0, u0 = rng.uniform(-0.5, 0.5, m.nv), rng.uniform(-0.5, 0.5, m.nv), rng.uniform(-3, 3, (steps, m.nu))
    q, v, u, a = chain_rollout(M, q0, v0, u0, dt)
    mm, cons = median_bounds(m, M, q[:steps, None], v[:steps, None], u[:, None], a[:, None], None, None)
    tables = RS.reference_tables(M, cost, 0.0, dt, steps)
    pen = al_loop(mm, M, cost, cons, tables, dt, q0, v0, u0, mu, 8, 0)
    aug = al_loop(mm, M, cost, cons, tables, dt, q0, v0, u0, mu, 8, 2)
    print("chain2, mu %.0f, 8 passes: infeasibility penalty %.4e, AL %.4e" % (mu, pen, aug))
    assert aug < pen


def test_the_library_exports_the_calls():
    lib = capi.lib()
    for name in ("idocp_rbd_score_al", "idocp_rbd_multiplier_update", "idocp_rbd_linearize_rollout_al", "idocp_rbd_ilqr_iterate_al", "idocp_rbd_ilqr_al_update"):
        assert hasattr(lib, name) and hasattr(lib, name + "_device"), name
    assert lib.idocp_rbd_objective_multiplier_rows(None) == 0
