"""idocp_rbd_ilqr_iterate_penalty on the GPU at n = 5, steps = 4, trials = 2, on the cases of test_rbd_penalty_gpu.py (bounds at the medians of the
first rollout, so every sample starts with a positive sq_violation): one iteration bit for bit the chain of the individual calls, in host form and
in device form on the caller's workspace; the merit cost + mu sq_violation per sample never rises over three iterations; with constraints = NULL the
iteration compares equal to idocp_rbd_ilqr_iterate_gn; and the effectiveness check -- mu chosen so that mu sq_violation is at least ten times the
cost at the start, the mean sq_violation after three iterations below the start's and below that of three idocp_rbd_ilqr_iterate_gn iterations
from the same start."""
import numpy as np
import pytest

import rbd_gauss_newton as GN
import rbd_gradients as G
import rbd_penalty as PN
import rbd_policy as PO
import rbd_score as RS
from idocp_amd import capi
from rbd_batch import DeviceArray, Rbd
from test_rbd_ilqr_gn_gpu import numpy_weights
from test_rbd_ilqr_gpu import ILQR, TRAJ, same
from test_rbd_penalty_gpu import N, STEPS, T0, case

pytestmark = pytest.mark.gpu

TRIALS = 2
CASES = [("anymal", "linearized"), ("anymal", "nonlinear"), ("chain2", None)]


def first(r, o, which, cone):
    """the rolled-out start as the dict the iteration takes: `violation` holds sq_violation"""
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone)
    c, _, _ = RS.score(r, o, q, v, u, a, f, active, terminal=True, want_stage=False)
    sq = PN.score_penalty(r, o, q[:STEPS], v[:STEPS], u, a, f, active)
    return dict(q_traj=q, v_traj=v, u_traj=u, a_traj=a, f_traj=f, cost=c, violation=sq)


def by_hand(r, M, cons, o, cost, which, cone, traj, consts, trials):
    """the chain of idocp_rbd_ilqr_iterate_penalty as individual calls"""
    mm, _, _, _, _, active, pts, ts, dt, _ = case(which, cone)
    t = {k: (None if x is None else x.copy()) for k, x in traj.items()}
    lin = PN.linearize_penalty(r, M, cons, o, consts["penalty"], t["q_traj"], t["v_traj"], t["u_traj"], active, ts, dt, pts,
                               want=("A_traj", "B_traj", "G_traj", "D_traj", "lx_traj", "lu_traj"))
    wx, wu, wxf = numpy_weights(mm, cost, dt)
    lqr = PN.backward_gn_diag(r, lin["A_traj"], lin["B_traj"], wx, wu, wxf, lin["lx_traj"], lin["lu_traj"], consts["regularization"], lin["G_traj"],
                              lin["D_traj"], outputs=("K_traj", "k_traj", "expected", "status"))
    K_cm = np.ascontiguousarray(lqr["K_traj"].transpose(0, 1, 3, 2)).reshape(STEPS, N, -1)
    state = dict(t, expected=lqr["expected"], alpha=np.ones(N), done=np.zeros(N, dtype=np.int32), alpha_accepted=np.zeros(N))
    for _ in range(trials):
        u_ff = G.step_torques(r, state["u_traj"], lqr["k_traj"], state["alpha"])
        qt, vt, ut, at, ft = PO.rollout_policy(r, state["q_traj"][0], state["v_traj"][0], STEPS, active, ts, dt, pts, u_ff=u_ff, K=K_cm,
                                               q_ref=state["q_traj"][:STEPS], v_ref=state["v_traj"][:STEPS])
        ct, _, _ = RS.score(r, o, qt, vt, ut, at, ft, active, terminal=True, want_stage=False)
        gt = PN.score_penalty(r, o, qt[:STEPS], vt[:STEPS], ut, at, ft, active)
        state.update(trial_q=qt, trial_v=vt, trial_u=ut, trial_a=at, trial_f=ft, trial_cost=ct, trial_violation=gt)
        state = G.accept(r, state, consts)
    return {k: state[k] for k in TRAJ}, {"alpha_accepted": state["alpha_accepted"], "lqr_status": lqr["status"], "expected": lqr["expected"]}


@pytest.mark.parametrize("which,cone", CASES)
def test_the_chained_iteration_equals_the_individual_calls(which, cone):
    mm, M, cost, cons, tables, active, pts, ts, dt, _ = case(which, cone)
    consts = dict(ILQR, penalty=25.0)
    r = Rbd(mm)
    o = RS.Objective(r, cost, cons, T0, dt, STEPS)
    traj = first(r, o, which, cone)
    new, out = PN.iterate_penalty(r, o, traj, consts, TRIALS, active, ts, dt, pts)
    want, want_out = by_hand(r, M, cons, o, cost, which, cone, traj, consts, TRIALS)
    for name in TRAJ:
        assert same(new[name], want[name]), (which, cone, name)
    for name in out:
        assert same(out[name], want_out[name]), (which, cone, name)
    assert (out["lqr_status"] == -1).all()
    print("%s %s: alpha accepted %s, sq_violation %s -> %s" % (which, cone, out["alpha_accepted"], traj["violation"], new["violation"]))
    # the device form on the caller's workspace: the same bits again
    nbytes = r.lib.idocp_rbd_ilqr_penalty_workspace_bytes(r.h, o.h, N, STEPS)
    Rc, nz = r.lib.idocp_rbd_objective_constraint_rows(o.h), 2 * mm.nv + mm.nu
    assert nbytes % 16 == 0 and nbytes >= r.lib.idocp_rbd_ilqr_gn_workspace_bytes(r.h, N, STEPS) + 8 * STEPS * N * (Rc + 1) * nz
    dev = {k: DeviceArray(x) for k, x in traj.items() if x is not None}
    dev.update(alpha_accepted=DeviceArray(np.zeros(N)), expected=DeviceArray(np.zeros((N, 2))), lqr_status=DeviceArray(np.zeros((N + 1) // 2)),
               workspace=DeviceArray(np.zeros(nbytes // 8)))
    d_pts = DeviceArray(pts) if pts is not None else None
    io = G.ilqr_struct({k: d.ptr.value for k, d in dev.items()}, consts, TRIALS)
    capi.check(PN.iterate_penalty_raw(r, o, N, STEPS, active, ts, dt, d_pts.ptr.value if d_pts else None, io, device=True), "idocp_rbd_ilqr_iterate_penalty_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    for name in TRAJ:
        if traj[name] is not None:
            assert same(dev[name].numpy(), new[name]), (which, cone, name)
    assert same(dev["alpha_accepted"].numpy(), out["alpha_accepted"]) and same(dev["expected"].numpy(), out["expected"])
    for d in list(dev.values()) + ([d_pts] if d_pts else []):
        d.free()
    o.close()
    r.close()


@pytest.mark.parametrize("which,cone", [("anymal", "linearized"), ("chain2", None)])
def test_without_constraints_it_is_the_gn_iteration(which, cone):
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone)
    r = Rbd(mm)
    o = RS.Objective(r, cost, None, T0, dt, STEPS)
    c, g, _ = RS.score(r, o, q, v, u, a, f, active, terminal=True, want_stage=False)
    traj = dict(q_traj=q, v_traj=v, u_traj=u, a_traj=a, f_traj=f, cost=c, violation=g)
    assert (g == 0).all() and (PN.score_penalty(r, o, q[:STEPS], v[:STEPS], u, a, f, active) == 0).all()
    consts = dict(ILQR, penalty=25.0)
    want, want_out = GN.iterate_gn(r, o, traj, consts, TRIALS, active, ts, dt, pts)
    got, got_out = PN.iterate_penalty(r, o, traj, consts, TRIALS, active, ts, dt, pts)
    for name in TRAJ:
        assert (want[name] is None and got[name] is None) or np.array_equal(got[name], want[name]), name
    for name in want_out:
        assert np.array_equal(got_out[name], want_out[name]), name
    o.close()
    r.close()


@pytest.mark.parametrize("which,cone", CASES)
def test_merit_never_rises_and_the_violation_falls(which, cone):
    """Measured on an MI355X, one run (mean over the 5 samples; start -> three penalty iterations | three GN iterations from the same start):
      ANYmal, linearized cone, mu 3.67:  cost 4.793 -> 4.209 | 0.0990,  sq_violation 22.02 -> 3.805 | 238.8
      ANYmal, FrictionCone, mu 0.276:    cost 4.793 -> 4.412 | 0.0990,  sq_violation 235.3 -> 170.0 | 238.8  (two of five samples take no step)
      chain2, mu 12.0:                   cost 10.69 -> 5.754 | 2.706,   sq_violation 25.85 -> 0.178 | 9.538
    The cost-only iteration drives ANYmal's violation UP by an order of magnitude under the linearized cone; the penalty brings it down."""
    mm, M, cost, cons, tables, active, pts, ts, dt, _ = case(which, cone)
    r = Rbd(mm)
    o = RS.Objective(r, cost, cons, T0, dt, STEPS)
    start = first(r, o, which, cone)
    assert (start["violation"] > 0).all()
    mu = float(10.0 * (start["cost"] / start["violation"]).max())      # mu sq_violation >= 10 cost on every sample
    assert (mu * start["violation"] >= 10.0 * start["cost"]).all()
    consts = dict(ILQR, penalty=mu)
    traj, merits = start, [start["cost"] + mu * start["violation"]]
    for it in range(3):
        traj, out = PN.iterate_penalty(r, o, traj, consts, TRIALS, active, ts, dt, pts)
        merits.append(traj["cost"] + mu * traj["violation"])
        print("%s %s penalty iteration %d: alpha %s, status %s" % (which, cone, it, out["alpha_accepted"], out["lqr_status"]))
    for before, after in zip(merits[:-1], merits[1:]):
        assert (after <= before).all(), (before, after)      # exactly: a rejected sample keeps its scores
    plain = dict(start)
    for it in range(3):
        plain, _ = GN.iterate_gn(r, o, plain, dict(ILQR), TRIALS, active, ts, dt, pts)
    q, v, u, a, f = (plain[k] for k in ("q_traj", "v_traj", "u_traj", "a_traj", "f_traj"))
    sq_gn = PN.score_penalty(r, o, q[:STEPS], v[:STEPS], u, a, f, active)
    print("%s %s mu %.3g: mean cost %.4g -> %.4g (GN %.4g); mean sq_violation %.4g -> %.4g (GN %.4g)" % (
        which, cone, mu, start["cost"].mean(), traj["cost"].mean(), plain["cost"].mean(), start["violation"].mean(), traj["violation"].mean(), sq_gn.mean()))
    assert traj["violation"].mean() < start["violation"].mean()
    assert traj["violation"].mean() < sq_gn.mean()
    o.close()
    r.close()


def test_more_than_one_score_window_is_the_windowed_chain_of_calls():
    """steps = IDOCP_RBD_SCORE_MAX_WINDOW + 6 on the chain of 2 joints, n = 2, one trial round: the trial scores are formed window by window with
    accumulate, the trial `violation` is sq_violation ALONE (the score call's L1 sum never enters it), and the iteration is bit for bit the chain of
    the individual calls windowed the same way."""
    import independent_rbd as IR
    from test_rbd_gauss_newton_host import full_cost
    from test_rbd_penalty_gpu import median_bounds
    W, n = capi.RBD_SCORE_MAX_WINDOW, 2
    steps, dt = W + 6, 0.002
    m, M = IR.chain(2, 1)
    rng = np.random.default_rng(97)
    cost = full_cost(m, rng)
    q0, v0, u = rng.uniform(-0.5, 0.5, (n, m.nv)), rng.uniform(-0.5, 0.5, (n, m.nv)), rng.uniform(-0.5, 0.5, (steps, n, m.nu))
    r0 = Rbd(m)
    q, v, a, _ = GN.F.rollout(r0, q0, v0, u, None, 0.0, dt, None)
    r0.close()
    assert np.isfinite(q).all()
    mm, cons = median_bounds(m, M, q[:steps], v[:steps], u, a, None, None)
    r = Rbd(mm)
    o = RS.Objective(r, cost, cons, T0, dt, steps)

    def scores(qt, vt, ut, at):      # (cost, sq_violation) window by window, as the iteration forms them
        c, _, _ = RS.score(r, o, qt[:W], vt[:W], ut[:W], at[:W], None, None, want_stage=False, want=("cost",))
        c, _, _ = RS.score(r, o, qt[W:], vt[W:], ut[W:], at[W:], None, None, first_step=W, terminal=True, accumulate=(c, None), want_stage=False, want=("cost",))
        sq = PN.score_penalty(r, o, qt[:W], vt[:W], ut[:W], at[:W])
        return c, PN.score_penalty(r, o, qt[W:steps], vt[W:steps], ut[W:], at[W:], first_step=W, accumulate=sq)

    c0, sq0 = scores(q, v, u, a)
    assert (sq0 > 0).all()
    consts = dict(ILQR, penalty=5.0)
    traj = dict(q_traj=q, v_traj=v, u_traj=u, a_traj=a, f_traj=None, cost=c0, violation=sq0)
    new, out = PN.iterate_penalty(r, o, traj, consts, 1, None, 0.0, dt, None)
    # by hand
    lin = PN.linearize_penalty(r, M, cons, o, 5.0, q, v, u, None, 0.0, dt, None, want=("A_traj", "B_traj", "G_traj", "D_traj", "lx_traj", "lu_traj"))
    wx, wu, wxf = numpy_weights(mm, cost, dt)
    lqr = PN.backward_gn_diag(r, lin["A_traj"], lin["B_traj"], wx, wu, wxf, lin["lx_traj"], lin["lu_traj"], consts["regularization"], lin["G_traj"], lin["D_traj"],
                              outputs=("K_traj", "k_traj", "expected", "status"))
    K_cm = np.ascontiguousarray(lqr["K_traj"].transpose(0, 1, 3, 2)).reshape(steps, n, -1)
    state = dict({k: (None if x is None else x.copy()) for k, x in traj.items()}, expected=lqr["expected"], alpha=np.ones(n), done=np.zeros(n, dtype=np.int32),
                 alpha_accepted=np.zeros(n))
    u_ff = G.step_torques(r, u, lqr["k_traj"], state["alpha"])
    qt, vt, ut, at, _ = PO.rollout_policy(r, q[0], v[0], steps, None, 0.0, dt, None, u_ff=u_ff, K=K_cm, q_ref=q[:steps], v_ref=v[:steps])
    ct, gt = scores(qt, vt, ut, at)
    state.update(trial_q=qt, trial_v=vt, trial_u=ut, trial_a=at, trial_f=None, trial_cost=ct, trial_violation=gt)
    state = G.accept(r, state, consts)
    print("two windows: alpha %s, status %s, cost %s -> %s, sq_violation %s -> %s" % (out["alpha_accepted"], out["lqr_status"], c0, new["cost"], sq0, new["violation"]))
    for name in TRAJ:
        assert same(new[name], state[name]), name
    assert same(out["alpha_accepted"], state["alpha_accepted"]) and same(out["expected"], lqr["expected"]) and same(out["lqr_status"], lqr["status"])
    assert (out["alpha_accepted"] > 0).any()      # (an accepted trial: its violation is the one written back)
    o.close()
    r.close()
