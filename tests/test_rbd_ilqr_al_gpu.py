"""idocp_rbd_ilqr_iterate_al and idocp_rbd_ilqr_al_update on the GPU at n = 5, steps = 4, trials = 2, on the cases of test_rbd_penalty_gpu.py: one
iteration bit for bit the chain of the individual calls, in host form and in device form on the caller's workspace; lambda = NULL equal to
idocp_rbd_ilqr_iterate_penalty bit for bit; over three rounds of (2 iterations, update) cost + mu sq_shifted per sample never rises within a round;
al_update leaves `violation` equal to a fresh idocp_rbd_score_al under lambda+ and mu_next; and the effectiveness comparison against the pure
penalty."""
import numpy as np
import pytest

import rbd_al as AL
import rbd_gradients as G
import rbd_penalty as PN
import rbd_policy as PO
import rbd_score as RS
from idocp_amd import capi
from rbd_batch import E_ARG, DeviceArray, Rbd
from test_rbd_al_gpu import multipliers
from test_rbd_ilqr_gn_gpu import numpy_weights
from test_rbd_ilqr_gpu import ILQR, TRAJ, same
from test_rbd_ilqr_penalty_gpu import CASES, TRIALS, first
from test_rbd_penalty_gpu import N, STEPS, T0, case

pytestmark = pytest.mark.gpu

MU = 25.0


def scored(r, o, which, cone, lam, mu=MU):
    """the start of test_rbd_ilqr_penalty_gpu.first with `violation` = sq_shifted under lam"""
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone)
    t = first(r, o, which, cone)
    t["violation"] = AL.score_al(r, o, mu, lam, q[:STEPS], v[:STEPS], u, a, f, active)
    return t


def by_hand(r, M, cons, o, cost, which, cone, traj, lam, consts, trials):
    """the chain of idocp_rbd_ilqr_iterate_al as individual calls"""
    mm, _, _, _, _, active, pts, ts, dt, _ = case(which, cone)
    t = {k: (None if x is None else x.copy()) for k, x in traj.items()}
    lin = AL.linearize_al(r, M, cons, o, consts["penalty"], lam, t["q_traj"], t["v_traj"], t["u_traj"], active, ts, dt, pts,
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
        gt = AL.score_al(r, o, consts["penalty"], lam, qt[:STEPS], vt[:STEPS], ut, at, ft, active)
        state.update(trial_q=qt, trial_v=vt, trial_u=ut, trial_a=at, trial_f=ft, trial_cost=ct, trial_violation=gt)
        state = G.accept(r, state, consts)
    return {k: state[k] for k in TRAJ}, {"alpha_accepted": state["alpha_accepted"], "lqr_status": lqr["status"], "expected": lqr["expected"]}


def small_multipliers(which, cone):
    """the draw of test_rbd_al_gpu.py on the iteration's rollout, scaled down so that the shifted problem stays near the start's"""
    return 0.05 * multipliers(which, cone, False)[0]


@pytest.mark.parametrize("which,cone", CASES)
def test_the_chained_iteration_equals_the_individual_calls(which, cone):
    mm, M, cost, cons, tables, active, pts, ts, dt, _ = case(which, cone)
    consts = dict(ILQR, penalty=MU)
    lam = small_multipliers(which, cone)
    r = Rbd(mm)
    o = RS.Objective(r, cost, cons, T0, dt, STEPS)
    traj = scored(r, o, which, cone, lam)
    new, out = AL.iterate_al(r, o, traj, lam, consts, TRIALS, active, ts, dt, pts)
    want, want_out = by_hand(r, M, cons, o, cost, which, cone, traj, lam, consts, TRIALS)
    for name in TRAJ:
        assert same(new[name], want[name]), (which, cone, name)
    for name in out:
        assert same(out[name], want_out[name]), (which, cone, name)
    print("%s %s: alpha accepted %s, sq_shifted %s -> %s" % (which, cone, out["alpha_accepted"], traj["violation"], new["violation"]))
    # the device form on the caller's workspace (the penalty one): the same bits again
    nbytes = r.lib.idocp_rbd_ilqr_penalty_workspace_bytes(r.h, o.h, N, STEPS)
    dev = {k: DeviceArray(x) for k, x in traj.items() if x is not None}
    dev.update(alpha_accepted=DeviceArray(np.zeros(N)), expected=DeviceArray(np.zeros((N, 2))), lqr_status=DeviceArray(np.zeros((N + 1) // 2)),
               workspace=DeviceArray(np.zeros(nbytes // 8)))
    d_pts = DeviceArray(pts) if pts is not None else None
    d_lam = DeviceArray(lam)
    io = G.ilqr_struct({k: d.ptr.value for k, d in dev.items()}, consts, TRIALS)
    capi.check(AL.iterate_al_raw(r, o, N, STEPS, active, ts, dt, d_pts.ptr.value if d_pts else None, io, d_lam.ptr.value, device=True), "idocp_rbd_ilqr_iterate_al_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    for name in TRAJ:
        if traj[name] is not None:
            assert same(dev[name].numpy(), new[name]), (which, cone, name)
    assert same(dev["alpha_accepted"].numpy(), out["alpha_accepted"]) and same(dev["expected"].numpy(), out["expected"])
    for d in list(dev.values()) + [d_lam] + ([d_pts] if d_pts else []):
        d.free()
    # lambda = NULL: idocp_rbd_ilqr_iterate_penalty bit for bit
    start = first(r, o, which, cone)
    pen, pen_out = PN.iterate_penalty(r, o, start, consts, TRIALS, active, ts, dt, pts)
    got, got_out = AL.iterate_al(r, o, start, None, consts, TRIALS, active, ts, dt, pts)
    for name in TRAJ:
        assert (pen[name] is None and got[name] is None) or np.array_equal(got[name], pen[name]), name
    for name in pen_out:
        assert np.array_equal(got_out[name], pen_out[name]), name
    # mu = 0 is refused
    rc = AL.iterate_al_raw(r, o, N, STEPS, active, ts, dt, pts, G.ilqr_struct({**{k: (None if x is None else x.copy()) for k, x in start.items()}, **got_out},
                                                                             dict(consts, penalty=0.0), TRIALS), None)
    assert rc == E_ARG and "penalty (mu) must be positive" in capi.last_error()
    o.close()
    r.close()


@pytest.mark.parametrize("which,cone", CASES)
def test_rounds_of_iterations_and_updates(which, cone):
    """Three rounds of (2 iterations, multiplier update) at the fixed mu of test_rbd_ilqr_penalty_gpu.py's effectiveness check (mu sq_violation
    at least ten times the cost at the start) against 6 iterations of the pure penalty at the same mu from the same start.  Within a round
    cost + mu sq_shifted never rises on any sample; after every al_update `violation` is a fresh idocp_rbd_score_al under lambda+.
    Measured on an MI355X, one run (mean over the 5 samples; start -> AL | penalty after 6 iterations each; DESIGN.md section 6 has the table):
      ANYmal, linearized cone, mu 3.67:  cost 4.793 -> 4.189 | 4.186,  sq_violation 22.02 -> 4.466 | 3.478,   largest infeasibility 20.65 | 19.50
      ANYmal, FrictionCone, mu 0.276:    cost 4.793 -> 4.447 | 4.354,  sq_violation 235.3 -> 161.2 | 169.7,   largest infeasibility 125.6 | 125.6
      chain2, mu 12.0:                   cost 10.69 -> 6.458 | 5.749,  sq_violation 25.85 -> 0.0113 | 0.168,  largest infeasibility 1.201 | 6.484
    On chain2 the multipliers end fifteen times lower than the penalty; on ANYmal the two end level (under the linearized cone AL is a little
    behind).  Asserted: only that the mean unshifted sq_violation ends below the start's -- it does on all three cases, none is left out."""
    mm, M, cost, cons, tables, active, pts, ts, dt, _ = case(which, cone)
    r = Rbd(mm)
    o = RS.Objective(r, cost, cons, T0, dt, STEPS)
    start = first(r, o, which, cone)
    assert (start["violation"] > 0).all()
    mu = float(10.0 * (start["cost"] / start["violation"]).max())
    consts = dict(ILQR, penalty=mu)
    L = r.lib.idocp_rbd_objective_multiplier_rows(o.h)
    lam = np.zeros((STEPS, N, L))
    traj = dict(start)      # (lambda = 0: sq_shifted is sq_violation)
    unshifted = lambda t: PN.score_penalty(r, o, t["q_traj"][:STEPS], t["v_traj"][:STEPS], t["u_traj"], t["a_traj"], t["f_traj"], active)      # noqa: E731
    for rnd in range(3):
        merits = [traj["cost"] + mu * traj["violation"]]
        for it in range(2):
            traj, out = AL.iterate_al(r, o, traj, lam, consts, TRIALS, active, ts, dt, pts)
            merits.append(traj["cost"] + mu * traj["violation"])
        for before, after in zip(merits[:-1], merits[1:]):
            assert (after <= before).all(), (rnd, before, after)      # exactly: a rejected sample keeps its scores
        lam, viol, inf, ch = AL.al_update(r, o, traj, lam, mu, mu, active)
        fresh = AL.score_al(r, o, mu, lam, traj["q_traj"][:STEPS], traj["v_traj"][:STEPS], traj["u_traj"], traj["a_traj"], traj["f_traj"], active)
        assert same(viol, fresh) and np.isfinite(inf).all() and np.isfinite(ch).all()
        traj = dict(traj, violation=viol)
        print("%s %s round %d: mean cost %.4g, mean sq_violation %.4g, max infeasibility %.4g, max multiplier change %.4g" % (
            which, cone, rnd, traj["cost"].mean(), unshifted(traj).mean(), inf.max(), ch.max()))
    pen = dict(start)
    for it in range(6):
        pen, _ = PN.iterate_penalty(r, o, pen, consts, TRIALS, active, ts, dt, pts)
    _, pinf, _ = AL.multiplier_update(r, o, mu, None, pen["q_traj"][:STEPS], pen["v_traj"][:STEPS], pen["u_traj"], pen["a_traj"], pen["f_traj"], active, L=L)
    sq_al = unshifted(traj)
    print("%s %s mu %.3g, 6 iterations: mean cost %.4g -> AL %.4g | penalty %.4g; mean sq_violation %.4g -> AL %.4g | penalty %.4g; max infeasibility AL %.4g | penalty %.4g" % (
        which, cone, mu, start["cost"].mean(), traj["cost"].mean(), pen["cost"].mean(), start["violation"].mean(), sq_al.mean(), pen["violation"].mean(),
        inf.max(), pinf.max()))
    assert sq_al.mean() < start["violation"].mean()
    o.close()
    r.close()
