"""idocp_rbd_ilqr_iterate_gn on the GPU at n = 5, steps = 4, trials = 2: one iteration bit for bit the chain of the individual calls
(idocp_rbd_linearize_rollout_cost, idocp_rbd_lqr_backward_gn, then the trial rounds of test_rbd_ilqr_gpu.py); the cost per sample under the FULL
objective -- the ANYmal workload's own, a_weight and f_weight set and u_weight zero -- never rises over the iterations; the objective that
idocp_rbd_ilqr_iterate refuses is taken here; with zero a_weight and f_weight the iteration agrees with the diagonal one at the 1e-11 of
test_rbd_gradients_gpu.py."""
import numpy as np
import pytest

import rbd_gauss_newton as GN
import rbd_gradients as G
import rbd_policy as PO
import rbd_score as RS
from idocp_amd import capi
from rbd_batch import E_UNSUPPORTED, DeviceArray, Rbd
from test_rbd_gauss_newton_host import full_cost
from test_rbd_gradients_gpu import BAR
from test_rbd_ilqr_gpu import ILQR, TRAJ, first_rollout, same, start

pytestmark = pytest.mark.gpu

N, STEPS, TRIALS = 5, 4, 2


def setting(which):
    """start() of test_rbd_ilqr_gpu.py under a cost with a_weight (and f_weight) set"""
    m, M, cost, active, pts, dt, ts, x0 = start(which, N, STEPS)
    return m, M, full_cost(m, np.random.default_rng(61)), active, pts, dt, ts, x0


def rolled_out(r, o, which):
    m, M, cost, active, pts, dt, ts, (q0, v0, u) = start(which, N, STEPS)
    q, v, a, f = GN.F.rollout(r, q0, v0, u, active, ts, dt, pts)
    c, g, _ = RS.score(r, o, q, v, u, a, f, active, terminal=True, want_stage=False)
    return dict(q_traj=q, v_traj=v, u_traj=u, a_traj=a, f_traj=f, cost=c, violation=g)


def numpy_weights(m, cost, dt):
    W = lambda name, n: np.array(getattr(cost, name)[:n])      # noqa: E731
    return dt * np.concatenate([W("q_weight", m.nv), W("v_weight", m.nv)]), dt * W("u_weight", m.nu), np.concatenate([W("qf_weight", m.nv), W("vf_weight", m.nv)])


def by_hand(r, M, o, cost, which, traj, consts, trials):
    """the chain of idocp_rbd_ilqr_iterate_gn as individual calls"""
    m, _, _, active, pts, dt, ts, _ = start(which, N, STEPS)
    t = {k: (None if x is None else x.copy()) for k, x in traj.items()}
    lin = GN.linearize_cost(r, M, o, t["q_traj"], t["v_traj"], t["u_traj"], active, ts, dt, pts, want=("A_traj", "B_traj", "G_traj", "lx_traj", "lu_traj"))
    wx, wu, wxf = numpy_weights(m, cost, dt)
    lqr = GN.backward_gn(r, lin["A_traj"], lin["B_traj"], wx, wu, wxf, lin["lx_traj"], lin["lu_traj"], consts["regularization"], lin["G_traj"],
                         outputs=("K_traj", "k_traj", "expected", "status"))
    K_cm = np.ascontiguousarray(lqr["K_traj"].transpose(0, 1, 3, 2)).reshape(STEPS, N, -1)
    state = dict(t, expected=lqr["expected"], alpha=np.ones(N), done=np.zeros(N, dtype=np.int32), alpha_accepted=np.zeros(N))
    for _ in range(trials):
        u_ff = G.step_torques(r, state["u_traj"], lqr["k_traj"], state["alpha"])
        qt, vt, ut, at, ft = PO.rollout_policy(r, state["q_traj"][0], state["v_traj"][0], STEPS, active, ts, dt, pts, u_ff=u_ff, K=K_cm,
                                               q_ref=state["q_traj"][:STEPS], v_ref=state["v_traj"][:STEPS])
        ct, gt, _ = RS.score(r, o, qt, vt, ut, at, ft, active, terminal=True, want_stage=False)
        state.update(trial_q=qt, trial_v=vt, trial_u=ut, trial_a=at, trial_f=ft, trial_cost=ct, trial_violation=gt)
        state = G.accept(r, state, consts)
    return {k: state[k] for k in TRAJ}, {"alpha_accepted": state["alpha_accepted"], "lqr_status": lqr["status"], "expected": lqr["expected"]}


@pytest.mark.parametrize("which", ["anymal", "chain2"])
def test_the_chained_iteration_equals_the_individual_calls(which):
    m, M, cost, active, pts, dt, ts, _ = setting(which)
    r = Rbd(m)
    o = RS.Objective(r, cost, None, 0.0, dt, STEPS)
    traj = rolled_out(r, o, which)
    new, out = GN.iterate_gn(r, o, traj, ILQR, TRIALS, active, ts, dt, pts)
    want, want_out = by_hand(r, M, o, cost, which, traj, ILQR, TRIALS)
    for name in TRAJ:
        assert same(new[name], want[name]), (which, name)
    for name in out:
        assert same(out[name], want_out[name]), (which, name)
    assert (out["lqr_status"] == -1).all()
    print("%s: alpha accepted %s, cost %s -> %s" % (which, out["alpha_accepted"], traj["cost"], new["cost"]))
    # the device form on the caller's workspace: the same bits again
    nbytes = r.lib.idocp_rbd_ilqr_gn_workspace_bytes(r.h, N, STEPS)
    R = r.lib.idocp_rbd_objective_residual_rows(o.h)
    assert nbytes % 16 == 0 and nbytes >= r.lib.idocp_rbd_ilqr_workspace_bytes(r.h, N, STEPS) + 8 * STEPS * N * R * (2 * m.nv + m.nu)
    dev = {k: DeviceArray(x) for k, x in traj.items() if x is not None}
    dev.update(alpha_accepted=DeviceArray(np.zeros(N)), expected=DeviceArray(np.zeros((N, 2))), lqr_status=DeviceArray(np.zeros((N + 1) // 2)),
               workspace=DeviceArray(np.zeros(nbytes // 8)))
    d_pts = DeviceArray(pts) if pts is not None else None
    io = G.ilqr_struct({k: d.ptr.value for k, d in dev.items()}, ILQR, TRIALS)
    capi.check(GN.iterate_gn_raw(r, o, N, STEPS, active, ts, dt, d_pts.ptr.value if d_pts else None, io, device=True), "idocp_rbd_ilqr_iterate_gn_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    for name in TRAJ:
        if traj[name] is not None:
            assert same(dev[name].numpy(), new[name]), (which, name)
    assert same(dev["alpha_accepted"].numpy(), out["alpha_accepted"]) and same(dev["expected"].numpy(), out["expected"])
    for d in list(dev.values()) + ([d_pts] if d_pts else []):
        d.free()
    o.close()
    r.close()


def test_the_full_cost_never_rises_and_the_diagonal_call_still_refuses():
    which = "anymal"
    m, M, cost, active, pts, dt, ts, _ = setting(which)
    assert max(cost.a_weight[:m.nv]) > 0 and max(cost.u_weight[:m.nu]) == 0.0 and cost.f_weight[0][2] > 0
    r = Rbd(m)
    o = RS.Objective(r, cost, None, 0.0, dt, STEPS)
    traj = rolled_out(r, o, which)
    out0 = {"alpha_accepted": np.zeros(N), "lqr_status": np.zeros(N, dtype=np.int32), "expected": np.zeros((N, 2))}
    io = G.ilqr_struct({**{k: x for k, x in traj.items() if x is not None}, **out0}, ILQR, TRIALS)
    rc = G.iterate_raw(r, o, N, STEPS, active, ts, dt, pts, io)
    assert rc == E_UNSUPPORTED and "a_weight" in capi.last_error(), (rc, capi.last_error())
    costs, took = [traj["cost"].copy()], np.zeros(N, dtype=bool)
    for it in range(3):
        traj, out = GN.iterate_gn(r, o, traj, ILQR, TRIALS, active, ts, dt, pts)
        costs.append(traj["cost"].copy())
        took |= out["alpha_accepted"] > 0
        print("iteration %d: cost %s, alpha %s" % (it, traj["cost"], out["alpha_accepted"]))
        assert (out["lqr_status"] == -1).all()      # (u_weight = 0, regularization 1e-6: Quu stands on the acceleration rows)
    for before, after in zip(costs[:-1], costs[1:]):
        assert (after <= before).all(), (before, after)      # exactly: a rejected sample keeps its cost
    assert took.all() and (costs[-1] < costs[0]).all()
    o.close()
    r.close()


@pytest.mark.parametrize("which", ["anymal", "chain2"])
def test_zero_weights_agree_with_the_diagonal_iteration(which):
    m, M, cost, active, pts, dt, ts, _ = start(which, N, STEPS)      # (a_weight = f_weight = 0)
    r = Rbd(m)
    o = RS.Objective(r, cost, None, 0.0, dt, STEPS)
    traj = first_rollout(r, o, which, N, STEPS)
    want, want_out = G.iterate(r, o, traj, ILQR, TRIALS, active, ts, dt, pts)
    got, got_out = GN.iterate_gn(r, o, traj, ILQR, TRIALS, active, ts, dt, pts)
    assert same(got_out["alpha_accepted"], want_out["alpha_accepted"]) and same(got_out["lqr_status"], want_out["lqr_status"])
    for name, a, b in [(k, got[k], want[k]) for k in TRAJ if want[k] is not None] + [("expected", got_out["expected"], want_out["expected"])]:
        d = G.distance(a, b)
        print("%s %s: %.2e (bar %.0e)" % (which, name, d, BAR))
        assert d <= BAR, (which, name, d)
    o.close()
    r.close()
