"""idocp_rbd_linearize_rollout on the GPU: 6 steps of ANYmal, n = 3, on a lift-off and a touchdown of the diagonal pair, so that one step carries
an impulse.  A_traj[k], B_traj[k] are the single-step call's bits on the stored slices; on the impulse step they are held to the referee's E
times them; the product of the A_traj[k] is held to central differences of idocp_rbd_rollout ITSELF along 4 fixed tangent directions, at
10 times the finite-difference bar of test_rbd_fd_derivatives_host.py."""
import ctypes as C

import numpy as np
import pytest

import rbd_cases as RC
import rbd_fd_derivatives as D
import rbd_forward as F
from rbd_batch import E_ARG, STAGE, Rbd
from idocp_amd import capi
from test_rbd_fd_derivatives_host import FD_BAR, STEPS

pytestmark = pytest.mark.gpu

ACTIVE = ((1, 1, 1, 1), (1, 1, 1, 1), (0, 1, 1, 0), (0, 1, 1, 0), (1, 1, 1, 1), (1, 1, 1, 1))      # touchdown of contacts 0 and 3 in front of step 4
TOUCHDOWN, K_IMP = (1, 0, 0, 1), 3                                                                  # A_traj[3] = E A_3
S, N, TS, DT = len(ACTIVE), RC.N, RC.TS, RC.DT
FLOOR, FACTOR = 1e-11, 4.0


def setup():
    m, M, (q, v, _, _, _, _) = RC.quadruped("anymal")
    rng = np.random.default_rng(404)
    q0, v0 = q.copy(), 0.3 * v
    pts = np.broadcast_to(F.foot_positions(m, q0), (S, N, 4, 3)).copy()      # the feet where they are at slice 0, held for all steps
    u = rng.uniform(-5, 5, (S, N, m.nu))
    return m, M, q0, v0, u, pts


def test_rollout_linearisation():
    m, M, q0, v0, u, pts = setup()
    nv = m.nv
    r = Rbd(m)
    q_traj, v_traj, _, _ = F.rollout(r, q0, v0, u, ACTIVE, TS, DT, pts, impulse=True)
    assert np.isfinite(q_traj).all() and np.isfinite(v_traj).all()
    A, B = D.linearize(r, q_traj, v_traj, u, ACTIVE, TS, DT, pts, impulse=True)
    assert np.isfinite(A).all() and np.isfinite(B).all()
    single = [D.derivatives(r, STAGE, q_traj[k], v_traj[k], u[k], ACTIVE[k], TS, DT, pts[k], outputs=("a", "A", "B")) for k in range(S)]
    for k in range(S):
        if k != K_IMP:
            assert np.array_equal(A[k], single[k]["A"]) and np.array_equal(B[k], single[k]["B"]), k
    # the impulse step: E from the referee at the pre-impulse state (q_traj[4], v_traj[3] + dt a)
    v_pre = v_traj[K_IMP] + DT * single[K_IMP]["a"]
    for i in range(N):
        refined, plain = D.reference(M, q_traj[K_IMP + 1, i], v_pre[i], None, TOUCHDOWN, impulse=True, refine="both")
        for got, one in ((A[K_IMP, i], single[K_IMP]["A"][i]), (B[K_IMP, i], single[K_IMP]["B"][i])):
            ref = refined["A"] @ one
            d_gpu, d_np = D.distance(got, ref), D.distance(plain["A"] @ one, ref)
            bar = max(FACTOR * d_np, FLOOR)
            print("impulse step, sample %d: GPU %.2e, FP64 numpy %.2e, bar %.2e" % (i, d_gpu, d_np, bar))
            assert d_gpu <= bar, (i, d_gpu, d_np, bar)
        assert D.distance(got, one) > 1e-6      # (E is not the identity: the step does carry an impulse)
    # the form without the impulse
    A0, _ = D.linearize(r, q_traj, v_traj, u, ACTIVE, TS, DT, pts, impulse=False)
    assert np.array_equal(A0[K_IMP], single[K_IMP]["A"])
    # the device form: the same bits as the host form
    from rbd_batch import DeviceArray
    dev = {k: DeviceArray(x) for k, x in (("u", u), ("pts", pts), ("q", q_traj), ("v", v_traj), ("A", np.full((S, N, 2 * nv, 2 * nv), np.nan)),
                                          ("B", np.full((S, N, m.nu, 2 * nv), np.nan)))}
    flat = F._act(np.asarray(ACTIVE).reshape(-1))
    capi.check(r.lib.idocp_rbd_linearize_rollout_device(r.h, N, S, flat, TS, DT, dev["u"].ptr, dev["pts"].ptr, dev["q"].ptr, dev["v"].ptr, dev["A"].ptr,
                                                        dev["B"].ptr, 1), "idocp_rbd_linearize_rollout_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "synchronize")
    assert np.array_equal(dev["A"].numpy().transpose(0, 1, 3, 2), A) and np.array_equal(dev["B"].numpy().transpose(0, 1, 3, 2), B)

    # ---- the product of the A_traj[k] against central differences of idocp_rbd_rollout itself
    lib = capi.lib()

    def integrate(qq, d, length):
        out = np.zeros(m.nq)
        capi.check(lib.idocp_model_integrate_configuration(C.byref(m), qq.ctypes.data, np.ascontiguousarray(d).ctypes.data, length, out.ctypes.data), "integrate")
        return out

    def subtract(qp, qm):
        out = np.zeros(nv)
        capi.check(lib.idocp_model_subtract_configuration(C.byref(m), np.ascontiguousarray(qp).ctypes.data, np.ascontiguousarray(qm).ctypes.data, out.ctypes.data), "subtract")
        return out

    rng = np.random.default_rng(7)
    dirs = rng.normal(size=(4, 2 * nv))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    cases = [(i, d, h, sgn) for i in range(N) for d in range(4) for h in STEPS for sgn in (1.0, -1.0)]
    qs = np.array([integrate(q0[i], dirs[d, :nv], sgn * h) for i, d, h, sgn in cases])
    vs = np.array([v0[i] + sgn * h * dirs[d, nv:] for i, d, h, sgn in cases])
    idx = np.array([i for i, _, _, _ in cases])
    qt, vt, _, _ = F.rollout(r, qs, vs, u[:, idx], ACTIVE, TS, DT, pts[:, idx], impulse=True)
    worst = 0.0
    for i in range(N):
        P = np.eye(2 * nv)
        for k in range(S):
            P = A[k, i] @ P
        for d in range(4):
            best = np.inf
            for h in STEPS:
                plus, minus = cases.index((i, d, h, 1.0)), cases.index((i, d, h, -1.0))
                fd = np.concatenate([subtract(qt[S, plus], qt[S, minus]), vt[S, plus] - vt[S, minus]]) / (2 * h)
                best = min(best, D.distance(fd, P @ dirs[d]))
            print("sample %d direction %d: |prod A d - central differences| = %.2e (bar %.2e)" % (i, d, best, 10 * FD_BAR))
            worst = max(worst, best)
    assert worst < 10 * FD_BAR, worst
    r.close()


def test_refusals_and_a_chain():
    m, M, q0, v0, u, pts = setup()
    r = Rbd(m)
    qt, vt = np.zeros((S + 1, N, m.nq)), np.zeros((S + 1, N, m.nv))
    A = np.zeros((S, N, 36, 36))
    WHO = "idocp_rbd_linearize_rollout"
    for args, text in (((N, 0, ACTIVE, TS, DT, u, pts, qt, vt, A, None, 1), WHO + ": steps must be at least 1"),
                       ((0, S, ACTIVE, TS, DT, u, pts, qt, vt, A, None, 1), WHO + ": n must be positive"),
                       ((N, S, ACTIVE, TS, DT, u, None, qt, vt, A, None, 1), "needs contact_points"),
                       ((N, S, ACTIVE, TS, DT, u, pts, None, vt, A, None, 1), "q and v are needed")):
        rc = D.linearize_raw(r, *args)
        assert rc == E_ARG and text in capi.last_error(), (rc, capi.last_error(), text)
    r.close()
    import independent_rbd as IR
    mc, _ = IR.chain(7, 0)
    rc_ = Rbd(mc)
    rng = np.random.default_rng(3)
    uc = rng.uniform(-5, 5, (3, 2, 7))
    qc, vc, _, _ = F.rollout(rc_, rng.uniform(-1, 1, (2, 7)), rng.uniform(-1, 1, (2, 7)), uc, dt=DT)
    Ac, Bc = D.linearize(rc_, qc, vc, uc, dt=DT)
    for k in range(3):
        one = D.derivatives(rc_, STAGE, qc[k], vc[k], uc[k], dt=DT, outputs=("A", "B"))
        assert np.array_equal(Ac[k], one["A"]) and np.array_equal(Bc[k], one["B"]), k
    rc_.close()
