"""idocp_rbd_lqr_backward on the GPU (rbd_lqr_kernel.hip): every output against the refined numpy referee of rbd_lqr.py on the quadruped shape and
on every chain length, at the rule of the rbd calls -- max(4 x the float64 referee's distance, 1e-11) from the refined referee --; a sample's bits
whatever the batch, the outputs asked for and the form of the call; failure of one sample that touches no other; the gains as
idocp_rbd_rollout_policy consumes them, held to central differences of that rollout; the refusals with their texts."""
import ctypes as C
import functools

import numpy as np
import pytest

import independent_rbd as IR
import rbd_cases as RC
import rbd_forward as F
import rbd_fd_derivatives as D
import rbd_lqr as L
import rbd_policy as PO
from helpers import ANYMAL_Q_STANDING, anymal_model
from idocp_amd import capi
from rbd_batch import E_ARG, Rbd
from test_rbd_fd_derivatives_host import FD_BAR, STEPS

pytestmark = pytest.mark.gpu

REG = 0.1
FLOAT_OUTPUTS = ("K_traj", "k_traj", "P0", "p0", "expected")


@functools.lru_cache(maxsize=None)
def quadruped_case():
    """(the random case, the refined referee, the float64 referee): 36 x 12, 6 steps, 3 samples, with gradients"""
    c = L.random_case(np.random.default_rng(36012), 36, 12, 6, 3)
    return c, L.referee_batch(c, REG, refined=True), L.referee_batch(c, REG)


def args(c, gradients=True):
    return (c["A"], c["B"], c["wx"], c["wu"], c["wxf"]) + ((c["lx"], c["lu"]) if gradients else (None, None))


def hold(got, refined, plain, names, what):
    for name in names:
        d_gpu, d_np = L.distance(got[name], refined[name]), L.distance(plain[name], refined[name])
        bar = max(L.FACTOR * d_np, L.FLOOR)
        print("%s %s: GPU %.2e, FP64 numpy %.2e, bar %.2e" % (what, name, d_gpu, d_np, bar))
        assert d_gpu <= bar, (what, name, d_gpu, d_np, bar)


def same(x, y):
    return np.array_equal(x, y, equal_nan=True)


def test_quadruped_shape():
    c, refined, plain = quadruped_case()
    r = Rbd(anymal_model())
    got = L.backward(r, *args(c), reg=REG)
    hold(got, refined, plain, FLOAT_OUTPUTS, "ANYmal")
    assert (got["status"] == -1).all()
    bare = L.backward(r, *args(c, gradients=False), reg=REG)
    assert same(bare["K_traj"], got["K_traj"]) and same(bare["P0"], got["P0"]) and (bare["status"] == -1).all()
    assert same(bare["p0"], np.zeros_like(bare["p0"]))
    r.close()


@pytest.mark.parametrize("nv", range(2, 9))
def test_chains(nv):
    mc, _ = IR.chain(nv, 0)
    c = L.random_case(np.random.default_rng(500 + nv), 2 * nv, nv, 4, 2)
    r = Rbd(mc)
    got = L.backward(r, *args(c), reg=REG)
    hold(got, L.referee_batch(c, REG, refined=True), L.referee_batch(c, REG), FLOAT_OUTPUTS, "chain of %d" % nv)
    assert (got["status"] == -1).all()
    r.close()


def test_bits():
    c, refined, plain = quadruped_case()
    r = Rbd(anymal_model())
    n = 2 * L.SAMPLES_PER_WORKGROUP + 1
    idx = np.arange(n) % 3
    big = {k: (x[:, idx] if k in ("A", "B", "lx", "lu") else x) for k, x in c.items()}
    batch = L.backward(r, *args(big), reg=REG)
    for i in range(n):
        j = idx[i]
        one = {k: (x[:, j:j + 1] if k in ("A", "B", "lx", "lu") else x) for k, x in c.items()}
        alone = L.backward(r, *args(one), reg=REG)
        for name in FLOAT_OUTPUTS:
            ax = 1 if name in ("K_traj", "k_traj") else 0
            assert same(np.take(batch[name], [i], axis=ax), alone[name]), (i, name)
    full = L.backward(r, *args(c), reg=REG)
    for outputs in (("K_traj",), ("status",), ("k_traj", "expected"), ("P0", "p0"), ("K_traj", "k_traj", "status")):
        part = L.backward(r, *args(c), reg=REG, outputs=outputs)
        for name in outputs:
            assert same(part[name], full[name]), (outputs, name)
    dev = L.backward(r, *args(c), reg=REG, device=True)
    for name in L.OUTPUTS:
        assert same(dev[name], full[name]), name
    # one step
    first = {k: (x[:1] if k in ("A", "B", "lu") else (x[:2] if k == "lx" else x)) for k, x in c.items()}
    got = L.backward(r, *args(first), reg=REG)
    hold(got, L.referee_batch(first, REG, refined=True), L.referee_batch(first, REG), FLOAT_OUTPUTS, "one step")
    assert (got["status"] == -1).all()
    r.close()


def broken(c, what):
    b = {k: (None if x is None else x.copy()) for k, x in c.items()}
    if what == "singular":
        b["B"][2, 1] = 0.0
    else:
        b["A"][4, 2, 7, 5] = np.nan
    return b


@pytest.mark.parametrize("what,sample,step", [("singular", 1, 2), ("nan", 2, 4)])
def test_isolation(what, sample, step):
    c, _, _ = quadruped_case()
    c = dict(c, wu=np.zeros(12))
    r = Rbd(anymal_model())
    clean = L.backward(r, *args(c), reg=0.0)
    assert (clean["status"] == -1).all() and all(np.isfinite(clean[name]).all() for name in FLOAT_OUTPUTS)
    got = L.backward(r, *args(broken(c, what)), reg=0.0)
    expect = np.full(3, -1)
    expect[sample] = step
    assert np.array_equal(got["status"], expect), got["status"]
    for name in ("K_traj", "k_traj"):
        assert np.isnan(got[name][:step + 1, sample]).all(), name
        assert same(got[name][step + 1:, sample], clean[name][step + 1:, sample]), name
    for name in ("P0", "p0", "expected"):
        assert np.isnan(got[name][sample]).all(), name
    others = [i for i in range(3) if i != sample]
    for name in FLOAT_OUTPUTS:
        ax = 1 if name in ("K_traj", "k_traj") else 0
        assert same(np.take(got[name], others, axis=ax), np.take(clean[name], others, axis=ax)), name
    r.close()


def test_the_policy_consumes_the_gains():
    """layout, sign and tangent convention against idocp_rbd_rollout_policy, not against the referee"""
    m = anymal_model()
    nv, nu, S, N, TS, DT = m.nv, m.nu, 4, 3, RC.TS, RC.DT
    active = ((1, 1, 1, 1),) * S
    rng = np.random.default_rng(909)
    q0 = np.tile(ANYMAL_Q_STANDING, (N, 1))
    v0 = 0.1 * rng.normal(size=(N, nv))
    pts = np.broadcast_to(F.foot_positions(m, q0), (S, N, 4, 3)).copy()
    u = rng.uniform(-5, 5, (S, N, nu))
    r = Rbd(m)
    q_traj, v_traj, _, _ = F.rollout(r, q0, v0, u, active, TS, DT, pts)
    A, B = D.linearize(r, q_traj, v_traj, u, active, TS, DT, pts)
    got = L.backward(r, A, B, np.ones(2 * nv), 1e-3 * np.ones(nu), 10.0 * np.ones(2 * nv), reg=0.0)
    assert (got["status"] == -1).all()
    K = got["K_traj"]                                            # [S][N][nu][2 nv]
    K_cm = np.ascontiguousarray(K.transpose(0, 1, 3, 2))         # the column-major blocks as the call wrote them
    lib = capi.lib()

    def integrate(qq, d, length):
        out = np.zeros(m.nq)
        capi.check(lib.idocp_model_integrate_configuration(C.byref(m), qq.ctypes.data, np.ascontiguousarray(d).ctypes.data, length, out.ctypes.data), "integrate")
        return out

    def subtract(qp, qm):
        out = np.zeros(nv)
        capi.check(lib.idocp_model_subtract_configuration(C.byref(m), np.ascontiguousarray(qp).ctypes.data, np.ascontiguousarray(qm).ctypes.data, out.ctypes.data), "subtract")
        return out

    dirs = np.random.default_rng(7).normal(size=(4, 2 * nv))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    cases = [(i, d, h, sgn) for i in range(N) for d in range(4) for h in STEPS for sgn in (1.0, -1.0)]
    qs = np.array([integrate(q0[i], dirs[d, :nv], sgn * h) for i, d, h, sgn in cases])
    vs = np.array([v0[i] + sgn * h * dirs[d, nv:] for i, d, h, sgn in cases])
    idx = np.array([i for i, _, _, _ in cases])
    qt, vt, _, _, _ = PO.rollout_policy(r, qs, vs, S, active, TS, DT, pts[:, idx], u_ff=u[:, idx], K=K_cm[:, idx], q_ref=q_traj[:S, idx], v_ref=v_traj[:S, idx])
    worst, teeth = 0.0, 0.0
    for i in range(N):
        closed, opened = np.eye(2 * nv), np.eye(2 * nv)
        for k in range(S):
            closed, opened = (A[k, i] + B[k, i] @ K[k, i]) @ closed, A[k, i] @ opened
        for d in range(4):
            best = np.inf
            for h in STEPS:
                plus, minus = cases.index((i, d, h, 1.0)), cases.index((i, d, h, -1.0))
                fd = np.concatenate([subtract(qt[S, plus], qt[S, minus]), vt[S, plus] - vt[S, minus]]) / (2 * h)
                best = min(best, D.distance(fd, closed @ dirs[d]))
            print("sample %d direction %d: |prod (A + B K) d - central differences| = %.2e (bar %.2e)" % (i, d, best, 10 * FD_BAR))
            worst = max(worst, best)
            teeth = max(teeth, D.distance(opened @ dirs[d], closed @ dirs[d]))
    assert worst < 10 * FD_BAR, worst
    assert teeth > 1e-3, teeth      # (the gains do move the final slice: an ignored or transposed K would not pass above)
    r.close()


def test_refusals():
    c, _, _ = quadruped_case()
    r = Rbd(anymal_model())
    S, N = 6, 3
    keep = L._inputs(*args(c))
    out = {"K_traj": np.zeros((S, N, 36, 12)), "k_traj": np.zeros((S, N, 12)), "expected": np.zeros((N, 2))}
    ok = {**keep, **out}

    def without(*names, **more):
        return {**{k: v for k, v in ok.items() if k not in names}, **more}

    bad_w = keep["x_weight"].copy(); bad_w[3] = -1.0                      # noqa: E702
    nan_w = keep["xf_weight"].copy(); nan_w[35] = np.nan                  # noqa: E702
    inf_w = keep["u_weight"].copy(); inf_w[0] = np.inf                    # noqa: E702
    cases = [((N, 0), ok, REG, "steps must be at least 1", True), ((0, S), ok, REG, "n must be positive", True),
             ((N, S), without("A_traj"), REG, "A_traj and B_traj are needed", True), ((N, S), without("B_traj"), REG, "A_traj and B_traj are needed", True)]
    cases += [((N, S), without(w), REG, "x_weight, u_weight and xf_weight are needed", True) for w in ("x_weight", "u_weight", "xf_weight")]
    cases += [((N, S), without("lx_traj", "k_traj", "expected"), REG, "lx_traj and lu_traj come together", True),
              ((N, S), without("lu_traj", "k_traj", "expected"), REG, "lx_traj and lu_traj come together", True),
              ((N, S), without("lx_traj", "lu_traj", "expected"), REG, "k_traj and expected need the gradients", True),
              ((N, S), without("lx_traj", "lu_traj", "k_traj"), REG, "k_traj and expected need the gradients", True),
              ((N, S), without("K_traj", "k_traj", "expected"), REG, "no output was asked for", True),
              ((N, S), ok, -1e-3, "regularization must be finite and non-negative", True),
              ((N, S), ok, np.nan, "regularization must be finite and non-negative", True),
              ((N, S), ok, np.inf, "regularization must be finite and non-negative", True),
              ((N, S), without(x_weight=bad_w), REG, "x_weight[3] must be finite and non-negative", False),
              ((N, S), without(xf_weight=nan_w), REG, "xf_weight[35] must be finite and non-negative", False),
              ((N, S), without(u_weight=inf_w), REG, "u_weight[0] must be finite and non-negative", False)]
    for (n, steps), arrays, reg, text, both in cases:
        for device in ((False, True) if both else (False,)):      # (the device form returns before it looks at what a pointer points to)
            who = "idocp_rbd_lqr_backward_device" if device else "idocp_rbd_lqr_backward"
            rc = L.backward_raw(r, n, steps, L.struct(arrays, reg), device=device)
            assert rc == E_ARG and capi.last_error().startswith(who + ": ") and text in capi.last_error(), (rc, capi.last_error(), who, text)
    for device in (False, True):
        who = "idocp_rbd_lqr_backward_device" if device else "idocp_rbd_lqr_backward"
        rc = L.backward_raw(r, N, S, None, device=device)
        assert rc == E_ARG and capi.last_error() == who + ": null handle or io", capi.last_error()
        fn = r.lib.idocp_rbd_lqr_backward_device if device else r.lib.idocp_rbd_lqr_backward
        rc = fn(None, N, S, C.byref(L.struct(ok, REG)))
        assert rc == E_ARG and capi.last_error() == who + ": null handle or io", capi.last_error()
    r.close()
