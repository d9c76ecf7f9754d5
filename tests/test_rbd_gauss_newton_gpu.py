"""idocp_rbd_linearize_rollout_cost on the GPU (rbd_residual_kernel.hip): ANYmal and chains of 2, 7 and 8 joints, n = 3 and n = 70 (more than one
workgroup of the residual kernel on both model kinds, the last one partly empty), 3 steps; on the quadruped the schedule has one lift-off and one
touchdown with its impulse, so that inactive rows are zero.  A_traj, B_traj bit for bit idocp_rbd_linearize_rollout's; G and rho bit for bit s times
the blocks of the derivative call at each slice; rho, lx, lu against the numpy referee of rbd_gauss_newton.py (which test_rbd_gauss_newton_host.py
holds to central differences) at the 1e-11 of test_rbd_gradients_gpu.py; a sample's bits whatever n, the outputs asked for and the form of the
call; a NaN that stays in its sample's slice; zero weights; every refusal."""
import functools

import numpy as np
import pytest

import independent_rbd as IR
import rbd_cases as RC
import rbd_fd_derivatives as D
import rbd_forward as F
import rbd_gauss_newton as GN
import rbd_gradients as G
import rbd_score as RS
from idocp_amd import capi
from rbd_batch import E_ARG, E_UNSUPPORTED, STAGE, Rbd
from test_rbd_gauss_newton_host import full_cost, without_rows
from test_rbd_gradients_gpu import BAR

pytestmark = pytest.mark.gpu

ACTIVE = ((1, 1, 1, 1), (0, 1, 1, 0), (1, 1, 1, 1))      # contacts 0 and 3 lift off after step 0 and touch down in front of step 2
S, NBIG, NREF, T0 = len(ACTIVE), 70, 3, 0.3
MODELS = ["anymal", "chain2", "chain7", "chain8"]


def same(x, y):
    return np.array_equal(x, y, equal_nan=True)


@functools.lru_cache(maxsize=None)
def case(which):
    """(model, model dict, cost, tables, active, pts, time step, dt, the rollout of NBIG samples q, v, u); the first NREF samples are the ones the
    referee is computed for"""
    rng = np.random.default_rng([23, len(which), int(which[-1]) if which != "anymal" else 0])
    if which == "anymal":
        m, M, (q, v, _, _, _, _) = RC.quadruped("anymal")
        idx = np.arange(NBIG) % RC.N
        q0, v0 = q[idx].copy(), 0.3 * v[idx]
        q0[:, 7:] += rng.uniform(-0.02, 0.02, (NBIG, 12)) * (np.arange(NBIG) >= RC.N)[:, None]
        active, ts, dt = ACTIVE, RC.TS, RC.DT
        pts = np.broadcast_to(F.foot_positions(m, q0), (S, NBIG, 4, 3)).copy()
        u = rng.uniform(-5, 5, (S, NBIG, m.nu))
        cost = full_cost(m)
    else:
        m, M = IR.chain(int(which[5:]), 1)
        active, pts, ts, dt = None, None, 0.0, 0.01
        q0, v0 = rng.uniform(-1, 1, (NBIG, m.nv)), rng.uniform(-1, 1, (NBIG, m.nv))
        u = rng.uniform(-5, 5, (S, NBIG, m.nu))
        cost = full_cost(m, rng)
    r = Rbd(m)
    q_traj, v_traj, _, _ = F.rollout(r, q0, v0, u, active, ts, dt, pts, impulse=True)
    r.close()
    assert np.isfinite(q_traj).all() and np.isfinite(v_traj).all()
    return m, M, cost, RS.reference_tables(M, cost, T0, dt, S), active, pts, ts, dt, (q_traj, v_traj, u)


@functools.lru_cache(maxsize=None)
def referee(which):
    m, M, cost, tables, active, pts, ts, dt, (q, v, u) = case(which)
    return GN.reference_cost_linearization_batch(m, M, cost, tables, dt, q[:, :NREF], v[:, :NREF], u[:, :NREF], active,
                                                 None if pts is None else pts[:, :NREF], ts)


def cut(which, n):
    m, M, cost, tables, active, pts, ts, dt, (q, v, u) = case(which)
    c = lambda x: None if x is None else np.ascontiguousarray(x[:, :n])      # noqa: E731
    return c(q), c(v), c(u), c(pts)


def run(r, o, which, n, **kw):
    m, M, cost, tables, active, pts, ts, dt, _ = case(which)
    q, v, u, p = cut(which, n)
    return GN.linearize_cost(r, M, o, q, v, u, active, ts, dt, p, impulse=True, **kw)


@pytest.mark.parametrize("n", [NREF, NBIG])
@pytest.mark.parametrize("which", MODELS)
def test_blocks_rows_and_gradients(which, n):
    m, M, cost, tables, active, pts, ts, dt, _ = case(which)
    q, v, u, p = cut(which, n)
    nv, nc, nx = m.nv, GN.contacts_of(m, M), 2 * m.nv
    r = Rbd(m)
    o = RS.Objective(r, cost, None, T0, dt, S)
    R = r.lib.idocp_rbd_objective_residual_rows(o.h)
    assert R == GN.residual_rows(nv, nc) == {"anymal": 32, "chain2": 4, "chain7": 8, "chain8": 8}[which]
    out = run(r, o, which, n)
    # 1. A_traj, B_traj: the bits of idocp_rbd_linearize_rollout
    A, B = D.linearize(r, q, v, u, active, ts, dt, p, impulse=True)
    assert same(out["A_traj"], A) and same(out["B_traj"], B)
    if nc:
        A0, _ = D.linearize(r, q, v, u, active, ts, dt, p, impulse=False)
        assert not same(A[1], A0[1])      # (step 2 does carry a touchdown impulse, and A_traj[1] its E)
    # 2. G and rho: s times the blocks of the derivative call at each slice, one rounded product each
    s = GN.scales(m, M, cost, dt)
    for k in range(S):
        d = D.derivatives(r, STAGE, q[k], v[k], u[k], active[k] if nc else None, ts, dt, p[k] if nc else None)
        Gw, rw = np.zeros((n, R, nx + m.nu)), np.zeros((n, R))
        Gw[:, :nv] = s[:nv, None] * np.concatenate([d["da_dq"], d["da_dv"], d["da_du"]], axis=2)
        rw[:, :nv] = s[:nv] * d["a"]
        for c in range(nc):
            if active[k][c]:
                rows = slice(nv + 3 * c, nv + 3 * c + 3)
                Gw[:, rows] = s[rows, None] * np.concatenate([d["df_dq"][:, 3 * c:3 * c + 3], d["df_dv"][:, 3 * c:3 * c + 3], d["df_du"][:, 3 * c:3 * c + 3]], axis=2)
                rw[:, rows] = s[rows] * (d["f"][:, c] - np.array(cost.f_ref[c][:]))
        assert same(out["G_traj"][k], Gw), (which, k)
        assert same(out["rho_traj"][k], rw), (which, k)
        assert np.abs(Gw[:, :nv]).max() > 1e-3
    if nc:
        assert (out["G_traj"][1][:, nv:nv + 3] == 0).all() and np.abs(out["G_traj"][0][:, nv:nv + 3]).max() > 0      # (the lifted foot's rows)
    # 3. rho, lx, lu against the numpy referee
    ref = referee(which)
    for name in ("rho_traj", "lx_traj", "lu_traj", "G_traj"):
        dist = G.distance(out[name][:, :NREF], ref[name])
        print("%s n %d %s: %.2e (bar %.0e)" % (which, n, name, dist, BAR))
        assert dist <= BAR, (which, name, dist)
    bare = G.reference_gradients_batch(m, M, cost, tables, dt, q[:, :NREF], v[:, :NREF], u[:, :NREF], terminal=True)
    assert G.distance(bare[1], ref["lu_traj"]) > 1e-4      # (G^T rho is not small)
    o.close()
    r.close()


@pytest.mark.parametrize("which", ["anymal", "chain7"])
def test_batch_outputs_and_form_do_not_change_a_bit(which):
    m = case(which)[0]
    r = Rbd(m)
    o = RS.Objective(r, case(which)[2], None, T0, case(which)[7], S)
    big = run(r, o, which, NBIG)
    small = run(r, o, which, NREF)
    one = run(r, o, which, 1)
    for name in GN.OUTPUTS:
        assert same(big[name][:, :NREF], small[name]) and same(big[name][:, :1], one[name]), name
    for want in (("G_traj",), ("lx_traj",), ("rho_traj", "lu_traj"), ("A_traj",)):
        part = run(r, o, which, NBIG, want=want)
        assert set(part) == set(want)
        for name in want:
            assert same(part[name], big[name]), (want, name)
    dev = run(r, o, which, NBIG, device=True)
    for name in GN.OUTPUTS:
        assert same(dev[name], big[name]), name
    o.close()
    r.close()


@pytest.mark.parametrize("which", ["anymal", "chain8"])
def test_a_nan_stays_in_its_samples_slice(which):
    m, M, cost, tables, active, pts, ts, dt, _ = case(which)
    q, v, u, p = cut(which, 5)
    r = Rbd(m)
    o = RS.Objective(r, cost, None, T0, dt, S)
    clean = GN.linearize_cost(r, M, o, q, v, u, active, ts, dt, p, impulse=False)
    assert all(np.isfinite(x).all() for x in clean.values())
    for name, k in (("q", 1), ("v", 2), ("u", 0)):
        bad = {"q": q.copy(), "v": v.copy(), "u": u.copy()}
        bad[name][k, 3, 1] = np.nan
        got = GN.linearize_cost(r, M, o, bad["q"], bad["v"], bad["u"], active, ts, dt, p, impulse=False)
        for out_name in GN.OUTPUTS:
            want = clean[out_name].copy()
            want[k, 3] = np.nan
            assert same(got[out_name], want), (name, out_name)
    o.close()
    r.close()


@pytest.mark.parametrize("which", ["anymal", "chain2"])
def test_zero_weights_give_zero_rows_and_the_diagonal_gradient(which):
    m, M, cost, tables, active, pts, ts, dt, _ = case(which)
    q, v, u, p = cut(which, NREF)
    bare = without_rows(cost)
    if which == "anymal":
        bare.set("u_weight", np.linspace(0.01, 0.02, m.nu))
    r = Rbd(m)
    o = RS.Objective(r, bare, None, T0, dt, S)
    out = GN.linearize_cost(r, M, o, q, v, u, active, ts, dt, p, impulse=True)
    lx, lu = G.gradients(r, o, q, v, u, terminal=True)
    assert (out["G_traj"] == 0).all() and (out["rho_traj"] == 0).all()
    assert np.array_equal(out["lx_traj"], lx) and np.array_equal(out["lu_traj"], lu)
    o.close()
    r.close()


def test_refusals():
    which, n = "anymal", NREF
    m, M, cost, tables, active, pts, ts, dt, _ = case(which)
    q, v, u, p = cut(which, n)
    r = Rbd(m)
    o = RS.Objective(r, cost, None, T0, dt, S)
    sh = GN.output_shapes(m, M, S, n)
    ok = {k: np.zeros(sh[k]) for k in GN.OUTPUTS}

    def refused(rc, who, text, code=E_ARG):
        assert rc == code and capi.last_error().startswith(who + ": ") and text in capi.last_error(), (rc, capi.last_error(), who, text)

    for device in (False, True):
        who = "idocp_rbd_linearize_rollout_cost" + ("_device" if device else "")
        call = lambda o_=o, n_=n, s_=S, io=GN.cost_struct(**ok), u_=u, p_=p, q_=q: GN.linearize_cost_raw(r, o_, n_, s_, active, ts, dt, u_, p_, q_, v, io, True, device)      # noqa: E731
        refused(call(n_=0), who, "n must be positive")
        refused(call(s_=0), who, "steps must be at least 1")
        refused(call(p_=None), who, "needs contact_points")
        refused(call(q_=None), who, "q and v are needed")
        refused(call(o_=None), who, "null objective or io")
        refused(call(io=None), who, "null objective or io")
        refused(call(io=GN.cost_struct()), who, "no output was asked for")
    who = "idocp_rbd_linearize_rollout_cost"
    short = RS.Objective(r, cost, None, T0, dt, S - 1)
    refused(GN.linearize_cost_raw(r, short, n, S, active, ts, dt, u, p, q, v, GN.cost_struct(**ok), True), who, "steps must lie within the objective's %d steps" % (S - 1))
    short.close()
    r2 = Rbd(m)
    refused(GN.linearize_cost_raw(r2, o, n, S, active, ts, dt, u, p, q, v, GN.cost_struct(**ok), True), who, "the objective was created on another handle")
    r2.close()
    neg = capi.Cost.from_buffer_copy(cost)
    neg.a_weight[2] = -0.1
    on = RS.Objective(r, neg, None, T0, dt, S)
    refused(GN.linearize_cost_raw(r, on, n, S, active, ts, dt, u, p, q, v, GN.cost_struct(**ok), True), who, "a negative a_weight", E_UNSUPPORTED)
    on.close()
    withu = capi.Cost.from_buffer_copy(cost)
    withu.set("u_weight", np.full(m.nu, 0.01))
    ou = RS.Objective(r, withu, None, T0, dt, S)
    refused(GN.linearize_cost_raw(r, ou, n, S, active, ts, dt, None, p, q, v, GN.cost_struct(**ok), True), who, "u_traj is NULL but a non-zero u_weight reads it")
    ou.close()
    # the existing calls still refuse the full cost
    lx = np.zeros(sh["lx_traj"])
    rc = G.gradients_raw(r, o, n, 0, S, True, G.gradient_struct(q_traj=q, v_traj=v, u_traj=u, lx_traj=lx))
    refused(rc, "idocp_rbd_objective_gradients", "a_weight", E_UNSUPPORTED)
    o.close()
    r.close()
