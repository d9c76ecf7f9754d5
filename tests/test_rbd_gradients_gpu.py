"""idocp_rbd_objective_gradients and the LQR weights of an objective on the GPU (rbd_gradient_kernel.hip): lx, lu against the numpy referee of
rbd_gradients.py (which test_rbd_gradients_host.py holds to central differences) at 1e-11 -- the tolerance of every test_rbd_*_gpu.py against its
numpy referee, relative to max(1, |ref|_inf) of the block like rbd_lqr.distance -- on ANYmal and on chains of 2 and 8 joints, n = 3 and 5 (the last
workgroup is partly empty), 1, 2 and 66 steps (more than one run of 64 items), with and without the terminal slice, at first_step > 0 under the
trotting and the constant reference; a sample's bits whatever the batch, the outputs asked for and the form of the call; a NaN that poisons its own
slice only; the arrays as idocp_rbd_lqr_backward_device consumes them; the weight tables; the refusals with their texts."""
import ctypes as C
import functools

import numpy as np
import pytest

import independent_rbd as IR
import rbd_gradients as G
import rbd_lqr as L
import rbd_score as RS
from helpers import anymal_model
from idocp_amd import capi
from rbd_batch import E_ARG, E_UNSUPPORTED, DeviceArray, Rbd
from test_rbd_gradients_host import gradient_cost, turned

pytestmark = pytest.mark.gpu

BAR = 1e-11
NMAX, SMAX, TOTAL = 5, 66, 70      # samples and steps of the random slices; steps of the objective
DT, T0 = 0.02, 0.3


def same(x, y):
    return np.array_equal(x, y, equal_nan=True)


@functools.lru_cache(maxsize=None)
def case(which, kind="constant"):
    """(model, model dict, cost, tables of TOTAL steps, random slices for NMAX samples and SMAX steps + the terminal slice)"""
    rng = np.random.default_rng([17, len(which), len(kind)])
    if which.startswith("chain"):
        m, M = IR.chain(int(which[5:]), 1)
        cost = gradient_cost(m, rng)
    else:
        m = anymal_model()
        M = IR.model_from_struct(m)
        cost = gradient_cost(m, trotting=kind == "trotting")
    tables = RS.reference_tables(M, cost, T0, DT, TOTAL)
    q = np.array([[turned(M, rng, tables[0][k], 0.3, 1.0) for _ in range(NMAX)] for k in range(SMAX + 1)])
    x = dict(q=q, v=rng.uniform(-1, 1, (SMAX + 1, NMAX, m.nv)), u=rng.uniform(-12, 12, (SMAX, NMAX, m.nu)))
    return m, M, cost, tables, x


def window(x, n, steps, terminal, first=0):
    s = lambda a, extra: np.ascontiguousarray(a[first:first + steps + extra, :n])      # noqa: E731
    return s(x["q"], int(terminal)), s(x["v"], int(terminal)), s(x["u"], 0)


def hold(got, want, what):
    for name, g, w in (("lx", got[0], want[0]), ("lu", got[1], want[1])):
        d = G.distance(g, w)
        print("%s %s: %.2e (bar %.0e)" % (what, name, d, BAR))
        assert d <= BAR, (what, name, d)


@pytest.mark.parametrize("n,steps", [(3, 1), (5, 2), (3, 66)])
@pytest.mark.parametrize("which", ["anymal", "chain2", "chain8"])
def test_gradients_against_the_numpy_referee(which, n, steps):
    m, M, cost, tables, x = case(which)
    r = Rbd(m)
    o = RS.Objective(r, cost, None, T0, DT, TOTAL)
    for terminal in (True, False):
        q, v, u = window(x, n, steps, terminal)
        got = G.gradients(r, o, q, v, u, terminal=terminal)
        want = G.reference_gradients_batch(m, M, cost, tables, DT, q, v, u, terminal=terminal)
        hold(got, want, "%s n %d steps %d terminal %d" % (which, n, steps, terminal))
        assert np.abs(want[0]).max() > 1e-3 and np.abs(want[1]).max() > 1e-3
    o.close()
    r.close()


@pytest.mark.parametrize("kind", ["trotting", "constant"])
def test_a_window_behind_the_first_step(kind):
    m, M, cost, tables, x = case("anymal", kind)
    r = Rbd(m)
    o = RS.Objective(r, cost, None, T0, DT, TOTAL)
    first, steps, n = 40, 5, 3      # (t = 1.1 .. 1.2: the trotting reference has moved on, and the slices were drawn about it)
    q, v, u = window(x, n, steps, True, first)
    got = G.gradients(r, o, q, v, u, first_step=first, terminal=True)
    hold(got, G.reference_gradients_batch(m, M, cost, tables, DT, q, v, u, first_step=first, terminal=True), "%s first_step %d" % (kind, first))
    if kind == "trotting":
        assert np.abs(tables[0][first] - tables[0][0]).max() > 1e-2
        wrong = G.reference_gradients_batch(m, M, cost, tables, DT, q, v, u, first_step=0, terminal=True)
        assert G.distance(got[0], wrong[0]) > 1e-3      # (the window's own reference is what is taken)
    o.close()
    r.close()


@pytest.mark.parametrize("which", ["anymal", "chain8"])
def test_batch_outputs_and_form_do_not_change_a_bit(which):
    m, M, cost, tables, x = case(which)
    r = Rbd(m)
    o = RS.Objective(r, cost, None, T0, DT, TOTAL)
    steps = 3
    q, v, u = window(x, NMAX, steps, True)
    lx, lu = G.gradients(r, o, q, v, u, terminal=True)
    for i in range(NMAX):
        ax, au = G.gradients(r, o, q[:, i:i + 1], v[:, i:i + 1], u[:, i:i + 1], terminal=True)
        assert same(ax[:, 0], lx[:, i]) and same(au[:, 0], lu[:, i]), i
    only_x, none = G.gradients(r, o, q, v, u, terminal=True, want=("lx_traj",))
    assert none is None and same(only_x, lx)
    none, only_u = G.gradients(r, o, q, v, u, terminal=True, want=("lu_traj",))
    assert none is None and same(only_u, lu)
    dx, du = G.gradients(r, o, q, v, u, terminal=True, device=True)
    assert same(dx, lx) and same(du, lu)
    o.close()
    r.close()


def test_a_nan_poisons_its_own_slice_only():
    m, M, cost, tables, x = case("anymal")
    r = Rbd(m)
    o = RS.Objective(r, cost, None, T0, DT, TOTAL)
    q, v, u = window(x, NMAX, 3, True)
    lx, lu = G.gradients(r, o, q, v, u, terminal=True)
    assert np.isfinite(lx).all() and np.isfinite(lu).all()
    for name, k in (("q", 1), ("v", 3), ("u", 2)):
        bad = {"q": q.copy(), "v": v.copy(), "u": u.copy()}
        bad[name][k, 2, 1] = np.nan
        bx, bu = G.gradients(r, o, bad["q"], bad["v"], bad["u"], terminal=True)
        wx, wu = lx.copy(), lu.copy()
        wx[k, 2] = np.nan
        if k < 3:
            wu[k, 2] = np.nan
        assert same(bx, wx) and same(bu, wu), name
    o.close()
    r.close()


def test_the_backward_pass_consumes_the_gradients_and_the_weights():
    """layout: lx, lu and the device weight tables go into idocp_rbd_lqr_backward_device as they are"""
    m, M, cost, tables, x = case("anymal")
    r = Rbd(m)
    o = RS.Objective(r, cost, None, T0, DT, TOTAL)
    steps, n, nx, nu = 4, 3, 2 * m.nv, m.nu
    q, v, u = window(x, n, steps, True)
    rng = np.random.default_rng(3)
    A = np.ascontiguousarray((np.eye(nx) + 0.1 * rng.normal(size=(steps, n, nx, nx))).transpose(0, 1, 3, 2))
    B = np.ascontiguousarray((0.1 * rng.normal(size=(steps, n, nx, nu))).transpose(0, 1, 3, 2))
    dev = {k: DeviceArray(a) for k, a in dict(q=q, v=v, u=u, A=A, B=B, lx=np.zeros((steps + 1, n, nx)), lu=np.zeros((steps, n, nu)), k=np.zeros((steps, n, nu)),
                                              e=np.zeros((n, 2)), status=np.zeros((n + 1) // 2)).items()}
    io = G.gradient_struct(q_traj=dev["q"].ptr.value, v_traj=dev["v"].ptr.value, u_traj=dev["u"].ptr.value, lx_traj=dev["lx"].ptr.value, lu_traj=dev["lu"].ptr.value)
    capi.check(G.gradients_raw(r, o, n, 0, steps, True, io, device=True), "idocp_rbd_objective_gradients_device")
    wx, wu, wxf = G.device_weights(o)
    lqr = L.struct(dict(A_traj=dev["A"].ptr.value, B_traj=dev["B"].ptr.value, x_weight=wx.value, u_weight=wu.value, xf_weight=wxf.value,
                        lx_traj=dev["lx"].ptr.value, lu_traj=dev["lu"].ptr.value, k_traj=dev["k"].ptr.value, expected=dev["e"].ptr.value,
                        status=dev["status"].ptr.value), 0.1)
    capi.check(L.backward_raw(r, n, steps, lqr, device=True), "idocp_rbd_lqr_backward_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    status = dev["status"].numpy().view(np.int32)[:n]
    assert (status == -1).all(), status
    kff, e = dev["k"].numpy(), dev["e"].numpy()
    assert np.isfinite(kff).all() and (e[:, 0] < 0).all() and (e[:, 1] > 0).all()
    # and the same numbers through the host forms and the referee of the recursion
    lx, lu = G.gradients(r, o, q, v, u, terminal=True)
    hx, hu, hxf = G.host_weights(o, m)
    want = L.referee_batch(dict(A=A.transpose(0, 1, 3, 2), B=B.transpose(0, 1, 3, 2), wx=hx, wu=hu, wxf=hxf, lx=lx, lu=lu), 0.1)
    assert L.distance(kff, want["k_traj"]) < 1e-9 and L.distance(e, want["expected"]) < 1e-9
    for d in dev.values():
        d.free()
    o.close()
    r.close()


@pytest.mark.parametrize("which", ["anymal", "chain2", "chain3"])
def test_weight_tables(which):
    m, M, cost, tables, x = case(which)
    r = Rbd(m)
    o = RS.Objective(r, cost, None, T0, DT, TOTAL)
    hx, hu, hxf = G.host_weights(o, m)
    W = lambda name, n: np.array(getattr(cost, name)[:n])      # noqa: E731
    assert same(hx, DT * np.concatenate([W("q_weight", m.nv), W("v_weight", m.nv)]))
    assert same(hu, DT * W("u_weight", m.nu))
    assert same(hxf, np.concatenate([W("qf_weight", m.nv), W("vf_weight", m.nv)]))
    dx, du, dxf = G.device_weights(o)
    assert same(G.download(dx, 2 * m.nv), hx) and same(G.download(du, m.nu), hu) and same(G.download(dxf, 2 * m.nv), hxf)
    o.close()
    r.close()


def test_refusals():
    m, M, cost, tables, x = case("anymal")
    r = Rbd(m)
    o = RS.Objective(r, cost, None, T0, DT, TOTAL)
    n, steps = 3, 2
    q, v, u = window(x, n, steps, True)
    lx, lu = np.zeros((steps + 1, n, 2 * m.nv)), np.zeros((steps, n, m.nu))
    ok = dict(q_traj=q, v_traj=v, u_traj=u, lx_traj=lx, lu_traj=lu)

    def without(*names):
        return G.gradient_struct(**{k: a for k, a in ok.items() if k not in names})

    def refused(rc, who, text, code=E_ARG):
        assert rc == code and capi.last_error().startswith(who + ": ") and text in capi.last_error(), (rc, capi.last_error(), who, text)

    for device in (False, True):
        who = "idocp_rbd_objective_gradients" + ("_device" if device else "")
        refused(G.gradients_raw(r, o, 0, 0, steps, True, without(), device), who, "n must be positive")
        refused(G.gradients_raw(r, o, n, 0, 0, True, without(), device), who, "steps must be at least 1")
        refused(G.gradients_raw(r, o, n, TOTAL - 1, 2, True, without(), device), who, "first_step + steps must lie within the objective's %d steps" % TOTAL)
        refused(G.gradients_raw(r, o, n, -1, 2, True, without(), device), who, "first_step + steps")
        refused(G.gradients_raw(r, o, n, 0, steps, True, without("q_traj"), device), who, "q_traj and v_traj are needed")
        refused(G.gradients_raw(r, o, n, 0, steps, True, without("u_traj"), device), who, "u_traj is NULL but a non-zero u_weight reads it")
        refused(G.gradients_raw(r, o, n, 0, steps, True, without("lx_traj", "lu_traj"), device), who, "no output was asked for")
        refused(G.gradients_raw(r, o, n, 0, steps, True, None, device), who, "null handle, objective or io")
        refused(G.gradients_raw(r, None, n, 0, steps, True, without(), device), who, "null handle, objective or io")
    # the window is NOT capped at IDOCP_RBD_SCORE_MAX_WINDOW: only the objective bounds it
    r2 = Rbd(m)
    refused(G.gradients_raw(r2, o, n, 0, steps, True, without()), "idocp_rbd_objective_gradients", "the objective was created on another handle")
    r2.close()
    # what the diagonal weights cannot hold: refused by the gradients and by both weight calls, the term named
    for field, text in (("a_weight", "a_weight"), ("f_weight", "f_weight")):
        bad = capi.Cost.from_buffer_copy(cost)
        if field == "a_weight":
            bad.a_weight[3] = 0.1
        else:
            bad.f_weight[2][1] = 0.1
        ob = RS.Objective(r, bad, None, T0, DT, TOTAL)
        refused(G.gradients_raw(r, ob, n, 0, steps, True, without()), "idocp_rbd_objective_gradients", text, E_UNSUPPORTED)
        refused(G.gradients_raw(r, ob, n, 0, steps, True, without(), True), "idocp_rbd_objective_gradients_device", text, E_UNSUPPORTED)
        p = C.c_void_p()
        refused(ob.lib.idocp_rbd_objective_lqr_weights_device(ob.h, C.byref(p), None, None), "idocp_rbd_objective_lqr_weights_device", text, E_UNSUPPORTED)
        refused(ob.lib.idocp_rbd_objective_get_lqr_weights(ob.h, lx.ctypes.data, None, None), "idocp_rbd_objective_get_lqr_weights", text, E_UNSUPPORTED)
        ob.close()
    # zero torque weights: u_traj may be NULL, and lu is zero
    bare = capi.Cost.from_buffer_copy(cost)
    bare.set("u_weight", np.zeros(m.nu))
    ob = RS.Objective(r, bare, None, T0, DT, TOTAL)
    bx, bu = G.gradients(r, ob, q, v, None, terminal=True)
    assert same(bx, G.gradients(r, o, q, v, u, terminal=True)[0]) and same(bu, np.zeros_like(bu))
    ob.close()
    o.close()
    r.close()
