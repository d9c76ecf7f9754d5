"""Batched forward dynamics with contacts, the explicit Euler step and the rollout (idocp_rbd_forward_dynamics_batch, idocp_rbd_rollout;
rbd_forward_kernel.hip) on the GPU.  The referee is the numpy model (tests/rbd_forward.py on gen_golden_rbd.py: its own Newton-Euler, its own
frame kinematics, the force map taken from rnea(f = e_i) - rnea(f = 0), a refined dense solve), the bar independent_rbd.BAR = 1e-11 with
helpers.rel_err -- what MJtJinv is held to.  Every answer also goes back through the EXISTING inverse call, which defines it:
tau = S^T u and C = 0 on the active rows."""
import ctypes as C
import functools

import numpy as np
import pytest

import independent_rbd as IR
import rbd_forward as F
from helpers import P, anymal_model, arr, rel_err
from idocp_amd import capi
from rbd_batch import E_ARG, IMPULSE, STAGE, DeviceArray, Rbd, random_samples
from test_other_quadrupeds_gpu import other_quadruped

pytestmark = pytest.mark.gpu
BAR = IR.BAR
N = 5                       # odd: the last workgroup has one live wavefront
TS = 0.04                   # Baumgarte time step
DT = 0.01                   # integration step
MASKS = tuple([(i >> 3) & 1, (i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(15, -1, -1))      # all 16 contact sets: dimf = 12, 9, 6, 3, 0
MODELS = ("anymal", 0, 1, 2)


@functools.lru_cache(maxsize=None)
def quadruped(which):
    """(struct, model dict, samples (q, v, u, pts), per-sample stage terms, per-sample impulse terms): the reference is computed once per model"""
    if which == "anymal":
        m, rng = anymal_model(), np.random.default_rng(77)
    else:
        m, rng = other_quadruped(which)
    M = IR.model_from_struct(m)
    q, v = random_samples(rng, N)[:2]
    u = rng.uniform(-20, 20, (N, m.nu))
    pts = F.foot_positions(m, q) + rng.uniform(-0.03, 0.03, (N, 4, 3))      # (the feet, a few centimetres off: moderate Baumgarte terms)
    stage = [F.sample_terms(M, q[i], v[i], pts[i], TS) for i in range(N)]
    imp = [F.sample_terms(M, q[i], v[i], impulse=True) for i in range(N)]
    return m, M, (q, v, u, pts), stage, imp


def rows_of(mask):
    return np.repeat(np.array(mask, dtype=bool), 3)


@pytest.mark.parametrize("mask", MASKS, ids=["".join(map(str, x)) for x in MASKS])
@pytest.mark.parametrize("which", MODELS, ids=[str(x) for x in MODELS])
def test_stage_mode_against_the_numpy_model_and_round_trip(which, mask):
    m, M, (q, v, u, pts), stage, _ = quadruped(which)
    r = Rbd(m)
    o = F.forward(r, STAGE, q, v, u, mask, TS, DT, contact_points=pts)
    ref = [F.solve_terms(stage[i], u[i], mask) for i in range(N)]
    errs = {"a": rel_err(o["a"], np.array([x[0] for x in ref])), "f": rel_err(o["f"].reshape(N, -1), np.array([x[1].reshape(-1) for x in ref]))}
    # the definition: the existing inverse call gives tau = S^T u and C = 0 on the active rows at (a, f)
    back = r.call(STAGE, q, v, o["a"], mask, TS, f=o["f"], contact_points=pts, outputs=("tau", "C"))
    tau = np.zeros((N, m.nv))
    tau[:, 6:] = u
    errs["tau"] = rel_err(back["tau"], tau)
    errs["C"] = float(np.abs(back["C"][:, rows_of(mask)]).max()) if any(mask) else 0.0
    # the step, against the library's host retraction and against the generator's
    qn = np.zeros_like(q)
    for i in range(N):
        capi.check(capi.lib().idocp_model_integrate_configuration(C.byref(m), P(arr(q[i])), P(arr(v[i])), DT, P(qn[i])), "integrate_configuration")
    errs["q_next"] = rel_err(o["q_next"], qn)
    errs["q_next_numpy"] = rel_err(o["q_next"], np.array([F.euler_step(M, q[i], v[i], o["a"][i], DT)[0] for i in range(N)]))
    errs["v_next"] = rel_err(o["v_next"], v + DT * o["a"])
    print("%s %s STAGE:" % (which, mask), {k: "%.2e" % e for k, e in errs.items()}, "|a| %.0f |f| %.0f" % (np.abs(o["a"]).max(), np.abs(o["f"]).max()))
    bad = {k: e for k, e in errs.items() if not e < BAR}
    assert not bad, bad
    assert (o["f"][:, ~np.array(mask, dtype=bool)] == 0).all()
    assert np.abs(np.linalg.norm(o["q_next"][:, 3:7], axis=1) - 1).max() <= 1e-15
    # dt = 0: q (to 1e-15) and v exactly
    z = F.forward(r, STAGE, q, v, u, mask, TS, 0.0, contact_points=pts, outputs=("q_next", "v_next"))
    assert np.abs(z["q_next"] - q).max() <= 1e-15 and (z["v_next"] == v).all()
    r.close()


@pytest.mark.parametrize("mask", MASKS, ids=["".join(map(str, x)) for x in MASKS])
@pytest.mark.parametrize("which", MODELS, ids=[str(x) for x in MODELS])
def test_impulse_mode_against_the_numpy_model_and_round_trip(which, mask):
    m, M, (q, v, u, pts), _, imp = quadruped(which)
    r = Rbd(m)
    o = F.forward(r, IMPULSE, q, v, u, mask, 0.0, DT)              # (u is ignored)
    ref = [F.solve_terms(imp[i], None, mask) for i in range(N)]
    errs = {"dv": rel_err(o["a"], np.array([x[0] for x in ref])), "lambda": rel_err(o["f"].reshape(N, -1), np.array([x[1].reshape(-1) for x in ref]))}
    back = r.call(IMPULSE, q, v, o["a"], mask, 0.0, f=o["f"], outputs=("tau", "C"))
    errs["tau"] = float(np.abs(back["tau"]).max())
    errs["C"] = float(np.abs(back["C"][:, rows_of(mask)]).max()) if any(mask) else 0.0
    errs["v_next"] = rel_err(o["v_next"], v + o["a"])
    print("%s %s IMPULSE:" % (which, mask), {k: "%.2e" % e for k, e in errs.items()})
    bad = {k: e for k, e in errs.items() if not e < BAR}
    assert not bad, bad
    assert (o["f"][:, ~np.array(mask, dtype=bool)] == 0).all()
    assert (o["q_next"] == q).all()
    if not any(mask):
        assert (o["a"] == 0).all()
    r.close()


@pytest.mark.parametrize("n", [1, 129])
def test_output_selection_and_device_form(n):
    m = anymal_model()
    rng = np.random.default_rng(5)
    q, v = random_samples(rng, n)[:2]
    u = rng.uniform(-20, 20, (n, m.nu))
    pts = F.foot_positions(m, q) + rng.uniform(-0.03, 0.03, (n, 4, 3))
    mask = [1, 0, 0, 1]
    r = Rbd(m)
    shapes = F.fd_shapes(m)
    for mode, ts in ((STAGE, TS), (IMPULSE, 0.0)):
        full = F.forward(r, mode, q, v, u, mask, ts, DT, contact_points=pts)
        assert all(np.isfinite(x).all() for x in full.values())
        for wanted in (("a",), ("f",), ("q_next", "v_next")):
            # host form: only the wanted outputs, the same bits as in the full call
            o = F.forward(r, mode, q, v, u, mask, ts, DT, contact_points=pts, outputs=wanted)
            for k in wanted:
                assert (o[k] == full[k]).all(), (mode, wanted, k)
            # device form: every output buffer exists and carries a sentinel; the ones not asked for come back untouched
            dev_in = {"q": DeviceArray(q), "v": DeviceArray(v), "u": DeviceArray(u), "contact_points": DeviceArray(pts)}
            dev_out = {k: DeviceArray(np.full((n,) + shapes[k], -777.0)) for k in F.FD_OUTPUTS}
            io = capi.RbdFdIO()
            for k, x in dev_in.items():
                setattr(io, k, x.ptr.value)
            for k in wanted:
                setattr(io, k, dev_out[k].ptr.value)
            capi.check(F.forward_raw(r, mode, n, mask, ts, DT, io, device=True), "idocp_rbd_forward_dynamics_batch_device")
            capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
            for k in F.FD_OUTPUTS:
                got = dev_out[k].numpy()
                if k in wanted:
                    assert (got == full[k]).all(), (mode, wanted, k)
                else:
                    assert (got == -777.0).all(), (mode, wanted, k)
            for x in list(dev_in.values()) + list(dev_out.values()):
                x.free()
    r.close()


SCHEDULE = ([1, 1, 1, 1], [1, 1, 1, 1], [1, 0, 0, 1], [1, 0, 0, 1], [1, 1, 1, 1], [1, 1, 1, 1])


def test_rollout_over_a_contact_schedule():
    m = anymal_model()
    M = IR.model_from_struct(m)
    n, steps = 2, len(SCHEDULE)                 # (every step is refereed by the numpy model: two states keep the case to seconds)
    rng = np.random.default_rng(9)
    q0, v0 = random_samples(rng, n)[:2]
    v0 = 0.3 * v0
    u = rng.uniform(-20, 20, (steps, n, m.nu))
    pts = np.repeat((F.foot_positions(m, q0) + rng.uniform(-0.02, 0.02, (n, 4, 3)))[None], steps, axis=0)
    r = Rbd(m)
    qt, vt, at, ft = F.rollout(r, q0, v0, u, SCHEDULE, TS, DT, pts, impulse=True)
    assert all(np.isfinite(x).all() for x in (qt, vt, at, ft))
    # the same chain made of single calls: bit for bit
    q, v = q0.copy(), v0.copy()
    jump = None
    for k in range(steps):
        new = [int(b and not a) for a, b in zip(SCHEDULE[k - 1], SCHEDULE[k])] if k else [0] * 4
        if any(new):
            assert k == 4 and new == [0, 1, 1, 0]
            imp = F.forward(r, IMPULSE, q, v, None, new, 0.0, DT)
            jump = (v.copy(), imp)
            v = imp["v_next"]
        assert (qt[k] == q).all() and (vt[k] == v).all(), k
        o = F.forward(r, STAGE, q, v, u[k], SCHEDULE[k], TS, DT, contact_points=pts[k])
        assert (at[k] == o["a"]).all() and (ft[k] == o["f"]).all(), k
        # every step against the numpy model AT THE GPU'S OWN STATE: nothing accumulates into the comparison
        ref = [F.reference(M, q[i], v[i], u[k][i], SCHEDULE[k], pts[k][i], TS) for i in range(n)]
        step = [F.euler_step(M, q[i], v[i], o["a"][i], DT) for i in range(n)]
        errs = {"a": rel_err(o["a"], np.array([x[0] for x in ref])), "f": rel_err(o["f"].reshape(n, -1), np.array([x[1].reshape(-1) for x in ref])),
                "q_next": rel_err(o["q_next"], np.array([x[0] for x in step])), "v_next": rel_err(o["v_next"], np.array([x[1] for x in step]))}
        print("rollout step %d:" % k, {key: "%.2e" % e for key, e in errs.items()})
        bad = {key: e for key, e in errs.items() if not e < BAR}
        assert not bad, (k, bad)
        q, v = o["q_next"], o["v_next"]
    assert (qt[steps] == q).all() and (vt[steps] == v).all()
    # the impulse in front of step 4, on contacts 1 and 2
    v_pre, imp = jump
    ref = [F.reference(M, qt[4][i], v_pre[i], None, [0, 1, 1, 0], impulse=True) for i in range(n)]
    errs = {"dv": rel_err(imp["a"], np.array([x[0] for x in ref])), "lambda": rel_err(imp["f"].reshape(n, -1), np.array([x[1].reshape(-1) for x in ref]))}
    print("touchdown impulse:", {key: "%.2e" % e for key, e in errs.items()})
    assert max(errs.values()) < BAR, errs
    assert np.abs(imp["a"]).max() > 1e-3                     # (there was a jump to take)
    # without the touchdown impulse: no velocity jump, v_traj[k + 1] = v_traj[k] + dt a_traj[k] all the way
    qn, vn, an, _ = F.rollout(r, q0, v0, u, SCHEDULE, TS, DT, pts, impulse=False)
    assert (qn[:5] == qt[:5]).all() and (vn[:4] == vt[:4]).all()
    assert rel_err(vn[1:], vn[:-1] + DT * an) < 1e-15
    assert not (vn[4] == vt[4]).all()
    # the device form of the rollout: bit for bit the host form
    dq, dv = DeviceArray(np.concatenate([q0[None], np.zeros((steps, n, m.nq))])), DeviceArray(np.concatenate([v0[None], np.zeros((steps, n, m.nv))]))
    du, dp, da, df = DeviceArray(u), DeviceArray(pts), DeviceArray(np.zeros((steps, n, m.nv))), DeviceArray(np.zeros((steps, n, 4, 3)))
    act = (C.c_int * (4 * steps))(*[x for s in SCHEDULE for x in s])
    capi.check(r.lib.idocp_rbd_rollout_device(r.h, n, steps, act, TS, DT, du.ptr, dp.ptr, dq.ptr, dv.ptr, da.ptr, df.ptr, 1), "idocp_rbd_rollout_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    assert (dq.numpy() == qt).all() and (dv.numpy() == vt).all() and (da.numpy() == at).all() and (df.numpy() == ft).all()
    for x in (dq, dv, du, dp, da, df):
        x.free()
    r.close()


def chain_runs():
    return [c[:4] for c in IR.chain_cases()] + [("arm6", 0, 0, False)]


@pytest.mark.parametrize("nv,seed,zaxes", [c[1:] for c in chain_runs()], ids=[c[0] for c in chain_runs()])
def test_chains(nv, seed, zaxes):
    m, M = IR.chain(nv, seed, zaxes)
    (q, v, _), _ = IR.chain_samples(nv, seed, zaxes)
    n, dim = N, m.nv
    assert q.shape[0] == n
    rng = np.random.default_rng([41, nv, seed])
    u = rng.uniform(-10, 10, (2, n, dim))
    r = Rbd(m)
    o = F.forward(r, STAGE, q, v, u[0], None, 0.0, DT)
    ref = []
    for i in range(n):
        t = IR.terms(M, q[i], v[i], np.zeros(dim))
        ref.append(np.linalg.solve(t["dtau_da"], u[0][i] - t["tau"]))
    errs = {"a": rel_err(o["a"], np.array(ref)), "q_next": rel_err(o["q_next"], q + DT * v), "v_next": rel_err(o["v_next"], v + DT * o["a"])}
    # round trip through idocp_rnea_derivatives
    tau, dq, dv, da = np.zeros((n, dim)), np.zeros((n, dim, dim)), np.zeros((n, dim, dim)), np.zeros((n, dim, dim))
    capi.check(capi.lib().idocp_rnea_derivatives(C.byref(m), n, P(arr(q)), P(arr(v)), P(arr(o["a"])), P(tau), P(dq), P(dv), P(da), 0), "idocp_rnea_derivatives")
    errs["tau"] = rel_err(tau, u[0])
    print("chain nv=%d seed=%d:" % (dim, seed), {k: "%.2e" % e for k, e in errs.items()}, "|a| %.0f" % np.abs(o["a"]).max())
    bad = {k: e for k, e in errs.items() if not e < BAR}
    assert not bad, bad
    # two-step rollout: bit for bit the single calls
    qt, vt, at, ft = F.rollout(r, q, v, u, None, 0.0, DT)
    assert ft is None
    o2 = F.forward(r, STAGE, o["q_next"], o["v_next"], u[1], None, 0.0, DT)
    assert (qt[1] == o["q_next"]).all() and (vt[1] == o["v_next"]).all() and (at[0] == o["a"]).all()
    assert (qt[2] == o2["q_next"]).all() and (vt[2] == o2["v_next"]).all() and (at[1] == o2["a"]).all()
    # only the acceleration
    assert (F.forward(r, STAGE, q, v, u[0], None, 0.0, DT, outputs=("a",))["a"] == o["a"]).all()
    r.close()


def test_refusals():
    lib = capi.lib()

    FD, RO = "idocp_rbd_forward_dynamics_batch", "idocp_rbd_rollout"
    NO_CONTACTS = ": a fixed-base chain has no contacts (f and contact_points must be NULL)"

    def refused(rc, what, text):
        """the code and the COMPLETE text of idocp_last_error()"""
        assert rc == E_ARG, what
        msg = lib.idocp_last_error().decode()
        assert msg == text, (what, msg)

    def io_of(**arrays):
        io = capi.RbdFdIO()
        for k, x in arrays.items():
            setattr(io, k, x.ctypes.data)
        return io

    n = 2
    # a chain with f, contact_points or IMPULSE mode
    m, _ = IR.chain(0, 0)
    r = Rbd(m)
    q, v, a = np.zeros((n, m.nq)), np.zeros((n, m.nv)), np.zeros((n, m.nv))
    junk = np.zeros((n, 12))
    refused(F.forward_raw(r, STAGE, n, None, 0.0, DT, io_of(q=q, v=v, a=a, f=junk)), "chain with f", FD + NO_CONTACTS)
    refused(F.forward_raw(r, STAGE, n, None, 0.0, DT, io_of(q=q, v=v, a=a, contact_points=junk)), "chain with contact_points", FD + NO_CONTACTS)
    refused(F.forward_raw(r, IMPULSE, n, None, 0.0, DT, io_of(q=q, v=v, a=a)), "chain in IMPULSE mode", FD + ": a fixed-base chain has no impulse mode")
    qt, vt = np.zeros((2, n, m.nq)), np.zeros((2, n, m.nv))
    refused(F.rollout_raw(r, n, 1, None, 0.0, DT, None, None, qt, vt, None, junk, 0), "chain rollout with f_traj", RO + NO_CONTACTS)
    refused(F.rollout_raw(r, n, 0, None, 0.0, DT, None, None, qt, vt, None, None, 0), "steps = 0", RO + ": steps must be at least 1")
    r.close()
    # a quadruped
    m = anymal_model()
    r = Rbd(m)
    q, v, a = np.zeros((n, m.nq)), np.zeros((n, m.nv)), np.zeros((n, m.nv))
    q[:, 6] = 1.0
    pts = np.zeros((n, 4, 3))
    good = dict(q=q, v=v, a=a, contact_points=pts)
    refused(F.forward_raw(r, STAGE, n, None, TS, DT, io_of(**good)), "no active", FD + ": the contact status `active` is needed")
    refused(F.forward_raw(r, STAGE, 0, [1, 1, 1, 1], TS, DT, io_of(**good)), "n = 0", FD + ": n must be positive")
    refused(F.forward_raw(r, STAGE, n, [1, 1, 1, 1], TS, float("nan"), io_of(**good)), "dt = nan", FD + ": dt must be finite")
    refused(F.forward_raw(r, STAGE, n, [1, 1, 1, 1], TS, float("inf"), io_of(**good)), "dt = inf", FD + ": dt must be finite")
    refused(F.forward_raw(r, STAGE, n, [1, 1, 1, 1], TS, DT, io_of(q=q, v=v, a=a)), "active contacts without contact_points", FD + ": STAGE mode with an active contact needs contact_points")
    refused(F.forward_raw(r, STAGE, n, [1, 1, 1, 1], 0.0, DT, io_of(**good)), "active contacts without a time step", FD + ": STAGE mode with an active contact needs a positive Baumgarte time_step")
    refused(F.forward_raw(r, 7, n, [1, 1, 1, 1], TS, DT, io_of(**good)), "unknown mode", FD + ": unknown mode")
    refused(F.forward_raw(r, STAGE, n, [1, 1, 1, 1], TS, DT, None), "null io", FD + ": null io")
    refused(F.forward_raw(r, STAGE, n, [1, 1, 1, 1], TS, DT, io_of(v=v, a=a, contact_points=pts)), "no q", FD + ": q and v are needed")
    # two conditions violated at once: the one tested first is the one reported (n before the mode, the mode before q and v, those before dt)
    refused(F.forward_raw(r, 7, 0, [1, 1, 1, 1], TS, DT, io_of(**good)), "n = 0 and an unknown mode", FD + ": n must be positive")
    refused(F.forward_raw(r, 7, n, [1, 1, 1, 1], TS, float("nan"), io_of(v=v, a=a)), "unknown mode, no q, dt = nan", FD + ": unknown mode")
    refused(F.forward_raw(r, STAGE, n, None, TS, float("nan"), io_of(**good)), "dt = nan and no active", FD + ": dt must be finite")
    refused(F.forward_raw(r, STAGE, n, [1, 1, 1, 1], 0.0, DT, io_of(q=q, v=v, a=a)), "no contact_points and no time step",
            FD + ": STAGE mode with an active contact needs contact_points")
    qt, vt = np.zeros((2, n, m.nq)), np.zeros((2, n, m.nv))
    refused(F.rollout_raw(r, n, 0, [1, 1, 1, 1], TS, DT, None, pts[None], qt, vt, None, None, 0), "steps = 0", RO + ": steps must be at least 1")
    refused(F.rollout_raw(r, n, 1, None, TS, DT, None, pts[None], qt, vt, None, None, 0), "rollout without active", RO + ": the contact status `active` is needed")
    refused(F.rollout_raw(r, n, 1, [1, 1, 1, 1], TS, float("nan"), None, pts[None], qt, vt, None, None, 0), "rollout with dt = nan", RO + ": dt must be finite")
    refused(F.rollout_raw(r, 0, 0, None, TS, DT, None, pts[None], qt, vt, None, None, 0), "steps = 0, n = 0 and no active", RO + ": steps must be at least 1")
    refused(F.rollout_raw(r, 0, 1, None, TS, DT, None, pts[None], qt, vt, None, None, 0), "n = 0 and no active", RO + ": n must be positive")
    refused(F.rollout_raw(r, n, 1, [1, 1, 1, 1], TS, DT, None, pts[None], None, vt, None, None, 0), "no q_traj", RO + ": q and v are needed")
    refused(F.rollout_raw(r, n, 1, [1, 1, 1, 1], TS, DT, None, None, qt, vt, None, None, 0, device=True), "device form: its texts carry the un-suffixed name",
            RO + ": STAGE mode with an active contact needs contact_points")
    refused(F.forward_raw(r, STAGE, 0, [1, 1, 1, 1], TS, DT, io_of(**good), device=True), "n = 0, device form", FD + ": n must be positive")
    # the refusals left the handle usable
    o = F.forward(r, STAGE, q, v, None, [0, 0, 0, 0], 0.0, DT)
    assert np.isfinite(o["a"]).all()
    r.close()


def test_singular_input_gives_nan_and_leaves_the_handle_exact():
    m, M, (q, v, u, pts), stage, _ = quadruped("anymal")
    mask = [1, 1, 1, 1]
    r = Rbd(m)
    good = F.forward(r, STAGE, q, v, u, mask, TS, DT, contact_points=pts)
    qb = q.copy()
    qb[1, 8] = np.nan                                        # a joint angle of sample 1
    o = F.forward(r, STAGE, qb, v, u, mask, TS, DT, contact_points=pts, fill=0.0)
    for k in F.FD_OUTPUTS:
        assert np.isnan(o[k][1]).all(), k
        keep = [0, 2, 3, 4]
        assert (o[k][keep] == good[k][keep]).all(), k         # (the other samples of the launch are untouched)
    again = F.forward(r, STAGE, q, v, u, mask, TS, DT, contact_points=pts)
    for k in F.FD_OUTPUTS:
        assert (again[k] == good[k]).all(), k
    r.close()
