"""Contact-frame kinematics and the rollout that latches its footholds (idocp_rbd_contact_kinematics_batch, idocp_rbd_rollout_footholds;
rbd_kinematics_kernel.hip) on the GPU.  The referee is the numpy model of tests/rbd_kinematics.py (gen_golden_rbd.frame_kinematics, the complex
step, rbd_forward.reference / euler_step and the latch rule), the bar independent_rbd.BAR = 1e-11 with helpers.rel_err; test_rbd_kinematics_host.py
holds that referee to the host calls."""
import ctypes as C
import functools

import numpy as np
import pytest

import independent_rbd as IR
import rbd_forward as F
import rbd_kinematics as K
import rbd_policy as PO
from helpers import ANYMAL_Q_STANDING, anymal_model, iiwa14_model, rel_err
from idocp_amd import capi
from rbd_batch import E_ARG, E_UNSUPPORTED, DeviceArray, Rbd
from test_other_quadrupeds_gpu import other_quadruped

pytestmark = pytest.mark.gpu
BAR = IR.BAR
TS, DT = 0.04, 0.01         # Baumgarte time step, integration step
MODELS = ("anymal", 0, 1, 2)
SCHEDULE = ([1, 1, 1, 1], [1, 1, 1, 1], [0, 1, 1, 0], [0, 1, 1, 0], [1, 1, 1, 1], [1, 1, 1, 1])


def model(which):
    return anymal_model() if which == "anymal" else other_quadruped(which)[0]


@functools.lru_cache(maxsize=None)
def anymal_batch():
    """(struct, 131 random states, the all-outputs answer of the host form): shared, never written to"""
    m = anymal_model()
    q, v = K.standing_samples(np.random.default_rng(41), 131)
    r = Rbd(m)
    full = K.kinematics(r, q, v)
    r.close()
    return m, q, v, full


def device_kinematics(r, q, v, outputs, n, tail=1):
    """device form with a buffer for EVERY output (n + tail samples, NaN-filled); only `outputs` are handed to the call"""
    dq, dv = DeviceArray(q), DeviceArray(v)
    dev = {k: DeviceArray(np.full((n + tail,) + K.kin_shapes(r.m)[k], np.nan)) for k in K.KIN_OUTPUTS}
    io = capi.RbdKinIO()
    io.q, io.v = dq.ptr.value, dv.ptr.value
    for k in outputs:
        setattr(io, k, dev[k].ptr.value)
    capi.check(K.kinematics_raw(r, n, io, device=True), K.KIN_NAME + "_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    got = {k: x.numpy() for k, x in dev.items()}
    for x in [dq, dv] + list(dev.values()):
        x.free()
    return got


@pytest.mark.parametrize("which", MODELS)
def test_against_the_referee(which):
    m = model(which)
    M = IR.model_from_struct(m)
    n = 3
    q, v = K.standing_samples(np.random.default_rng(11), n)
    r = Rbd(m)
    got = K.kinematics(r, q, v)
    r.close()
    ref = [K.reference(M, q[i], v[i]) for i in range(n)]
    errs = {"points": rel_err(got["points"].reshape(n, -1), np.array([x["points"].reshape(-1) for x in ref])),
            "rotation": rel_err(got["rotation"].reshape(n, -1), np.array([x["rotation"].reshape(-1) for x in ref])),
            "velocity": rel_err(got["velocity"].reshape(n, -1), np.array([x["velocity"].reshape(-1) for x in ref])),
            "jacobian": rel_err(got["jacobian"].reshape(n, -1), np.array([x["jacobian"].T.reshape(-1) for x in ref]))}
    print(which, {k: "%.2e" % e for k, e in errs.items()})
    bad = {k: e for k, e in errs.items() if not e < BAR}
    assert not bad, (which, bad)
    host = np.abs(got["points"] - F.foot_positions(m, q)).max()
    assert host < 1e-13, host
    Jv = np.einsum("ncr,nc->nr", got["jacobian"], v)                 # (jacobian comes as [column][row])
    assert rel_err(got["velocity"].reshape(n, -1), Jv) < 1e-13
    # the structural zeros are stored: contact c has no column of another leg
    for c in range(4):
        other = [6 + 3 * l + j for l in range(4) if l != c for j in range(3)]
        assert (got["jacobian"][:, other, 3 * c:3 * c + 3] == 0.0).all()


@pytest.mark.parametrize("n", (1, 2, 17, 131))
def test_any_n_bit_for_bit(n):
    m, q, v, full = anymal_batch()
    r = Rbd(m)
    got = K.kinematics(r, q[:n], v[:n], tail=1)
    for k in K.KIN_OUTPUTS:
        assert np.isnan(got[k][n]).all(), (k, "the tail was written")
        assert np.isfinite(got[k][:n]).all(), k
        assert (got[k][:n] == full[k][:n]).all(), (k, "a sample depends on the batch around it")
    # the same states launched alone (a few of them: every launch is a host round trip)
    for i in sorted({0, n // 2, n - 1}):
        one = K.kinematics(r, q[i:i + 1], v[i:i + 1], tail=1)
        for k in K.KIN_OUTPUTS:
            assert (one[k][0] == got[k][i]).all() and np.isnan(one[k][1]).all(), (k, i)
    r.close()


def test_output_selection_and_forms():
    m, q, v, full = anymal_batch()
    n = 17
    r = Rbd(m)
    for wanted in [(k,) for k in K.KIN_OUTPUTS] + [("points", "jacobian"), K.KIN_OUTPUTS]:
        host = K.kinematics(r, q[:n], v[:n] if "velocity" in wanted else None, outputs=wanted)
        for k in wanted:
            assert (host[k] == full[k][:n]).all(), (wanted, k)
        dev = device_kinematics(r, q[:n], v[:n], wanted, n)
        for k in K.KIN_OUTPUTS:
            if k in wanted:
                assert (dev[k][:n] == full[k][:n]).all() and np.isnan(dev[k][n]).all(), (wanted, k)
            else:
                assert np.isnan(dev[k]).all(), (wanted, k, "an output that was not asked for was written")
    r.close()


def test_a_non_finite_sample_stays_alone():
    m, q, v, full = anymal_batch()
    r = Rbd(m)
    for where, value in ((8, np.nan), (1, np.inf), (5, np.nan)):
        bad = q[:3].copy()
        bad[1, where] = value
        got = K.kinematics(r, bad, v[:3])
        for k in K.KIN_OUTPUTS:
            assert not np.isfinite(got[k][1]).any(), (where, k)
            assert (got[k][[0, 2]] == full[k][[0, 2]]).all(), (where, k)
    bad_v = v[:3].copy()
    bad_v[1, 9] = np.nan
    got = K.kinematics(r, q[:3], bad_v)
    assert not np.isfinite(got["velocity"][1]).any()
    assert (got["velocity"][[0, 2]] == full["velocity"][[0, 2]]).all() and (got["points"] == full["points"][:3]).all()
    r.close()


@functools.lru_cache(maxsize=None)
def rollout_case():
    """(struct, model dict, q0, v0, u, pts0): two perturbed starts about standing, slow enough to stay up for six steps"""
    m = anymal_model()
    rng = np.random.default_rng(23)
    q0 = np.tile(ANYMAL_Q_STANDING, (2, 1))
    q0[:, :3] += rng.uniform(-0.1, 0.1, (2, 3))
    quat = q0[:, 3:7] + rng.uniform(-0.05, 0.05, (2, 4))
    q0[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    q0[:, 7:] += rng.uniform(-0.1, 0.1, (2, 12))
    v0 = rng.uniform(-0.3, 0.3, (2, 18))
    u = rng.uniform(-20, 20, (len(SCHEDULE), 2, 12))
    pts0 = F.foot_positions(m, q0) + rng.uniform(-0.02, 0.02, (2, 4, 3))
    return m, IR.model_from_struct(m), q0, v0, u, pts0


@pytest.mark.parametrize("latch_first", (0, 1))
@pytest.mark.parametrize("impulse", (0, 1))
def test_latched_rollout_step_by_step(impulse, latch_first):
    m, M, q0, v0, u, pts0 = rollout_case()
    n, steps = 2, len(SCHEDULE)
    r = Rbd(m)
    pts, qt, vt, _, at, ft = K.footholds(r, q0, v0, steps, SCHEDULE, TS, DT, pts0, u=u, impulse=impulse, latch_first=latch_first)
    r.close()
    assert all(np.isfinite(x).all() for x in (pts, qt, vt, at, ft))
    for k in range(steps):
        foot = np.array([K.reference_points(M, qt[k][i]) for i in range(n)])
        for c in range(4):
            if K.stays(SCHEDULE, k, c, latch_first):
                before = pts[k - 1][:, c] if k > 0 else pts0[:, c]
                assert (pts[k][:, c] == before).all(), (k, c, "a carried point changed")
            else:
                err = rel_err(pts[k][:, c], foot[:, c])
                assert err < BAR, (k, c, err)
        # the step itself against the numpy model AT THE GPU'S OWN STATE AND POINTS: nothing accumulates into the comparison
        ref = [F.reference(M, qt[k][i], vt[k][i], u[k][i], SCHEDULE[k], pts[k][i], TS) for i in range(n)]
        step = [F.euler_step(M, qt[k][i], vt[k][i], at[k][i], DT) for i in range(n)]
        errs = {"a": rel_err(at[k], np.array([x[0] for x in ref])), "f": rel_err(ft[k].reshape(n, -1), np.array([x[1].reshape(-1) for x in ref])),
                "q_next": rel_err(qt[k + 1], np.array([x[0] for x in step]))}
        new = [int(b and not a) for a, b in zip(SCHEDULE[k], SCHEDULE[k + 1])] if k + 1 < steps else [0] * 4
        v_next = np.array([x[1] for x in step])
        if impulse and any(new):                # (slice k + 1 holds the post-impulse velocity)
            v_next = np.array([v_next[i] + F.reference(M, qt[k + 1][i], v_next[i], None, new, impulse=True)[0] for i in range(n)])
        errs["v_next"] = rel_err(vt[k + 1], v_next)
        print("impulse %d latch_first %d step %d:" % (impulse, latch_first, k), {key: "%.2e" % e for key, e in errs.items()})
        bad = {key: e for key, e in errs.items() if not e < BAR}
        assert not bad, (k, bad)
    # the touchdown latched the two returning feet where each plant's own foot was: not at the caller's points
    assert np.abs(pts[4][:, [0, 3]] - pts0[:, [0, 3]]).max() > 1e-3
    if not latch_first:
        assert (pts[0] == pts0).all() and (pts[1] == pts0).all() and (pts[3][:, [1, 2]] == pts0[:, [1, 2]]).all()
    else:
        assert rel_err(pts[0].reshape(n, -1), F.foot_positions(m, q0).reshape(n, -1)) < BAR and (pts[1] == pts[0]).all()


def test_the_whole_rollout_against_the_numpy_latched_rollout():
    m, M, q0, v0, u, pts0 = rollout_case()
    steps = 4                                    # (lift-off at step 2; end to end at the bar test_rbd_policy_gpu.py holds its five-step closed loop to)
    r = Rbd(m)
    pts, qt, vt, _, at, ft = K.footholds(r, q0, v0, steps, SCHEDULE[:steps], TS, DT, pts0, u=u[:steps], impulse=1, latch_first=1)
    r.close()
    for i in range(2):
        rp, rq, rv, ra, rf = K.latched_rollout(M, q0[i], v0[i], steps, SCHEDULE[:steps], pts0[i], TS, DT, True, True, lambda k, q, v: u[k][i])
        errs = {"points": rel_err(pts[:, i].reshape(steps, -1), rp.reshape(steps, -1)), "q": rel_err(PO.same_rotation(qt[:, i], rq), rq), "v": rel_err(vt[:, i], rv),
                "a": rel_err(at[:, i], ra), "f": rel_err(ft[:, i].reshape(steps, -1), rf.reshape(steps, -1))}
        print("sample %d:" % i, {k: "%.2e" % e for k, e in errs.items()})
        assert max(errs.values()) < BAR, errs


def test_tied_to_the_existing_rollouts():
    m, M, q0, v0, u, pts0 = rollout_case()
    n, steps = 2, len(SCHEDULE)
    r = Rbd(m)
    # open loop
    pts, qt, vt, _, at, ft = K.footholds(r, q0, v0, steps, SCHEDULE, TS, DT, pts0, u=u, impulse=1, latch_first=1)
    q2, v2, a2, f2 = F.rollout(r, q0, v0, u, SCHEDULE, TS, DT, pts, impulse=True)
    for name, x, y in (("q", qt, q2), ("v", vt, v2), ("a", at, a2), ("f", ft, f2)):
        assert (x == y).all(), name
    # no torques at all: u = NULL and policy = NULL
    ptz, qz, vz, _, az, fz = K.footholds(r, q0, v0, steps, SCHEDULE, TS, DT, pts0, impulse=1, latch_first=0)
    q2, v2, a2, f2 = F.rollout(r, q0, v0, np.zeros_like(u), SCHEDULE, TS, DT, ptz, impulse=True)
    for name, x, y in (("q", qz, q2), ("v", vz, v2), ("a", az, a2), ("f", fz, f2)):
        assert (x == y).all(), name
    # closed loop: shared gains and references, per-sample feedforward, bounds
    rng = np.random.default_rng(3)
    policy = dict(shared_gains=True, shared_ref=True, u_ff=u, K=PO.random_gains(rng, (steps,), m.nu, m.nv, norm=30.0),
                  q_ref=np.tile(ANYMAL_Q_STANDING, (steps, 1)), v_ref=np.zeros((steps, m.nv)), u_min=np.full(m.nu, -40.0), u_max=np.full(m.nu, 40.0))
    ptc, qc, vc, uc, ac, fc = K.footholds(r, q0, v0, steps, SCHEDULE, TS, DT, pts0, impulse=1, latch_first=1, policy=policy)
    q2, v2, u2, a2, f2 = PO.rollout_policy(r, q0, v0, steps, SCHEDULE, TS, DT, ptc, impulse=True, **policy)
    for name, x, y in (("q", qc, q2), ("v", vc, v2), ("u", uc, u2), ("a", ac, a2), ("f", fc, f2)):
        assert np.isfinite(x).all() and (x == y).all(), name
    assert not (uc == u).all()                   # (the feedback acted)
    # the device form: bit for bit the host form
    dq, dv = DeviceArray(np.concatenate([q0[None], np.zeros((steps, n, m.nq))])), DeviceArray(np.concatenate([v0[None], np.zeros((steps, n, m.nv))]))
    du, da, df = DeviceArray(u), DeviceArray(np.zeros((steps, n, m.nv))), DeviceArray(np.zeros((steps, n, 4, 3)))
    dp = DeviceArray(np.concatenate([pts0[None], np.full((steps - 1, n, 4, 3), np.nan)]))

    class Ptr:                                   # (what footholds_struct reads of an array)
        def __init__(self, d):
            self.ctypes = type("c", (), {"data": d.ptr.value})

    io = K.footholds_struct(Ptr(dp), Ptr(dq), Ptr(dv), u=Ptr(du), a_traj=Ptr(da), f_traj=Ptr(df))
    capi.check(K.footholds_raw(r, n, steps, SCHEDULE, TS, DT, io, 1, 1, device=True), K.ROLL_NAME + "_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    for name, x, y in (("points", dp, pts), ("q", dq, qt), ("v", dv, vt), ("a", da, at), ("f", df, ft)):
        assert (x.numpy() == y).all(), name
    for x in (dq, dv, du, da, df, dp):
        x.free()
    r.close()


def test_latched_points_follow_the_sample():
    """two plants that differ by a base translation d: every latched or tracked point differs by d -- what constant footholds cannot give"""
    m, M, q0, v0, u, pts0 = rollout_case()
    steps = len(SCHEDULE)
    d = np.array([0.3, -0.2, 0.05])
    qa = np.stack([q0[0], q0[0]])
    qa[1, :3] += d
    va, ua = np.stack([v0[0], v0[0]]), np.stack([u[:, 0], u[:, 0]], axis=1)
    r = Rbd(m)
    pts, qt = K.footholds(r, qa, va, steps, SCHEDULE, TS, DT, np.zeros((2, 4, 3)), u=ua, impulse=1, latch_first=1)[:2]
    r.close()
    assert np.isfinite(pts).all()
    assert np.abs(pts[:, 1] - pts[:, 0] - d).max() < 1e-14
    assert np.abs(qt[:, 1, :3] - qt[:, 0, :3] - d).max() < 1e-14


def expect_refusal(r, rc, code, text):
    assert rc == code, (rc, text)
    got = r.lib.idocp_last_error().decode()
    assert got == text, (got, text)


def test_refusals_leave_the_handle_usable():
    m, q, v, full = anymal_batch()
    lib = capi.lib()
    lib.idocp_last_error.restype = C.c_char_p
    r = Rbd(m)
    n = 3
    qs, vs = np.ascontiguousarray(q[:n]), np.ascontiguousarray(v[:n])
    out = np.zeros((n, 4, 3))

    def kin_io(**kw):
        io = capi.RbdKinIO()
        for k, x in kw.items():
            setattr(io, k, x.ctypes.data if x is not None else None)
        return io

    steps = 2
    act = [[1, 1, 1, 1], [1, 0, 0, 1]]
    qt, vt, pt = np.zeros((steps + 1, n, 19)), np.zeros((steps + 1, n, 18)), np.zeros((steps, n, 4, 3))
    qt[0], vt[0] = qs, vs
    uu = np.zeros((steps, n, 12))
    pol, keep = PO.policy_struct(u_ff=uu)
    pol_k, keep_k = PO.policy_struct(K=np.zeros((steps, n, 12 * 36)))
    pol_b, keep_b = PO.policy_struct(u_min=np.full(12, 1.0), u_max=np.full(12, -1.0))
    chain = Rbd(iiwa14_model())
    for device in (False, True):
        kn, rn = K.KIN_NAME + ("_device" if device else ""), K.ROLL_NAME + ("_device" if device else "")
        kin = lambda io, nn=n, h=r: K.kinematics_raw(h, nn, io, device=device)      # noqa: E731
        expect_refusal(r, kin(kin_io(q=qs, points=out), h=chain), E_UNSUPPORTED, kn + ": a fixed-base chain has no contact frames")
        expect_refusal(r, kin(None), E_ARG, kn + ": null handle or io")
        expect_refusal(r, kin(kin_io(q=qs, points=out), nn=0), E_ARG, kn + ": n must be positive")
        expect_refusal(r, kin(kin_io(points=out)), E_ARG, kn + ": q is needed")
        expect_refusal(r, kin(kin_io(q=qs, velocity=out)), E_ARG, kn + ": velocity needs v")
        expect_refusal(r, kin(kin_io(q=qs, v=vs)), E_ARG, kn + ": no output was asked for")

        def roll(io, nn=n, ss=steps, a=act, ts=TS, h=r):
            return K.footholds_raw(h, nn, ss, a, ts, DT, io, 1, 1, device=device)
        good = lambda **kw: K.footholds_struct(pt, qt, vt, **kw)      # noqa: E731
        expect_refusal(r, roll(good(), h=chain), E_UNSUPPORTED, rn + ": a fixed-base chain has no contact frames")
        expect_refusal(r, roll(None), E_ARG, rn + ": null handle or io")
        expect_refusal(r, roll(good(), nn=-1), E_ARG, rn + ": n must be positive")
        expect_refusal(r, roll(good(), ss=0), E_ARG, rn + ": steps must be at least 1")
        needed = rn + ": contact_points, q_traj, v_traj and active are needed"
        expect_refusal(r, roll(K.footholds_struct(None, qt, vt)), E_ARG, needed)
        expect_refusal(r, roll(K.footholds_struct(pt, None, vt)), E_ARG, needed)
        expect_refusal(r, roll(K.footholds_struct(pt, qt, None)), E_ARG, needed)
        expect_refusal(r, roll(good(), a=None), E_ARG, needed)
        expect_refusal(r, roll(good(u=uu, pol=pol)), E_ARG, rn + ": u and policy exclude one another")
        expect_refusal(r, roll(good(pol=pol_k)), E_ARG, rn + ": gains K need the references q_ref and v_ref")
        if not device:      # (the bounds of the device form are device memory and are not looked at)
            expect_refusal(r, roll(good(pol=pol_b)), E_ARG, rn + ": u_min[0] <= u_max[0] does not hold (or a bound is NaN)")
        expect_refusal(r, roll(good(), ts=0.0), E_ARG, rn + ": an active contact needs a positive Baumgarte time_step")
        expect_refusal(r, roll(good(), ts=-1.0), E_ARG, rn + ": an active contact needs a positive Baumgarte time_step")
    null = C.c_void_p()
    assert lib.idocp_rbd_contact_kinematics_batch(null, n, C.byref(kin_io(q=qs, points=out))) == E_ARG
    assert lib.idocp_rbd_rollout_footholds(null, n, steps, F._act(np.asarray(act).reshape(-1)), TS, DT, C.byref(K.footholds_struct(pt, qt, vt)), 1, 1) == E_ARG
    del keep, keep_k, keep_b
    chain.close()
    # with every contact open no time step is needed, and the handle still computes the right answer
    assert K.footholds_raw(r, n, 1, [[0, 0, 0, 0]], 0.0, DT, K.footholds_struct(pt, qt, vt), 1, 1) == 0
    got = K.kinematics(r, qs, vs)
    for k in K.KIN_OUTPUTS:
        assert (got[k] == full[k][:n]).all(), k
    assert (pt[0] == full["points"][:n]).all()      # (the latch of that open step: the same kernel, the same bits)
    r.close()
