"""The affine feedback policy on the GPU (idocp_rbd_feedback_torques_batch, idocp_rbd_rollout_policy; rbd_policy_kernel.hip) against the numpy referee
of tests/rbd_policy.py: the torques on gen_golden_rbd.difference (pinned to idocp_model_subtract_configuration by test_rbd_policy_host.py), the closed
loop on rbd_forward.reference and rbd_forward.euler_step.  The bar is the project's bar for rigid-body terms, independent_rbd.BAR = 1e-11 with
helpers.rel_err (per sample, relative to max(1, |.|_inf)).

Inputs of every comparison: relative base rotations between q and q_ref of at most 2 rad, gains of infinity norm (largest absolute row sum) 50,
dt = 1e-2 or 1e-3, contact points from foot_positions.

The bar of the rollouts.  Before it was fixed the numpy closed loop was run twice on this file's own inputs (sample 2, both schedules, five steps), the
second time with every entry of q0 moved by one ulp: the trajectories (q, v, u, a, f) moved by at most 4.3e-14 (schedule a) and 7.1e-14 (schedule b) in rel_err.
That is below 1e-12, so the gains keep their norm of 50 and the bar stays 1e-11.

What is refereed how.  One step of the numpy model costs tenths of a second per quadruped sample, so the closed loop END TO END is refereed on the samples named
in REFEREED (a tail wavefront, the last sample behind full blocks), computed once for five steps and shared by every (steps, n) case.  EVERY sample
of every case is held, step by step at the device's own state, to the referee's torques at the bar and to the single forward-dynamics call
(refereed by test_rbd_forward_dynamics_gpu.py) bit for bit; test_a_launch_of_131_equals_131_launches_of_one ties every sample of the large launch to
the launch of one."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import independent_rbd as IR
import rbd_forward as F
import rbd_policy as RP
from helpers import ANYMAL_URDF, ROOT, anymal_model, rel_err
from idocp_amd import capi
from rbd_batch import E_ARG, IMPULSE, STAGE, DeviceArray, Rbd, random_samples
from test_other_quadrupeds_gpu import other_quadruped

pytestmark = pytest.mark.gpu
BAR = IR.BAR
TS = 0.04                   # Baumgarte time step
GAIN_NORM = 50.0
NMAX = 130


def quat_mul(a, b):
    """(x, y, z, w) of a * b"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


# ------------------------------------------------------------------ 1. one evaluation

@functools.lru_cache(maxsize=None)
def evaluation_case(which):
    """NMAX samples of a quadruped and the referee's torques for per-sample and shared gains / references; a case of n samples takes the first n.
    Sample 1: q == q_ref and v == v_ref bit for bit; sample 2: a base rotation of 1e-10 rad (the small-angle branch of the logarithm)."""
    if which == "anymal":
        m, rng = anymal_model(), np.random.default_rng(177)
    else:
        m, rng = other_quadruped(which)
    M = IR.model_from_struct(m)
    n, nv, nu = NMAX, m.nv, m.nu
    q_ref, v_ref = random_samples(rng, n)[:2]
    v = v_ref + rng.uniform(-1, 1, (n, nv))
    u_ff = rng.uniform(-20, 20, (n, nu))
    K = RP.random_gains(rng, (n,), nu, nv, GAIN_NORM)
    assert abs(np.abs(RP.gain_matrix(M, K[3])).sum(axis=1).max() - GAIN_NORM) < 1e-9
    axis = np.array([0.6, -0.48, 0.64])
    tiny = np.concatenate([axis * math.sin(0.5e-10), [math.cos(0.5e-10)]])
    q_of, ref_of = {}, {}
    for shared_ref in (False, True):
        qr = np.repeat(q_ref[:1], n, axis=0) if shared_ref else q_ref
        vr = np.repeat(v_ref[:1], n, axis=0) if shared_ref else v_ref
        q, vv = RP.perturbed_configurations(M, rng, qr), v.copy()
        q[1], vv[1] = qr[1], vr[1]
        q[2] = qr[2]
        q[2, 3:7] = quat_mul(qr[2, 3:7], tiny)
        angle = np.linalg.norm(F.RBD.difference(M, qr[2], q[2])[3:6])
        assert 0.9e-10 < angle < 1.1e-10, angle
        assert max(np.linalg.norm(F.RBD.difference(M, qr[i], q[i])[3:6]) for i in range(n)) <= 2.0 + 1e-9
        q_of[shared_ref] = (q, vv)
        for shared_gains in (False, True):
            ref_of[shared_gains, shared_ref] = np.array([RP.reference_torques(M, q[i], vv[i], u_ff[i], K[0 if shared_gains else i], qr[i], vr[i]) for i in range(n)])
    return m, M, dict(q_ref=q_ref, v_ref=v_ref, u_ff=u_ff, K=K), q_of, ref_of


@pytest.mark.parametrize("shared_ref", [False, True], ids=["own_ref", "shared_ref"])
@pytest.mark.parametrize("shared_gains", [False, True], ids=["own_gains", "shared_gains"])
@pytest.mark.parametrize("n", [1, 2, 3, 65, 130])      # one wavefront, a full pair, an odd tail, tails behind full blocks
@pytest.mark.parametrize("which", ["anymal", 1], ids=["anymal", "other1"])
def test_one_evaluation_against_the_numpy_referee(which, n, shared_gains, shared_ref):
    m, M, x, q_of, ref_of = evaluation_case(which)
    q, v = q_of[shared_ref]
    r = Rbd(m)
    u = RP.feedback_torques(r, q[:n], v[:n], shared_gains, shared_ref, u_ff=x["u_ff"][:n], K=x["K"][:1] if shared_gains else x["K"][:n],
                            q_ref=x["q_ref"][:1] if shared_ref else x["q_ref"][:n], v_ref=x["v_ref"][:1] if shared_ref else x["v_ref"][:n])
    want = ref_of[shared_gains, shared_ref][:n]
    err = rel_err(u, want)
    print("%s n=%d shared gains %d ref %d: %.2e, |u| %.0f" % (which, n, shared_gains, shared_ref, err, np.abs(want).max()))
    assert err < BAR, err
    if n >= 2:
        assert np.array_equal(u[1], x["u_ff"][1])                 # q == q_ref, v == v_ref: the state difference is exactly zero
    if n >= 3:
        assert not np.array_equal(u[2], x["u_ff"][2])             # (the tiny rotation is seen)
    r.close()


# ------------------------------------------------------------------ 2. saturation

def test_saturation_clamps_to_the_bounds_bit_for_bit():
    m, M, x, q_of, ref_of = evaluation_case("anymal")
    n = 65
    (q, v), free = q_of[False], ref_of[False, False][:n]
    # per joint, bounds half way between two neighbours of the sorted unclamped torques of the referee, about 30 % of the samples outside on each side
    order = np.sort(free, axis=0)
    lo, hi = 0.5 * (order[19] + order[20]), 0.5 * (order[44] + order[45])
    low, high = free < lo, free > hi
    assert low.mean() >= 0.25 and high.mean() >= 0.25
    assert min(np.abs(free - lo).min(), np.abs(free - hi).min()) > 1e-6      # no rounding difference can flip a branch
    pol = dict(u_ff=x["u_ff"][:n], K=x["K"][:n], q_ref=x["q_ref"][:n], v_ref=x["v_ref"][:n])
    r = Rbd(m)
    for u_min, u_max in ((lo, hi), (lo, None), (None, hi), (None, None)):
        u = RP.feedback_torques(r, q[:n], v[:n], u_min=u_min, u_max=u_max, **pol)
        want = np.array([RP.reference_torques(M, q[i], v[i], x["u_ff"][i], x["K"][i], x["q_ref"][i], x["v_ref"][i], u_min, u_max) for i in range(n)])
        inside = np.ones_like(low)
        if u_min is not None:
            assert np.array_equal(u[low], np.broadcast_to(lo, u.shape)[low])
            inside &= ~low
        if u_max is not None:
            assert np.array_equal(u[high], np.broadcast_to(hi, u.shape)[high])
            inside &= ~high
        assert rel_err(u, want) < BAR
        assert rel_err(u[inside], free[inside]) < BAR
    r.close()


# ------------------------------------------------------------------ 3. chains

CHAIN_DT = {2: 1e-2, 7: 1e-3, 8: 1e-2}


@functools.lru_cache(maxsize=None)
def chain_case(nv):
    m, M = IR.chain(nv, 1)
    rng = np.random.default_rng([53, nv])
    n, steps = 128, 3
    x = dict(q0=rng.uniform(-2.5, 2.5, (n, nv)), v0=rng.uniform(-3, 3, (n, nv)), u_ff=rng.uniform(-10, 10, (steps, n, nv)),
             K=RP.random_gains(rng, (steps, n), nv, nv, GAIN_NORM), q_ref=rng.uniform(-2.5, 2.5, (steps, n, nv)), v_ref=rng.uniform(-3, 3, (steps, n, nv)))
    return m, M, x


@functools.lru_cache(maxsize=None)
def chain_loop(nv, i):
    m, M, x = chain_case(nv)
    return RP.closed_loop(M, x["q0"][i], x["v0"][i], 3, None, None, None, CHAIN_DT[nv], False,
                          lambda k: dict(u_ff=x["u_ff"][k, i], K=x["K"][k, i], q_ref=x["q_ref"][k, i], v_ref=x["v_ref"][k, i]))


@pytest.mark.parametrize("n", [64, 65, 128])             # the block edges of the chain kernels
@pytest.mark.parametrize("nv", [2, 7, 8])
def test_chains(nv, n):
    m, M, x = chain_case(nv)
    dt, steps = CHAIN_DT[nv], 3
    pol = {k: x[k][:, :n] for k in ("u_ff", "K", "q_ref", "v_ref")}
    r = Rbd(m)
    # one evaluation: slice 0 of the policy, every sample
    u = RP.feedback_torques(r, x["q0"][:n], x["v0"][:n], **{k: a[0] for k, a in pol.items()})
    want = np.array([RP.reference_torques(M, x["q0"][i], x["v0"][i], x["u_ff"][0, i], x["K"][0, i], x["q_ref"][0, i], x["v_ref"][0, i]) for i in range(n)])
    errs = {"u": rel_err(u, want)}
    # three steps
    qt, vt, ut, at, ft = RP.rollout_policy(r, x["q0"][:n], x["v0"][:n], steps, None, 0.0, dt, **pol)
    assert ft is None and np.array_equal(ut[0], u)
    for k in range(steps):
        want = np.array([RP.reference_torques(M, qt[k, i], vt[k, i], x["u_ff"][k, i], x["K"][k, i], x["q_ref"][k, i], x["v_ref"][k, i]) for i in range(n)])
        errs["u at the device's state, step %d" % k] = rel_err(ut[k], want)
        o = F.forward(r, STAGE, qt[k], vt[k], ut[k], None, 0.0, dt)
        assert np.array_equal(at[k], o["a"]) and np.array_equal(qt[k + 1], o["q_next"]) and np.array_equal(vt[k + 1], o["v_next"]), k
    for i in sorted({0, 63, n - 1}):
        ref = chain_loop(nv, i)
        for name, got, w in zip("qvua", (qt, vt, ut, at), ref):
            errs["%s of sample %d" % (name, i)] = rel_err(got[:, i], w)
    print("chain nv=%d n=%d:" % (nv, n), {k: "%.2e" % e for k, e in errs.items()})
    bad = {k: e for k, e in errs.items() if not e < BAR}
    assert not bad, bad
    r.close()


# ------------------------------------------------------------------ 4. rollout, ANYmal

STEPS = 5
SCHEDULES = {"a": ([[1, 1, 1, 1]] * STEPS, 1e-2, 0), "b": ([[1, 0, 0, 1]] + [[1, 1, 1, 1]] * (STEPS - 1), 1e-3, 1)}      # (masks, dt, touchdown_impulse)
REFEREED = {3: (2,), 131: (2, 130)}


@functools.lru_cache(maxsize=None)
def rollout_case():
    m = anymal_model()
    M = IR.model_from_struct(m)
    rng = np.random.default_rng(31)
    n, nv, nu = 131, m.nv, m.nu
    q0, v0 = random_samples(rng, n)[:2]
    v0 = 0.3 * v0
    x = dict(q0=q0, v0=v0, u_ff=rng.uniform(-20, 20, (STEPS, n, nu)), K=RP.random_gains(rng, (STEPS, n), nu, nv, GAIN_NORM),
             # (1.5 rad at the start: five steps of at most 1e-2 s do not carry the base beyond 2 rad from its reference)
             q_ref=np.array([RP.perturbed_configurations(M, rng, q0, angle=1.5) for _ in range(STEPS)]), v_ref=v0 + rng.uniform(-1, 1, (STEPS, n, nv)),
             pts=np.repeat((F.foot_positions(m, q0) + rng.uniform(-0.02, 0.02, (n, 4, 3)))[None], STEPS, axis=0))
    return m, M, x


def sample_policy(x, i):
    return lambda k: dict(u_ff=x["u_ff"][k, i], K=x["K"][k, i], q_ref=x["q_ref"][k, i], v_ref=x["v_ref"][k, i])


@functools.lru_cache(maxsize=None)
def numpy_closed_loop(schedule, i):
    m, M, x = rollout_case()
    masks, dt, impulse = SCHEDULES[schedule]
    return RP.closed_loop(M, x["q0"][i], x["v0"][i], STEPS, masks, x["pts"][:, i], TS, dt, impulse, sample_policy(x, i))


def device_rollout(r, x, n, steps, schedule, want_u=True, **override):
    masks, dt, impulse = SCHEDULES[schedule]
    pol = {k: x[k][:steps, :n] for k in ("u_ff", "K", "q_ref", "v_ref")}
    pol.update(override)
    return RP.rollout_policy(r, x["q0"][:n], x["v0"][:n], steps, masks[:steps], TS, dt, x["pts"][:steps, :n], impulse, want_u, **pol)


def new_contacts(masks, k):
    return [int(b and not a) for a, b in zip(masks[k - 1], masks[k])] if k else [0] * 4


@pytest.mark.parametrize("n", [3, 131])
@pytest.mark.parametrize("steps", [1, 2, 5])
@pytest.mark.parametrize("schedule", ["a", "b"])
def test_rollout_against_the_numpy_closed_loop(schedule, steps, n):
    m, M, x = rollout_case()
    masks, dt, impulse = SCHEDULES[schedule]
    r = Rbd(m)
    qt, vt, ut, at, ft = device_rollout(r, x, n, steps, schedule)
    assert all(np.isfinite(a).all() for a in (qt, vt, ut, at, ft))
    errs = {}
    # every sample, step by step at the device's own state: the referee's torques, and the single forward calls bit for bit
    for k in range(steps):
        want = np.array([RP.reference_torques(M, qt[k, i], vt[k, i], **sample_policy(x, i)(k)) for i in range(n)])
        errs["u at the device's state, step %d" % k] = rel_err(ut[k], want)
        o = F.forward(r, STAGE, qt[k], vt[k], ut[k], masks[k], TS, dt, contact_points=x["pts"][k, :n])
        v_next = o["v_next"]
        if impulse and k + 1 < steps and any(new_contacts(masks, k + 1)):
            v_next = F.forward(r, IMPULSE, o["q_next"], v_next, None, new_contacts(masks, k + 1), 0.0, dt)["v_next"]
            assert np.abs(v_next - o["v_next"]).max() > 1e-3           # (there was a jump: the policy of step k + 1 must see the velocity behind it)
        assert np.array_equal(at[k], o["a"]) and np.array_equal(ft[k], o["f"]) and np.array_equal(qt[k + 1], o["q_next"]) and np.array_equal(vt[k + 1], v_next), k
    # the closed loop end to end
    for i in REFEREED[n]:
        q, v, u, a, f = numpy_closed_loop(schedule, i)
        # (a touchdown in front of step `steps` is not taken by a rollout that ends there: its last velocity is the pre-impulse one)
        cut = steps if impulse and steps < STEPS and any(new_contacts(masks, steps)) else steps + 1
        errs["q of sample %d" % i] = rel_err(RP.same_rotation(qt[:, i], q[:steps + 1]), q[:steps + 1])
        errs["v of sample %d" % i] = rel_err(vt[:cut, i], v[:cut])
        for name, got, w in (("u", ut, u), ("a", at, a), ("f", ft, f)):
            errs["%s of sample %d" % (name, i)] = rel_err(got[:, i].reshape(steps, -1), w[:steps].reshape(steps, -1))
    print("rollout %s steps=%d n=%d:" % (schedule, steps, n), {k: "%.2e" % e for k, e in errs.items()})
    bad = {k: e for k, e in errs.items() if not e < BAR}
    assert not bad, bad
    r.close()


# ------------------------------------------------------------------ 5. identities that need no referee

def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_no_gains_and_zero_gains_reproduce_the_open_loop_rollout():
    m, M, x = rollout_case()
    masks, dt, impulse = SCHEDULES["b"]
    n, steps = 131, 2
    r = Rbd(m)
    qo, vo, ao, fo = F.rollout(r, x["q0"], x["v0"], x["u_ff"][:steps], masks[:steps], TS, dt, x["pts"][:steps], impulse=True)
    for K in (None, np.zeros_like(x["K"][:steps])):
        q, v, u, a, f = device_rollout(r, x, n, steps, "b", K=K)
        assert same((q, v, u, a, f), (qo, vo, x["u_ff"][:steps], ao, fo)), K is None
    # K = NULL: the references are not read
    q, v, u, a, f = device_rollout(r, x, n, steps, "b", K=None, q_ref=None, v_ref=None)
    assert same((q, v, u, a, f), (qo, vo, x["u_ff"][:steps], ao, fo))
    r.close()


def test_a_reference_from_the_open_loop_rollout_is_a_fixed_point():
    m, M, x = rollout_case()
    masks, dt, impulse = SCHEDULES["b"]
    n = 3
    r = Rbd(m)
    open_loop = F.rollout(r, x["q0"][:n], x["v0"][:n], x["u_ff"][:, :n], masks, TS, dt, x["pts"][:, :n], impulse=True)
    q, v, u, a, f = device_rollout(r, x, n, STEPS, "b", q_ref=open_loop[0][:STEPS], v_ref=open_loop[1][:STEPS])
    tol = 1e-13 * max(1.0, GAIN_NORM)
    errs = [rel_err(got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)) for got, want in zip((q, v, a, f, u), open_loop + (x["u_ff"][:, :n],))]
    print("closed loop around the open-loop trajectory:", ["%.2e" % e for e in errs])
    assert max(errs) <= tol, errs
    r.close()


def test_device_form_equals_host_form():
    m, M, x = rollout_case()
    masks, dt, impulse = SCHEDULES["b"]
    n, steps, nu = 131, 2, m.nu
    rng = np.random.default_rng(6)
    u_min, u_max = rng.uniform(-30, -5, nu), rng.uniform(5, 30, nu)
    r = Rbd(m)
    host = device_rollout(r, x, n, steps, "b", u_min=u_min, u_max=u_max)
    assert (host[2] == u_min).any() and (host[2] == u_max).any()
    u_one = RP.feedback_torques(r, x["q0"], x["v0"], u_ff=x["u_ff"][0], K=x["K"][0], q_ref=x["q_ref"][0], v_ref=x["v_ref"][0], u_min=u_min, u_max=u_max)
    assert np.array_equal(u_one, host[2][0])
    d = {k: DeviceArray(x[k][:steps]) for k in ("u_ff", "K", "q_ref", "v_ref", "pts")}
    d.update(u_min=DeviceArray(u_min), u_max=DeviceArray(u_max), q=DeviceArray(np.concatenate([x["q0"][None], np.zeros((steps, n, m.nq))])),
             v=DeviceArray(np.concatenate([x["v0"][None], np.zeros((steps, n, m.nv))])), u=DeviceArray(np.zeros((steps, n, nu))),
             a=DeviceArray(np.zeros((steps, n, m.nv))), f=DeviceArray(np.zeros((steps, n, 4, 3))), u1=DeviceArray(np.zeros((n, nu))))
    pol = capi.RbdPolicy()
    for k in capi.RbdPolicy.ARRAYS:
        setattr(pol, k, d[k].ptr.value)
    capi.check(r.lib.idocp_rbd_feedback_torques_batch_device(r.h, n, d["q"].ptr, d["v"].ptr, C.byref(pol), d["u1"].ptr), "idocp_rbd_feedback_torques_batch_device")
    act = (C.c_int * (4 * steps))(*[b for s in masks[:steps] for b in s])
    capi.check(r.lib.idocp_rbd_rollout_policy_device(r.h, n, steps, act, TS, dt, C.byref(pol), d["pts"].ptr, d["q"].ptr, d["v"].ptr, d["u"].ptr, d["a"].ptr,
                                                     d["f"].ptr, impulse), "idocp_rbd_rollout_policy_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    assert np.array_equal(d["u1"].numpy(), u_one)
    assert same([d[k].numpy() for k in "qvuaf"], host)
    for a in d.values():
        a.free()
    r.close()


def test_a_launch_of_131_equals_131_launches_of_one():
    m, M, x = rollout_case()
    n = 131
    r = Rbd(m)
    big = device_rollout(r, x, n, STEPS, "b")
    masks, dt, impulse = SCHEDULES["b"]
    for i in range(n):
        one = RP.rollout_policy(r, x["q0"][i:i + 1], x["v0"][i:i + 1], STEPS, masks, TS, dt, x["pts"][:, i:i + 1], impulse,
                                **{k: x[k][:, i:i + 1] for k in ("u_ff", "K", "q_ref", "v_ref")})
        assert same(one, [a[:, i:i + 1] for a in big]), i
    r.close()


def test_without_u_traj_the_trajectories_are_the_same():
    m, M, x = rollout_case()
    r = Rbd(m)
    for n in (3, 131, 3):                                  # (the handle's torque buffer grows once and is kept)
        with_u = device_rollout(r, x, n, 2, "b")
        without = device_rollout(r, x, n, 2, "b", want_u=False)
        assert without[2] is None and same([without[k] for k in (0, 1, 3, 4)], [with_u[k] for k in (0, 1, 3, 4)]), n
    r.close()


# ------------------------------------------------------------------ 6. NaN

def test_a_nan_reference_poisons_its_own_sample_only():
    m, M, x = rollout_case()
    n, steps = 5, 3
    r = Rbd(m)
    good = device_rollout(r, x, n, steps, "a")
    q_ref = x["q_ref"][:steps, :n].copy()
    q_ref[0, 1, 9] = np.nan
    q, v, u, a, f = device_rollout(r, x, n, steps, "a", q_ref=q_ref)
    assert np.isnan(u[:, 1]).all() and np.isnan(a[:, 1]).all() and np.isnan(f[:, 1]).all() and np.isnan(v[1:, 1]).all() and np.isnan(q[2:, 1]).all()
    keep = [0, 2, 3, 4]
    assert same([arr[:, keep] for arr in (q, v, u, a, f)], [arr[:, keep] for arr in good])
    # one evaluation: NaN and infinity, in the gains and in the state
    for name, value in (("K", np.nan), ("K", np.inf), ("v_ref", -np.inf), ("u_ff", np.nan)):
        pol = {k: x[k][0, :n].copy() for k in ("u_ff", "K", "q_ref", "v_ref")}
        pol[name][3, 1] = value
        u1 = RP.feedback_torques(r, x["q0"][:n], x["v0"][:n], **pol)
        assert np.isnan(u1[3]).all(), (name, value)
        others = [0, 1, 2, 4]
        assert np.array_equal(u1[others], good[2][0][others]), (name, value)
    again = device_rollout(r, x, n, steps, "a")
    assert same(again, good)
    r.close()


# ------------------------------------------------------------------ refusals (they need a handle, and a handle needs a device)

def test_refusals():
    lib = capi.lib()
    m, M, x = rollout_case()
    n, steps, nu = 2, 1, m.nu

    def refused(rc, call, what, text=None):
        """the code and the COMPLETE text of idocp_last_error(): the call's name, then TEXTS[what] or the text given"""
        assert rc == E_ARG, what
        msg = lib.idocp_last_error().decode()
        assert msg == call + (text or TEXTS[what]), (what, msg)

    NO_CONTACTS = ": a fixed-base chain has no contacts (f and contact_points must be NULL)"
    TEXTS = {"null policy": ": null policy", "null policy, device form": ": null policy",
             "K without q_ref": ": gains K need the references q_ref and v_ref", "K without v_ref": ": gains K need the references q_ref and v_ref",
             "u_min > u_max": ": u_min[5] <= u_max[5] does not hold (or a bound is NaN)",
             "NaN in u_min": ": u_min[11] <= u_max[11] does not hold (or a bound is NaN)", "NaN in u_max": ": u_min[11] <= u_max[11] does not hold (or a bound is NaN)",
             "n = 0": ": n must be positive", "no q": ": q, v and u are needed", "no u": ": q, v and u are needed",
             "steps = 0": ": steps must be at least 1", "no active": ": the contact status `active` is needed", "dt = nan": ": dt must be finite",
             "active contacts without contact_points": ": STAGE mode with an active contact needs contact_points",
             "active contacts without a time step": ": STAGE mode with an active contact needs a positive Baumgarte time_step",
             "no q_traj": ": q and v are needed", "chain with contact_points": NO_CONTACTS, "chain with f_traj": NO_CONTACTS}

    r = Rbd(m)
    q, v, u = x["q0"][:n].copy(), x["v0"][:n].copy(), np.zeros((n, nu))
    arrays = dict(u_ff=x["u_ff"][0, :n], K=x["K"][0, :n], q_ref=x["q_ref"][0, :n], v_ref=x["v_ref"][0, :n])
    bad_pair = (np.full(nu, 1.0), np.full(nu, 1.0))
    bad_pair[0][5] = 1.5
    nan_bound = np.full(nu, 1.0)
    nan_bound[11] = np.nan
    bad_policies = {"K without q_ref": dict(arrays, q_ref=None), "K without v_ref": dict(arrays, v_ref=None), "u_min > u_max": dict(arrays, u_min=bad_pair[0], u_max=bad_pair[1]),
                    "NaN in u_min": dict(arrays, u_min=nan_bound), "NaN in u_max": dict(arrays, u_max=nan_bound)}
    qt, vt = np.zeros((2, n, m.nq)), np.zeros((2, n, m.nv))
    qt[0], vt[0] = q, v
    pts = x["pts"][:1, :n].copy()
    act = [[1, 1, 1, 1]]
    call = "idocp_rbd_feedback_torques_batch"
    refused(RP.torques_raw(r, n, q, v, None, u), call, "null policy")
    for what, arr in bad_policies.items():
        pol, keep = RP.policy_struct(**arr)
        refused(RP.torques_raw(r, n, q, v, pol, u), call, what)
    pol, keep = RP.policy_struct(**arrays)
    refused(RP.torques_raw(r, 0, q, v, pol, u), call, "n = 0")
    refused(RP.torques_raw(r, n, None, v, pol, u), call, "no q")
    refused(RP.torques_raw(r, n, q, v, pol, None), call, "no u")
    refused(RP.torques_raw(r, n, q, v, None, u, device=True), call + "_device", "null policy, device form")
    # two conditions violated at once: the one tested first is the one reported
    refused(RP.torques_raw(r, 0, None, v, None, u), call, "n = 0, no q and a null policy", ": n must be positive")
    refused(RP.torques_raw(r, n, None, v, None, u), call, "no q and a null policy", ": q, v and u are needed")
    bad, keep2 = RP.policy_struct(**dict(arrays, q_ref=None, u_min=nan_bound))
    refused(RP.torques_raw(r, n, q, v, bad, u), call, "K without q_ref and NaN in u_min", ": gains K need the references q_ref and v_ref")
    call = "idocp_rbd_rollout_policy"
    refused(RP.rollout_policy_raw(r, n, steps, act, TS, 1e-2, None, pts, qt, vt, None, None, None, 0), call, "null policy")
    refused(RP.rollout_policy_raw(r, n, steps, act, TS, 1e-2, None, pts, qt, vt, None, None, None, 0, device=True), call + "_device", "null policy, device form")
    for what, arr in bad_policies.items():
        bad, keep2 = RP.policy_struct(**arr)
        refused(RP.rollout_policy_raw(r, n, steps, act, TS, 1e-2, bad, pts, qt, vt, None, None, None, 0), call, what)
    # the refusals of idocp_rbd_rollout, under this call's name
    refused(RP.rollout_policy_raw(r, n, 0, act, TS, 1e-2, pol, pts, qt, vt, None, None, None, 0), call, "steps = 0")
    refused(RP.rollout_policy_raw(r, n, steps, None, TS, 1e-2, pol, pts, qt, vt, None, None, None, 0), call, "no active")
    refused(RP.rollout_policy_raw(r, n, steps, act, TS, float("nan"), pol, pts, qt, vt, None, None, None, 0), call, "dt = nan")
    refused(RP.rollout_policy_raw(r, n, steps, act, TS, 1e-2, pol, None, qt, vt, None, None, None, 0), call, "active contacts without contact_points")
    refused(RP.rollout_policy_raw(r, n, steps, act, 0.0, 1e-2, pol, pts, qt, vt, None, None, None, 0), call, "active contacts without a time step")
    refused(RP.rollout_policy_raw(r, n, steps, act, TS, 1e-2, pol, pts, None, vt, None, None, None, 0), call, "no q_traj")
    refused(RP.rollout_policy_raw(r, n, 0, None, TS, 1e-2, None, pts, qt, vt, None, None, None, 0), call, "steps = 0, no active and a null policy",
            ": steps must be at least 1")
    refused(RP.rollout_policy_raw(r, n, steps, act, TS, 1e-2, None, None, qt, vt, None, None, None, 0), call, "no contact_points and a null policy",
            ": STAGE mode with an active contact needs contact_points")
    refused(RP.rollout_policy_raw(r, 0, steps, act, TS, 1e-2, pol, pts, qt, vt, None, None, None, 0, device=True), call + "_device", "n = 0, device form",
            ": n must be positive")
    # the refusals left the handle usable
    assert np.isfinite(RP.feedback_torques(r, q, v, **arrays)).all()
    r.close()
    # a chain takes active = NULL and contact_points = NULL, and nothing else
    mc, Mc, xc = chain_case(2)
    r = Rbd(mc)
    polc, keepc = RP.policy_struct(**{k: xc[k][:1, :n] for k in ("u_ff", "K", "q_ref", "v_ref")})
    qt, vt = np.zeros((2, n, 2)), np.zeros((2, n, 2))
    junk = np.zeros((1, n, 12))
    refused(RP.rollout_policy_raw(r, n, 1, None, 0.0, 1e-2, polc, junk, qt, vt, None, None, None, 0), call, "chain with contact_points")
    refused(RP.rollout_policy_raw(r, n, 1, None, 0.0, 1e-2, polc, None, qt, vt, None, None, junk, 0), call, "chain with f_traj")
    assert RP.rollout_policy_raw(r, n, 1, None, 0.0, 1e-2, polc, None, qt, vt, None, None, None, 0) == 0
    r.close()


# ------------------------------------------------------------------ 7. the example

def test_anymal_closed_loop_rollout_example():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "anymal_closed_loop_rollout"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(ROOT, "examples", "anymal_closed_loop_rollout"), ANYMAL_URDF], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    print(r.stdout)
    closed = re.search(r"closed loop: max final \|x \(-\) x_ref\| = (\S+)", r.stdout)
    opened = re.search(r"open loop:   max final \|x \(-\) x_ref\| = (\S+)", r.stdout)
    assert closed and opened, r.stdout
    assert math.isfinite(float(closed.group(1))) and math.isfinite(float(opened.group(1))), r.stdout
