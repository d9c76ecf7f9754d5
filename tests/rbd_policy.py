"""Shared by test_rbd_policy_gpu.py / test_rbd_policy_host.py: the closed-loop calls of the idocp_rbd_* handle (idocp_rbd_feedback_torques_batch,
idocp_rbd_rollout_policy; include/idocp_hip.h) on numpy arrays, and their numpy referee -- the torques on gen_golden_rbd.difference, the closed loop
on rbd_forward.reference and rbd_forward.euler_step."""
import ctypes as C

import numpy as np

import rbd_forward as F
from idocp_amd import capi
from rbd_forward import RBD

ARRAYS = capi.RbdPolicy.ARRAYS


def policy_struct(shared_gains=False, shared_ref=False, **arrays):
    """(idocp_rbd_policy_t, the arrays it points to); an array left out or None is NULL"""
    keep = {k: np.ascontiguousarray(x, dtype=np.float64) for k, x in arrays.items() if x is not None}
    assert set(keep) <= set(ARRAYS), keep.keys()
    pol = capi.RbdPolicy()
    for k, x in keep.items():
        setattr(pol, k, x.ctypes.data)
    pol.shared_gains, pol.shared_ref = int(shared_gains), int(shared_ref)
    return pol, keep


def torques_raw(r, n, q, v, pol, u, device=False):
    fn = r.lib.idocp_rbd_feedback_torques_batch_device if device else r.lib.idocp_rbd_feedback_torques_batch
    ptr = lambda x: x.ctypes.data if x is not None else None      # noqa: E731
    return fn(r.h, n, ptr(q), ptr(v), C.byref(pol) if pol is not None else None, ptr(u))


def feedback_torques(r, q, v, shared_gains=False, shared_ref=False, **arrays):
    """host form; returns u [n][nu]"""
    q, v = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
    pol, keep = policy_struct(shared_gains, shared_ref, **arrays)
    u = np.full((q.shape[0], r.m.nu), -777.0)
    capi.check(torques_raw(r, q.shape[0], q, v, pol, u), "idocp_rbd_feedback_torques_batch")
    del keep
    return u


def rollout_policy_raw(r, n, steps, active, time_step, dt, pol, pts, q_traj, v_traj, u_traj, a_traj, f_traj, impulse, device=False):
    fn = r.lib.idocp_rbd_rollout_policy_device if device else r.lib.idocp_rbd_rollout_policy
    flat = F._act(np.asarray(active).reshape(-1)) if active is not None else None
    ptr = lambda x: x.ctypes.data if x is not None else None      # noqa: E731
    return fn(r.h, n, steps, flat, time_step, dt, C.byref(pol) if pol is not None else None, ptr(pts), ptr(q_traj), ptr(v_traj), ptr(u_traj), ptr(a_traj),
              ptr(f_traj), int(impulse))


def rollout_policy(r, q0, v0, steps, active=None, time_step=0.0, dt=0.0, contact_points=None, impulse=False, want_u=True, shared_gains=False,
                   shared_ref=False, **arrays):
    """host form; returns (q_traj, v_traj, u_traj, a_traj, f_traj); f_traj is None on a chain, u_traj None without want_u"""
    m, n = r.m, np.asarray(q0).shape[0]
    q_traj, v_traj = np.full((steps + 1, n, m.nq), np.nan), np.full((steps + 1, n, m.nv), np.nan)
    q_traj[0], v_traj[0] = q0, v0
    u_traj = np.full((steps, n, m.nu), -777.0) if want_u else None
    a_traj = np.full((steps, n, m.nv), -777.0)
    f_traj = np.full((steps, n, m.ncontacts, 3), -777.0) if m.ncontacts else None
    pts = np.ascontiguousarray(contact_points, dtype=np.float64) if contact_points is not None else None
    pol, keep = policy_struct(shared_gains, shared_ref, **arrays)
    capi.check(rollout_policy_raw(r, n, steps, active, time_step, dt, pol, pts, q_traj, v_traj, u_traj, a_traj, f_traj, impulse), "idocp_rbd_rollout_policy")
    del keep
    return q_traj, v_traj, u_traj, a_traj, f_traj


# ------------------------------------------------------------------ the numpy referee

def gain_matrix(M, K):
    """the nu x 2 nv matrix of one column-major gain block"""
    nv = M["nv"]
    return np.asarray(K, dtype=np.float64).reshape(2 * nv, -1).T


def reference_torques(M, q, v, u_ff=None, K=None, q_ref=None, v_ref=None, u_min=None, u_max=None):
    """One sample: clamp(u_ff + K [q (-) q_ref ; v - v_ref]) with gen_golden_rbd.difference (its own SE(3) logarithm); K: the column-major block"""
    nv = M["nv"]
    nu = nv - 6 if M.get("floating") else nv
    u = np.zeros(nu) if u_ff is None else np.array(u_ff, dtype=np.float64)
    if K is not None:
        dx = np.concatenate([RBD.difference(M, np.asarray(q_ref, dtype=np.float64), np.asarray(q, dtype=np.float64)), np.asarray(v) - np.asarray(v_ref)])
        u = u + gain_matrix(M, K) @ dx
    if u_min is not None:
        u = np.maximum(u, u_min)
    if u_max is not None:
        u = np.minimum(u, u_max)
    return u


def closed_loop(M, q0, v0, steps, schedule, pts, time_step, dt, impulse, policy):
    """One sample of the numpy closed loop: per step the touchdown impulse if any, the referee torques at the state the step starts from, reference(),
    euler_step().  policy(k) -> the keyword arguments of reference_torques for step k; schedule: [steps][ncontacts] or None on a chain; pts: [steps][nc][3].
    Returns (q [steps + 1], v [steps + 1] -- slice k the post-impulse velocity --, u, a, f [steps])."""
    q, v = np.array(q0, dtype=np.float64), np.array(v0, dtype=np.float64)
    nc = len(M["contacts"])
    qs, vs, us, As, fs = [q], [], [], [], []
    for k in range(steps):
        mask = list(schedule[k]) if nc else []
        if nc and impulse and k > 0:
            new = [int(b and not a) for a, b in zip(schedule[k - 1], schedule[k])]
            if any(new):
                v = v + F.reference(M, q, v, None, new, impulse=True)[0]
        vs.append(v)
        u = reference_torques(M, q, v, **policy(k))
        a, f = F.reference(M, q, v, u, mask, pts[k] if nc else None, time_step)
        q, v = F.euler_step(M, q, v, a, dt)
        qs.append(q); us.append(u); As.append(a); fs.append(f)
    vs.append(v)
    return np.array(qs), np.array(vs), np.array(us), np.array(As), np.array(fs)


def same_rotation(q, q_ref):
    """q with the base quaternion on the side of q_ref's (the quaternion double cover), for comparisons of configurations"""
    q = np.array(q, dtype=np.float64)
    flip = np.sum(q[..., 3:7] * np.asarray(q_ref)[..., 3:7], axis=-1) < 0
    q[..., 3:7] = np.where(flip[..., None], -q[..., 3:7], q[..., 3:7])
    return q


def random_gains(rng, shape, nu, nv, norm=50.0):
    """column-major gain blocks [shape][nu * 2 nv] whose largest absolute row sum (the infinity norm) is `norm` each"""
    K = rng.uniform(-1, 1, tuple(shape) + (2 * nv, nu))
    K *= norm / np.abs(K).sum(axis=-2).max(axis=-1)[..., None, None]
    return K.reshape(tuple(shape) + (nu * 2 * nv,))


def perturbed_configurations(M, rng, q_ref, angle=2.0, lin=0.3, joint=0.5):
    """q = q_ref (+) d with a base rotation of at most `angle` rad (the logarithm is ill-conditioned near pi), per row of q_ref"""
    q_ref = np.asarray(q_ref)
    out = np.zeros_like(q_ref)
    for i in range(q_ref.shape[0]):
        d = rng.uniform(-joint, joint, M["nv"])
        if M.get("floating"):
            ax = rng.normal(size=3)
            d[:3] = rng.uniform(-lin, lin, 3)
            d[3:6] = ax / np.linalg.norm(ax) * rng.uniform(0.05, angle)
        out[i] = RBD.integrate(M, q_ref[i], d)
    return out
