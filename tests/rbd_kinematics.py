"""Shared by test_rbd_kinematics_gpu.py / test_rbd_kinematics_host.py: the contact-frame kinematics and the foothold rollout of the idocp_rbd_*
handle (idocp_rbd_contact_kinematics_batch, idocp_rbd_rollout_footholds; include/idocp_hip.h) on numpy arrays, and their numpy referee:
gen_golden_rbd.frame_kinematics for the frames, rbd_forward.reference / euler_step and the latch rule for the rollout.  Nothing in the referee
calls the library's arithmetic."""
import ctypes as C

import numpy as np

import rbd_forward as F
import rbd_policy as PO
from helpers import ANYMAL_Q_STANDING
from idocp_amd import capi
from rbd_forward import RBD

KIN_OUTPUTS = capi.RbdKinIO.OUTPUTS
KIN_NAME, ROLL_NAME = "idocp_rbd_contact_kinematics_batch", "idocp_rbd_rollout_footholds"


def kin_shapes(m):
    """per-sample shape of every output; the column-major jacobian as numpy sees it: [column][row]"""
    return {"points": (m.ncontacts, 3), "rotation": (m.ncontacts, 3, 3), "velocity": (m.ncontacts, 3), "jacobian": (m.nv, 3 * m.ncontacts)}


def kinematics_raw(r, n, io, device=False):
    fn = r.lib.idocp_rbd_contact_kinematics_batch_device if device else r.lib.idocp_rbd_contact_kinematics_batch
    return fn(r.h, n, C.byref(io) if io is not None else None)


def kinematics(r, q, v=None, outputs=KIN_OUTPUTS, tail=0):
    """host form; returns {name: array [n + tail][...]}, the jacobian as [column][row]; the `tail` extra samples of every output are NaN and are
    not the call's to write"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    n = q.shape[0]
    v = np.ascontiguousarray(v, dtype=np.float64) if v is not None else None
    out = {name: np.full((n + tail,) + kin_shapes(r.m)[name], np.nan) for name in outputs}
    io = capi.RbdKinIO()
    io.q, io.v = q.ctypes.data, (v.ctypes.data if v is not None else None)
    for name, x in out.items():
        setattr(io, name, x.ctypes.data)
    capi.check(kinematics_raw(r, n, io), KIN_NAME)
    return out


def footholds_struct(pts, q_traj, v_traj, u=None, pol=None, u_traj=None, a_traj=None, f_traj=None):
    """idocp_rbd_foothold_rollout_t over numpy arrays (or anything with .ctypes.data); pol: a capi.RbdPolicy or None"""
    ptr = lambda x: x.ctypes.data if x is not None else None      # noqa: E731
    io = capi.RbdFootholdRollout()
    io.u, io.policy = ptr(u), (C.pointer(pol) if pol is not None else None)
    io.contact_points, io.q_traj, io.v_traj, io.u_traj, io.a_traj, io.f_traj = ptr(pts), ptr(q_traj), ptr(v_traj), ptr(u_traj), ptr(a_traj), ptr(f_traj)
    return io


def footholds_raw(r, n, steps, active, time_step, dt, io, impulse, latch_first, device=False):
    fn = r.lib.idocp_rbd_rollout_footholds_device if device else r.lib.idocp_rbd_rollout_footholds
    flat = F._act(np.asarray(active).reshape(-1)) if active is not None else None
    return fn(r.h, n, steps, flat, time_step, dt, C.byref(io) if io is not None else None, int(impulse), int(latch_first))


def footholds(r, q0, v0, steps, active, time_step, dt, pts0, u=None, impulse=False, latch_first=False, policy=None):
    """host form; pts0 [n][nc][3]: slice 0 of contact_points; policy: the keyword arguments of rbd_policy.policy_struct or None.
    Returns (contact_points, q_traj, v_traj, u_traj or None, a_traj, f_traj)."""
    m, n = r.m, np.asarray(q0).shape[0]
    q_traj, v_traj = np.full((steps + 1, n, m.nq), np.nan), np.full((steps + 1, n, m.nv), np.nan)
    q_traj[0], v_traj[0] = q0, v0
    pts = np.full((steps, n, m.ncontacts, 3), np.nan)
    pts[0] = pts0
    a_traj, f_traj = np.full((steps, n, m.nv), -777.0), np.full((steps, n, m.ncontacts, 3), -777.0)
    u = np.ascontiguousarray(u, dtype=np.float64) if u is not None else None
    pol, keep, u_traj = None, None, None
    if policy is not None:
        pol, keep = PO.policy_struct(**policy)
        u_traj = np.full((steps, n, m.nu), -777.0)
    io = footholds_struct(pts, q_traj, v_traj, u, pol, u_traj, a_traj, f_traj)
    capi.check(footholds_raw(r, n, steps, active, time_step, dt, io, impulse, latch_first), ROLL_NAME)
    del keep
    return pts, q_traj, v_traj, u_traj, a_traj, f_traj


def standing_samples(rng, n):
    """(q, v): base position +-0.5, random unit quaternions, joints +-0.5 about the standing pose, velocities +-1"""
    q = np.tile(ANYMAL_Q_STANDING, (n, 1))
    q[:, :3] = rng.uniform(-0.5, 0.5, (n, 3))
    quat = rng.normal(size=(n, 4))
    q[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    q[:, 7:] += rng.uniform(-0.5, 0.5, (n, 12))
    return q, rng.uniform(-1, 1, (n, 18))


# ------------------------------------------------------------------ the numpy referee

def reference(M, q, v):
    """One sample from gen_golden_rbd.frame_kinematics (p, R and the LOCAL velocity per contact): points = p, rotation = R,
    velocity = R v_local[:3], jacobian [3 nc][nv] = column r the world velocity under the unit tangent e_r, by the complex step on v."""
    q, v = np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64)
    nv, z = M["nv"], np.zeros(M["nv"])
    fk = RBD.frame_kinematics(M, q, v, z)
    R = [np.asarray(x["R"]).real for x in fk]
    out = {"points": np.array([np.asarray(x["p"]).real for x in fk]), "rotation": np.array(R),
           "velocity": np.array([Rc @ np.asarray(x["v"][:3]).real for Rc, x in zip(R, fk)])}
    J = np.zeros((3 * len(fk), nv))
    for k in range(nv):
        fs = RBD.frame_kinematics(M, q, z + F._step(nv, k), z)
        J[:, k] = np.concatenate([Rc @ (x["v"][:3].imag / 1e-30) for Rc, x in zip(R, fs)])
    out["jacobian"] = J
    return out


def reference_points(M, q):
    return np.array([np.asarray(x["p"]).real for x in RBD.frame_kinematics(M, np.asarray(q, dtype=np.float64), np.zeros(M["nv"]), np.zeros(M["nv"]))])


def stays(active, k, c, latch_first):
    return bool(active[k][c]) and (bool(active[k - 1][c]) if k > 0 else not latch_first)


def latched_rollout(M, q0, v0, steps, active, pts0, time_step, dt, impulse, latch_first, torques):
    """One sample of the numpy latched rollout: per step the contact points by the rule (carried where stays(), the referee's points(q) elsewhere),
    the touchdown impulse if any, torques(k, q, v) -> u or None, rbd_forward.reference, euler_step.
    Returns (points [steps][nc][3], q [steps + 1], v [steps + 1] -- slice k the post-impulse velocity --, a, f [steps])."""
    q, v = np.array(q0, dtype=np.float64), np.array(v0, dtype=np.float64)
    nc = len(M["contacts"])
    prev = np.array(pts0, dtype=np.float64)
    ps, qs, vs, As, fs = [], [q], [], [], []
    for k in range(steps):
        foot = reference_points(M, q)
        pts = np.array([prev[c] if stays(active, k, c, latch_first) else foot[c] for c in range(nc)])
        if impulse and k > 0:
            new = [int(b and not a) for a, b in zip(active[k - 1], active[k])]
            if any(new):
                v = v + F.reference(M, q, v, None, new, impulse=True)[0]
        vs.append(v)
        a, f = F.reference(M, q, v, torques(k, q, v), list(active[k]), pts, time_step)
        q, v = F.euler_step(M, q, v, a, dt)
        ps.append(pts); qs.append(q); As.append(a); fs.append(f)
        prev = pts
    vs.append(v)
    return np.array(ps), np.array(qs), np.array(vs), np.array(As), np.array(fs)
