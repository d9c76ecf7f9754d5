"""Shared by test_rbd_forward_dynamics_gpu.py / test_rbd_forward_dynamics_host.py: the forward-dynamics calls of the idocp_rbd_* handle
(idocp_rbd_forward_dynamics_batch, idocp_rbd_rollout; include/idocp_hip.h) on numpy arrays, and the numpy referee of their answers."""
import ctypes as C
import sys

import numpy as np

from helpers import GOLDEN
from idocp_amd import capi
from rbd_batch import IMPULSE, STAGE, Rbd      # noqa: F401

sys.path.insert(0, GOLDEN)
import gen_golden_kkt as G      # noqa: E402
import gen_golden_rbd as RBD      # noqa: E402
import independent_rbd as IR      # noqa: E402

FD_OUTPUTS = capi.RbdFdIO.OUTPUTS


def fd_shapes(m):
    return {"a": (m.nv,), "f": (m.ncontacts, 3), "q_next": (m.nq,), "v_next": (m.nv,)}


def _act(active):
    return (C.c_int * len(active))(*[int(x) for x in active]) if active is not None else None


def forward_raw(r, mode, n, active, time_step, dt, io, device=False):
    fn = r.lib.idocp_rbd_forward_dynamics_batch_device if device else r.lib.idocp_rbd_forward_dynamics_batch
    return fn(r.h, mode, n, _act(active), time_step, dt, C.byref(io) if io is not None else None)


def forward(r, mode, q, v, u=None, active=None, time_step=0.0, dt=0.0, contact_points=None, outputs=FD_OUTPUTS, fill=np.nan, buffers=None):
    """host form; returns {name: array [n][...]}.  buffers: arrays to write into instead of fresh ones (the sentinel checks)"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    n = q.shape[0]
    keep = {"q": q, "v": np.ascontiguousarray(v, dtype=np.float64)}
    for name, x in (("u", u), ("contact_points", contact_points)):
        if x is not None:
            keep[name] = np.ascontiguousarray(x, dtype=np.float64)
    shapes = fd_shapes(r.m)
    if not r.m.ncontacts:
        outputs = tuple(name for name in outputs if name != "f")      # (a chain has no contact forces: f must stay NULL)
    out = {name: (buffers[name] if buffers else np.full((n,) + shapes[name], fill)) for name in outputs}
    io = capi.RbdFdIO()
    for name, x in list(keep.items()) + list(out.items()):
        setattr(io, name, x.ctypes.data)
    capi.check(forward_raw(r, mode, n, active, time_step, dt, io), "idocp_rbd_forward_dynamics_batch")
    return out


def rollout_raw(r, n, steps, active, time_step, dt, u, pts, q_traj, v_traj, a_traj, f_traj, impulse, device=False):
    fn = r.lib.idocp_rbd_rollout_device if device else r.lib.idocp_rbd_rollout
    flat = _act(np.asarray(active).reshape(-1)) if active is not None else None
    ptr = lambda x: x.ctypes.data if x is not None else None      # noqa: E731
    return fn(r.h, n, steps, flat, time_step, dt, ptr(u), ptr(pts), ptr(q_traj), ptr(v_traj), ptr(a_traj), ptr(f_traj), int(impulse))


def rollout(r, q0, v0, u, active=None, time_step=0.0, dt=0.0, contact_points=None, impulse=False):
    """host form; u [steps][n][nu]; returns (q_traj, v_traj, a_traj, f_traj); f_traj is None on a chain"""
    u = np.ascontiguousarray(u, dtype=np.float64)
    steps, n = u.shape[:2]
    m = r.m
    q_traj, v_traj = np.full((steps + 1, n, m.nq), np.nan), np.full((steps + 1, n, m.nv), np.nan)
    q_traj[0], v_traj[0] = q0, v0
    a_traj = np.full((steps, n, m.nv), np.nan)
    f_traj = np.full((steps, n, m.ncontacts, 3), np.nan) if m.ncontacts else None
    pts = np.ascontiguousarray(contact_points, dtype=np.float64) if contact_points is not None else None
    capi.check(rollout_raw(r, n, steps, active, time_step, dt, u, pts, q_traj, v_traj, a_traj, f_traj, impulse), "idocp_rbd_rollout")
    return q_traj, v_traj, a_traj, f_traj


# ------------------------------------------------------------------ the numpy referee

def _step(nv, k):
    e = np.zeros(nv, complex)
    e[k] = 1e-30j
    return e


def mass_matrix(M, q, v, gravity=True):
    """dID/da by the complex step on a alone (the third block of gen_golden_rbd.rnea_derivatives, a third of its work)"""
    nv, z = M["nv"], np.zeros(M["nv"])
    return np.array([RBD.rnea(M, q, v, z + _step(nv, k), None, gravity=gravity).imag / 1e-30 for k in range(nv)]).T


def contact_rows(M, q, v, mask, pts, time_step, impulse=False):
    """(J, b) over the active rows from the independent model's frame kinematics.  STAGE: b = C(q, v, 0), the Baumgarte residual as
    point_contact.hxx:67-87 states it (classical LOCAL acceleration + (2 / D) LOCAL velocity + (1 / D^2) (p - p_ref)), J = dC/da by the complex
    step on a.  IMPULSE: b = J v, the LOCAL linear velocity of the contact frames, J by the complex step on v."""
    act = np.array(mask, dtype=bool)
    Ma = dict(M)
    Ma["contacts"] = [c for c, on in zip(M["contacts"], act) if on]
    nv, z = M["nv"], np.zeros(M["nv"])
    if not act.any():
        return np.zeros((0, nv)), np.zeros(0)
    fk = RBD.frame_kinematics(Ma, q, v, z)
    if impulse:
        b = np.concatenate([x["v"][:3].real for x in fk])
        J = np.array([np.concatenate([x["v"][:3].imag for x in RBD.frame_kinematics(Ma, q, v + _step(nv, k), z)]) / 1e-30 for k in range(nv)]).T
        return J, b
    ref = np.asarray(pts, dtype=np.float64).reshape(-1, 3)[act]
    b = np.concatenate([x["a"][:3].real + np.cross(x["v"][3:].real, x["v"][:3].real) + 2.0 / time_step * x["v"][:3].real
                        + (x["p"].real - ref[c]) / time_step ** 2 for c, x in enumerate(fk)])
    J = np.array([np.concatenate([x["a"][:3].imag for x in RBD.frame_kinematics(Ma, q, v, z + _step(nv, k))]) / 1e-30 for k in range(nv)]).T
    return J, b


def force_map(M, q, v, mask, impulse=False):
    """G [nv][3 nactive]: tau(f = e_i) - tau(f = 0) from the model's own rnea, so that no sign or frame convention of the forces is assumed"""
    nc, z = len(M["contacts"]), np.zeros(M["nv"])
    vv = z if impulse else v
    t0 = RBD.rnea(M, q, vv, z, None, gravity=not impulse)
    cols = []
    for c in range(nc):
        if not mask[c]:
            continue
        for r in range(3):
            f = np.zeros((nc, 3))
            f[c, r] = 1.0
            cols.append(RBD.rnea(M, q, vv, z, IR.joint_forces(M, f, [bool(x) for x in mask]), gravity=not impulse) - t0)
    return np.array(cols).T.reshape(M["nv"], -1)


def sample_terms(M, q, v, pts=None, time_step=None, impulse=False):
    """What the answers of ONE sample are made of, with every contact active (a status selects rows and columns of it): h, M, and on a model with
    contacts J, b and G = dID/df (it comes out as -J^T).  IMPULSE: no gravity and no velocity in the dynamics, J v for b."""
    q, v = np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64)
    nc, z = len(M["contacts"]), np.zeros(M["nv"])
    vv = z if impulse else v
    t = {"h": RBD.rnea(M, q, vv, z, None, gravity=not impulse), "M": mass_matrix(M, q, vv, gravity=not impulse)}
    if nc:
        t["J"], t["b"] = contact_rows(M, q, v, [1] * nc, pts, time_step, impulse)
        t["G"] = force_map(M, q, v, [1] * nc, impulse)
    return t


def solve_terms(t, u, mask):
    """(a, f[nc][3]) from sample_terms by a refined dense solve of [M G; J 0] [a; f] = [S^T u - h; -b] over the active rows"""
    nv = t["h"].size
    nc = t["b"].size // 3 if "b" in t else 0
    tau = np.zeros(nv)
    if u is not None:
        tau[nv - len(u):] = u
    rhs = tau - t["h"]
    rows = np.repeat(np.array(mask, dtype=bool), 3) if nc else np.zeros(0, dtype=bool)
    if not rows.any():
        a, _ = G.solve_refined(t["M"], rhs.reshape(-1, 1))
        return a.reshape(-1), np.zeros((nc, 3))
    J, b, Gm = t["J"][rows], t["b"][rows], t["G"][:, rows]
    nf = J.shape[0]
    K = np.block([[t["M"], Gm], [J, np.zeros((nf, nf))]])
    x, _ = G.solve_refined(K, np.concatenate([rhs, -b]).reshape(-1, 1))
    x = x.reshape(-1)
    f = np.zeros(3 * nc)
    f[rows] = x[nv:]
    return x[:nv], f.reshape(nc, 3)


def reference(M, q, v, u, mask, pts=None, time_step=None, impulse=False):
    """One sample of the numpy model: (a, f) of STAGE mode or (dv, lambda) of IMPULSE mode (u is ignored there)"""
    return solve_terms(sample_terms(M, q, v, pts, time_step, impulse), None if impulse else u, mask)


def euler_step(M, q, v, a, dt):
    """the OCP's explicit Euler step with gen_golden_rbd.integrate.  The generator returns the quaternion with w >= 0, the library the one on the
    side of q's (the same rotation: the quaternion double cover), so the generator's is brought to that side -- as test_model_lie_host.py does"""
    q = np.asarray(q, dtype=np.float64)
    qn = RBD.integrate(M, q, dt * np.asarray(v))
    if M.get("floating") and np.dot(qn[3:7], q[3:7]) < 0:
        qn[3:7] *= -1
    return qn, np.asarray(v) + dt * np.asarray(a)


def foot_positions(m, q):
    """idocp_model_contact_positions for every sample"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    out = np.zeros((q.shape[0], m.ncontacts, 3))
    lib = capi.lib()
    for i in range(q.shape[0]):
        capi.check(lib.idocp_model_contact_positions(C.byref(m), q[i].ctypes.data_as(C.POINTER(C.c_double)), out[i].ctypes.data_as(C.POINTER(C.c_double))),
                   "idocp_model_contact_positions")
    return out
