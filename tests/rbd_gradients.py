"""Shared by test_rbd_gradients_host.py / test_rbd_gradients_gpu.py / test_rbd_ilqr_gpu.py: the calls idocp_rbd_objective_gradients,
idocp_rbd_objective_*_lqr_weights, idocp_rbd_ilqr_step_torques, idocp_rbd_ilqr_accept and idocp_rbd_ilqr_iterate of the idocp_rbd_* handle
(include/idocp_hip.h) on numpy arrays, and their numpy referees:

  gradients      lx = s [J^T (wq o e); wv o (v - v_ref_k)], lu = dt wu o (u - u_ref) with e = q (-) q_ref(t_k) on gen_golden_rbd.difference (its own SE(3)
                 logarithm) and J = Jlog6 of the relative base placement written out here in numpy; test_rbd_gradients_host.py holds this referee to
                 central differences of rbd_score.reference_score, which never see this Jlog6
  step torques   u + alpha k, u itself where alpha is 0
  accept         the rules of the header, one sample at a time, the copies by numpy.where
A plain module: the CPU test imports it too."""
import ctypes as C

import numpy as np

import rbd_forward as F
import rbd_score as RS
from idocp_amd import capi
from rbd_forward import RBD

ITEMS_PER_WORKGROUP = 64      # RBD_GRADIENT_ITEMS of idocp_amd/csrc/rbd_launch.hpp
ACCEPT_GROUP = 32             # RBD_ILQR_GROUP


# ------------------------------------------------------------------ the calls

def gradient_struct(**arrays):
    io = capi.RbdGradientIO()
    for k, x in arrays.items():
        if x is not None:
            setattr(io, k, x.ctypes.data if isinstance(x, np.ndarray) else x)
    return io


def gradients_raw(r, o, n, first_step, steps, terminal, io, device=False):
    fn = r.lib.idocp_rbd_objective_gradients_device if device else r.lib.idocp_rbd_objective_gradients
    return fn(r.h, o.h if isinstance(o, RS.Objective) else o, n, first_step, steps, int(terminal), C.byref(io) if io is not None else None)


def gradients(r, o, q, v, u=None, first_step=0, terminal=False, want=("lx_traj", "lu_traj"), device=False):
    """q [steps (+ 1)][n][nq], v, u [steps][n][nu] or None; returns (lx [steps (+ 1)][n][2 nv], lu [steps][n][nu]), None where not asked for"""
    c = lambda x: np.ascontiguousarray(x, dtype=np.float64) if x is not None else None      # noqa: E731
    q, v, u = c(q), c(v), c(u)
    slices, n = q.shape[:2]
    steps = slices - (1 if terminal else 0)
    out = {"lx_traj": np.full((slices, n, 2 * r.m.nv), -777.0) if "lx_traj" in want else None,
           "lu_traj": np.full((steps, n, r.m.nu), -777.0) if "lu_traj" in want else None}
    if not device:
        capi.check(gradients_raw(r, o, n, first_step, steps, terminal, gradient_struct(q_traj=q, v_traj=v, u_traj=u, **out)), "idocp_rbd_objective_gradients")
        return out["lx_traj"], out["lu_traj"]
    from rbd_batch import DeviceArray
    dev = {k: DeviceArray(x) for k, x in dict(q_traj=q, v_traj=v, u_traj=u, **out).items() if x is not None}
    capi.check(gradients_raw(r, o, n, first_step, steps, terminal, gradient_struct(**{k: d.ptr.value for k, d in dev.items()}), device=True),
               "idocp_rbd_objective_gradients_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    res = tuple(dev[k].numpy() if k in dev else None for k in ("lx_traj", "lu_traj"))
    for d in dev.values():
        d.free()
    return res


def host_weights(o, m):
    """(x_weight [2 nv], u_weight [nu], xf_weight [2 nv]) of idocp_rbd_objective_get_lqr_weights"""
    x, u, xf = np.full(2 * m.nv, np.nan), np.full(m.nu, np.nan), np.full(2 * m.nv, np.nan)
    capi.check(o.lib.idocp_rbd_objective_get_lqr_weights(o.h, x.ctypes.data, u.ctypes.data, xf.ctypes.data), "idocp_rbd_objective_get_lqr_weights")
    return x, u, xf


def device_weights(o):
    """the three device pointers of idocp_rbd_objective_lqr_weights_device"""
    x, u, xf = C.c_void_p(), C.c_void_p(), C.c_void_p()
    capi.check(o.lib.idocp_rbd_objective_lqr_weights_device(o.h, C.byref(x), C.byref(u), C.byref(xf)), "idocp_rbd_objective_lqr_weights_device")
    return x, u, xf


def download(ptr, count):
    x = np.empty(count)
    capi.check(capi.lib().idocp_device_download(x.ctypes.data, ptr, x.nbytes), "idocp_device_download")
    return x


def step_torques(r, u, k, alpha, device=False):
    c = lambda x: np.ascontiguousarray(x, dtype=np.float64)      # noqa: E731
    u, k, alpha = c(u), c(k), c(alpha)
    steps, n = u.shape[:2]
    out = np.full(u.shape, -777.0)
    if not device:
        capi.check(r.lib.idocp_rbd_ilqr_step_torques(r.h, n, steps, u.ctypes.data, k.ctypes.data, alpha.ctypes.data, out.ctypes.data), "idocp_rbd_ilqr_step_torques")
        return out
    from rbd_batch import DeviceArray
    du, dk, da, do = DeviceArray(u), DeviceArray(k), DeviceArray(alpha), DeviceArray(out)
    capi.check(r.lib.idocp_rbd_ilqr_step_torques_device(r.h, n, steps, du.ptr, dk.ptr, da.ptr, do.ptr), "idocp_rbd_ilqr_step_torques_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    out = do.numpy()
    for d in (du, dk, da, do):
        d.free()
    return out


ACCEPT_FLOATS = capi.RbdIlqrAcceptIO.CURRENT + capi.RbdIlqrAcceptIO.TRIAL + ("expected", "alpha", "alpha_accepted")


def accept_struct(arrays, consts):
    io = capi.RbdIlqrAcceptIO()
    for k, x in arrays.items():
        if x is not None:
            setattr(io, k, x.ctypes.data if isinstance(x, np.ndarray) else x)
    for k in capi.RbdIlqrAcceptIO.CONSTANTS:
        setattr(io, k, float(consts[k]))
    return io


def accept(r, state, consts, device=False):
    """state: {field: array} of idocp_rbd_ilqr_accept_io_t (done as int32); returns the state after the call, the inputs left unchanged"""
    s = {k: (np.ascontiguousarray(x, dtype=np.int32 if k == "done" else np.float64).copy() if x is not None else None) for k, x in state.items()}
    steps, n = s["u_traj"].shape[:2]
    if not device:
        capi.check(r.lib.idocp_rbd_ilqr_accept(r.h, n, steps, C.byref(accept_struct(s, consts))), "idocp_rbd_ilqr_accept")
        return s
    from rbd_batch import DeviceArray
    dev = {k: DeviceArray(x.view(np.float64) if k == "done" else x) for k, x in s.items() if x is not None and (k != "done" or n % 2 == 0)}
    if "done" not in dev:
        dev["done"] = DeviceArray(np.append(s["done"], 0).astype(np.int32).view(np.float64))
    capi.check(r.lib.idocp_rbd_ilqr_accept_device(r.h, n, steps, C.byref(accept_struct({k: d.ptr.value for k, d in dev.items()}, consts))), "idocp_rbd_ilqr_accept_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    for k, d in dev.items():
        s[k] = d.numpy().view(np.int32)[:n].copy() if k == "done" else d.numpy()
        d.free()
    return s


# ------------------------------------------------------------------ the numpy referees

def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def jlog6(R, p):
    """Jlog6 of the placement (R, p), [row, column] on (linear, angular): d log6(M exp6(eps)) / d eps at 0.  The closed form of pinocchio
    (Jlog3 of the rotation in the diagonal blocks, the coupling block from the translation), written for numpy"""
    c = min(1.0, max(-1.0, (np.trace(R) - 1) / 2))
    t = float(np.arccos(c))
    w = RBD.log3(R)
    t2 = t * t
    if t < 1e-4:
        alpha = beta = 1.0 / 12 + t2 / 720
        diag = 0.5 * (2 - t2 / 6)
        bdot = 1.0 / 360
    else:
        st, ct = np.sin(t), np.cos(t)
        alpha = 1 / t2 - st / (2 * t * (1 - ct))
        diag = 0.5 * t * st / (1 - ct)
        beta = alpha
        bdot = -2 / (t2 * t2) + (1 + st / t) / (t2 * 2 * (1 - ct))
    A = alpha * np.outer(w, w) + diag * np.eye(3) + 0.5 * skew(w)
    wTp = w @ p
    v3 = (bdot * wTp) * w - (t2 * bdot + 2 * beta) * p
    Cm = np.outer(v3, w) + beta * np.outer(w, p) + wTp * beta * np.eye(3) + 0.5 * skew(p)
    J = np.zeros((6, 6))
    J[:3, :3], J[3:, 3:], J[:3, 3:] = A, A, Cm @ A
    return J


def difference_jacobian(M, q_ref, q):
    """d (q (-) q_ref) / d dq with q (+) dq: the identity but for the 6 x 6 Jlog6 of the base"""
    J = np.eye(M["nv"])
    if M.get("floating"):
        R0, R1 = RBD.quat_to_R(*q_ref[3:7]), RBD.quat_to_R(*q[3:7])
        J[:6, :6] = jlog6(R0.T @ R1, R0.T @ (q[:3] - q_ref[:3]))
    return J


def reference_gradients(model, M, cost, tables, dt, q, v, u=None, first_step=0, terminal=False):
    """One sample: q [steps (+ 1)][nq], v, u [steps][nu] or None.  Returns (lx [steps (+ 1)][2 nv], lu [steps][nu]); a non-finite entry in what a
    slice reads makes that slice's lx and lu NaN"""
    nv, nu = model.nv, model.nu
    steps = len(q) - (1 if terminal else 0)
    q_tab, v_tab = tables
    W = lambda name, n: np.array(getattr(cost, name)[:n])      # noqa: E731
    lx, lu = np.zeros((len(q), 2 * nv)), np.zeros((steps, nu))
    for k in range(len(q)):
        term = k == steps
        read = [q[k], v[k]] + ([u[k]] if (u is not None and not term) else [])
        if not all(np.isfinite(x).all() for x in read):
            lx[k] = np.nan
            if not term:
                lu[k] = np.nan
            continue
        s = 1.0 if term else dt
        e = RBD.difference(M, q_tab[first_step + k], q[k])
        J = difference_jacobian(M, q_tab[first_step + k], q[k])
        lx[k, :nv] = s * (J.T @ (W("qf_weight" if term else "q_weight", nv) * e))
        lx[k, nv:] = s * (W("vf_weight" if term else "v_weight", nv) * (v[k] - v_tab[first_step + k]))
        if not term and u is not None:
            lu[k] = dt * (W("u_weight", nu) * (u[k] - W("u_ref", nu)))
    return lx, lu


def reference_gradients_batch(model, M, cost, tables, dt, q, v, u=None, first_step=0, terminal=False):
    n = q.shape[1]
    one = [reference_gradients(model, M, cost, tables, dt, q[:, i], v[:, i], None if u is None else u[:, i], first_step, terminal) for i in range(n)]
    return np.stack([o[0] for o in one], axis=1), np.stack([o[1] for o in one], axis=1)


def reference_step_torques(u, k, alpha):
    """u [steps][n][nu] + alpha [n] k, u itself where alpha is 0"""
    a = np.asarray(alpha)[None, :, None]
    with np.errstate(invalid="ignore"):
        return np.where(a == 0.0, u, u + a * k)


def reference_accept(state, consts):
    """the rules of idocp_rbd_ilqr_accept on a state {field: array}; returns the new state"""
    s = {k: (None if x is None else np.array(x)) for k, x in state.items()}
    n = len(s["cost"])
    pen, arm, shrink, amin = (consts[k] for k in ("penalty", "armijo", "shrink", "alpha_min"))
    accepted = np.zeros(n, dtype=bool)
    for i in range(n):
        if s["done"][i] != 0:
            continue
        al, (e0, e1) = s["alpha"][i], s["expected"][i]
        merit, trial = s["cost"][i] + pen * s["violation"][i], s["trial_cost"][i] + pen * s["trial_violation"][i]
        with np.errstate(invalid="ignore"):
            ok = bool(np.isfinite(s["trial_cost"][i]) and np.isfinite(s["trial_violation"][i]) and trial <= merit + arm * (al * e0 + (al * al) * e1))
        accepted[i] = ok
        if ok:
            s["cost"][i], s["violation"][i], s["done"][i], s["alpha_accepted"][i] = s["trial_cost"][i], s["trial_violation"][i], 1, al
        else:
            nxt = al * shrink
            s["alpha"][i] = 0.0 if nxt < amin else nxt
    for cur, tri in (("q_traj", "trial_q"), ("v_traj", "trial_v"), ("u_traj", "trial_u"), ("a_traj", "trial_a"), ("f_traj", "trial_f")):
        if s.get(cur) is not None and s.get(tri) is not None:
            sel = accepted.reshape((1, n) + (1,) * (s[cur].ndim - 2))
            s[cur] = np.where(sel, s[tri], s[cur])
    return s


def distance(x, ref):
    """rbd_lqr.distance: the largest deviation relative to max(1, |ref|_inf) of the block"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    return float(np.abs(x - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


# ------------------------------------------------------------------ one iteration

def ilqr_struct(arrays, consts, trials):
    io = capi.RbdIlqrIO()
    for k, x in arrays.items():
        if x is not None:
            setattr(io, k, x.ctypes.data if isinstance(x, np.ndarray) else x)
    for k in capi.RbdIlqrIO.CONSTANTS:
        setattr(io, k, float(consts[k]))
    io.trials = int(trials)
    return io


def iterate_raw(r, o, n, steps, active, time_step, dt, pts, io, impulse=False, device=False):
    fn = r.lib.idocp_rbd_ilqr_iterate_device if device else r.lib.idocp_rbd_ilqr_iterate
    flat = F._act(np.asarray(active).reshape(-1)) if active is not None else None
    p = pts.ctypes.data if isinstance(pts, np.ndarray) else pts
    return fn(r.h, o.h if isinstance(o, RS.Objective) else o, n, steps, flat, time_step, dt, p, C.byref(io) if io is not None else None, int(impulse))


def iterate(r, o, traj, consts, trials, active=None, time_step=0.0, dt=0.0, pts=None, u_min=None, u_max=None):
    """host form on a trajectory {q_traj, v_traj, u_traj, a_traj, f_traj, cost, violation}; returns (the new trajectory, {alpha_accepted, lqr_status,
    expected}); the inputs are left unchanged"""
    t = {k: (None if x is None else np.ascontiguousarray(x, dtype=np.float64).copy()) for k, x in traj.items()}
    steps, n = t["u_traj"].shape[:2]
    out = {"alpha_accepted": np.full(n, -777.0), "lqr_status": np.full(n, -7, dtype=np.int32), "expected": np.full((n, 2), -777.0)}
    keep = {"u_min": None if u_min is None else np.ascontiguousarray(u_min, dtype=np.float64), "u_max": None if u_max is None else np.ascontiguousarray(u_max, dtype=np.float64)}
    pts = None if pts is None else np.ascontiguousarray(pts, dtype=np.float64)
    io = ilqr_struct({**t, **out, **keep}, consts, trials)
    capi.check(iterate_raw(r, o, n, steps, active, time_step, dt, pts, io), "idocp_rbd_ilqr_iterate")
    return t, out
