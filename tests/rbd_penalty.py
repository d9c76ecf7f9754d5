"""Shared by test_rbd_penalty_host.py / test_rbd_penalty_gpu.py / test_rbd_lqr_gn_diag_gpu.py / test_rbd_ilqr_penalty_gpu.py: the calls
idocp_rbd_score_penalty, idocp_rbd_linearize_rollout_penalty, idocp_rbd_lqr_backward_gn_diag and idocp_rbd_ilqr_iterate_penalty of the idocp_rbd_*
handle (include/idocp_hip.h) on numpy arrays, and their numpy referee, written from the definition in the header:

  rows      sigma, Gc, D and the diagonal gradient of one slice from the forward solution and the blocks of rbd_fd_derivatives.reference; a lower /
            upper pair is ONE signed row b = max(0, x - hi) - max(0, lo - x), a row is active iff g > 0
  merit     rbd_gauss_newton.reference_cost_linearization for the cost plus Gc^T sigma plus the diagonal terms
  backward  rbd_gauss_newton.referee_gn with diag(D_k) added to the stage Hessian
A plain module: the CPU test imports it too."""
import ctypes as C
import math

import numpy as np

import rbd_fd_derivatives as D
import rbd_forward as F
import rbd_gauss_newton as GN
import rbd_gradients as GR
import rbd_lqr as L
import rbd_score as RS
from idocp_amd import capi

OUTPUTS = capi.RbdPenaltyLinearizationIO.OUTPUTS


def cone_count(cons):
    return 0 if cons is None else (5 if cons.linearized_friction_cone else (2 if cons.friction_cone else 0))


def constraint_rows(m, M, cons):
    """Rc = roundup4(nu + ncone ncontacts); 0 without constraints"""
    if cons is None:
        return 0
    return (m.nu + cone_count(cons) * GN.contacts_of(m, M) + 3) // 4 * 4


# ------------------------------------------------------------------ the calls

def _ptr(x):
    return (x.ctypes.data if isinstance(x, np.ndarray) else x) if x is not None else None


def score_penalty_raw(r, o, n, first_step, steps, active, accumulate, q, v, u, a, f, sq, device=False):
    fn = r.lib.idocp_rbd_score_penalty_device if device else r.lib.idocp_rbd_score_penalty
    flat = F._act(np.asarray(active).reshape(-1)) if active is not None else None
    return fn(r.h, o.h if isinstance(o, RS.Objective) else o, n, first_step, steps, flat, int(accumulate), _ptr(q), _ptr(v), _ptr(u), _ptr(a), _ptr(f), _ptr(sq))


def score_penalty(r, o, q, v, u=None, a=None, f=None, active=None, first_step=0, accumulate=None):
    """host form on the window's slices [steps][n][..]; accumulate: the array the call adds to (left unchanged)"""
    c = lambda x: np.ascontiguousarray(x, dtype=np.float64) if x is not None else None      # noqa: E731
    q, v, u, a, f = c(q), c(v), c(u), c(a), c(f)
    steps, n = q.shape[:2]
    sq = np.array(accumulate, dtype=np.float64) if accumulate is not None else np.full(n, -777.0)
    capi.check(score_penalty_raw(r, o, n, first_step, steps, active, accumulate is not None, q, v, u, a, f, sq), "idocp_rbd_score_penalty")
    return sq


def penalty_struct(**arrays):
    io = capi.RbdPenaltyLinearizationIO()
    for k, x in arrays.items():
        if x is not None:
            setattr(io, k, _ptr(x))
    return io


def output_shapes(m, M, cons, steps, n):
    sh = GN.output_shapes(m, M, steps, n)
    R, nz = sh["G_traj"][2] + constraint_rows(m, M, cons), 2 * m.nv + m.nu
    sh["G_traj"], sh["rho_traj"], sh["D_traj"] = (steps, n, R, nz), (steps, n, R), (steps, n, nz)
    return sh


def linearize_penalty_raw(r, o, n, steps, active, time_step, dt, u, pts, q_traj, v_traj, io, mu, impulse, device=False):
    fn = r.lib.idocp_rbd_linearize_rollout_penalty_device if device else r.lib.idocp_rbd_linearize_rollout_penalty
    flat = F._act(np.asarray(active).reshape(-1)) if active is not None else None
    return fn(r.h, o.h if isinstance(o, RS.Objective) else o, n, steps, flat, time_step, dt, _ptr(u), _ptr(pts), _ptr(q_traj), _ptr(v_traj),
              C.byref(io) if io is not None else None, float(mu), int(impulse))


def linearize_penalty(r, M, cons, o, mu, q_traj, v_traj, u, active=None, time_step=0.0, dt=0.0, pts=None, impulse=False, want=OUTPUTS, device=False):
    """returns {name: array} of the outputs asked for; A_traj, B_traj turned to [row, column]"""
    c = lambda x: np.ascontiguousarray(x, dtype=np.float64) if x is not None else None      # noqa: E731
    q_traj, v_traj, u, pts = c(q_traj), c(v_traj), c(u), c(pts)
    steps, n = q_traj.shape[0] - 1, q_traj.shape[1]
    sh = output_shapes(r.m, M, cons, steps, n)
    out = {k: np.full(sh[k], -777.0) for k in want}
    if not device:
        capi.check(linearize_penalty_raw(r, o, n, steps, active, time_step, dt, u, pts, q_traj, v_traj, penalty_struct(**out), mu, impulse),
                   "idocp_rbd_linearize_rollout_penalty")
    else:
        from rbd_batch import DeviceArray
        dev = {k: DeviceArray(x) for k, x in dict(u=u, pts=pts, q=q_traj, v=v_traj, **out).items() if x is not None}
        p = lambda k: dev[k].ptr.value if k in dev else None      # noqa: E731
        capi.check(linearize_penalty_raw(r, o, n, steps, active, time_step, dt, p("u"), p("pts"), p("q"), p("v"), penalty_struct(**{k: p(k) for k in out}), mu,
                                         impulse, True), "idocp_rbd_linearize_rollout_penalty_device")
        capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
        out = {k: dev[k].numpy() for k in out}
        for d in dev.values():
            d.free()
    for k in ("A_traj", "B_traj"):
        if k in out:
            out[k] = out[k].transpose(0, 1, 3, 2).copy()
    return out


def backward_gn_diag_raw(r, n, steps, io, g_rows, G_traj, D_traj, device=False):
    fn = r.lib.idocp_rbd_lqr_backward_gn_diag_device if device else r.lib.idocp_rbd_lqr_backward_gn_diag
    return fn(r.h, n, steps, C.byref(io) if io is not None else None, int(g_rows), _ptr(G_traj), _ptr(D_traj))


def backward_gn_diag(r, A, B, wx, wu, wxf, lx=None, lu=None, reg=0.0, G_traj=None, D_traj=None, outputs=None):
    """rbd_gauss_newton.backward_gn with D_traj [steps][n][nx + nu] (None: NULL), host form"""
    steps, n, nx, nu = np.asarray(B).shape
    if outputs is None:
        outputs = L.OUTPUTS if lx is not None else ("K_traj", "P0", "p0", "status")
    keep = L._inputs(A, B, wx, wu, wxf, lx, lu)
    Gt = None if G_traj is None else np.ascontiguousarray(G_traj, dtype=np.float64)
    Dt = None if D_traj is None else np.ascontiguousarray(D_traj, dtype=np.float64)
    sh = L.shapes(nx, nu, steps, n)
    out = {name: (np.full(sh[name], -7, dtype=np.int32) if name == "status" else np.full(sh[name], -777.0)) for name in outputs}
    capi.check(backward_gn_diag_raw(r, n, steps, L.struct({**keep, **out}, reg), 0 if Gt is None else Gt.shape[2], Gt, Dt), "idocp_rbd_lqr_backward_gn_diag")
    return L._turn(out)


def iterate_penalty_raw(r, o, n, steps, active, time_step, dt, pts, io, impulse=False, device=False):
    fn = r.lib.idocp_rbd_ilqr_iterate_penalty_device if device else r.lib.idocp_rbd_ilqr_iterate_penalty
    flat = F._act(np.asarray(active).reshape(-1)) if active is not None else None
    return fn(r.h, o.h if isinstance(o, RS.Objective) else o, n, steps, flat, time_step, dt, _ptr(pts), C.byref(io) if io is not None else None, int(impulse))


def iterate_penalty(r, o, traj, consts, trials, active=None, time_step=0.0, dt=0.0, pts=None, impulse=False):
    """rbd_gradients.iterate on idocp_rbd_ilqr_iterate_penalty: `violation` of traj holds sq_violation, consts["penalty"] is mu"""
    t = {k: (None if x is None else np.ascontiguousarray(x, dtype=np.float64).copy()) for k, x in traj.items()}
    steps, n = t["u_traj"].shape[:2]
    out = {"alpha_accepted": np.full(n, -777.0), "lqr_status": np.full(n, -7, dtype=np.int32), "expected": np.full((n, 2), -777.0)}
    pts = None if pts is None else np.ascontiguousarray(pts, dtype=np.float64)
    io = GR.ilqr_struct({**t, **out}, consts, trials)
    capi.check(iterate_penalty_raw(r, o, n, steps, active, time_step, dt, pts, io, impulse), "idocp_rbd_ilqr_iterate_penalty")
    return t, out


# ------------------------------------------------------------------ the numpy referee

def signed_box(x, lo, hi, lower=True, upper=True):
    return (max(0.0, x - hi) if upper else 0.0) - (max(0.0, lo - x) if lower else 0.0)


def cone_gradients(cons, f):
    """[(g, dg/df)] of the cone rows of one contact"""
    fx, fy, fz = (float(x) for x in f)
    if cons.linearized_friction_cone:
        mm = cons.mu / math.sqrt(2.0)
        Jc = np.array([[0, 0, -1], [1, 0, -mm], [-1, 0, -mm], [0, 1, -mm], [0, -1, -mm]], dtype=np.float64)
        return [(float(Jc[i] @ np.array([fx, fy, fz])), Jc[i]) for i in range(5)]
    m2 = cons.mu * cons.mu
    return [(-fz, np.array([0.0, 0.0, -1.0])), (fx * fx + fy * fy - m2 * fz * fz, np.array([2 * fx, 2 * fy, -2 * m2 * fz]))]


def reference_penalty_rows(m, M, cons, mu, dt, q, v, u, mask=None, pts=None, time_step=None, refine=True, solution=None):
    """ONE sample, ONE slice: {sigma [Rc], Gc [Rc][nz], D [nz], gdiag [nz], h [every active row's g, a flat list], sq = dt 1/2 sum h^2}.
    solution: (a, f) and the blocks where the caller has them (else rbd_fd_derivatives.reference)"""
    nv, nu, nq, nc = m.nv, m.nu, m.nq, GN.contacts_of(m, M)
    Rc, nz, nx = constraint_rows(m, M, cons), 2 * m.nv + m.nu, 2 * m.nv
    out = {"sigma": np.zeros(Rc), "Gc": np.zeros((Rc, nz)), "D": np.zeros(nz), "gdiag": np.zeros(nz), "h": [], "sq": 0.0}
    if cons is None:
        return out
    read = [q, v, u] + ([pts] if pts is not None else [])
    if not all(np.isfinite(np.asarray(x)).all() for x in read):
        return {k: (np.full_like(x, np.nan) if isinstance(x, np.ndarray) else math.nan) for k, x in out.items()}
    mask = [int(x) for x in mask] if nc else []
    d = solution if solution is not None else D.reference(M, q, v, u, mask, pts, time_step, dt, refine=refine)
    s, h = math.sqrt(dt * mu), []
    lim = lambda name: np.array(getattr(m, name)[:nu])      # noqa: E731
    boxes = ((cons.joint_position_limits, np.asarray(q)[nq - nu:], lim("q_min"), lim("q_max"), nv - nu),
             (cons.joint_velocity_limits, np.asarray(v)[nv - nu:], -lim("v_max"), lim("v_max"), nv + nv - nu),
             (cons.joint_torque_limits, np.asarray(u), -lim("u_max"), lim("u_max"), nx))
    for on, x, lo, hi, col in boxes:
        for j in range(nu):
            if on:
                b = signed_box(x[j], lo[j], hi[j])
                out["D"][col + j] = dt * mu if b != 0 else 0.0
                out["gdiag"][col + j] = dt * mu * b
                h.append(abs(b))
    da = np.hstack([d["da_dq"], d["da_dv"], d["da_du"]])
    a = np.asarray(d["a"])
    for j in range(nu):
        b = signed_box(a[nv - nu + j], cons.a_min[j], cons.a_max[j], cons.joint_acceleration_lower_limit, cons.joint_acceleration_upper_limit)
        out["sigma"][j] = s * b
        out["Gc"][j] = s * da[nv - nu + j] if b != 0 else 0.0
        h.append(abs(b))
    ncone = cone_count(cons)
    if ncone and nc:
        df = np.hstack([d["df_dq"], d["df_dv"], d["df_du"]])
        for c in range(nc):
            if mask[c]:
                for i, (g, dg) in enumerate(cone_gradients(cons, np.asarray(d["f"])[c])):
                    row = nu + ncone * c + i
                    if g > 0:
                        out["sigma"][row] = s * g
                        out["Gc"][row] = s * (dg @ df[3 * c:3 * c + 3])
                        h.append(g)
    out["h"] = [x for x in h if x > 0]
    out["sq"] = dt * 0.5 * math.fsum(x * x for x in out["h"])
    return out


def reference_penalty_linearization(m, M, cost, cons, mu, tables, dt, q, v, u, active=None, pts=None, time_step=None, refine=True):
    """ONE sample: {rho_traj [steps][R + Rc], G_traj, D_traj, lx_traj, lu_traj, sq_violation} -- the cost rows of rbd_gauss_newton first"""
    steps, nx = len(u), 2 * m.nv
    ref = GN.reference_cost_linearization(m, M, cost, tables, dt, q, v, u, active, pts, time_step, refine)
    rho, Gt, Dt, sq = [], [], [], []
    for k in range(steps):
        p = reference_penalty_rows(m, M, cons, mu, dt, q[k], v[k], u[k], None if active is None else active[k], None if pts is None else pts[k], time_step, refine)
        rho.append(np.concatenate([ref["rho_traj"][k], p["sigma"]]))
        Gt.append(np.vstack([ref["G_traj"][k], p["Gc"]]))
        Dt.append(p["D"])
        sq.append(p["sq"])
        grad = p["Gc"].T @ p["sigma"] + p["gdiag"]
        ref["lx_traj"][k] = ref["lx_traj"][k] + grad[:nx]
        ref["lu_traj"][k] = ref["lu_traj"][k] + grad[nx:]
    return {"rho_traj": np.array(rho), "G_traj": np.array(Gt), "D_traj": np.array(Dt), "lx_traj": ref["lx_traj"], "lu_traj": ref["lu_traj"],
            "sq_violation": math.fsum(sq)}


def reference_penalty_linearization_batch(m, M, cost, cons, mu, tables, dt, q, v, u, active=None, pts=None, time_step=None, refine=True):
    n = q.shape[1]
    one = [reference_penalty_linearization(m, M, cost, cons, mu, tables, dt, q[:, i], v[:, i], u[:, i], active, None if pts is None else pts[:, i], time_step, refine)
           for i in range(n)]
    return {k: np.stack([np.asarray(o[k]) for o in one], axis=1 if np.ndim(one[0][k]) else 0) for k in one[0]}


def referee_gn_diag(A, B, wx, wu, wxf, lx, lu, reg, Gt, Dt, refined=False):
    """ONE sample: rbd_gauss_newton.referee_gn with diag(D_k) in the stage Hessian -- written out, not delegated: Qxx += diag(Dx), Quu += diag(Du)"""
    T = np.longdouble if refined else np.float64
    A, B, Gt, Dt = (np.asarray(x, dtype=T) for x in (A, B, Gt, Dt))
    steps, nx, nu = B.shape
    lx = np.zeros((steps + 1, nx), dtype=T) if lx is None else np.asarray(lx, dtype=T)
    lu = np.zeros((steps, nu), dtype=T) if lu is None else np.asarray(lu, dtype=T)
    Wx, Wu, P = np.diag(np.asarray(wx, dtype=T)), np.diag(np.asarray(wu, dtype=T) + T(reg)), np.diag(np.asarray(wxf, dtype=T))
    p = lx[steps].copy()
    K, kf = np.zeros((steps, nu, nx), dtype=T), np.zeros((steps, nu), dtype=T)
    e = np.zeros(2, dtype=T)
    for k in range(steps - 1, -1, -1):
        Gx, Gu = Gt[k][:, :nx], Gt[k][:, nx:]
        Qx, Qu = lx[k] + A[k].T @ p, lu[k] + B[k].T @ p
        PA = P @ A[k]
        Qxx = Wx + np.diag(Dt[k][:nx]) + A[k].T @ PA + Gx.T @ Gx
        Qux = B[k].T @ PA + Gu.T @ Gx
        Quu = Wu + np.diag(Dt[k][nx:]) + B[k].T @ (P @ B[k]) + Gu.T @ Gu
        rhs = np.hstack([Qux, Qu[:, None]])
        sol = L._solve_refined(Quu, rhs) if refined else np.linalg.solve(Quu, rhs)
        K[k], kf[k] = -sol[:, :nx], -sol[:, nx]
        X = Qxx + Qux.T @ K[k]
        P = (X + X.T) / 2
        p = Qx + Qux.T @ kf[k]
        e += np.array([kf[k] @ Qu, kf[k] @ Quu @ kf[k] / 2])
    f = lambda x: np.asarray(x, dtype=np.float64)      # noqa: E731
    return {"K_traj": f(K), "k_traj": f(kf), "P0": f(P), "p0": f(p), "expected": f(e)}


def referee_gn_diag_batch(c, Dt, reg=0.0, refined=False):
    steps, n = c["B"].shape[:2]
    one = [referee_gn_diag(c["A"][:, i], c["B"][:, i], c["wx"], c["wu"], c["wxf"], None if c["lx"] is None else c["lx"][:, i],
                           None if c["lu"] is None else c["lu"][:, i], reg, c["G"][:, i], Dt[:, i], refined) for i in range(n)]
    return {"K_traj": np.stack([o["K_traj"] for o in one], axis=1), "k_traj": np.stack([o["k_traj"] for o in one], axis=1),
            "P0": np.stack([o["P0"] for o in one]), "p0": np.stack([o["p0"] for o in one]), "expected": np.stack([o["expected"] for o in one])}
