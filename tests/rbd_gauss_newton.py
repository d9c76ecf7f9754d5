"""Shared by test_rbd_gauss_newton_host.py / test_rbd_gauss_newton_gpu.py / test_rbd_lqr_gn_gpu.py / test_rbd_ilqr_gn_gpu.py: the calls
idocp_rbd_linearize_rollout_cost, idocp_rbd_lqr_backward_gn and idocp_rbd_ilqr_iterate_gn of the idocp_rbd_* handle (include/idocp_hip.h) on numpy
arrays, and their numpy referees, written from the definitions of the header:

  rows           rho and G of one slice from the blocks of rbd_fd_derivatives.reference (refined dense solves), s = sqrt(dt w)
  gradients      rbd_gradients.reference_gradients for the diagonal terms plus Gx^T rho, Gu^T rho
  backward pass  the recursion of rbd_lqr.referee with G^T G in the stage Hessian, float64 or long double with a refined Quu solve
  dense KKT      rbd_lqr.dense_kkt with the dense stage Hessian inserted: no Riccati formula
A plain module: the CPU test imports it too.  Matrices are [row, column] on this side."""
import ctypes as C

import numpy as np

import rbd_fd_derivatives as D
import rbd_forward as F
import rbd_gradients as GR
import rbd_lqr as L
import rbd_score as RS
from idocp_amd import capi

OUTPUTS = capi.RbdCostLinearizationIO.OUTPUTS


def residual_rows(nv, ncontacts):
    return (nv + 3 * ncontacts + 3) // 4 * 4


def contacts_of(m, M):
    return m.ncontacts if M.get("floating") else 0


def scales(m, M, cost, dt):
    """s [R] = sqrt(dt w): the accelerations, the contact forces, zero on the padding"""
    nv, nc = m.nv, contacts_of(m, M)
    s = np.zeros(residual_rows(nv, nc))
    s[:nv] = np.sqrt(dt * np.array(cost.a_weight[:nv]))
    for c in range(nc):
        s[nv + 3 * c:nv + 3 * c + 3] = np.sqrt(dt * np.array(cost.f_weight[c][:]))
    return s


# ------------------------------------------------------------------ the calls

def linearize_cost_raw(r, o, n, steps, active, time_step, dt, u, pts, q_traj, v_traj, io, impulse, device=False):
    fn = r.lib.idocp_rbd_linearize_rollout_cost_device if device else r.lib.idocp_rbd_linearize_rollout_cost
    flat = F._act(np.asarray(active).reshape(-1)) if active is not None else None
    ptr = lambda x: (x.ctypes.data if isinstance(x, np.ndarray) else x) if x is not None else None      # noqa: E731
    return fn(r.h, o.h if isinstance(o, RS.Objective) else o, n, steps, flat, time_step, dt, ptr(u), ptr(pts), ptr(q_traj), ptr(v_traj),
              C.byref(io) if io is not None else None, int(impulse))


def cost_struct(**arrays):
    io = capi.RbdCostLinearizationIO()
    for k, x in arrays.items():
        if x is not None:
            setattr(io, k, x.ctypes.data if isinstance(x, np.ndarray) else x)
    return io


def output_shapes(m, M, steps, n):
    nv, nu = m.nv, m.nu
    nx, R = 2 * nv, residual_rows(nv, contacts_of(m, M))
    return {"A_traj": (steps, n, nx, nx), "B_traj": (steps, n, nu, nx), "G_traj": (steps, n, R, nx + nu), "rho_traj": (steps, n, R),
            "lx_traj": (steps + 1, n, nx), "lu_traj": (steps, n, nu)}


def linearize_cost(r, M, o, q_traj, v_traj, u, active=None, time_step=0.0, dt=0.0, pts=None, impulse=False, want=OUTPUTS, device=False):
    """returns {name: array} of the outputs asked for; A_traj, B_traj turned to [row, column]"""
    c = lambda x: np.ascontiguousarray(x, dtype=np.float64) if x is not None else None      # noqa: E731
    q_traj, v_traj, u, pts = c(q_traj), c(v_traj), c(u), c(pts)
    steps, n = q_traj.shape[0] - 1, q_traj.shape[1]
    sh = output_shapes(r.m, M, steps, n)
    out = {k: np.full(sh[k], -777.0) for k in want}
    if not device:
        capi.check(linearize_cost_raw(r, o, n, steps, active, time_step, dt, u, pts, q_traj, v_traj, cost_struct(**out), impulse), "idocp_rbd_linearize_rollout_cost")
    else:
        from rbd_batch import DeviceArray
        dev = {k: DeviceArray(x) for k, x in dict(u=u, pts=pts, q=q_traj, v=v_traj, **out).items() if x is not None}
        p = lambda k: dev[k].ptr.value if k in dev else None      # noqa: E731
        capi.check(linearize_cost_raw(r, o, n, steps, active, time_step, dt, p("u"), p("pts"), p("q"), p("v"), cost_struct(**{k: p(k) for k in out}), impulse, True),
                   "idocp_rbd_linearize_rollout_cost_device")
        capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
        out = {k: dev[k].numpy() for k in out}
        for d in dev.values():
            d.free()
    for k in ("A_traj", "B_traj"):
        if k in out:
            out[k] = out[k].transpose(0, 1, 3, 2).copy()
    return out


def backward_gn_raw(r, n, steps, io, g_rows, G_traj, device=False):
    fn = r.lib.idocp_rbd_lqr_backward_gn_device if device else r.lib.idocp_rbd_lqr_backward_gn
    g = (G_traj.ctypes.data if isinstance(G_traj, np.ndarray) else G_traj) if G_traj is not None else None
    return fn(r.h, n, steps, C.byref(io) if io is not None else None, int(g_rows), g)


def backward_gn(r, A, B, wx, wu, wxf, lx=None, lu=None, reg=0.0, G_traj=None, outputs=None, device=False):
    """rbd_lqr.backward with G_traj [steps][n][g_rows][nx + nu] (None: g_rows = 0)"""
    steps, n, nx, nu = np.asarray(B).shape
    if outputs is None:
        outputs = L.OUTPUTS if lx is not None else ("K_traj", "P0", "p0", "status")
    keep = L._inputs(A, B, wx, wu, wxf, lx, lu)
    Gt = None if G_traj is None else np.ascontiguousarray(G_traj, dtype=np.float64)
    g_rows = 0 if Gt is None else Gt.shape[2]
    sh = L.shapes(nx, nu, steps, n)
    out = {name: (np.full(sh[name], -7, dtype=np.int32) if name == "status" else np.full(sh[name], -777.0)) for name in outputs}
    if not device:
        capi.check(backward_gn_raw(r, n, steps, L.struct({**keep, **out}, reg), g_rows, Gt), "idocp_rbd_lqr_backward_gn")
        return L._turn(out)
    from rbd_batch import DeviceArray
    dev = {name: DeviceArray(x) for name, x in keep.items() if x is not None}
    for name, x in out.items():
        dev[name] = DeviceArray(np.zeros((n + 1) // 2) if name == "status" else x)
    dG = DeviceArray(Gt) if Gt is not None else None
    capi.check(backward_gn_raw(r, n, steps, L.struct({name: d.ptr.value for name, d in dev.items()}, reg), g_rows, dG.ptr.value if dG else None, True),
               "idocp_rbd_lqr_backward_gn_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    for name in out:
        out[name] = dev[name].numpy().view(np.int32)[:n].copy() if name == "status" else dev[name].numpy()
    for d in list(dev.values()) + ([dG] if dG else []):
        d.free()
    return L._turn(out)


def iterate_gn_raw(r, o, n, steps, active, time_step, dt, pts, io, impulse=False, device=False):
    fn = r.lib.idocp_rbd_ilqr_iterate_gn_device if device else r.lib.idocp_rbd_ilqr_iterate_gn
    flat = F._act(np.asarray(active).reshape(-1)) if active is not None else None
    p = pts.ctypes.data if isinstance(pts, np.ndarray) else pts
    return fn(r.h, o.h if isinstance(o, RS.Objective) else o, n, steps, flat, time_step, dt, p, C.byref(io) if io is not None else None, int(impulse))


def iterate_gn(r, o, traj, consts, trials, active=None, time_step=0.0, dt=0.0, pts=None, impulse=False):
    """rbd_gradients.iterate on idocp_rbd_ilqr_iterate_gn"""
    t = {k: (None if x is None else np.ascontiguousarray(x, dtype=np.float64).copy()) for k, x in traj.items()}
    steps, n = t["u_traj"].shape[:2]
    out = {"alpha_accepted": np.full(n, -777.0), "lqr_status": np.full(n, -7, dtype=np.int32), "expected": np.full((n, 2), -777.0)}
    pts = None if pts is None else np.ascontiguousarray(pts, dtype=np.float64)
    io = GR.ilqr_struct({**t, **out}, consts, trials)
    capi.check(iterate_gn_raw(r, o, n, steps, active, time_step, dt, pts, io, impulse), "idocp_rbd_ilqr_iterate_gn")
    return t, out


# ------------------------------------------------------------------ the numpy referees

def reference_rows(m, M, cost, dt, q, v, u, mask=None, pts=None, time_step=None, refine=True):
    """ONE sample, ONE slice: (rho [R], G [R][nz]) from the definitions of the header; NaN throughout where an input is not finite"""
    nv, nu, nc = m.nv, m.nu, contacts_of(m, M)
    R, nz = residual_rows(nv, nc), 2 * nv + nu
    read = [q, v, u] + ([pts] if pts is not None else [])
    if not all(np.isfinite(np.asarray(x)).all() for x in read):
        return np.full(R, np.nan), np.full((R, nz), np.nan)
    mask = [int(x) for x in mask] if nc else []
    d = D.reference(M, q, v, u, mask, pts, time_step, dt, refine=refine)
    s = scales(m, M, cost, dt)
    rho, Gm = np.zeros(R), np.zeros((R, nz))
    rho[:nv] = s[:nv] * d["a"]
    Gm[:nv] = s[:nv, None] * np.hstack([d["da_dq"], d["da_dv"], d["da_du"]])
    for c in range(nc):
        if mask[c]:
            rows = slice(nv + 3 * c, nv + 3 * c + 3)
            rho[rows] = s[rows] * (np.asarray(d["f"])[c] - np.array(cost.f_ref[c][:]))
            Gm[rows] = s[rows, None] * np.hstack([d["df_dq"][3 * c:3 * c + 3], d["df_dv"][3 * c:3 * c + 3], d["df_du"][3 * c:3 * c + 3]])
    return rho, Gm


def reference_cost_linearization(m, M, cost, tables, dt, q, v, u, active=None, pts=None, time_step=None, refine=True):
    """ONE sample: q [steps + 1][nq], v, u [steps][nu], active [steps][nc], pts [steps][nc][3].  Returns {rho_traj, G_traj, lx_traj, lu_traj}"""
    steps, nx = len(u), 2 * m.nv
    lx, lu = GR.reference_gradients(m, M, cost, tables, dt, q, v, u, terminal=True)
    rho, Gt = [], []
    for k in range(steps):
        rk, Gk = reference_rows(m, M, cost, dt, q[k], v[k], u[k], None if active is None else active[k], None if pts is None else pts[k], time_step, refine)
        rho.append(rk)
        Gt.append(Gk)
        lx[k] = lx[k] + Gk[:, :nx].T @ rk
        lu[k] = lu[k] + Gk[:, nx:].T @ rk
    return {"rho_traj": np.array(rho), "G_traj": np.array(Gt), "lx_traj": lx, "lu_traj": lu}


def reference_cost_linearization_batch(m, M, cost, tables, dt, q, v, u, active=None, pts=None, time_step=None, refine=True):
    n = q.shape[1]
    one = [reference_cost_linearization(m, M, cost, tables, dt, q[:, i], v[:, i], u[:, i], active, None if pts is None else pts[:, i], time_step, refine)
           for i in range(n)]
    return {k: np.stack([o[k] for o in one], axis=1) for k in one[0]}


def referee_gn(A, B, wx, wu, wxf, lx=None, lu=None, reg=0.0, Gt=None, refined=False):
    """ONE sample: the recursion of rbd_lqr.referee with Qxx += Gx^T Gx, Qux += Gu^T Gx, Quu += Gu^T Gu; Gt [steps][rows][nx + nu] or None"""
    T = np.longdouble if refined else np.float64
    A, B = np.asarray(A, dtype=T), np.asarray(B, dtype=T)
    steps, nx, nu = B.shape
    Gt = np.zeros((steps, 0, nx + nu), dtype=T) if Gt is None else np.asarray(Gt, dtype=T)
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
        Qxx, Qux, Quu = Wx + A[k].T @ PA + Gx.T @ Gx, B[k].T @ PA + Gu.T @ Gx, Wu + B[k].T @ (P @ B[k]) + Gu.T @ Gu
        rhs = np.hstack([Qux, Qu[:, None]])
        sol = L._solve_refined(Quu, rhs) if refined else np.linalg.solve(Quu, rhs)
        K[k], kf[k] = -sol[:, :nx], -sol[:, nx]
        X = Qxx + Qux.T @ K[k]
        P = (X + X.T) / 2
        p = Qx + Qux.T @ kf[k]
        e += np.array([kf[k] @ Qu, kf[k] @ Quu @ kf[k] / 2])
    f = lambda x: np.asarray(x, dtype=np.float64)      # noqa: E731
    return {"K_traj": f(K), "k_traj": f(kf), "P0": f(P), "p0": f(p), "expected": f(e)}


def referee_gn_batch(c, reg=0.0, refined=False):
    """referee_gn on every sample of a case {A, B, wx, wu, wxf, lx, lu, G}; arrays shaped like backward_gn()'s return"""
    steps, n = c["B"].shape[:2]
    one = [referee_gn(c["A"][:, i], c["B"][:, i], c["wx"], c["wu"], c["wxf"], None if c["lx"] is None else c["lx"][:, i],
                      None if c["lu"] is None else c["lu"][:, i], reg, None if c.get("G") is None else c["G"][:, i], refined) for i in range(n)]
    return {"K_traj": np.stack([o["K_traj"] for o in one], axis=1), "k_traj": np.stack([o["k_traj"] for o in one], axis=1),
            "P0": np.stack([o["P0"] for o in one]), "p0": np.stack([o["p0"] for o in one]), "expected": np.stack([o["expected"] for o in one])}


def random_case_gn(rng, nx, nu, steps, n, g_rows, g_scale=0.1):
    """rbd_lqr.random_case and G = g_scale N(0, 1) [steps][n][g_rows][nx + nu]: the scale of B"""
    c = L.random_case(rng, nx, nu, steps, n)
    c["G"] = g_scale * rng.normal(size=(steps, n, g_rows, nx + nu))
    return c


def dense_kkt_gn(A, B, wx, wu, wxf, lx, lu, reg, Gt, x0):
    """ONE sample, no Riccati formula: rbd_lqr.dense_kkt with the stage cost gaining |Gx_k x_k + Gu_k u_k|^2 / 2 -- the dense stage Hessian over
    (x_k, u_k), x_0 given.  Returns (du [steps][nu], the optimal cost)."""
    steps, nx, nu = np.asarray(B).shape
    nU, nX = steps * nu, steps * nx
    H, g = np.zeros((nU + nX, nU + nX)), np.zeros(nU + nX)
    Cm, d = np.zeros((nX, nU + nX)), np.zeros(nX)
    const = 0.5 * x0 @ (np.asarray(wx) * x0) + lx[0] @ x0
    for k in range(steps):
        iu, ix = slice(k * nu, (k + 1) * nu), slice(nU + k * nx, nU + (k + 1) * nx)      # u_k, x_(k+1)
        Gx, Gu = Gt[k][:, :nx], Gt[k][:, nx:]
        H[iu, iu] += np.diag(np.asarray(wu) + reg) + Gu.T @ Gu
        g[iu] += lu[k]
        H[ix, ix] += np.diag(wx if k + 1 < steps else wxf)
        g[ix] += lx[k + 1]
        if k == 0:
            g[iu] += Gu.T @ (Gx @ x0)
            const += 0.5 * (Gx @ x0) @ (Gx @ x0)
        else:
            ixk = slice(nU + (k - 1) * nx, nU + k * nx)                                  # x_k
            H[ixk, ixk] += Gx.T @ Gx
            H[iu, ixk] += Gu.T @ Gx
            H[ixk, iu] += Gx.T @ Gu
        Cm[k * nx:(k + 1) * nx, ix] = np.eye(nx)
        Cm[k * nx:(k + 1) * nx, iu] = -B[k]
        if k == 0:
            d[:nx] = A[0] @ x0
        else:
            Cm[k * nx:(k + 1) * nx, nU + (k - 1) * nx:nU + k * nx] = -A[k]
    KKT = np.block([[H, Cm.T], [Cm, np.zeros((nX, nX))]])
    z = L.G.solve_refined(KKT, np.concatenate([-g, d]))[0][:nU + nX]
    return z[:nU].reshape(steps, nu), float(0.5 * z @ H @ z + g @ z + const)
