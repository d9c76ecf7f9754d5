"""Shared by test_rbd_fd_derivatives_host.py / test_rbd_fd_derivatives_gpu.py: the derivative call of the idocp_rbd_* handle
(idocp_rbd_forward_dynamics_derivatives_batch; include/idocp_hip.h) on numpy arrays, and the numpy referee of its answers.

The referee shares no formula with the kernels.  It takes the forward solution (a, f) from rbd_forward.reference, the complex-step dID/d(q, v) and
dC/d(q, v) AT that solution from independent_rbd.terms / rbd_cases.impulse_rows, builds the dense K = [M J^T; J 0] over the active rows and solves
d[a; -f] = -K^-1 [dID; dC] with iterative refinement in np.longdouble (gen_golden_kkt.solve_refined); `refine=False` is the plain FP64 numpy
solve, the yardstick of the GPU bar.  The top rows of A come from the complex step on the group product itself: exp6(dt v)^-1 exp6(eps e_r)
exp6(dt v) and exp6(dt v)^-1 exp6(dt (v + eps e_r)) are I + eps X + O(eps^2), so the imaginary part of the 4 x 4 product IS the tangent, without a
logarithm or a closed-form Jacobian."""
import ctypes as C

import numpy as np

import independent_rbd as IR
import rbd_cases as RC
import rbd_forward as F
from idocp_amd import capi
from rbd_batch import IMPULSE, STAGE      # noqa: F401

G, RBD = IR.G, IR.RBD
FDD_OUTPUTS = capi.RbdFddIO.OUTPUTS
CONTACT_OUTPUTS = ("f", "df_dq", "df_dv", "df_du")
TORQUE_OUTPUTS = ("da_du", "df_du", "B")
H = 1e-30


def fdd_shapes(m):
    """per-sample shape of every output as numpy sees the column-major blocks: [column][row]"""
    nv, nu, nf = m.nv, m.nu, 3 * m.ncontacts
    return {"a": (nv,), "f": (m.ncontacts, 3), "da_dq": (nv, nv), "da_dv": (nv, nv), "da_du": (nu, nv), "df_dq": (nv, nf), "df_dv": (nv, nf),
            "df_du": (nu, nf), "A": (2 * nv, 2 * nv), "B": (nu, 2 * nv)}


def outputs_of(m, mode):
    out = FDD_OUTPUTS
    if not m.ncontacts:
        out = tuple(k for k in out if k not in CONTACT_OUTPUTS)
    if mode == IMPULSE:
        out = tuple(k for k in out if k not in TORQUE_OUTPUTS)
    return out


def derivatives_raw(r, mode, n, active, time_step, dt, io, device=False):
    fn = r.lib.idocp_rbd_forward_dynamics_derivatives_batch_device if device else r.lib.idocp_rbd_forward_dynamics_derivatives_batch
    return fn(r.h, mode, n, F._act(active), time_step, dt, C.byref(io) if io is not None else None)


def derivatives(r, mode, q, v, u=None, active=None, time_step=0.0, dt=0.0, contact_points=None, outputs=None, fill=np.nan):
    """host form; returns {name: array [n][...]} with the matrices turned to [row, column]"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    n = q.shape[0]
    keep = {"q": q, "v": np.ascontiguousarray(v, dtype=np.float64)}
    for name, x in (("u", u), ("contact_points", contact_points)):
        if x is not None:
            keep[name] = np.ascontiguousarray(x, dtype=np.float64)
    shapes = fdd_shapes(r.m)
    outputs = outputs_of(r.m, mode) if outputs is None else outputs
    out = {name: np.full((n,) + shapes[name], fill) for name in outputs}
    io = capi.RbdFddIO()
    for name, x in list(keep.items()) + list(out.items()):
        setattr(io, name, x.ctypes.data)
    capi.check(derivatives_raw(r, mode, n, active, time_step, dt, io), "idocp_rbd_forward_dynamics_derivatives_batch")
    return {name: (x.transpose(0, 2, 1).copy() if (x.ndim == 3 and name != "f") else x) for name, x in out.items()}


def set_chunk(r, max_samples):
    capi.check(r.lib.idocp_rbd_set_derivatives_chunk(r.h, int(max_samples)), "idocp_rbd_set_derivatives_chunk")


# ------------------------------------------------------------------ the numpy referee

def _hat(x):
    return np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]], dtype=complex)


def exp6(xi):
    """4 x 4 homogeneous matrix of exp6 of xi = (lin, ang), complex-safe (the angle is sqrt(w . w), not a norm)"""
    xi = np.asarray(xi, dtype=complex)
    w, K = xi[3:], _hat(xi[3:])
    t2 = w @ w
    t = np.sqrt(t2)
    if abs(t) < 1e-6:
        a, b, c = 1 - t2 / 6 + t2 * t2 / 120, 0.5 - t2 / 24 + t2 * t2 / 720, 1.0 / 6 - t2 / 120 + t2 * t2 / 5040
    else:
        a, b, c = np.sin(t) / t, (1 - np.cos(t)) / t2, (t - np.sin(t)) / (t2 * t)
    T = np.eye(4, dtype=complex)
    T[:3, :3] += a * K + b * K @ K
    T[:3, 3] = (np.eye(3) + b * K + c * K @ K) @ xi[:3]
    return T


def _vee(X):
    return np.array([X[0, 3], X[1, 3], X[2, 3], X[2, 1], X[0, 2], X[1, 0]]).imag / H


def retraction_blocks(vb, dt):
    """(d/dq, d/dv) of q (+) dt v on a free-flyer, 6 x 6 each, in the tangent at q_next (the factor dt of d/dv included)"""
    E = exp6(dt * np.asarray(vb))
    Ei = np.linalg.inv(E)
    Jq, Jv = np.zeros((6, 6)), np.zeros((6, 6))
    for r in range(6):
        e = np.zeros(6, complex)
        e[r] = 1j * H
        Jq[:, r] = _vee(Ei @ exp6(e) @ E)
        Jv[:, r] = _vee(Ei @ exp6(dt * (np.asarray(vb) + e)))
    return Jq, Jv


def baumgarte_jacobians(M, q, v, a, mask, pts, time_step):
    """(dC/dq, dC/dv) over the active rows: the complex step on the Baumgarte residual ITSELF (rbd_forward.contact_rows states it), not the
    reference's derivative formula (gen_golden_rbd.baumgarte), which differs from it in the term of w x v_lin"""
    act = np.array(mask, dtype=bool)
    Ma = dict(M)
    Ma["contacts"] = [c for c, on in zip(M["contacts"], act) if on]
    ref = np.asarray(pts, dtype=np.float64).reshape(-1, 3)[act]
    nv = M["nv"]

    def residual(fk):
        return np.concatenate([x["a"][:3] + np.cross(x["v"][3:], x["v"][:3]) + 2.0 / time_step * x["v"][:3] + (x["p"] - ref[c]) / time_step ** 2
                               for c, x in enumerate(fk)])

    dq = np.array([residual(RBD.frame_kinematics(Ma, q, v, a, dq_seed=F._step(nv, k))).imag / H for k in range(nv)]).T
    dv = np.array([residual(RBD.frame_kinematics(Ma, q, v + F._step(nv, k), a)).imag / H for k in range(nv)]).T
    return dq, dv


def _solve(K, R, refine):
    return G.solve_refined(K, R)[0] if refine else np.linalg.solve(K, R)


def reference(M, q, v, u, mask, pts=None, time_step=None, dt=0.0, impulse=False, refine=True):
    """every output of ONE sample, matrices as [row, column]; f [nc][3]; the contact blocks have 3 nc rows, zero where inactive.
    refine = "both": the pair (refined, plain FP64) from the same terms"""
    q, v = np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64)
    nv, nc = M["nv"], len(M["contacts"])
    nu = nv - 6 if M.get("floating") else nv
    mask = [int(x) for x in mask] if nc else []
    rows = np.repeat(np.array(mask, dtype=bool), 3)
    a, f = F.reference(M, q, v, u, mask, pts, time_step, impulse)
    dimf = int(rows.sum())
    if impulse:
        t = IR.terms(M, q, v, a, f, active=mask)
        dIDq, dIDv, Mm = t["dimp_dq"], np.zeros((nv, nv)), t["dimp_da"]
        ir = RC.impulse_rows(M, q, v + a, mask)
        dCq, dCv, J = ir["imp_dCdq"], ir["imp_J"], ir["imp_J"]
    else:
        t = IR.terms(M, q, v, a, f if nc else None, pts if dimf else None, time_step, active=mask if nc else None, impulse_forms=False)
        dIDq, dIDv, Mm = t["dtau_dq"], t["dtau_dv"], t["dtau_da"]
        if dimf:
            J = t["dCda"]
            dCq, dCv = baumgarte_jacobians(M, q, v, a, mask, pts, time_step)
        else:
            dCq = dCv = J = np.zeros((0, nv))
    K = np.block([[Mm, J.T], [J, np.zeros((dimf, dimf))]])
    St = np.zeros((nv + dimf, nu))
    St[nv - nu:nv] = np.eye(nu)
    R = np.block([[dIDq, dIDv], [dCq, dCv]])
    scale = 1.0 if impulse else dt
    top = np.hstack([np.eye(nv), np.zeros((nv, nv))])
    if not impulse:
        top[:, nv:] = dt * np.eye(nv)
        if M.get("floating"):
            top[:6, :6], top[:6, nv:nv + 6] = retraction_blocks(v[:6], dt)

    def assemble(refined):
        X, Xu = -_solve(K, R, refined), _solve(K, St, refined)
        out = {"a": a, "f": f, "da_dq": X[:nv, :nv], "da_dv": X[:nv, nv:], "da_du": Xu[:nv]}
        for name, blk in (("df_dq", -X[nv:, :nv]), ("df_dv", -X[nv:, nv:]), ("df_du", -Xu[nv:])):
            full = np.zeros((3 * nc, blk.shape[1]))
            full[rows] = blk
            out[name] = full
        out["A"] = np.vstack([top, np.hstack([scale * out["da_dq"], np.eye(nv) + scale * out["da_dv"]])])
        out["B"] = np.vstack([np.zeros((nv, nu)), scale * out["da_du"]])
        return out

    return (assemble(True), assemble(False)) if refine == "both" else assemble(refine)


def distance(x, ref):
    """largest deviation relative to max(1, |ref|_inf) of the block"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    return float(np.abs(x - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


# ------------------------------------------------------------------ the chunk plan, stated in Python (idocp_amd/csrc/rbd_fdd_plan.hpp)

CAP_DOUBLES = (256 << 20) // 8


def plan(nv, nf, n, limit=0, cap=CAP_DOUBLES):
    per = nv + nf + (0 if nf else nv) + 2 * nv * nv + 2 * nf * nv + (nv + nf) ** 2
    chunk = min(n, max(1, cap // per))
    if limit > 0:
        chunk = min(chunk, limit)
    return {"chunk": chunk, "nchunks": -(-n // chunk), "total": chunk * per}


# ------------------------------------------------------------------ the rollout linearisation

def linearize_raw(r, n, steps, active, time_step, dt, u, pts, q_traj, v_traj, A_traj, B_traj, impulse, device=False):
    fn = r.lib.idocp_rbd_linearize_rollout_device if device else r.lib.idocp_rbd_linearize_rollout
    flat = F._act(np.asarray(active).reshape(-1)) if active is not None else None
    ptr = lambda x: x.ctypes.data if x is not None else None      # noqa: E731
    return fn(r.h, n, steps, flat, time_step, dt, ptr(u), ptr(pts), ptr(q_traj), ptr(v_traj), ptr(A_traj), ptr(B_traj), int(impulse))


def linearize(r, q_traj, v_traj, u, active=None, time_step=0.0, dt=0.0, contact_points=None, impulse=False):
    """host form; returns (A_traj [steps][n][2 nv][2 nv], B_traj [steps][n][2 nv][nu]) as [row, column]"""
    u = np.ascontiguousarray(u, dtype=np.float64)
    steps, n = u.shape[:2]
    nx, nu = 2 * r.m.nv, r.m.nu
    A, B = np.full((steps, n, nx, nx), np.nan), np.full((steps, n, nu, nx), np.nan)
    pts = np.ascontiguousarray(contact_points, dtype=np.float64) if contact_points is not None else None
    capi.check(linearize_raw(r, n, steps, active, time_step, dt, u, pts, np.ascontiguousarray(q_traj), np.ascontiguousarray(v_traj), A, B, impulse),
               "idocp_rbd_linearize_rollout")
    return A.transpose(0, 1, 3, 2).copy(), B.transpose(0, 1, 3, 2).copy()
