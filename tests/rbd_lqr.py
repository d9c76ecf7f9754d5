"""Shared by test_rbd_lqr_host.py / test_rbd_lqr_gpu.py: the calls idocp_rbd_lqr_backward(_device) of the idocp_rbd_* handle (include/idocp_hip.h) on
numpy arrays, and the numpy referee of the recursion the header states:

    P = Wxf, p = lx[steps];   for k = steps - 1 .. 0:
      Qx = lx[k] + A^T p, Qu = lu[k] + B^T p, Qxx = Wx + A^T P A, Qux = B^T P A, Quu = Wu + reg I + B^T P B,
      K_k = -Quu^-1 Qux, k_k = -Quu^-1 Qu,  P <- (X + X^T) / 2 with X = Qxx + Qux^T K_k,  p <- Qx + Qux^T k_k

The referee has a plain float64 form and a form in np.longdouble whose Quu solve is iteratively refined (gen_golden_kkt.solve_refined).  A plain
module: the CPU test imports it too.  Matrices are [row, column] on this side; the calls take and give column-major blocks."""
import ctypes as C
import os
import sys

import numpy as np

from idocp_amd import capi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_golden_kkt as G      # noqa: E402

OUTPUTS = capi.RbdLqrIO.OUTPUTS
SAMPLES_PER_WORKGROUP = 1       # RBD_LQR_WAVES of idocp_amd/csrc/rbd_launch.hpp: one wavefront, one sample, per workgroup
FLOOR, FACTOR = 1e-11, 4.0      # the rule of the rbd calls (test_rbd_linearize_rollout_gpu.py)


def shapes(nx, nu, steps, n):
    """shape of every output as numpy sees the column-major blocks: [column][row]"""
    return {"K_traj": (steps, n, nx, nu), "k_traj": (steps, n, nu), "P0": (n, nx, nx), "p0": (n, nx), "expected": (n, 2), "status": (n,)}


def random_case(rng, nx, nu, steps, n, gradients=True):
    """the inputs of every random case: A = I + 0.1 N(0, 1), B = 0.1 N(0, 1), weights uniform in [0.5, 2], gradients N(0, 1)"""
    c = {"A": np.eye(nx) + 0.1 * rng.normal(size=(steps, n, nx, nx)), "B": 0.1 * rng.normal(size=(steps, n, nx, nu)),
         "wx": rng.uniform(0.5, 2.0, nx), "wu": rng.uniform(0.5, 2.0, nu), "wxf": rng.uniform(0.5, 2.0, nx), "lx": None, "lu": None}
    if gradients:
        c["lx"], c["lu"] = rng.normal(size=(steps + 1, n, nx)), rng.normal(size=(steps, n, nu))
    return c


def struct(arrays, reg):
    """idocp_rbd_lqr_io_t over a dict {field: pointer-or-array}; a field left out or None is NULL"""
    io = capi.RbdLqrIO()
    for name, x in arrays.items():
        if x is not None:
            setattr(io, name, x.ctypes.data if isinstance(x, np.ndarray) else x)
    io.regularization = float(reg)
    return io


def backward_raw(r, n, steps, io, device=False):
    fn = r.lib.idocp_rbd_lqr_backward_device if device else r.lib.idocp_rbd_lqr_backward
    return fn(r.h, n, steps, C.byref(io) if io is not None else None)


def _inputs(A, B, wx, wu, wxf, lx, lu):
    f = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)      # noqa: E731
    return {"A_traj": f(np.asarray(A).transpose(0, 1, 3, 2)), "B_traj": f(np.asarray(B).transpose(0, 1, 3, 2)), "x_weight": f(wx), "u_weight": f(wu),
            "xf_weight": f(wxf), "lx_traj": f(lx), "lu_traj": f(lu)}


def _turn(out):
    """the matrices to [row, column]"""
    res = dict(out)
    if "K_traj" in res:
        res["K_traj"] = res["K_traj"].transpose(0, 1, 3, 2).copy()
    if "P0" in res:
        res["P0"] = res["P0"].transpose(0, 2, 1).copy()
    return res


def backward(r, A, B, wx, wu, wxf, lx=None, lu=None, reg=0.0, outputs=None, device=False):
    """A [steps][n][nx][nx], B [steps][n][nx][nu] as [row, column]; returns {name: array}, K_traj [steps][n][nu][nx] and P0 [n][nx][nx] as
    [row, column].  outputs: default everything the gradients allow.  device: every array through device memory, the same return."""
    steps, n, nx, nu = np.asarray(B).shape
    if outputs is None:
        outputs = OUTPUTS if lx is not None else ("K_traj", "P0", "p0", "status")
    keep = _inputs(A, B, wx, wu, wxf, lx, lu)
    sh = shapes(nx, nu, steps, n)
    out = {name: (np.full(sh[name], -7, dtype=np.int32) if name == "status" else np.full(sh[name], -777.0)) for name in outputs}
    if not device:
        capi.check(backward_raw(r, n, steps, struct({**keep, **out}, reg)), "idocp_rbd_lqr_backward")
        return _turn(out)
    from rbd_batch import DeviceArray
    dev = {name: DeviceArray(x) for name, x in keep.items() if x is not None}
    for name, x in out.items():
        dev[name] = DeviceArray(np.zeros((n + 1) // 2) if name == "status" else x)
    capi.check(backward_raw(r, n, steps, struct({name: d.ptr.value for name, d in dev.items()}, reg), device=True), "idocp_rbd_lqr_backward_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    for name in out:
        out[name] = dev[name].numpy().view(np.int32)[:n].copy() if name == "status" else dev[name].numpy()
    for d in dev.values():
        d.free()
    return _turn(out)


# ------------------------------------------------------------------ the numpy referee

def referee(A, B, wx, wu, wxf, lx=None, lu=None, reg=0.0, refined=False):
    """ONE sample: A [steps][nx][nx], B [steps][nx][nu], lx [steps + 1][nx], lu [steps][nu].  refined: np.longdouble throughout, the Quu solve by
    gen_golden_kkt.solve_refined.  Returns K [steps][nu][nx], k [steps][nu], P0, p0, expected [2] (float64)."""
    T = np.longdouble if refined else np.float64
    A, B = np.asarray(A, dtype=T), np.asarray(B, dtype=T)
    steps, nx, nu = B.shape
    lx = np.zeros((steps + 1, nx), dtype=T) if lx is None else np.asarray(lx, dtype=T)
    lu = np.zeros((steps, nu), dtype=T) if lu is None else np.asarray(lu, dtype=T)
    Wx, Wu, P = np.diag(np.asarray(wx, dtype=T)), np.diag(np.asarray(wu, dtype=T) + T(reg)), np.diag(np.asarray(wxf, dtype=T))
    p = lx[steps].copy()
    K, kf = np.zeros((steps, nu, nx), dtype=T), np.zeros((steps, nu), dtype=T)
    e = np.zeros(2, dtype=T)
    for k in range(steps - 1, -1, -1):
        Qx, Qu = lx[k] + A[k].T @ p, lu[k] + B[k].T @ p
        PA = P @ A[k]
        Qxx, Qux, Quu = Wx + A[k].T @ PA, B[k].T @ PA, Wu + B[k].T @ (P @ B[k])
        rhs = np.hstack([Qux, Qu[:, None]])
        if refined:
            sol = _solve_refined(Quu, rhs)
        else:
            sol = np.linalg.solve(Quu, rhs)
        K[k], kf[k] = -sol[:, :nx], -sol[:, nx]
        X = Qxx + Qux.T @ K[k]
        P = (X + X.T) / 2
        p = Qx + Qux.T @ kf[k]
        e += np.array([kf[k] @ Qu, kf[k] @ Quu @ kf[k] / 2])
    f = lambda x: np.asarray(x, dtype=np.float64)      # noqa: E731
    return {"K_traj": f(K), "k_traj": f(kf), "P0": f(P), "p0": f(p), "expected": f(e)}


def _solve_refined(Quu, rhs):
    """solve_refined on the float64 rounding of the system, then two more rounds with the residual of the long-double system ITSELF, so that the
    answer is that system's to a long double's precision"""
    K64 = np.asarray(Quu, dtype=np.float64)
    z = G.solve_refined(K64, np.asarray(rhs, dtype=np.float64))[0].astype(np.longdouble)
    for _ in range(2):
        res = np.asarray(rhs - Quu @ z, dtype=np.float64)
        z = z + G.solve_refined(K64, res)[0].astype(np.longdouble)
    return z


def referee_batch(c, reg=0.0, refined=False):
    """the referee on every sample of a random_case; arrays shaped like backward()'s return"""
    steps, n = c["B"].shape[:2]
    one = [referee(c["A"][:, i], c["B"][:, i], c["wx"], c["wu"], c["wxf"], None if c["lx"] is None else c["lx"][:, i],
                   None if c["lu"] is None else c["lu"][:, i], reg, refined) for i in range(n)]
    return {"K_traj": np.stack([o["K_traj"] for o in one], axis=1), "k_traj": np.stack([o["k_traj"] for o in one], axis=1),
            "P0": np.stack([o["P0"] for o in one]), "p0": np.stack([o["p0"] for o in one]), "expected": np.stack([o["expected"] for o in one])}


def distance(x, ref):
    """largest deviation relative to max(1, |ref|_inf) of the block"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    return float(np.abs(x - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


def closed_loop(A, B, K, kf, x0):
    """ONE sample: the du sequence [steps][nu] and the states [steps + 1][nx] of u = K x + k on x+ = A x + B u"""
    steps, nx, nu = np.asarray(B).shape
    x, us, xs = np.asarray(x0, dtype=np.float64), [], [np.asarray(x0, dtype=np.float64)]
    for k in range(steps):
        u = K[k] @ x + kf[k]
        x = A[k] @ x + B[k] @ u
        us.append(u)
        xs.append(x)
    return np.array(us), np.array(xs)


def dense_kkt(A, B, wx, wu, wxf, lx, lu, reg, x0):
    """ONE sample, no Riccati formula: the KKT system of  min sum_k (x_k' Wx x_k / 2 + lx_k' x_k + u_k' (Wu + reg I) u_k / 2 + lu_k' u_k)
    + x_S' Wxf x_S / 2 + lx_S' x_S  s.t. x_(k+1) = A_k x_k + B_k u_k, x_0 given -- unknowns [u_0 .. u_(S-1) | x_1 .. x_S | multipliers], solved
    densely with iterative refinement.  Returns (du [steps][nu], the optimal cost)."""
    steps, nx, nu = np.asarray(B).shape
    nU, nX = steps * nu, steps * nx
    H, g = np.zeros((nU + nX, nU + nX)), np.zeros(nU + nX)
    Cm, d = np.zeros((nX, nU + nX)), np.zeros(nX)
    for k in range(steps):
        iu, ix = slice(k * nu, (k + 1) * nu), slice(nU + k * nx, nU + (k + 1) * nx)      # u_k, x_(k+1)
        H[iu, iu], g[iu] = np.diag(np.asarray(wu) + reg), lu[k]
        H[ix, ix], g[ix] = np.diag(wx if k + 1 < steps else wxf), lx[k + 1]
        Cm[k * nx:(k + 1) * nx, ix] = np.eye(nx)
        Cm[k * nx:(k + 1) * nx, iu] = -B[k]
        if k == 0:
            d[:nx] = A[0] @ x0
        else:
            Cm[k * nx:(k + 1) * nx, nU + (k - 1) * nx:nU + k * nx] = -A[k]
    KKT = np.block([[H, Cm.T], [Cm, np.zeros((nX, nX))]])
    z = G.solve_refined(KKT, np.concatenate([-g, d]))[0][:nU + nX]
    cost = 0.5 * z @ H @ z + g @ z + 0.5 * x0 @ (np.asarray(wx) * x0) + lx[0] @ x0
    return z[:nU].reshape(steps, nu), float(cost)
