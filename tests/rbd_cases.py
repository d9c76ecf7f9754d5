"""Shared by test_rbd_contact_sets_host.py / test_rbd_contact_sets_gpu.py: the cases the quadruped kernels of the rigid-body API
(rbd_batch_kernel.hip, rbd_forward_kernel.hip) are held on -- all 16 contact sets, hard states, positions in the batch -- and the referee's
answers for them.  The referee is the numpy model evaluated at test time (independent_rbd.py, rbd_forward.py on gen_golden_rbd.py); nothing
here calls the oracle or the library's arithmetic.  A plain module: the references are computed once per (model, mask) or per state and shared."""
import functools

import numpy as np

import independent_rbd as IR
import rbd_forward as F
from helpers import anymal_model, rel_err
from rbd_batch import random_samples

RBD = IR.RBD

ALL_MASKS = tuple(tuple((i >> (3 - c)) & 1 for c in range(4)) for i in range(16))
HARD_MASKS = ((1, 1, 1, 1), (1, 1, 1, 0), (0, 0, 1, 0))      # dimf = 12, 9 and 3 with a first active contact that is neither 0 nor 1
MODELS = ("anymal", 1)                                       # ANYmal and other_quadruped(1)
N = 3                       # odd: the last workgroup has one live wavefront
TS = 0.04                   # Baumgarte time step
STIFF_TS = 1e-3             # 1 / TS^2 = 1e6
DT = 0.01                   # integration step
HARD_NAMES = ("straight", "pi", "w_zero", "w_negative", "fast", "stiff", "far", "rest")


def mask_id(mask):
    return "".join(str(int(x)) for x in mask)


def rows_of(mask):
    return np.repeat(np.array(mask, dtype=bool), 3)


def tiled(x, n):
    """sample i of the batch is sample i mod len(x)"""
    x = np.asarray(x)
    return np.ascontiguousarray(x[np.arange(n) % x.shape[0]])


def dist(x, ref):
    """helpers.rel_err; a quantity over no rows at all (no active contact) has the distance 0 when the shapes agree"""
    x, ref = np.asarray(x), np.asarray(ref)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    return rel_err(x, ref) if ref.size else 0.0


def feet(M, q):
    """world positions of the contact frames from the independent model's frame kinematics"""
    z = np.zeros(M["nv"])
    return np.array([x["p"] for x in RBD.frame_kinematics(M, q, z, z)])


# ------------------------------------------------------------------ random samples on two models, for every mask

@functools.lru_cache(maxsize=None)
def quadruped(which):
    """(struct, model dict, (q, v, a, f, pts, u)[N]) of ANYmal or other_quadruped(which); contact points a few centimetres off the feet"""
    from test_other_quadrupeds_gpu import other_quadruped
    if which == "anymal":
        m, rng = anymal_model(), np.random.default_rng(177)
    else:
        m, rng = other_quadruped(which)
    M = IR.model_from_struct(m)
    q, v, a, f, _ = random_samples(rng, N)
    pts = np.array([feet(M, q[i]) for i in range(N)]) + rng.uniform(-0.03, 0.03, (N, 4, 3))
    u = rng.uniform(-20, 20, (N, m.nu))
    return m, M, (q, v, a, f, pts, u)


def impulse_rows(M, q, v, mask):
    """The impulse-mode contact rows over the active contacts from the independent model: C = J v (the LOCAL linear velocity of the contact
    frames at the velocity v), dCdv = dCda = J by the complex step on v (rbd_forward.contact_rows), dCdq by the complex step on q through
    frame_kinematics' dq_seed."""
    nv, z = M["nv"], np.zeros(M["nv"])
    J, C = F.contact_rows(M, q, v, mask, None, None, impulse=True)
    if not any(mask):
        return {"imp_C": C, "imp_J": J, "imp_dCdq": np.zeros((0, nv))}
    Ma = dict(M)
    Ma["contacts"] = [c for c, on in zip(M["contacts"], mask) if on]
    dq = np.array([np.concatenate([x["v"][:3].imag for x in RBD.frame_kinematics(Ma, q, v, z, dq_seed=F._step(nv, k))]) / 1e-30 for k in range(nv)]).T
    return {"imp_C": C, "imp_J": J, "imp_dCdq": dq}


def inverse_terms(M, q, v, a, f, pts, time_step, mask):
    """every output of idocp_rbd_contact_dynamics_batch for one sample and one contact set, both modes: independent_rbd.terms(active = mask)
    and the impulse rows at the velocity v + dv (a is dv there)"""
    t = IR.terms(M, q, v, a, f, pts, time_step, active=mask)
    t.update(impulse_rows(M, q, np.asarray(v) + np.asarray(a), mask))
    return t


@functools.lru_cache(maxsize=None)
def inverse_reference(which, mask):
    m, M, (q, v, a, f, pts, _) = quadruped(which)
    return [inverse_terms(M, q[i], v[i], a[i], f[i], pts[i], TS, mask) for i in range(N)]


# what the independent model holds of each mode: {output of the call: its name among inverse_terms}; the contact outputs over the active rows
STAGE_HELD = {k: k for k in ("tau", "dtau_dq", "dtau_dv", "dtau_da", "C", "dCdq", "dCdv", "dCda", "MJtJinv")}
IMPULSE_HELD = {"tau": "tau_impulse", "dtau_dq": "dimp_dq", "dtau_da": "dimp_da", "C": "imp_C", "dCdq": "imp_dCdq", "dCdv": "imp_J", "dCda": "imp_J",
                "MJtJinv": "MJtJinv"}
CONTACT_OUTPUTS = ("C", "dCdq", "dCdv", "dCda")


@functools.lru_cache(maxsize=None)
def forward_terms(which):
    """rbd_forward.sample_terms of every sample with all four contacts (a mask selects rows and columns): (stage, impulse)"""
    m, M, (q, v, a, f, pts, u) = quadruped(which)
    return ([F.sample_terms(M, q[i], v[i], pts[i], TS) for i in range(N)], [F.sample_terms(M, q[i], v[i], impulse=True) for i in range(N)])


# ------------------------------------------------------------------ hard states (ANYmal)

def hard_states(rng):
    """{name: (q, v, u, pts, time_step)}: one ANYmal sample each, at the places the random generator of the other tests never goes"""
    m = anymal_model()
    M = IR.model_from_struct(m)

    def draw():
        q, v = random_samples(rng, 1)[:2]
        return q[0], v[0], rng.uniform(-20, 20, m.nu)

    def near(q, off=0.03):
        return feet(M, q) + rng.uniform(-off, off, (4, 3))

    out = {}
    q, v, u = draw()
    q[7:] = 0.0                                                     # straight legs
    out["straight"] = (q, v, u, near(q), TS)
    q, v, u = draw()
    q[7:] = rng.choice([-np.pi, np.pi, -np.pi / 2, np.pi / 2], 12)
    out["pi"] = (q, v, u, near(q), TS)
    q, v, u = draw()
    q[3:7] = (0.6, 0.8, 0.0, 0.0)                                    # (x, y, z, w): a half turn, w = 0
    out["w_zero"] = (q, v, u, near(q), TS)
    q, v, u = draw()
    quat = np.append(rng.normal(size=3), -(0.5 + abs(rng.normal())))
    q[3:7] = quat / np.linalg.norm(quat)
    out["w_negative"] = (q, v, u, near(q), TS)
    q, v, u = draw()
    out["fast"] = (q, 20.0 * v, u, near(q), TS)
    q, v, u = draw()
    out["stiff"] = (q, v, u, near(q), STIFF_TS)
    q, v, u = draw()
    d = rng.normal(size=(4, 3))
    out["far"] = (q, v, u, feet(M, q) + 0.5 * d / np.linalg.norm(d, axis=1, keepdims=True), TS)
    q, v, u = draw()
    out["rest"] = (q, np.zeros(m.nv), np.zeros(m.nu), near(q), TS)      # (and the u = NULL call on the same state)
    assert tuple(out) == HARD_NAMES
    return out


@functools.lru_cache(maxsize=None)
def hard_cases():
    """(struct, model dict, {name: dict(q, v, u, pts, time_step, a, f)}): hard_states and an acceleration and forces for the inverse call"""
    m = anymal_model()
    rng = np.random.default_rng(2718)
    out = {}
    for name, (q, v, u, pts, ts) in hard_states(rng).items():
        out[name] = dict(q=q, v=v, u=u, pts=pts, time_step=ts, a=rng.uniform(-2, 2, m.nv), f=rng.uniform(-30, 30, (4, 3)))
    return m, IR.model_from_struct(m), out


@functools.lru_cache(maxsize=None)
def hard_inverse_reference(name, mask):
    _, M, cases = hard_cases()
    s = cases[name]
    return inverse_terms(M, s["q"], s["v"], s["a"], s["f"], s["pts"], s["time_step"], mask)


@functools.lru_cache(maxsize=None)
def hard_forward_terms(name):
    _, M, cases = hard_cases()
    s = cases[name]
    return F.sample_terms(M, s["q"], s["v"], s["pts"], s["time_step"]), F.sample_terms(M, s["q"], s["v"], impulse=True)


# ------------------------------------------------------------------ the referee judged: conditioning, its own residual, a second form

def kkt_system(t, u, mask):
    """(K, rhs) of rbd_forward.solve_terms over the active rows: [M G; J 0] [a; f] = [S^T u - h; -b]"""
    nv, rows = t["h"].size, rows_of(mask)
    tau = np.zeros(nv)
    if u is not None:
        tau[nv - len(u):] = u
    J, b, Gm = t["J"][rows], t["b"][rows], t["G"][:, rows]
    nf = J.shape[0]
    return np.block([[t["M"], Gm], [J, np.zeros((nf, nf))]]), np.concatenate([tau - t["h"], -b])


def conditioning(t, mask):
    """(cond([M J^T; J 0]), cond(J M^-1 J^T)) over the active rows"""
    J = t["J"][rows_of(mask)]
    nf = J.shape[0]
    K = np.block([[t["M"], J.T], [J, np.zeros((nf, nf))]])
    return float(np.linalg.cond(K)), (float(np.linalg.cond(J @ np.linalg.solve(t["M"], J.T))) if nf else 1.0)


def kkt_residual(t, u, mask, a, f):
    """the residual of the referee's own (a, f) in its own system, in long double, scaled by the largest entry of the right-hand side"""
    K, rhs = kkt_system(t, u, mask)
    x = np.concatenate([a, np.asarray(f).reshape(-1)[rows_of(mask)]]).astype(np.longdouble)
    return float(np.abs(K.astype(np.longdouble) @ x - rhs.astype(np.longdouble)).max() / max(1.0, np.abs(rhs).max()))


def solve_longdouble(A, B):
    """Gaussian elimination with partial pivoting in np.longdouble (numpy's own solvers are double only)"""
    A, B = np.array(A, dtype=np.longdouble), np.array(B, dtype=np.longdouble).reshape(A.shape[0], -1)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]], B[[k, p]] = A[[p, k]], B[[p, k]]
        w = A[k + 1:, k] / A[k, k]
        A[k + 1:] -= np.outer(w, A[k])
        B[k + 1:] -= np.outer(w, B[k])
    for k in range(n - 1, -1, -1):
        B[k] = (B[k] - A[k, k + 1:] @ B[k + 1:]) / A[k, k]
    return B


def solve_schur(t, u, mask):
    """The model's answer a second way: the Schur form a = y - T S^-1 (J y + b), y = M^-1 r, T = M^-1 G, S = J T, in np.longdouble -- the
    evaluation order of the kernel, not of rbd_forward.solve_terms (one refined solve of the whole system)."""
    nv, rows = t["h"].size, rows_of(mask)
    nc = rows.size // 3
    tau = np.zeros(nv)
    if u is not None:
        tau[nv - len(u):] = u
    y = solve_longdouble(t["M"], tau - t["h"]).reshape(-1)
    f = np.zeros(3 * nc)
    if rows.any():
        J, b, Gm = t["J"][rows].astype(np.longdouble), t["b"][rows].astype(np.longdouble), t["G"][:, rows]
        T = solve_longdouble(t["M"], Gm)
        g = solve_longdouble(J @ T, J @ y + b).reshape(-1)
        y = y - T @ g
        f[rows] = g.astype(np.float64)
    return y.astype(np.float64), f.reshape(nc, 3)
