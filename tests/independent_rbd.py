"""The independent rigid-body model of tests/golden/gen_golden_rbd.py (numpy body-frame Newton-Euler, complex-step derivatives, its own URDF walk, its own
frame kinematics and Baumgarte assembly) evaluated AT TEST TIME, for the models the committed rbd_*.json / contact_anymal.json do not cover: fixed-base
chains with arbitrary unit axes and joint / inertial rpy, and quadrupeds that exist only as a perturbed model struct.  Shared by
test_independent_rbd_host.py (URDF reader and oracle) and test_independent_rbd_gpu.py (the kernels): the same models, the same samples, the same answers,
the same bars.  Nothing here calls the oracle or the library's arithmetic; capi is used to READ a model struct only."""
import functools
import os
import sys
import tempfile

import numpy as np

from arm_chains import ARM6_URDF, random_arm_urdf
from helpers import GOLDEN
from idocp_amd import capi

sys.path.insert(0, GOLDEN)
import gen_golden_kkt as G      # noqa: E402
import gen_golden_rbd as RBD      # noqa: E402

# rel_err bar of every quantity: the one tests/test_golden_rbd.py / tests/test_golden_rbd_gpu.py hold the same quantities to on the two committed robots
BAR = 1e-11
CHAIN_SAMPLES, QUADRUPED_SAMPLES, QUADRUPED_DT = 5, 3, 0.04
QUADRUPED_SEEDS = (0, 1, 2)
PARTIAL_MASK = [1, 0, 0, 1]


def model_from_struct(m):
    """gen_golden_rbd's model dict from a capi.Model (for models that exist only as a struct, e.g. other_quadruped(seed))."""
    n = m.njoints
    M = dict(njoints=n, nq=m.nq, nv=m.nv, floating=int(m.has_floating_base),
             parent=[int(m.parent[i]) for i in range(n)], jtype=[int(m.jtype[i]) for i in range(n)],
             idx_q=[int(m.idx_q[i]) for i in range(n)], idx_v=[int(m.idx_v[i]) for i in range(n)],
             axis=[np.array(m.axis[i][:]) for i in range(n)],
             plc_R=[np.array(m.plc_R[i][:]).reshape(3, 3) for i in range(n)], plc_p=[np.array(m.plc_p[i][:]) for i in range(n)],
             body=[(float(m.mass[i]), np.array(m.com[i][:]), np.array(m.inertia[i][:]).reshape(3, 3)) for i in range(n)],      # (inertia about the com)
             contacts=[(int(m.contact_frame_id[c]), int(m.contact_joint[c]), np.array(m.contact_R[c][:]).reshape(3, 3), np.array(m.contact_p[c][:]))
                       for c in range(m.ncontacts)],
             gravity=np.array(m.gravity[:]))
    return M


def joint_forces(M, f, active):
    """contact forces as generate() enters them: local contact frame -> parent joint frame, (force, moment about the joint origin)"""
    fc = np.asarray(f, dtype=np.float64).reshape(len(M["contacts"]), 3)
    fext = np.zeros((M["njoints"], 6))
    for c, (_, jid, Rc, pc) in enumerate(M["contacts"]):
        if active[c]:
            fl = Rc @ fc[c]
            fext[jid, 0:3] += fl
            fext[jid, 3:6] += np.cross(pc, fl)
    return fext


def terms(M, q, v, a, f=None, contact_points=None, time_step=None, active=None, impulse_forms=True):
    """One sample from the generator's own functions, matrices as [row, column].
    tau, dtau_dq, dtau_dv, dtau_da (with the forces f[nc][3] of the active contacts, if given); on a model with contacts the impulse forms
    (no gravity, v = 0) tau_impulse, dimp_dq, dimp_da; with contact_points and time_step the Baumgarte C, dCdq, dCdv, dCda over the ACTIVE rows,
    MJtJinv = [M J^T; J 0]^-1 (J = dCda; identity columns through gen_golden_kkt.solve_refined) and cond = cond([M J^T; J 0])."""
    q, v, a = (np.asarray(x, dtype=np.float64) for x in (q, v, a))
    nc, nv = len(M["contacts"]), M["nv"]
    act = [True] * nc if active is None else [bool(x) for x in active]
    fext = joint_forces(M, f, act) if f is not None else None
    out = {"tau": RBD.rnea(M, q, v, a, fext)}
    out["dtau_dq"], out["dtau_dv"], out["dtau_da"] = RBD.rnea_derivatives(M, q, v, a, fext)
    if nc and impulse_forms:      # (impulse_forms = False: a caller that holds a regular stage only)
        z = np.zeros(nv)
        out["tau_impulse"] = RBD.rnea(M, q, z, a, fext, gravity=False)
        out["dimp_dq"], _, out["dimp_da"] = RBD.rnea_derivatives(M, q, z, a, fext, gravity=False)
    if contact_points is not None:
        Ma = dict(M)
        Ma["contacts"] = [c for c, on in zip(M["contacts"], act) if on]
        pts = np.asarray(contact_points, dtype=np.float64).reshape(nc, 3)[np.array(act, dtype=bool)]
        out["C"], out["dCdq"], out["dCdv"], out["dCda"] = RBD.baumgarte(Ma, q, v, a, pts, time_step)[:4]
        J = out["dCda"]
        K = np.block([[out["dtau_da"], J.T], [J, np.zeros((J.shape[0], J.shape[0]))]])
        out["MJtJinv"], _ = G.solve_refined(K, np.eye(K.shape[0]))
        out["cond"] = float(np.linalg.cond(K))
    return out


# ------------------------------------------------------------------ the fixed-base chains

def chain_cases():
    """(id, nv, seed, zaxes) of every chain of test_other_arms_gpu.CHAINS"""
    from test_other_arms_gpu import CHAINS
    return [("arm%d_%d%s" % (nv, seed, "_z" if zaxes else ""), nv, seed, zaxes) for nv, seed, zaxes in CHAINS]


@functools.lru_cache(maxsize=None)
def chain(nv, seed, zaxes=False, inertial_rpy=False):
    """(struct from the library's URDF reader, model dict from the generator's own URDF walk) of a random chain; nv = 0: the committed six-joint arm"""
    if nv == 0:
        return capi.model_from_urdf(ARM6_URDF), RBD.load_model(ARM6_URDF)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "chain.urdf")
        with open(path, "w") as fh:
            fh.write(random_arm_urdf(nv, seed, zaxes, inertial_rpy=inertial_rpy))
        return capi.model_from_urdf(path), RBD.load_model(path)


@functools.lru_cache(maxsize=None)
def chain_samples(nv, seed, zaxes=False, inertial_rpy=False):
    """(q, v, a)[CHAIN_SAMPLES][nv] in the ranges of test_other_arms_gpu.check_rnea_derivatives and terms() of every sample"""
    M = chain(nv, seed, zaxes, inertial_rpy)[1]
    n, dim = CHAIN_SAMPLES, M["nv"]
    rng = np.random.default_rng([31, nv, seed, int(zaxes)])      # (the inertial rpy changes the model, not the samples)
    q, v, a = rng.uniform(-2.5, 2.5, (n, dim)), rng.uniform(-3, 3, (n, dim)), rng.uniform(-5, 5, (n, dim))
    return (q, v, a), [terms(M, q[i], v[i], a[i]) for i in range(n)]


# ------------------------------------------------------------------ quadrupeds that are not ANYmal

@functools.lru_cache(maxsize=None)
def quadruped(seed):
    """(perturbed struct, its model dict, (q, v, a, f, pts), terms with all four contacts) of other_quadruped(seed), the samples drawn the way the
    `other` fixture of test_rbd_batch_gpu.py draws its own"""
    from test_other_quadrupeds_gpu import other_quadruped
    from rbd_batch import random_samples
    m, rng = other_quadruped(seed)
    M = model_from_struct(m)
    q, v, a, f, pts = random_samples(rng, QUADRUPED_SAMPLES)
    return m, M, (q, v, a, f, pts), [terms(M, q[i], v[i], a[i], f[i], pts[i], QUADRUPED_DT) for i in range(QUADRUPED_SAMPLES)]


@functools.lru_cache(maxsize=None)
def quadruped_partial(seed):
    """terms of the same samples with the contacts of PARTIAL_MASK (the forces of the other two do not act, their rows are not there)"""
    _, M, (q, v, a, f, pts), _ = quadruped(seed)
    return [terms(M, q[i], v[i], a[i], f[i], pts[i], QUADRUPED_DT, active=PARTIAL_MASK) for i in range(QUADRUPED_SAMPLES)]


def stack(answers, key):
    return np.array([x[key] for x in answers])
