"""The URDF reader and the oracle's rigid-body terms on GENERAL geometry against the independent model (tests/independent_rbd.py: gen_golden_rbd.py's
numpy body-frame Newton-Euler with complex-step derivatives and its own URDF walk, evaluated at test time).  CPU only.

tests/test_golden_rbd.py pins reader and oracle on iiwa14 (every axis +z) and ANYmal (x / y / y, identity placements) -- the patterns the kernels carry
specialised instantiations for.  Here: fixed-base chains of 2 .. 8 joints with arbitrary unit axes and joint rpy (test_other_arms_gpu.CHAINS), the same
chains with an inertial rpy on every link, the committed six-joint arm, and quadrupeds that exist only as a perturbed struct (other_quadruped(0..2)) --
the models on which the oracle alone checks the kernels everywhere else.  test_independent_rbd_gpu.py holds the kernels to the same answers at the same
bars.  The impulse-mode contact rows (impulse velocity and its derivatives) are held to the independent model in test_rbd_contact_sets_host.py / _gpu.py."""
import ctypes as C

import numpy as np
import pytest

import independent_rbd as IR
from helpers import P, arr, oracle, rel_err
from rbd_batch import oracle_terms

# (id, nv, seed, zaxes, inertial rpy); nv = 0: the committed six-joint arm
CHAIN_MODELS = ([(name, nv, seed, z, False) for name, nv, seed, z in IR.chain_cases()]
                + [(name + "_inertial_rpy", nv, seed, z, True) for name, nv, seed, z in IR.chain_cases()] + [("arm6", 0, 0, False, False)])
chains = pytest.mark.parametrize("nv,seed,zaxes,inertial_rpy", [c[1:] for c in CHAIN_MODELS], ids=[c[0] for c in CHAIN_MODELS])


@chains
def test_urdf_reader_matches_the_independent_urdf_walk(nv, seed, zaxes, inertial_rpy):
    """capi.model_from_urdf against gen_golden_rbd.load_model field by field, at the tolerances of test_golden_rbd.test_urdf_reader_matches_golden_model"""
    m, g = IR.chain(nv, seed, zaxes, inertial_rpy)
    assert (m.njoints, m.nq, m.nv, m.has_floating_base, m.nu, m.ncontacts) == (g["njoints"], g["nq"], g["nv"], 0, g["nv"], 0)
    assert m.njoints == (nv or 6)
    turned = False
    for i in range(m.njoints):
        assert m.parent[i] == g["parent"][i] and m.jtype[i] == g["jtype"][i]
        assert m.idx_q[i] == g["idx_q"][i] and m.idx_v[i] == g["idx_v"][i]
        mass, com, inertia = g["body"][i]
        np.testing.assert_allclose(m.axis[i][:], g["axis"][i], atol=1e-15)
        np.testing.assert_allclose(m.plc_R[i][:], g["plc_R"][i].reshape(-1), atol=1e-15)
        np.testing.assert_allclose(m.plc_p[i][:], g["plc_p"][i], atol=1e-15)
        np.testing.assert_allclose(m.mass[i], mass, rtol=1e-15)
        np.testing.assert_allclose(m.com[i][:], com, atol=1e-15)
        np.testing.assert_allclose(m.inertia[i][:], inertia.reshape(-1), atol=1e-15)
        assert m.q_min[i] == g["q_min"][i] and m.q_max[i] == g["q_max"][i] and m.v_max[i] == g["v_max"][i] and m.u_max[i] == g["u_max"][i]
        assert abs(np.linalg.norm(m.axis[i][:]) - 1) < 1e-15
        assert np.linalg.eigvalsh(np.array(m.inertia[i][:]).reshape(3, 3)).min() > 0      # (every link has a rotational inertia to get wrong)
        turned |= bool(np.abs(inertia - IR.chain(nv, seed, zaxes, False)[1]["body"][i][2]).max() > 1e-4)
    assert turned == inertial_rpy                              # (the option does reach the inertia, and nothing else does)
    assert np.array_equal(m.gravity[:], g["gravity"])


@chains
def test_oracle_rnea_and_derivatives_on_the_chains(nv, seed, zaxes, inertial_rpy):
    m, _ = IR.chain(nv, seed, zaxes, inertial_rpy)
    (q, v, a), ref = IR.chain_samples(nv, seed, zaxes, inertial_rpy)
    n = m.nv
    ol = oracle()
    worst = {}
    for i in range(IR.CHAIN_SAMPLES):
        tau, dq, dv, da = np.zeros(n), np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
        ol.oracle_rnea(C.byref(m), P(arr(q[i])), P(arr(v[i])), P(arr(a[i])), None, 1, P(tau))
        ol.oracle_rnea_derivatives(C.byref(m), P(arr(q[i])), P(arr(v[i])), P(arr(a[i])), None, 1, P(dq), P(dv), P(da))
        for k, x in (("tau", tau), ("dtau_dq", dq.T), ("dtau_dv", dv.T), ("dtau_da", da.T)):      # (the oracle writes column-major)
            worst[k] = max(worst.get(k, 0.0), rel_err(x, ref[i][k]))
    print("oracle against the independent model:", {k: "%.2e" % e for k, e in worst.items()})
    bad = {k: e for k, e in worst.items() if not e < IR.BAR}
    assert not bad, bad


STAGE_KEYS = ("tau", "dtau_dq", "dtau_dv", "dtau_da", "C", "dCdq", "dCdv", "dCda", "MJtJinv")
IMPULSE_KEYS = (("tau", "tau_impulse"), ("dtau_dq", "dimp_dq"), ("dtau_da", "dimp_da"))


@pytest.mark.parametrize("seed", IR.QUADRUPED_SEEDS)
def test_oracle_terms_on_other_quadrupeds(seed):
    """the oracle's entry points as test_rbd_batch_gpu.oracle_terms calls them: tau with four contact forces, its three derivative blocks, the
    Baumgarte terms, MJtJinv, and the impulse tau, dtau_dq, dtau_da"""
    m, _, (q, v, a, f, pts), full = IR.quadruped(seed)
    worst = {}
    for i in range(IR.QUADRUPED_SAMPLES):
        stage, imp = oracle_terms(oracle(), m, q[i], v[i], a[i], f[i], pts[i], IR.QUADRUPED_DT)
        print("quadruped %d sample %d: cond([M J^T; J 0]) = %.3e" % (seed, i, full[i]["cond"]))
        for k in STAGE_KEYS:
            worst[k] = max(worst.get(k, 0.0), rel_err(stage[k], full[i][k]))
        for k, kref in IMPULSE_KEYS:
            worst[kref] = max(worst.get(kref, 0.0), rel_err(imp[k], full[i][kref]))
    print("oracle against the independent model:", {k: "%.2e" % e for k, e in worst.items()})
    bad = {k: e for k, e in worst.items() if not e < IR.BAR}
    assert not bad, bad
