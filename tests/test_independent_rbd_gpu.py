"""The general-geometry kernels against the independent rigid-body model (tests/independent_rbd.py: gen_golden_rbd.py's numpy body-frame Newton-Euler,
complex-step derivatives, its own Baumgarte assembly, a refined dense inverse of [M J^T; J 0]) -- the same models, samples, answers and bars as
test_independent_rbd_host.py holds the URDF reader and the oracle to.

* idocp_rnea_derivatives on fixed-base chains of 2 .. 8 joints with arbitrary unit axes and joint rpy (UnLaunch<2..8>, the two-round form at 8 joints), the
  committed six-joint arm, and the two all-z chains in both instantiations (the +z one and, through IDOCP_GENERAL_AXES, the general one);
* idocp_rbd_contact_dynamics_batch on quadrupeds that are not ANYmal (general leg sweeps), stage and impulse mode, four contacts and two.

Elsewhere these paths are checked against the oracle, which reads the same model struct and was extended to general geometry together with the kernels; an
error the two share (an rpy convention, a general axis in the analytic derivatives, an inertial rotation) shows only here.  The impulse-mode contact rows
(impulse velocity and its derivatives), every contact set and the hard states: test_rbd_contact_sets_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import independent_rbd as IR
from helpers import P, arr, rel_err
from idocp_amd import capi
from rbd_batch import IMPULSE, STAGE, Rbd, packed_mjtjinv

pytestmark = pytest.mark.gpu

# (id, nv, seed, zaxes, forced general instantiation); nv = 0: the committed six-joint arm
CHAIN_RUNS = ([(name, nv, seed, z, False) for name, nv, seed, z in IR.chain_cases()] + [("arm6", 0, 0, False, False)]
              + [(name + "_general_axes", nv, seed, z, True) for name, nv, seed, z in IR.chain_cases() if z])


@pytest.mark.parametrize("nv,seed,zaxes,general", [c[1:] for c in CHAIN_RUNS], ids=[c[0] for c in CHAIN_RUNS])
def test_rnea_derivatives_on_the_chains(monkeypatch, nv, seed, zaxes, general):
    if general:
        monkeypatch.setenv("IDOCP_GENERAL_AXES", "1")          # (read per call)
    m, _ = IR.chain(nv, seed, zaxes)
    (q, v, a), ref = IR.chain_samples(nv, seed, zaxes)
    n, dim = IR.CHAIN_SAMPLES, m.nv
    q, v, a = arr(q), arr(v), arr(a)
    tau, dq, dv, da = np.zeros((n, dim)), np.zeros((n, dim, dim)), np.zeros((n, dim, dim)), np.zeros((n, dim, dim))
    capi.check(capi.lib().idocp_rnea_derivatives(C.byref(m), n, P(q), P(v), P(a), P(tau), P(dq), P(dv), P(da), 0), "idocp_rnea_derivatives")
    got = {"tau": tau, "dtau_dq": dq.transpose(0, 2, 1), "dtau_dv": dv.transpose(0, 2, 1), "dtau_da": da.transpose(0, 2, 1)}      # (column-major blocks)
    errs = {k: rel_err(x, IR.stack(ref, k)) for k, x in got.items()}
    print("idocp_rnea_derivatives against the independent model:", {k: "%.2e" % e for k, e in errs.items()})
    bad = {k: e for k, e in errs.items() if not e < IR.BAR}
    assert not bad, bad


@pytest.mark.parametrize("mode", [STAGE, IMPULSE], ids=["stage", "impulse"])
@pytest.mark.parametrize("seed", IR.QUADRUPED_SEEDS)
def test_contact_dynamics_batch_on_other_quadrupeds(seed, mode):
    m, _, (q, v, a, f, pts), full = IR.quadruped(seed)
    part = IR.quadruped_partial(seed)
    nv = m.nv
    r = Rbd(m)
    # what the independent model holds of each mode: {output: its name among the answers}
    if mode == STAGE:
        held = {k: k for k in ("tau", "dtau_dq", "dtau_dv", "dtau_da", "C", "dCdq", "dCdv", "dCda")}
    else:
        held = {"tau": "tau_impulse", "dtau_dq": "dimp_dq", "dtau_da": "dimp_da"}
    for mask, ref in (([1, 1, 1, 1], full), (IR.PARTIAL_MASK, part)):
        rows = np.repeat(np.array(mask, dtype=bool), 3)
        dimf = int(rows.sum())
        o = r.call(mode, q, v, a, mask, IR.QUADRUPED_DT if mode == STAGE else 0.0, f=f, contact_points=pts)
        errs = {}
        for k, kref in held.items():
            x = o[k]
            if k in ("C", "dCdq", "dCdv", "dCda"):
                assert (x[:, ~rows] == 0).all(), k               # (the rows of an inactive contact)
                x = x[:, rows]
            errs[k] = rel_err(x, IR.stack(ref, kref))
        errs["MJtJinv"] = rel_err(np.array([packed_mjtjinv(x, nv, dimf) for x in o["MJtJinv"]]), IR.stack(ref, "MJtJinv"))
        print("quadruped %d, mode %d, contacts %s against the independent model:" % (seed, mode, mask), {k: "%.2e" % e for k, e in errs.items()})
        bad = {k: e for k, e in errs.items() if not e < IR.BAR}
        assert not bad, (mask, bad)
        if mode == IMPULSE:
            assert (o["dtau_dv"] == 0).all()
    r.close()
