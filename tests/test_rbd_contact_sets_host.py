"""The referee and the cases of test_rbd_contact_sets_gpu.py, checked before any kernel is judged by them.  CPU only.

* every case (every hard state x the masks it is used with, every random sample x 16 masks, the forward file's samples included) is well
  conditioned: cond([M J^T; J 0]) < 1e5, so the 1e-11 bar is the referee's to keep;
* the referee's own (a, f) leaves a KKT residual below 1e-13 of the right-hand side, and its answer a second way (the Schur form in long
  double, the kernel's evaluation order) is the same to 1e-12;
* the oracle, where it has an entry point for the quantity (all four contacts only: a mask is forces set to zero and rows selected), gives
  the independent model's answers on all 16 masks and on the hard states, at independent_rbd.BAR;
* the oracle's impulse-mode contact rows (oracle_impulse_terms C, dCdq, dCdv) against the independent impulse rows of rbd_cases."""
import numpy as np
import pytest

import independent_rbd as IR
import rbd_cases as RC
import rbd_forward as F
from helpers import oracle, rel_err
from rbd_batch import oracle_terms

masks = pytest.mark.parametrize("mask", RC.ALL_MASKS, ids=[RC.mask_id(x) for x in RC.ALL_MASKS])
hard_masks = pytest.mark.parametrize("mask", RC.HARD_MASKS, ids=[RC.mask_id(x) for x in RC.HARD_MASKS])
hard_names = pytest.mark.parametrize("name", RC.HARD_NAMES)


def forward_cases():
    """(id, stage terms, impulse terms, u, masks) of every sample the forward side is refereed on"""
    from test_rbd_forward_dynamics_gpu import MASKS, MODELS, N, quadruped
    assert sorted(tuple(x) for x in MASKS) == sorted(RC.ALL_MASKS)
    for which in MODELS:
        _, _, (q, v, u, pts), stage, imp = quadruped(which)
        for i in range(N):
            yield "forward file %s sample %d" % (which, i), stage[i], imp[i], u[i], RC.ALL_MASKS
    for which in RC.MODELS:
        u = RC.quadruped(which)[2][5]
        stage, imp = RC.forward_terms(which)
        for i in range(RC.N):
            yield "%s sample %d" % (which, i), stage[i], imp[i], u[i], RC.ALL_MASKS
    _, _, cases = RC.hard_cases()
    for name in RC.HARD_NAMES:
        stage, imp = RC.hard_forward_terms(name)
        yield name, stage, imp, cases[name]["u"], RC.HARD_MASKS


def test_hard_states_are_what_they_say():
    _, M, cases = RC.hard_cases()
    assert tuple(cases) == RC.HARD_NAMES
    for name, s in cases.items():
        assert abs(np.linalg.norm(s["q"][3:7]) - 1) < 1e-15, name
    assert (cases["straight"]["q"][7:] == 0).all()
    assert np.isin(np.abs(cases["pi"]["q"][7:]), (np.pi, np.pi / 2)).all() and (np.abs(cases["pi"]["q"][7:]) == np.pi).any()
    assert cases["w_zero"]["q"][6] == 0 and cases["w_negative"]["q"][6] < -0.3
    assert np.abs(cases["fast"]["v"]).max() > 10
    assert cases["stiff"]["time_step"] == 1e-3 and all(s["time_step"] == RC.TS for k, s in cases.items() if k != "stiff")
    d = np.linalg.norm(cases["far"]["pts"] - RC.feet(M, cases["far"]["q"]), axis=1)
    assert np.abs(d - 0.5).max() < 1e-12
    assert not cases["rest"]["v"].any() and not cases["rest"]["u"].any()
    x = np.arange(15.0).reshape(5, 3)
    assert np.array_equal(RC.tiled(x, 12)[:5], x) and np.array_equal(RC.tiled(x, 12)[10:], x[:2]) and RC.tiled(x, 12).shape == (12, 3)
    assert len(set(RC.ALL_MASKS)) == 16


def test_every_case_is_well_conditioned_and_the_referee_solves_it():
    worst = {"cond K": 0.0, "cond S": 0.0, "residual": 0.0, "two forms": 0.0, "|a|": 0.0, "|f|": 0.0}
    ncases = 0
    for name, stage, imp, u, mask_set in forward_cases():
        for mask in mask_set:
            ck, cs = RC.conditioning(stage, mask)
            assert ck < 1e5, (name, mask, ck)
            worst["cond K"], worst["cond S"] = max(worst["cond K"], ck), max(worst["cond S"], cs)
            for mode, t, uu in (("stage", stage, u), ("impulse", imp, None)):
                a, f = F.solve_terms(t, uu, mask)
                res = RC.kkt_residual(t, uu, mask, a, f)
                assert res < 1e-13, (name, mask, mode, res)
                a2, f2 = RC.solve_schur(t, uu, mask)
                two = max(rel_err(a2, a), rel_err(f2, f))
                assert two < 1e-12, (name, mask, mode, two)
                worst["residual"], worst["two forms"] = max(worst["residual"], res), max(worst["two forms"], two)
                worst["|a|"], worst["|f|"] = max(worst["|a|"], np.abs(a).max()), max(worst["|f|"], np.abs(f).max())
                ncases += 1
    print("%d cases:" % ncases, {k: "%.2e" % e for k, e in worst.items()})


def test_inverse_cases_are_well_conditioned():
    """cond([M J^T; J 0]) as independent_rbd.terms reports it for the very matrices MJtJinv is refereed with"""
    worst = 0.0
    for which in RC.MODELS:
        for mask in RC.ALL_MASKS:
            worst = max([worst] + [t["cond"] for t in RC.inverse_reference(which, mask)])
    for name in RC.HARD_NAMES:
        for mask in RC.HARD_MASKS:
            worst = max(worst, RC.hard_inverse_reference(name, mask)["cond"])
    print("worst cond([M J^T; J 0]) of the inverse cases: %.2e" % worst)
    assert worst < 1e5


def check_oracle(m, s, time_step, mask, ref, worst):
    """the oracle's answers for one sample and one mask (forces of the inactive contacts set to zero, rows of the active ones selected)"""
    act, rows = np.array(mask, dtype=bool), RC.rows_of(mask)
    stage, imp = oracle_terms(oracle(), m, s["q"], s["v"], s["a"], s["f"] * act[:, None], s["pts"], time_step)
    got = {k: stage[k] for k in ("tau", "dtau_dq", "dtau_dv", "dtau_da")}
    got.update({k: stage[k][rows] for k in RC.CONTACT_OUTPUTS})
    if all(mask):
        got["MJtJinv"] = stage["MJtJinv"]                     # (the oracle's entry point inverts with all four contacts only)
    for k, x in got.items():
        worst[k] = max(worst.get(k, 0.0), RC.dist(x, ref[k]))
    for k, kref in (("tau", "tau_impulse"), ("dtau_dq", "dimp_dq"), ("dtau_da", "dimp_da")):
        worst[kref] = max(worst.get(kref, 0.0), RC.dist(imp[k], ref[kref]))
    for k, kref in (("C", "imp_C"), ("dCdq", "imp_dCdq"), ("dCdv", "imp_J")):
        worst[kref] = max(worst.get(kref, 0.0), RC.dist(imp[k][rows], ref[kref]))


@masks
@pytest.mark.parametrize("which", RC.MODELS, ids=[str(x) for x in RC.MODELS])
def test_oracle_on_every_contact_set(which, mask):
    m, _, (q, v, a, f, pts, _) = RC.quadruped(which)
    ref = RC.inverse_reference(which, mask)
    worst = {}
    for i in range(RC.N):
        check_oracle(m, dict(q=q[i], v=v[i], a=a[i], f=f[i], pts=pts[i]), RC.TS, mask, ref[i], worst)
    print("oracle against the independent model, %s %s:" % (which, RC.mask_id(mask)), {k: "%.2e" % e for k, e in worst.items()})
    bad = {k: e for k, e in worst.items() if not e < IR.BAR}
    assert not bad, bad


@hard_masks
@hard_names
def test_oracle_on_the_hard_states(name, mask):
    m, _, cases = RC.hard_cases()
    worst = {}
    check_oracle(m, cases[name], cases[name]["time_step"], mask, RC.hard_inverse_reference(name, mask), worst)
    print("oracle against the independent model, %s %s:" % (name, RC.mask_id(mask)), {k: "%.2e" % e for k, e in worst.items()})
    bad = {k: e for k, e in worst.items() if not e < IR.BAR}
    assert not bad, bad


def test_impulse_rows_are_the_velocity_of_the_feet():
    """the new independent rows against a finite difference of the foot positions: J v is the world velocity of the foot turned into the
    contact frame (what the impulse-velocity constraint is), to the accuracy of a central difference"""
    _, M, (q, v, a, f, pts, _) = RC.quadruped("anymal")
    r = RC.impulse_rows(M, q[0], v[0], (1, 1, 1, 1))
    h = 1e-6
    z = np.zeros(M["nv"])
    fk = IR.RBD.frame_kinematics(M, q[0], z, z)
    num = (RC.feet(M, IR.RBD.integrate(M, q[0], h * v[0])) - RC.feet(M, IR.RBD.integrate(M, q[0], -h * v[0]))) / (2 * h)
    local = np.concatenate([fk[c]["R"].T @ num[c] for c in range(4)])
    assert rel_err(r["imp_C"], local) < 1e-8
    assert rel_err(r["imp_J"] @ v[0], r["imp_C"]) < 1e-14
