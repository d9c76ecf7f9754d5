"""idocp_rbd_linearize_rollout_al on the GPU (the AL form of rbd_residual_kernel.hip) on the cases and multipliers of test_rbd_al_gpu.py (n = 5,
steps = 4): every output against the numpy referee of rbd_al.py at the 1e-11 of test_rbd_penalty_gpu.py; A, B and the cost rows bit for bit the
penalty call's; lambda = NULL and all zeros give every output of the penalty call bit for bit; a sample's bits whatever n, the outputs asked for and
the form of the call; a NaN multiplier stays in its sample's slice; mu = 0 is refused."""
import functools

import numpy as np
import pytest

import rbd_al as AL
import rbd_gradients as G
import rbd_penalty as PN
import rbd_score as RS
from idocp_amd import capi
from rbd_batch import E_ARG, Rbd
from test_rbd_al_gpu import multipliers
from test_rbd_gradients_gpu import BAR
from test_rbd_penalty_gpu import CASES, MU, N, STEPS, T0, case, same

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def referee(which, cone):
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone, True)
    lam = multipliers(which, cone)[0]
    return AL.reference_al_linearization_batch(mm, M, cost, cons, MU, lam, tables, dt, q, v, u, active, pts, ts)


def run(r, o, which, cone, lam, n=N, mu=MU, **kw):
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone, True)
    c = lambda x: None if x is None else np.ascontiguousarray(x[:, :n])      # noqa: E731
    return AL.linearize_al(r, M, cons, o, mu, c(lam), c(q), c(v), c(u), active, ts, dt, c(pts), **kw)


@pytest.mark.parametrize("which,cone", CASES)
def test_rows_diagonal_and_gradients(which, cone):
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone, True)
    lam = multipliers(which, cone)[0]
    ref = referee(which, cone)
    r = Rbd(mm)
    o = RS.Objective(r, cost, cons, T0, dt, STEPS)
    R = r.lib.idocp_rbd_objective_residual_rows(o.h)
    # 1. against the referee
    out = run(r, o, which, cone, lam)
    for name in ("G_traj", "rho_traj", "D_traj", "lx_traj", "lu_traj"):
        dist = G.distance(out[name], ref[name])
        print("%s %s %s: %.2e (bar %.0e)" % (which, cone, name, dist, BAR))
        assert dist <= BAR, (which, cone, name, dist)
    assert ((out["G_traj"][:, :, R:] != 0).any(axis=3) == (ref["G_traj"][:, :, R:] != 0).any(axis=3)).all()      # (the same rows are active)
    assert same(out["D_traj"], ref["D_traj"])
    # 2. A, B and the cost rows: the bits of the penalty call; the constraint rows are not its
    pen = PN.linearize_penalty(r, M, cons, o, MU, q, v, u, active, ts, dt, pts)
    assert same(out["A_traj"], pen["A_traj"]) and same(out["B_traj"], pen["B_traj"])
    assert same(out["G_traj"][:, :, :R], pen["G_traj"][:, :, :R]) and same(out["rho_traj"][:, :, :R], pen["rho_traj"][:, :, :R])
    assert not same(out["rho_traj"], pen["rho_traj"]) and not same(out["D_traj"], pen["D_traj"]) and G.distance(out["lu_traj"], pen["lu_traj"]) > 1e-3
    # 3. lambda = NULL and all zeros: every output of the penalty call
    for zero in (None, np.zeros_like(lam)):
        got = run(r, o, which, cone, zero)
        for name in PN.OUTPUTS:
            assert np.array_equal(got[name], pen[name]), name
    # 4. a sample's bits whatever n, the outputs asked for and the form of the call
    one = run(r, o, which, cone, lam, n=1)
    for name in PN.OUTPUTS:
        assert same(out[name][:, :1], one[name]), name
    for want in (("G_traj",), ("D_traj",), ("lx_traj", "rho_traj"), ("lu_traj", "A_traj")):
        part = run(r, o, which, cone, lam, want=want)
        for name in want:
            assert same(part[name], out[name]), (want, name)
    dev = run(r, o, which, cone, lam, device=True)
    for name in PN.OUTPUTS:
        assert same(dev[name], out[name]), name
    # 5. a NaN multiplier stays in its sample's slice
    base = multipliers(which, cone)[3]
    bad = lam.copy()
    bad[2, 3, int(np.argmax(base[2, 3] != 0))] = np.nan
    got = run(r, o, which, cone, bad)
    for name in PN.OUTPUTS:
        want = out[name].copy()
        if name not in ("A_traj", "B_traj"):      # (the dynamics blocks do not read the multipliers)
            want[2, 3] = np.nan
        assert same(got[name], want), name
    # 6. mu = 0 is refused here
    sh = PN.output_shapes(mm, M, cons, STEPS, N)
    ok = {k: np.zeros(sh[k]) for k in PN.OUTPUTS}
    rc = AL.linearize_al_raw(r, o, N, STEPS, active, ts, dt, u, pts, q, v, PN.penalty_struct(**ok), 0.0, lam, False)
    assert rc == E_ARG and capi.last_error().startswith("idocp_rbd_linearize_rollout_al: ") and "mu must be positive and finite" in capi.last_error()
    o.close()
    r.close()
