"""idocp_rbd_lqr_backward_gn_diag on the GPU (the third form of rbd_lqr_kernel.hpp) at n = 5, steps = 4 on the shapes of the quadruped (nx 36, nu 12,
32 + 32 rows: the cap of 64) and of a chain (nx 4, nu 2, 8 rows): D_traj = NULL bit for bit idocp_rbd_lqr_backward_gn; a random non-negative D
against the numpy recursion of rbd_lqr.py with diag(D_k) in the stage Hessian (rbd_penalty.referee_gn_diag, long double with a refined Quu solve)
by the rule of test_rbd_lqr_gn_gpu.py; the same diagonal delivered as extra rows sqrt(d_c) e_c of G to the EXISTING call -- an independent path to
the same answer -- at that bar; a negative or non-finite D entry fails its sample alone, at its step."""
import numpy as np
import pytest

import rbd_gauss_newton as GN
import rbd_lqr as L
import rbd_penalty as PN
from helpers import anymal_model
from independent_rbd import chain
from rbd_batch import E_ARG, Rbd

pytestmark = pytest.mark.gpu

N, STEPS = 5, 4
SHAPES = [("anymal", 36, 12, 64), ("chain2", 4, 2, 8)]


def same(x, y):
    return np.array_equal(x, y, equal_nan=True)


def model_of(which):
    return anymal_model() if which == "anymal" else chain(int(which[5:]), 1)[0]


def random_case(which, nx, nu, rows):
    rng = np.random.default_rng([77, nx, rows])
    c = GN.random_case_gn(rng, nx, nu, STEPS, N, rows)
    Dt = rng.uniform(0.0, 0.5, (STEPS, N, nx + nu)) * (rng.uniform(size=(STEPS, N, nx + nu)) < 0.5)      # (half of the entries are zero, as in use)
    return c, Dt


def hold(got, c, Dt, what, reg=1e-6):
    """the rule of test_rbd_lqr_gn_gpu.py: against the long-double referee at max(FACTOR times the distance of the float64 referee, FLOOR)"""
    refined, plain = PN.referee_gn_diag_batch(c, Dt, reg, refined=True), PN.referee_gn_diag_batch(c, Dt, reg)
    bars = {}
    for name in ("K_traj", "k_traj", "P0", "p0", "expected"):
        d_gpu, d_np = L.distance(got[name], refined[name]), L.distance(plain[name], refined[name])
        bars[name] = max(L.FACTOR * d_np, L.FLOOR)
        print("%s %s: GPU %.2e, FP64 numpy %.2e, bar %.2e" % (what, name, d_gpu, d_np, bars[name]))
        assert d_gpu <= bars[name], (what, name, d_gpu, bars[name])
    return bars


def call(r, c, G_traj, D_traj, reg=1e-6, **kw):
    return PN.backward_gn_diag(r, c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"], reg, G_traj, D_traj, **kw)


@pytest.mark.parametrize("which,nx,nu,rows", SHAPES)
def test_null_diagonal_is_the_gn_call_and_a_diagonal_meets_the_referee(which, nx, nu, rows):
    c, Dt = random_case(which, nx, nu, rows)
    r = Rbd(model_of(which))
    gn = GN.backward_gn(r, c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"], 1e-6, c["G"])
    null = call(r, c, c["G"], None)
    for name in gn:
        assert same(null[name], gn[name]), name
    got = call(r, c, c["G"], Dt)
    assert (got["status"] == -1).all() and not same(got["K_traj"], gn["K_traj"])
    hold(got, c, Dt, which)
    # zeros reproduce the GN numbers (the sum (H + w) + 0)
    zeros = call(r, c, c["G"], np.zeros_like(Dt))
    for name in gn:
        assert np.array_equal(zeros[name], gn[name]), name
    r.close()


@pytest.mark.parametrize("which,nx,nu,rows", [("anymal", 36, 12, 8), ("chain2", 4, 2, 4)])
def test_the_diagonal_as_extra_rows_of_the_existing_call(which, nx, nu, rows):
    """rows + nz (rounded up to 4) <= 64: G gains the rows sqrt(d_c) e_c, and idocp_rbd_lqr_backward_gn must agree"""
    c, Dt = random_case(which, nx, nu, rows)
    nz = nx + nu
    total = (rows + nz + 3) // 4 * 4
    assert total <= 64
    wide = np.zeros((STEPS, N, total, nz))
    wide[:, :, :rows] = c["G"]
    wide[:, :, rows + np.arange(nz), np.arange(nz)] = np.sqrt(Dt)
    r = Rbd(model_of(which))
    got = call(r, c, c["G"], Dt)
    other = GN.backward_gn(r, c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"], 1e-6, wide)
    assert (got["status"] == -1).all() and (other["status"] == -1).all()
    bars = hold(got, c, Dt, which + " diagonal")
    hold(other, c, Dt, which + " extra rows")
    for name, bar in bars.items():      # (both within the bar of the referee: of one another within two)
        d = L.distance(got[name], other[name])
        print("%s %s: diagonal against extra rows %.2e (bar %.2e)" % (which, name, d, 2 * bar))
        assert d <= 2 * bar, (which, name, d)
    r.close()


@pytest.mark.parametrize("which,nx,nu,rows", SHAPES)
def test_a_bad_entry_fails_only_its_sample(which, nx, nu, rows):
    c, Dt = random_case(which, nx, nu, rows)
    r = Rbd(model_of(which))
    clean = call(r, c, c["G"], Dt)
    for value, k, i in ((-1e-3, 2, 1), (np.nan, 0, 3), (np.inf, 3, 4)):
        bad = Dt.copy()
        bad[k, i, nx + 1] = value
        got = call(r, c, c["G"], bad)
        assert got["status"][i] == k and np.isnan(got["K_traj"][:k + 1, i]).all() and np.isnan(got["P0"][i]).all()
        if k + 1 < STEPS:
            assert same(got["K_traj"][k + 1:, i], clean["K_traj"][k + 1:, i])
        keep = np.arange(N) != i
        for name in clean:
            axis = 1 if name in ("K_traj", "k_traj") else 0
            assert same(np.compress(keep, got[name], axis=axis), np.compress(keep, clean[name], axis=axis)), (value, name)
    # D without G is refused
    io = L.struct({**L._inputs(c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"]), "K_traj": np.zeros(L.shapes(nx, nu, STEPS, N)["K_traj"])}, 1e-6)
    assert PN.backward_gn_diag_raw(r, N, STEPS, io, 0, None, Dt) == E_ARG
    r.close()
