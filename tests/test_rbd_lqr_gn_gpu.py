"""idocp_rbd_lqr_backward_gn on the GPU (the GN form of rbd_lqr_kernel.hip): random A, B drawn as rbd_lqr.random_case draws them and G of the
scale of B (test_rbd_gauss_newton_host.py: the float64 and the long-double referee differ by 1e-15 on these inputs, so G is not scaled down),
shapes (36, 12) with 4 and 32 rows, (16, 8) with 8, (4, 2) with 4, 1 and 3 steps, n = 1 and 3.  Outputs against the refined referee of
rbd_gauss_newton.py by the rule of test_rbd_lqr_gpu.py -- max(FACTOR times the distance of the float64 numpy referee, FLOOR) --; G = NULL bit for
bit idocp_rbd_lqr_backward; a case whose Quu is positive definite through Gu alone; a NaN in G that fails its sample at its step; the refusals."""
import numpy as np
import pytest

import independent_rbd as IR
import rbd_gauss_newton as GN
import rbd_lqr as L
from helpers import anymal_model
from idocp_amd import capi
from rbd_batch import E_ARG, Rbd

pytestmark = pytest.mark.gpu

REG = 0.1
SHAPES = [(36, 12, 4), (36, 12, 32), (16, 8, 8), (4, 2, 4)]


def same(x, y):
    return np.array_equal(x, y, equal_nan=True)


def model_of(nx):
    return anymal_model() if nx == 36 else IR.chain(nx // 2, 1)[0]


def hold(got, c, reg, what):
    refined, plain = GN.referee_gn_batch(c, reg, refined=True), GN.referee_gn_batch(c, reg)
    for name in ("K_traj", "k_traj", "P0", "p0", "expected"):
        d_gpu, d_np = L.distance(got[name], refined[name]), L.distance(plain[name], refined[name])
        bar = max(L.FACTOR * d_np, L.FLOOR)
        print("%s %s: GPU %.2e, FP64 numpy %.2e, bar %.2e" % (what, name, d_gpu, d_np, bar))
        assert d_gpu <= bar, (what, name, d_gpu, bar)
    assert (got["status"] == -1).all(), got["status"]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("nx,nu,rows", SHAPES)
def test_against_the_referee(nx, nu, rows, steps, n):
    c = GN.random_case_gn(np.random.default_rng([41, nx, rows, steps, n]), nx, nu, steps, n, rows)
    r = Rbd(model_of(nx))
    got = GN.backward_gn(r, c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"], REG, c["G"])
    hold(got, c, REG, "(%d, %d) rows %d steps %d n %d" % (nx, nu, rows, steps, n))
    # G is in the answer: the diagonal referee is far away
    diag = L.referee_batch(c, REG)
    assert L.distance(got["K_traj"], diag["K_traj"]) > 1e-3
    # the device form, and a sample alone: the same bits
    dev = GN.backward_gn(r, c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"], REG, c["G"], device=True)
    alone = GN.backward_gn(r, c["A"][:, -1:], c["B"][:, -1:], c["wx"], c["wu"], c["wxf"], c["lx"][:, -1:], c["lu"][:, -1:], REG, c["G"][:, -1:])
    for name in got:
        assert same(dev[name], got[name]), name
        ax = 0 if name in ("P0", "p0", "expected", "status") else 1
        assert same(np.take(got[name], [n - 1], axis=ax), alone[name]), name
    only = GN.backward_gn(r, c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"], REG, c["G"], outputs=("k_traj",))
    assert same(only["k_traj"], got["k_traj"])
    r.close()


@pytest.mark.parametrize("nx,nu", [(36, 12), (16, 8), (4, 2)])
def test_without_rows_it_is_the_existing_call_bit_for_bit(nx, nu):
    c = L.random_case(np.random.default_rng([43, nx]), nx, nu, 3, 3)
    r = Rbd(model_of(nx))
    for device in (False, True):
        want = L.backward(r, c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"], REG, device=device)
        got = GN.backward_gn(r, c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"], REG, None, device=device)
        for name in want:
            assert same(got[name], want[name]), (name, device)
    r.close()


@pytest.mark.parametrize("nx,nu,rows", [(36, 12, 32), (4, 2, 4)])
def test_quu_positive_definite_through_the_rows_alone(nx, nu, rows):
    """u_weight = 0 and regularization = 0, B = 0 at the last step: B^T P B vanishes there, and the diagonal call fails where the rows carry Quu"""
    c = GN.random_case_gn(np.random.default_rng([47, nx]), nx, nu, 3, 3, rows)
    c["wu"] = np.zeros(nu)
    c["B"][-1] = 0.0
    r = Rbd(model_of(nx))
    got = GN.backward_gn(r, c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"], 0.0, c["G"])
    hold(got, c, 0.0, "(%d, %d) Quu through Gu" % (nx, nu))
    diag = L.backward(r, c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"], 0.0)
    assert (diag["status"] == 2).all(), diag["status"]
    r.close()


@pytest.mark.parametrize("nx,nu,rows", [(36, 12, 32), (16, 8, 8)])
def test_a_nan_in_the_rows_fails_its_sample_at_its_step(nx, nu, rows):
    steps, n = 3, 3
    c = GN.random_case_gn(np.random.default_rng([53, nx]), nx, nu, steps, n, rows)
    r = Rbd(model_of(nx))
    clean = GN.backward_gn(r, c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"], REG, c["G"])
    bad = c["G"].copy()
    bad[1, 2, rows - 1, nx + nu - 1] = np.nan      # (the last entry of the block of step 1, sample 2)
    got = GN.backward_gn(r, c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"], REG, bad)
    assert list(got["status"]) == [-1, -1, 1]
    for name in ("K_traj", "k_traj"):
        assert same(got[name][:, :2], clean[name][:, :2]) and same(got[name][2, 2], clean[name][2, 2]), name      # (the steps behind keep their values)
        assert np.isnan(got[name][:2, 2]).all(), name
    for name in ("P0", "p0", "expected"):
        assert same(got[name][:2], clean[name][:2]) and np.isnan(got[name][2]).all(), name
    r.close()


def test_refusals():
    nx, nu, rows, steps, n = 4, 2, 4, 2, 3
    c = GN.random_case_gn(np.random.default_rng(59), nx, nu, steps, n, rows)
    r = Rbd(model_of(nx))
    keep = L._inputs(c["A"], c["B"], c["wx"], c["wu"], c["wxf"], c["lx"], c["lu"])
    keep["K_traj"] = np.zeros((steps, n, nx, nu))
    Gt = np.ascontiguousarray(c["G"])
    for device in (False, True):
        who = "idocp_rbd_lqr_backward_gn" + ("_device" if device else "")
        for g_rows, G_, text in ((3, Gt, "g_rows must be a multiple of 4 within 4 .. 64"), (6, Gt, "g_rows must be a multiple of 4"), (68, Gt, "within 4 .. 64"),
                                 (-4, Gt, "within 4 .. 64"), (0, Gt, "G_traj and g_rows come together"), (4, None, "G_traj and g_rows come together")):
            rc = GN.backward_gn_raw(r, n, steps, L.struct(keep, REG), g_rows, G_, device)
            assert rc == E_ARG and capi.last_error().startswith(who + ": ") and text in capi.last_error(), (rc, capi.last_error(), g_rows)
        rc = GN.backward_gn_raw(r, 0, steps, L.struct(keep, REG), rows, Gt, device)
        assert rc == E_ARG and "n must be positive" in capi.last_error()
    r.close()
