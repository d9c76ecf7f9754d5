"""idocp_rbd_lqr_backward without a GPU: the library exports both forms and capi.RbdLqrIO mirrors the header's structure; the numpy referee of
rbd_lqr.py is held to an answer that shares no formula with it -- a dense solve of the whole LQR KKT system (states, controls, multipliers) --
and its float64 form is held to its long-double form on the inputs the GPU tests use (the conditioning claim their bar rests on)."""
import os
import re

import numpy as np
import pytest

import rbd_lqr as L
from idocp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KKT_BAR = 1e-11
CONDITIONING_BAR = 1e-13


def test_symbols_and_structure():
    lib = capi.lib()
    for name in ("idocp_rbd_lqr_backward", "idocp_rbd_lqr_backward_device"):
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "idocp_hip.h")).read()
    body = re.search(r"typedef struct idocp_rbd_lqr_io \{(.*?)\} idocp_rbd_lqr_io_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [x.strip(" *") for x in re.sub(r"^(const\s+)?(double|int)\s*", "", decl).split(",")]
    assert fields == [name for name, _ in capi.RbdLqrIO._fields_], fields
    assert dict(capi.RbdLqrIO._fields_)["regularization"] is capi.C.c_double


@pytest.mark.parametrize("nx,nu", [(36, 12), (4, 2)])
def test_referee_against_a_dense_kkt_solve(nx, nu):
    steps = 5
    rng = np.random.default_rng(2024 + nx)
    c = L.random_case(rng, nx, nu, steps, 1)
    A, B, lx, lu = c["A"][:, 0], c["B"][:, 0], c["lx"][:, 0], c["lu"][:, 0]
    x0, reg = rng.normal(size=nx), 0.25
    ref = L.referee(A, B, c["wx"], c["wu"], c["wxf"], lx, lu, reg)
    du_dense, cost_dense = L.dense_kkt(A, B, c["wx"], c["wu"], c["wxf"], lx, lu, reg, x0)
    du, _ = L.closed_loop(A, B, ref["K_traj"], ref["k_traj"], x0)
    cost = 0.5 * x0 @ ref["P0"] @ x0 + ref["p0"] @ x0 + ref["expected"][0] + ref["expected"][1]
    d_u, d_c = L.distance(du, du_dense), abs(cost - cost_dense) / max(1.0, abs(cost_dense))
    print("(%d, %d): closed loop against the dense du %.2e, cost %.15g against %.15g (%.2e)" % (nx, nu, d_u, cost, cost_dense, d_c))
    assert d_u <= KKT_BAR and d_c <= KKT_BAR, (d_u, d_c)


@pytest.mark.parametrize("nx,nu,steps", [(36, 12, 6), (16, 8, 4), (4, 2, 4)])
def test_float64_referee_sits_on_the_long_double_one(nx, nu, steps):
    c = L.random_case(np.random.default_rng(11 + nx), nx, nu, steps, 2)
    plain, refined = L.referee_batch(c, 0.1), L.referee_batch(c, 0.1, refined=True)
    for name in ("K_traj", "k_traj", "P0", "p0", "expected"):
        d = L.distance(plain[name], refined[name])
        print("(%d, %d) %s: float64 against long double %.2e" % (nx, nu, name, d))
        assert d < CONDITIONING_BAR, (name, d)
    assert np.abs(refined["P0"]).max() < 20.0
