"""The referee of the forward-dynamics derivatives (tests/rbd_fd_derivatives.py) and the chunk plan of the call, without a GPU.

The referee's da / df blocks are held to central differences of the referee's OWN forward dynamics (rbd_forward.reference at q (+) eps e_r,
v + eps e_r, u + eps e_j), the top rows of its A to central differences of the host's idocp_model_integrate_configuration /
idocp_model_subtract_configuration -- the definition include/idocp_hip.h gives.  Of eps in {1e-5, 1e-6, 1e-7} the best one counts.  FD_BAR is
pinned from one measurement on this code (the largest best-of-three distance was 1.83e-8, on ANYmal with the contacts 1001 in STAGE mode) with a margin of 10.
The chunk plan (idocp_amd/csrc/rbd_fdd_plan.hpp) is held to its rule by a stand-alone program under the address and undefined-behaviour
sanitizers, and to its Python statement through the cases the program prints."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import independent_rbd as IR
import rbd_cases as RC
import rbd_fd_derivatives as D
from helpers import ROOT
from idocp_amd import capi

FD_BAR = 1.9e-7
STEPS = (1e-5, 1e-6, 1e-7)
Q_DIRS, V_DIRS, U_DIRS = (0, 4, 7, 16), (2, 3, 9, 17), (0, 11)
DT = RC.DT


def central(fun, eps):
    return (fun(eps) - fun(-eps)) / (2 * eps)


def unit(n, k, eps):
    e = np.zeros(n)
    e[k] = eps
    return e


def best(columns):
    """the smallest distance over the step sizes; columns: [(finite-difference column, referee column)] per step"""
    return min(D.distance(fd, ref) for fd, ref in columns)


@pytest.mark.parametrize("impulse", (False, True), ids=("stage", "impulse"))
@pytest.mark.parametrize("mask", ((1, 0, 0, 1), (0, 0, 0, 0)), ids=RC.mask_id)
def test_referee_against_central_differences_of_its_forward_dynamics(mask, impulse):
    m, M, (q, v, _, _, pts, u) = RC.quadruped("anymal")
    q, v, pts, u = q[0], v[0], pts[0], u[0]
    ref = D.reference(M, q, v, u, mask, pts, RC.TS, DT, impulse)

    def af(qq, vv, uu):
        a, f = D.F.reference(M, qq, vv, uu, mask, pts, RC.TS, impulse)
        return np.concatenate([a, f.reshape(-1)])

    worst = 0.0
    for k in Q_DIRS:
        d = best([(central(lambda e: af(D.RBD.integrate(M, q, unit(m.nv, k, e)), v, u), h), np.concatenate([ref["da_dq"][:, k], ref["df_dq"][:, k]])) for h in STEPS])
        worst = max(worst, d)
    for k in V_DIRS:
        d = best([(central(lambda e: af(q, v + unit(m.nv, k, e), u), h), np.concatenate([ref["da_dv"][:, k], ref["df_dv"][:, k]])) for h in STEPS])
        worst = max(worst, d)
    if not impulse:
        for k in U_DIRS:
            d = best([(central(lambda e: af(q, v, u + unit(m.nu, k, e)), h), np.concatenate([ref["da_du"][:, k], ref["df_du"][:, k]])) for h in STEPS])
            worst = max(worst, d)
    print("%s %s: worst best-of-three distance %.2e (bar %.2e)" % (RC.mask_id(mask), "impulse" if impulse else "stage", worst, FD_BAR))
    assert worst < FD_BAR


def test_referee_top_rows_against_the_host_retraction():
    m, M, (q, v, _, _, _, _) = RC.quadruped("anymal")
    lib = capi.lib()

    def integrate(qq, d, length):
        out = np.zeros(m.nq)
        d = np.ascontiguousarray(d)
        capi.check(lib.idocp_model_integrate_configuration(C.byref(m), qq.ctypes.data, d.ctypes.data, length, out.ctypes.data), "integrate")
        return out

    def subtract(qp, qm):
        out = np.zeros(m.nv)
        capi.check(lib.idocp_model_subtract_configuration(C.byref(m), qp.ctypes.data, qm.ctypes.data, out.ctypes.data), "subtract")
        return out

    worst = 0.0
    for i in range(RC.N):
        for scale in (1.0, 30.0):      # dt |w| of about 0.01 and 0.3 rad
            vi = scale * v[i]
            Jq, Jv = D.retraction_blocks(vi[:6], DT)
            q_next = integrate(q[i], vi, DT)
            for r in range(6):
                cq = [(central(lambda e: subtract(integrate(integrate(q[i], unit(m.nv, r, 1.0), e), vi, DT), q_next), h)[:6], Jq[:, r]) for h in STEPS]
                cv = [(central(lambda e: subtract(integrate(q[i], vi + unit(m.nv, r, e), DT), q_next), h)[:6], Jv[:, r]) for h in STEPS]
                worst = max(worst, best(cq), best(cv))
    print("top rows of A: worst best-of-three distance %.2e (bar %.2e)" % (worst, FD_BAR))
    assert worst < FD_BAR


def test_chain_referee_against_central_differences():
    _, M = IR.chain(7, 0)
    rng = np.random.default_rng(11)
    q, v, u = rng.uniform(-2, 2, 7), rng.uniform(-2, 2, 7), rng.uniform(-10, 10, 7)
    ref = D.reference(M, q, v, u, [], dt=DT)
    acc = lambda qq, vv, uu: D.F.reference(M, qq, vv, uu, [])[0]      # noqa: E731
    worst = 0.0
    for k in (0, 3, 6):
        worst = max(worst, best([(central(lambda e: acc(q + unit(7, k, e), v, u), h), ref["da_dq"][:, k]) for h in STEPS]),
                    best([(central(lambda e: acc(q, v + unit(7, k, e), u), h), ref["da_dv"][:, k]) for h in STEPS]),
                    best([(central(lambda e: acc(q, v, u + unit(7, k, e)), h), ref["da_du"][:, k]) for h in STEPS]))
    print("chain: worst best-of-three distance %.2e (bar %.2e)" % (worst, FD_BAR))
    assert worst < FD_BAR
    assert np.array_equal(ref["A"][:7], np.hstack([np.eye(7), DT * np.eye(7)]))


def test_chunk_plan_under_the_sanitizers_and_against_its_python_statement(tmp_path):
    exe = str(tmp_path / "rbd_fdd_plan")
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "idocp_amd/csrc"), os.path.join(ROOT, "tests/cpp/rbd_fdd_plan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rbd fdd plan: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    cases = re.findall(r"plan (\d+) (\d+) (\d+) (\d+): chunk (\d+) nchunks (\d+) total (\d+)", r.stdout)
    assert len(cases) == 3
    for nv, nf, n, limit, chunk, nchunks, total in (tuple(int(x) for x in c) for c in cases):
        assert D.plan(nv, nf, n, limit) == {"chunk": chunk, "nchunks": nchunks, "total": total}
    p = D.plan(18, 12, 122880)
    assert p["total"] * 8 <= 256 << 20 and (p["chunk"] + 1) * 2010 * 8 > 256 << 20


def test_right_jacobian_of_exp6_on_both_sides_of_its_switch(tmp_path):
    """lieDIntegrateArg1 (dev_lie.hpp; host and device code alike) at zero, on both sides of 0.05 rad and at large angles against the inverse of
    Jlog6, as a stand-alone program under the sanitizers"""
    exe = str(tmp_path / "lie_dintegrate_arg1")
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "idocp_amd/csrc"), os.path.join(ROOT, "tests/cpp/lie_dintegrate_arg1.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lie dintegrate arg1: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
