"""Fixed-base chains other than iiwa14 on the host side of the C ABI (no compute call): 2 .. 8 revolute joints pass the model
check of the fixed-base entry points, a longer chain or a branched one is refused naming the range, and the six-joint
example compiles against include/."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from arm_chains import arm6_model, random_arm, random_arm_urdf
from helpers import P, arr, unocp_problem
from idocp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DEVICE, E_UNSUPPORTED = -1, -3, -4


def device_count():
    n = C.c_int()
    capi.lib().idocp_device_count(C.byref(n))
    return n.value


def create(fn, m):
    cost, cons = unocp_problem(m)
    h = C.c_void_p()
    rc = fn(C.byref(m), C.byref(cost), C.byref(cons), 1.0, 10, 1, 0, C.byref(h))
    if rc == 0:
        capi.lib().idocp_unocp_destroy(h)
    return rc


def entry_points():
    lib = capi.lib()

    def shard(m, cost, cons, T, N, batch, device, out):
        return lib.idocp_unparnmpc_create_shard(m, cost, cons, T, N, 0, N // 2, batch, device, out)
    return [lib.idocp_unocp_create, lib.idocp_unparnmpc_create, shard]


def refused(rc, what):
    assert rc == E_UNSUPPORTED, (what, rc)
    assert b"2 .. 8 revolute joints" in capi.lib().idocp_last_error(), capi.lib().idocp_last_error()


@pytest.mark.parametrize("nv", range(2, 9))
def test_chains_of_two_to_eight_joints_pass_the_model_check(tmp_path, nv):
    m = random_arm(nv, 1, tmp_path)
    assert m.nv == nv and m.njoints == nv
    expect = 0 if device_count() > 0 else E_DEVICE          # without a GPU: the device check, never the model check
    for fn in entry_points():
        assert create(fn, m) == expect, capi.lib().idocp_last_error()


def test_the_six_joint_arm_passes_the_model_check():
    m = arm6_model()
    assert m.nv == 6 and m.njoints == 6 and not m.has_floating_base
    expect = 0 if device_count() > 0 else E_DEVICE
    for fn in entry_points():
        assert create(fn, m) == expect, capi.lib().idocp_last_error()


def test_nine_joints_are_refused_with_the_range(tmp_path):
    m = random_arm(9, 1, tmp_path)
    assert m.nv == 9
    for fn in entry_points():
        refused(create(fn, m), fn)
    n = 3
    q, v, a = arr(np.zeros((n, 9))), arr(np.zeros((n, 9))), arr(np.zeros((n, 9)))
    tau, d = np.zeros((n, 9)), np.zeros((n, 9, 9))
    refused(capi.lib().idocp_rnea_derivatives(C.byref(m), n, P(q), P(v), P(a), P(tau), P(d), P(d), P(d), 0), "rnea_derivatives")


def test_one_joint_is_refused_with_the_range(tmp_path):
    m = random_arm(1, 1, tmp_path)
    assert m.nv == 1
    for fn in entry_points():
        refused(create(fn, m), fn)


def test_a_branched_chain_is_refused_with_the_range(tmp_path):
    # four revolute joints where the last hangs off the second link: not a serial chain
    text = random_arm_urdf(4, 3)
    text = text.replace('<parent link="link_3"/><child link="link_4"/>', '<parent link="link_2"/><child link="link_4"/>')
    path = os.path.join(str(tmp_path), "branched.urdf")
    with open(path, "w") as f:
        f.write(text)
    m = capi.model_from_urdf(path)
    assert m.nv == 4 and list(m.parent)[:4] != [-1, 0, 1, 2]
    for fn in entry_points():
        refused(create(fn, m), fn)
    n = 2
    q = arr(np.zeros((n, 4)))
    tau, d = np.zeros((n, 4)), np.zeros((n, 4, 4))
    refused(capi.lib().idocp_rnea_derivatives(C.byref(m), n, P(q), P(q), P(q), P(tau), P(d), P(d), P(d), 0), "rnea_derivatives")


def test_iiwa14_halo_sizes_are_unchanged():
    lib = capi.lib()
    assert [lib.idocp_unparnmpc_halo_size(k) for k in range(5)] == [14, 14, 196, 14, 14]
    assert lib.idocp_unparnmpc_halo_size_of(None, 0) == 0


def test_six_joint_example_compiles_against_include():
    r = subprocess.run(["g++", "-O0", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only",
                        os.path.join(ROOT, "examples", "arm6_unocp.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "arm6_unocp" in open(os.path.join(ROOT, "examples", "Makefile")).read()
