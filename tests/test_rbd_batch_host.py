"""The batched rigid-body API on the host side of the C ABI (no compute call): exported symbols and the size of idocp_rbd_io_t, the model check
(a quadruped with its contacts on the tip joints or a fixed-base chain of 2 .. 8 revolute joints, anything else refused naming both), the argument
checks, no CPU fallback, and the facade's new Robot methods compile."""
import ctypes as C
import os
import subprocess

import numpy as np

from arm_chains import random_arm, random_arm_urdf
from helpers import P, anymal_model, arr
from idocp_amd import capi
from rbd_batch import E_ARG, E_DEVICE, E_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_count():
    n = C.c_int()
    capi.lib().idocp_device_count(C.byref(n))
    return n.value


def create(m):
    h = C.c_void_p()
    rc = capi.lib().idocp_rbd_create(C.byref(m), 0, C.byref(h))
    if rc == 0:
        capi.lib().idocp_rbd_destroy(h)
    else:
        assert not h.value
    return rc


def refused(m):
    assert create(m) == E_UNSUPPORTED
    msg = capi.lib().idocp_last_error()
    assert b"2 .. 8 revolute joints" in msg and b"quadruped" in msg and b"4 legs x 3" in msg, msg


def test_symbols_and_the_size_of_the_io_struct():
    lib = capi.lib()
    for name in ("idocp_rbd_create", "idocp_rbd_destroy", "idocp_rbd_synchronize", "idocp_rbd_stream", "idocp_rbd_contact_dynamics_batch",
                 "idocp_rbd_contact_dynamics_batch_device"):
        assert hasattr(lib, name), name
    assert C.sizeof(capi.RbdIO) == 14 * C.sizeof(C.c_void_p)           # 5 inputs, 9 outputs
    assert [f[0] for f in capi.RbdIO._fields_] == ["q", "v", "a", "f", "contact_points", "tau", "dtau_dq", "dtau_dv", "dtau_da", "C", "dCdq", "dCdv", "dCda",
                                                   "MJtJinv"]
    assert (capi.RBD_STAGE, capi.RBD_IMPULSE) == (0, 1)


def test_accepted_models_reach_the_device_check():
    expect = 0 if device_count() > 0 else E_DEVICE
    assert create(anymal_model()) == expect, capi.last_error()
    if expect:
        assert b"no CPU fallback" in capi.lib().idocp_last_error()


def test_a_chain_reaches_the_device_check(tmp_path):
    expect = 0 if device_count() > 0 else E_DEVICE
    assert create(random_arm(5, 1, tmp_path)) == expect, capi.last_error()
    if expect:
        assert b"no CPU fallback" in capi.lib().idocp_last_error()


def test_other_shapes_are_refused_with_the_accepted_ones(tmp_path):
    refused(random_arm(9, 1, tmp_path))
    text = random_arm_urdf(4, 3).replace('<parent link="link_3"/><child link="link_4"/>', '<parent link="link_2"/><child link="link_4"/>')
    path = os.path.join(str(tmp_path), "branched.urdf")
    with open(path, "w") as f:
        f.write(text)
    m = capi.model_from_urdf(path)
    assert m.nv == 4 and list(m.parent)[:4] != [-1, 0, 1, 2]
    refused(m)
    m = anymal_model()
    m.contact_joint[2] = m.contact_joint[2] - 1                  # a contact on a knee link instead of the tip joint of its leg
    refused(m)


def test_null_pointers_are_argument_errors():
    lib = capi.lib()
    m = anymal_model()
    h = C.c_void_p()
    assert lib.idocp_rbd_create(None, 0, C.byref(h)) == E_ARG
    assert lib.idocp_rbd_create(C.byref(m), 0, None) == E_ARG
    io = capi.RbdIO()
    act = (C.c_int * 4)(1, 1, 1, 1)
    for fn in (lib.idocp_rbd_contact_dynamics_batch, lib.idocp_rbd_contact_dynamics_batch_device):
        assert fn(None, 0, 1, act, 0.05, C.byref(io)) == E_ARG
    assert lib.idocp_rbd_synchronize(None) == E_ARG
    assert lib.idocp_rbd_stream(None) is None
    lib.idocp_rbd_destroy(None)


def test_facade_sources_compile_against_include():
    for src in (os.path.join("tests", "cpp", "robot_dynamics.cpp"), os.path.join("examples", "anymal_inverse_dynamics.cpp")):
        r = subprocess.run(["g++", "-O0", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only", os.path.join(ROOT, src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    assert "anymal_inverse_dynamics" in open(os.path.join(ROOT, "examples", "Makefile")).read()


def test_idocp_rnea_derivatives_still_refuses_a_quadruped():
    m = anymal_model()
    n = 2
    q, v = arr(np.zeros((n, m.nq))), arr(np.zeros((n, m.nv)))
    tau, d = np.zeros((n, m.nv)), np.zeros((n, m.nv, m.nv))
    assert capi.lib().idocp_rnea_derivatives(C.byref(m), n, P(q), P(v), P(v), P(tau), P(d), P(d), P(d), 0) == E_UNSUPPORTED
    assert b"2 .. 8 revolute joints" in capi.lib().idocp_last_error()
