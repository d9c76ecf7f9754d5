"""The closed-loop calls (idocp_rbd_feedback_torques_batch, idocp_rbd_rollout_policy) without a GPU: the exported symbols, the ctypes mirror of
idocp_rbd_policy_t against the header, the refusal that needs no handle (every other refusal needs one, and a handle needs a device: they are in
test_rbd_policy_gpu.py, as the forward-dynamics tests split theirs), the facade's addition compiles and links, and the numpy referee of the torques
(rbd_policy.reference_torques on gen_golden_rbd.difference) against the library's own host subtraction."""
import ctypes as C
import os
import subprocess

import numpy as np

import independent_rbd as IR
import rbd_policy as RP
from helpers import P, ROOT, anymal_model, arr
from idocp_amd import capi
from rbd_batch import random_samples

E_ARG = -1
INCLUDE = os.path.join(ROOT, "include")
CALLS = ("idocp_rbd_feedback_torques_batch", "idocp_rbd_feedback_torques_batch_device", "idocp_rbd_rollout_policy", "idocp_rbd_rollout_policy_device")

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "idocp_hip.h"
#define FIELD(name) printf(#name " %zu %zu\n", offsetof(idocp_rbd_policy_t, name), sizeof(((idocp_rbd_policy_t*)0)->name))
int main(void) {
  printf("sizeof %zu\n", sizeof(idocp_rbd_policy_t));
  FIELD(u_ff); FIELD(K); FIELD(q_ref); FIELD(v_ref); FIELD(u_min); FIELD(u_max); FIELD(shared_gains); FIELD(shared_ref);
  return 0;
}
"""


def test_symbols_are_exported_and_the_mirror_matches_the_header(tmp_path):
    r = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in r.stdout.splitlines() if line.strip()}
    assert set(CALLS) <= exported, set(CALLS) - exported
    lib = capi.lib()
    for name in CALLS:
        assert getattr(lib, name).restype is C.c_int and len(getattr(lib, name).argtypes) == (6 if "torques" in name else 14), name
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    r = subprocess.run(["gcc", "-std=c99", "-I" + INCLUDE, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(lines[0].split()[1]) == C.sizeof(capi.RbdPolicy)
    fields = [x.split() for x in lines[1:] if x]
    assert [x[0] for x in fields] == [name for name, _ in capi.RbdPolicy._fields_]      # (the order of the struct)
    for name, offset, size in fields:
        d = getattr(capi.RbdPolicy, name)
        assert (d.offset, d.size) == (int(offset), int(size)), name


def test_null_handle_is_an_argument_error_that_names_the_call():
    lib = capi.lib()
    pol = capi.RbdPolicy()
    act = (C.c_int * 4)(1, 1, 1, 1)
    x = np.zeros(19)
    for name in CALLS[:2]:
        assert getattr(lib, name)(None, 1, x.ctypes.data, x.ctypes.data, C.byref(pol), x.ctypes.data) == E_ARG
        assert name.encode() in lib.idocp_last_error()
    for name in CALLS[2:]:
        assert getattr(lib, name)(None, 1, 1, act, 0.05, 0.01, C.byref(pol), None, None, None, None, None, None, 1) == E_ARG
        assert name.encode() in lib.idocp_last_error()


def test_facade_addition_compiles_and_links_without_gpu(tmp_path):
    exe = str(tmp_path / "closed_loop_surface")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + INCLUDE, os.path.join(ROOT, "tests/cpp/closed_loop_surface.cpp"),
                        "-L" + os.path.join(ROOT, "idocp_amd/lib"), "-lidocp_hip", "-Wl,-rpath," + os.path.join(ROOT, "idocp_amd/lib"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "closed loop surface: ok" in r.stdout, r.stdout + r.stderr


def test_referee_torques_agree_with_the_library_subtraction():
    """50 random ANYmal pairs (relative base rotation up to 2 rad, as the GPU tests draw them).  reference_torques with gains that SELECT rows of the
    state difference returns q (-) q_ref and v - v_ref themselves: held to idocp_model_subtract_configuration at the bar of test_model_lie_host.py
    (1e-12 absolute), so the referee the GPU tests use is the library's own definition of the tangent."""
    m = anymal_model()
    M = IR.model_from_struct(m)
    lib = capi.lib()
    rng = np.random.default_rng(2024)
    n, nv, nu = 50, m.nv, m.nu
    q_ref, v_ref = random_samples(rng, n)[:2]
    q, v = RP.perturbed_configurations(M, rng, q_ref), rng.uniform(-1, 1, (n, nv))
    worst = 0.0
    for i in range(n):
        want = np.zeros(nv)
        capi.check(lib.idocp_model_subtract_configuration(C.byref(m), P(arr(q[i])), P(arr(q_ref[i])), P(want)), "subtract")
        want = np.concatenate([want, v[i] - v_ref[i]])
        got = np.zeros(2 * nv)
        for block in range(3):                      # nu = 12 rows of the 36 at a time
            S = np.zeros((nu, 2 * nv))
            S[np.arange(nu), block * nu + np.arange(nu)] = 1.0
            got[block * nu:(block + 1) * nu] = RP.reference_torques(M, q[i], v[i], None, S.T.reshape(-1), q_ref[i], v_ref[i])
        worst = max(worst, np.abs(got - want).max())
        assert np.linalg.norm(want[3:6]) <= 2.0 + 1e-9
    print("referee torques against idocp_model_subtract_configuration: %.2e" % worst)
    assert worst <= 1e-12, worst
    # u_ff, the gains' layout (column-major nu x 2 nv) and the clamp, on numbers that can be checked by hand
    K = np.zeros((nu, 2 * nv))
    K[2, nv + 7] = 3.0                              # u[2] += 3 (v[7] - v_ref[7])
    u = RP.reference_torques(M, q_ref[0], v[0], np.arange(nu, dtype=float), K.T.reshape(-1), q_ref[0], v_ref[0], u_min=np.full(nu, 1.0), u_max=np.full(nu, 10.5))
    want = np.arange(nu, dtype=float)
    want[2] += 3.0 * (v[0][7] - v_ref[0][7])
    assert np.array_equal(u, np.clip(want, 1.0, 10.5))
