"""The referee of the contact-frame kinematics (tests/rbd_kinematics.py) and the schedule of the foothold rollout, without a GPU.

The referee's points are held to the host's idocp_model_contact_positions, its world Jacobian to central differences of that call through
idocp_model_integrate_configuration -- the definition include/idocp_hip.h gives (column r = d/d eps points(q (+) eps e_r)).  The schedule header
(idocp_amd/csrc/rbd_foothold_plan.hpp) is held to the rule by a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import independent_rbd as IR
import rbd_forward as F
import rbd_kinematics as K
from helpers import ROOT, anymal_model
from idocp_amd import capi
from test_other_quadrupeds_gpu import other_quadruped

MODELS = ("anymal", 0, 1, 2)
STEP = 1e-6


def model(which):
    return anymal_model() if which == "anymal" else other_quadruped(which)[0]


def integrate(m, q, d, length):
    out = np.zeros(m.nq)
    capi.check(capi.lib().idocp_model_integrate_configuration(C.byref(m), q.ctypes.data, d.ctypes.data, length, out.ctypes.data), "integrate")
    return out


@pytest.mark.parametrize("which", MODELS)
def test_referee_points_and_jacobian_against_the_host_call(which):
    m = model(which)
    M = IR.model_from_struct(m)
    q, v = K.standing_samples(np.random.default_rng(5), 3)
    host = F.foot_positions(m, q)
    for i in range(3):
        ref = K.reference(M, q[i], v[i])
        err = np.abs(ref["points"] - host[i]).max()
        assert err < 1e-13, (which, i, err)
        # central differences of the host call with step h.  Truncation: along a unit tangent one coordinate moves at unit rate, so a point
        # turns about a joint (or the base origin) on a lever L and |p'''| <= L, the error (h^2 / 6) L; the base translations are exact.
        # Rounding: the host's point carries a few ulps of its magnitude P -- the chain is a dozen rotate-and-add steps, 16 ulps is taken --
        # and the difference of two such points is divided by 2 h: 16 eps P / h.  L: twice the largest distance of a foot from the base origin
        # bounds every lever (a joint lies between the two).
        lever = 2 * np.linalg.norm(host[i] - q[i, :3], axis=1).max()
        bar = STEP ** 2 / 6 * lever + 16 * np.finfo(float).eps * max(1.0, np.abs(host[i]).max()) / STEP
        J = np.zeros((12, m.nv))
        for r in range(m.nv):
            e = np.zeros(m.nv)
            e[r] = 1.0
            plus, minus = integrate(m, q[i], e, STEP), integrate(m, q[i], e, -STEP)
            J[:, r] = (F.foot_positions(m, plus[None]) - F.foot_positions(m, minus[None])).reshape(-1) / (2 * STEP)
        err = np.abs(ref["jacobian"] - J).max()
        print("%s sample %d: |J - central differences| = %.2e (bar %.2e)" % (which, i, err, bar))
        assert err < bar, (which, i, err, bar)
        assert np.abs(ref["velocity"].reshape(-1) - ref["jacobian"] @ v[i]).max() < 1e-13


def test_foothold_schedule_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "rbd_foothold_plan")
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "idocp_amd/csrc"), os.path.join(ROOT, "tests/cpp/rbd_foothold_plan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rbd foothold plan: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
