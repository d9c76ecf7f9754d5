"""The yardstick of the sampling calls without a GPU.

1. idocp_amd/csrc/rbd_sampler.hpp -- the text the perturbation kernel compiles -- as a stand-alone program under the address and undefined-behaviour
   sanitizers (tests/cpp/rbd_sampler_host.cpp): Philox4x32-10 against the published known-answer vectors, the uniform conversion at its end points,
   and a table of words and uniforms that the Python referee of tests/rbd_sample.py must reproduce bit for bit.
2. The referee's normals over 65 536 draws along each axis of the counter (sample, step, torque, draw): mean, variance and lag-one correlation
   within five standard deviations of their sampling error -- 5 / sqrt(N), 5 sqrt(2 / N), 5 / sqrt(N).  Derived bounds on a fixed sequence, not
   measured ones.
3. The six calls exist, the mirror matches the header, and the refusals that need no device are pinned to their full text."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import rbd_sample as RS
from helpers import ROOT
from idocp_amd import capi

N = 65536
CALLS = ("idocp_rbd_perturb_torques", "idocp_rbd_importance_weights", "idocp_rbd_weighted_mean")


@pytest.fixture(scope="module")
def sampler_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rbd_sampler") / "rbd_sampler_host")
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "idocp_amd/csrc"), os.path.join(ROOT, "tests/cpp/rbd_sampler_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rbd sampler: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_philox_known_answers_and_uniform_end_points_under_the_sanitizers(sampler_program):
    assert "FAIL" not in sampler_program


def test_referee_philox_known_answers():
    ones = 0xFFFFFFFF
    assert RS.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert RS.philox4x32_10((ones,) * 4, (ones,) * 2) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert RS.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    assert RS.uniforms((0, 0, 0, 0)) == (2.0 ** -53, 0.0)
    assert RS.uniforms((ones,) * 4) == (1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53)


def test_referee_matches_the_kernels_header_bit_for_bit(sampler_program):
    rows = [line.split()[1:] for line in sampler_program.splitlines() if line.startswith("table ")]
    assert len(rows) == 3 * 2 * 3 * 4 * 3
    for seed, draw, step, i, pair, r0, r1, r2, r3, b1, b2 in rows:
        got = RS.words(int(seed), int(draw), int(step), int(i), int(pair))
        assert got == tuple(int(x, 16) for x in (r0, r1, r2, r3)), (seed, draw, step, i, pair)
        u1, u2 = RS.uniforms(got)
        assert struct.pack("<d", u1) == int(b1, 16).to_bytes(8, "little") and struct.pack("<d", u2) == int(b2, 16).to_bytes(8, "little")


@pytest.mark.parametrize("axis", ["sample", "step", "torque", "draw"])
def test_referee_normals_have_the_moments_of_a_standard_normal(axis):
    seed = 20260101
    if axis == "sample":
        x = [RS.z(seed, 3, 5, i, 4) for i in range(1, N + 1)]
    elif axis == "step":
        x = [RS.z(seed, 3, k, 17, 4) for k in range(N)]
    elif axis == "torque":
        x = [RS.z(seed, 3, 5, 17, j) for j in range(N)]      # (cosine and sine of one pair are neighbours here)
    else:
        x = [RS.z(seed, d, 5, 17, 4) for d in range(N)]
    x = np.array(x)
    mean, var = x.mean(), x.var()
    lag = float(np.mean((x[:-1] - mean) * (x[1:] - mean)) / var)
    print("%s: mean %.5f var %.5f lag-one correlation %.5f max |z| %.3f" % (axis, mean, var, lag, np.abs(x).max()))
    assert abs(mean) <= 5.0 / math.sqrt(N)
    assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / N)
    assert abs(lag) <= 5.0 / math.sqrt(N)
    assert np.abs(x).max() <= RS.Z_MAX


def test_sample_zero_is_the_nominal_and_the_largest_normal_is_bounded():
    assert RS.z(1, 2, 3, 0, 4) == 0.0 and RS.z(1, 2, 3, 0, 5) == 0.0
    rho = math.sqrt(-2.0 * math.log(RS.uniforms((0, 0, 0, 0))[0]))
    assert rho == pytest.approx(RS.Z_MAX, rel=1e-15) and 8.57 < RS.Z_MAX < 8.58


def test_the_calls_exist_and_the_mirror_matches_the_header():
    lib = capi.lib()
    text = open(os.path.join(ROOT, "include", "idocp_hip.h")).read()
    for name in CALLS:
        for form in ("", "_device"):
            assert hasattr(lib, name + form)
            assert re.search(r"\bint %s%s\(" % (name, form), text)
            assert getattr(lib, name + form).argtypes is not None
    for macro, value in (("IDOCP_RBD_REDUCE_CHUNK", capi.RBD_REDUCE_CHUNK), ("IDOCP_RBD_WEIGHT_STATS", capi.RBD_WEIGHT_STATS),
                         ("IDOCP_RBD_MEAN_MAX_COLUMNS", capi.RBD_MEAN_MAX_COLUMNS)):
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == value
    assert capi.RBD_WEIGHT_STATS == 5 and 1 <= capi.RBD_MEAN_MAX_COLUMNS == 64
    # the argument lists, by count and by the two integer arguments of the seed
    assert len(lib.idocp_rbd_perturb_torques.argtypes) == 11 and len(lib.idocp_rbd_importance_weights.argtypes) == 8
    assert len(lib.idocp_rbd_weighted_mean.argtypes) == 7
    import ctypes as C
    assert lib.idocp_rbd_perturb_torques_device.argtypes[8:10] == [C.c_ulonglong, C.c_uint]


def test_refusals_without_a_device_are_pinned_to_their_text():
    """no CPU fallback: without a GPU there is no handle, so all a call can do here is refuse"""
    lib = capi.lib()
    x = np.zeros(4)
    p = x.ctypes.data
    for form in ("", "_device"):
        assert getattr(lib, "idocp_rbd_perturb_torques" + form)(None, 1, 0, 1, p, p, None, None, 0, 0, p) == -1
        assert lib.idocp_last_error() == b"idocp_rbd_perturb_torques" + form.encode() + b": null handle"
        assert getattr(lib, "idocp_rbd_importance_weights" + form)(None, 1, p, None, 0.0, 1.0, p, p) == -1
        assert lib.idocp_last_error() == b"idocp_rbd_importance_weights" + form.encode() + b": null handle"
        assert getattr(lib, "idocp_rbd_weighted_mean" + form)(None, 1, 1, 1, p, p, p) == -1
        assert lib.idocp_last_error() == b"idocp_rbd_weighted_mean" + form.encode() + b": null handle"
