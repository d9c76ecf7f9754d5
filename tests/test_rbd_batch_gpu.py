"""The batched rigid-body API (idocp_rbd_*, include/idocp_hip.h; rbd_batch_kernel.hip) on the GPU: inverse dynamics with contact forces, the
Baumgarte / impulse-velocity terms, their derivatives and MJtJinv for many samples in one call -- against the independent vectors of tests/golden
(the bar test_golden_rbd_gpu.py holds the stage kernels to), against the oracle on quadrupeds that are not ANYmal, on partial contact sets, with
selected outputs, through device pointers, on fixed-base chains (bit for bit what idocp_rnea_derivatives gives) and through the facade's Robot."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from arm_chains import arm6_model
from helpers import GOLDEN, ROOT, P, anymal_model, arr, iiwa14_model, oracle, rel_err
from idocp_amd import capi
from rbd_batch import (ALL_OUTPUTS, E_ARG, IMPULSE, STAGE, DeviceArray, Rbd, oracle_terms, out_shapes, packed_mjtjinv,      # noqa: F401
                       random_samples)
from test_other_quadrupeds_gpu import other_quadruped

pytestmark = pytest.mark.gpu
NV, NQ, NF = 18, 19, 12
ALL = [1, 1, 1, 1]


def golden(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)["samples"]


def stack(samples, key):
    return np.array([np.asarray(s[key], dtype=np.float64) for s in samples])


def test_stage_terms_against_the_independent_vectors():
    """rbd_anymal.json (tau and its derivatives with four contact forces) and contact_anymal.json (Baumgarte terms, MJtJinv): one call each."""
    r = Rbd(anymal_model())
    s = golden("rbd_anymal.json")
    o = r.call(STAGE, stack(s, "q"), stack(s, "v"), stack(s, "a"), ALL, 0.05, f=stack(s, "f"), outputs=("tau", "dtau_dq", "dtau_dv", "dtau_da"))
    errs = {k: rel_err(o[k], stack(s, k)) for k in ("tau", "dtau_dq", "dtau_dv", "dtau_da")}
    print("rbd_anymal.json, STAGE:", errs)
    assert max(errs.values()) < 1e-11, errs
    s = golden("contact_anymal.json")
    dts = {x["time_step"] for x in s}
    assert len(dts) == 1                                   # (one time step for the call)
    o = r.call(STAGE, stack(s, "q"), stack(s, "v"), stack(s, "a"), ALL, dts.pop(), contact_points=stack(s, "contact_points"))
    errs = {k: rel_err(o[k], stack(s, k)) for k in ("C", "dCdq", "dCdv", "dCda")}
    errs["MJtJinv"] = rel_err(np.array([packed_mjtjinv(x, NV, NF) for x in o["MJtJinv"]]), stack(s, "MJtJinv"))
    print("contact_anymal.json, STAGE:", errs)
    assert max(errs.values()) < 1e-11, errs


def test_impulse_terms_against_the_independent_vectors():
    r = Rbd(anymal_model())
    s = golden("rbd_anymal.json")
    o = r.call(IMPULSE, stack(s, "q"), stack(s, "v"), stack(s, "a"), ALL, 0.0, f=stack(s, "f"), outputs=("tau", "dtau_dq", "dtau_dv", "dtau_da"))
    errs = (rel_err(o["tau"], stack(s, "tau_impulse")), rel_err(o["dtau_dq"], stack(s, "dimp_dq")), rel_err(o["dtau_da"], stack(s, "dimp_ddv")))
    print("rbd_anymal.json, IMPULSE:", errs)
    assert max(errs) < 1e-11, errs
    assert (o["dtau_dv"] == 0).all()


NMAX = 130


@pytest.fixture(scope="module", params=[0, 1, 2])
def other(request):
    """model, samples and the oracle's answers for them, computed once per seed"""
    m, rng = other_quadruped(request.param)
    q, v, a, f, pts = random_samples(rng, NMAX)
    dt = 0.04
    ref = [oracle_terms(oracle(), m, q[i], v[i], a[i], f[i], pts[i], dt) for i in range(NMAX)]
    stage = {k: np.array([x[0][k] for x in ref]) for k in ref[0][0]}
    imp = {k: np.array([x[1][k] for x in ref]) for k in ref[0][1]}
    return m, (q, v, a, f, pts, dt), stage, imp


@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_other_quadrupeds_against_the_oracle(other, n):
    m, (q, v, a, f, pts, dt), stage, imp = other
    r = Rbd(m)
    o = r.call(STAGE, q[:n], v[:n], a[:n], ALL, dt, f=f[:n], contact_points=pts[:n])
    o["MJtJinv"] = np.array([packed_mjtjinv(x, NV, NF) for x in o["MJtJinv"]])
    errs = {k: rel_err(o[k], stage[k][:n]) for k in stage}
    print("STAGE n=%d:" % n, errs)
    for k, e in errs.items():
        if k != "MJtJinv":
            assert e < 1e-10, (k, e)
    if not errs["MJtJinv"] < 1e-10:
        # the referee rule of the project: at most four times as far from the long-double answer as the FP64 oracle
        hp = oracle(hp=True)
        for i in range(n):
            if rel_err(o["MJtJinv"][i], stage["MJtJinv"][i]) < 1e-10:
                continue
            ref = oracle_terms(hp, m, q[i], v[i], a[i], f[i], pts[i], dt)[0]["MJtJinv"]
            d_gpu, d_oracle = rel_err(o["MJtJinv"][i], ref), rel_err(stage["MJtJinv"][i], ref)
            print("MJtJinv sample %d: GPU %.3e, FP64 oracle %.3e from the long-double oracle" % (i, d_gpu, d_oracle))
            assert d_gpu <= 4.0 * d_oracle, (i, d_gpu, d_oracle)
    o = r.call(IMPULSE, q[:n], v[:n], a[:n], ALL, 0.0, f=f[:n])
    errs = {k: rel_err(o[k], imp[k][:n]) for k in imp}
    errs["dCda"] = rel_err(o["dCda"], imp["dCdv"][:n])
    print("IMPULSE n=%d:" % n, errs)
    assert max(errs.values()) < 1e-10, errs
    assert (o["dtau_dv"] == 0).all()


@pytest.mark.parametrize("mask", [[1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 0, 0]])
def test_partial_contact_sets(mask):
    m = anymal_model()
    rng = np.random.default_rng(11)
    n = 5
    q, v, a, f, pts = random_samples(rng, n)
    r = Rbd(m)
    full = r.call(STAGE, q, v, a, ALL, 0.03, f=f * np.array(mask)[None, :, None], contact_points=pts)
    part = r.call(STAGE, q, v, a, mask, 0.03, f=f, contact_points=pts)
    assert rel_err(part["tau"], full["tau"]) < 1e-12
    rows = np.repeat(np.array(mask, dtype=bool), 3)
    for k in ("C", "dCdq", "dCdv", "dCda"):
        x, y = part[k], full[k]
        assert np.array_equal(x[:, rows], y[:, rows]), k
        assert (x[:, ~rows] == 0).all(), k
    dimf = int(rows.sum())
    for i in range(n):
        M, J = part["dtau_da"][i], part["dCda"][i][rows]
        K = np.block([[M, J.T], [J, np.zeros((dimf, dimf))]])
        Kinv = packed_mjtjinv(part["MJtJinv"][i], NV, dimf)
        assert rel_err(Kinv @ K, np.eye(NV + dimf)) < 1e-9
        if dimf == 0:
            assert rel_err(Kinv, np.linalg.inv(M)) < 1e-9


def test_selected_outputs_and_device_pointers():
    m = anymal_model()
    rng = np.random.default_rng(12)
    n = 7
    q, v, a, f, pts = random_samples(rng, n)
    r = Rbd(m)
    host = r.call(STAGE, q, v, a, ALL, 0.05, f=f, contact_points=pts, fill=0.0)
    shapes = out_shapes(m)
    POISON = -7.25
    d_in = {k: DeviceArray(x) for k, x in (("q", q), ("v", v), ("a", a), ("f", f), ("contact_points", pts))}
    d_out = {k: DeviceArray(np.full((n,) + shapes[k], POISON)) for k in ALL_OUTPUTS}
    # only tau requested: nothing else is written
    io = capi.RbdIO()
    for k, t in d_in.items():
        setattr(io, k, t.ptr)
    io.tau = d_out["tau"].ptr
    assert r.call_raw(STAGE, n, ALL, 0.05, io, device=True) == 0, capi.last_error()
    assert r.lib.idocp_rbd_synchronize(r.h) == 0
    assert np.array_equal(d_out["tau"].numpy(), host["tau"])
    for k in ALL_OUTPUTS[1:]:
        assert (d_out[k].numpy() == POISON).all(), k
    # the same through the host form: a call that asks for tau alone gives the same tau
    assert np.array_equal(r.call(STAGE, q, v, a, ALL, 0.05, f=f, contact_points=pts, outputs=("tau",))["tau"], host["tau"])
    # every output through device pointers: bit for bit the host form
    for k, t in d_out.items():
        setattr(io, k, t.ptr)
    assert r.call_raw(STAGE, n, ALL, 0.05, io, device=True) == 0, capi.last_error()
    assert r.lib.idocp_rbd_synchronize(r.h) == 0
    for k in ALL_OUTPUTS:
        x = d_out[k].numpy()
        if k == "MJtJinv":
            assert np.array_equal(x, host[k]), k                  # (all four contacts: the packed block fills the slot)
        else:
            assert np.array_equal(x.transpose(0, 2, 1) if x.ndim == 3 else x, host[k]), k
    # a copy of a result inside device memory (idocp_device_copy) holds the same numbers
    copy = DeviceArray(np.zeros((n,) + shapes["dCda"]))
    capi.check(r.lib.idocp_device_copy(copy.ptr, d_out["dCda"].ptr, copy.nbytes), "idocp_device_copy")
    assert np.array_equal(copy.numpy().transpose(0, 2, 1), host["dCda"])
    # an output without the input it needs
    io.contact_points = None
    CALL = b"idocp_rbd_contact_dynamics_batch"               # (the device form reports under the same name)

    def refused(rc, text):
        assert rc == E_ARG, text
        assert capi.lib().idocp_last_error() == CALL + text

    refused(r.call_raw(STAGE, n, ALL, 0.05, io, device=True), b": C in STAGE mode needs contact_points")
    refused(r.call_raw(2, n, ALL, 0.05, io, device=True), b": unknown mode")
    refused(r.call_raw(STAGE, 0, ALL, 0.05, io, device=True), b": n must be positive")
    # two conditions violated at once: the one tested first is the one reported, by both forms
    for device in (True, False):
        refused(r.call_raw(2, 0, ALL, 0.05, io, device=device), b": n must be positive")
        refused(r.call_raw(2, n, None, 0.05, io, device=device), b": unknown mode")
        refused(r.call_raw(STAGE, n, None, 0.0, io, device=device), b": the contact status `active` is needed")
        refused(r.call_raw(STAGE, n, ALL, 0.0, io, device=device), b": C in STAGE mode needs contact_points")
    io.contact_points = d_in["contact_points"].ptr
    refused(r.call_raw(STAGE, n, ALL, 0.0, io, device=True), b": the Baumgarte terms need a positive time_step")
    io.q = None
    refused(r.call_raw(STAGE, n, ALL, 0.05, io, device=True), b": q, v and a are needed")
    assert r.lib.idocp_rbd_contact_dynamics_batch(r.h, STAGE, n, None, 0.05, None) == E_ARG
    assert capi.lib().idocp_last_error() == CALL + b": null handle or io"


@pytest.mark.parametrize("mode", [STAGE, IMPULSE])
@pytest.mark.parametrize("mask", [ALL, [1, 0, 0, 1]])
def test_subsets_of_the_outputs_are_bit_for_bit_the_full_call(mode, mask):
    """The kernel runs fewer items when no d / dq, d / dv output is wanted (the a seeds and the four nominal items: its own decoding of the item
    index and of the base rows; in the impulse mode the a seeds are the velocity seeds of the kinematic pass), and the four nominal items alone for
    tau / C.  Every such selection gives the numbers of the call that asks for everything, and the 70 samples take the ragged last workgroup."""
    m = anymal_model()
    rng = np.random.default_rng(14)
    n = 70
    q, v, a, f, pts = random_samples(rng, n)
    r = Rbd(m)
    full = r.call(mode, q, v, a, mask, 0.05, f=f, contact_points=pts, fill=0.0)
    for outputs in (("dtau_da", "dCda", "MJtJinv"), ("MJtJinv",), ("dCda",), ("tau", "dtau_da"), ("tau", "C"), ("C",), ("dCdq",), ("dtau_dv", "C")):
        part = r.call(mode, q, v, a, mask, 0.05, f=f, contact_points=pts, outputs=outputs, fill=0.0)
        for k in outputs:
            assert np.array_equal(part[k], full[k]), (outputs, k)


@pytest.mark.parametrize("which", ["iiwa14", "arm6"])
def test_fixed_base_chains_match_idocp_rnea_derivatives_bit_for_bit(which):
    m = iiwa14_model() if which == "iiwa14" else arm6_model()
    nv, n = m.nv, 9
    rng = np.random.default_rng(13)
    q, v, a = rng.uniform(-1, 1, (n, nv)), rng.uniform(-1, 1, (n, nv)), rng.uniform(-2, 2, (n, nv))
    tau, dq, dv, da = np.zeros((n, nv)), np.zeros((n, nv, nv)), np.zeros((n, nv, nv)), np.zeros((n, nv, nv))
    capi.check(capi.lib().idocp_rnea_derivatives(C.byref(m), n, P(arr(q)), P(arr(v)), P(arr(a)), P(tau), P(dq), P(dv), P(da), 0), "idocp_rnea_derivatives")
    r = Rbd(m)
    o = r.call(STAGE, q, v, a, None, 0.0, outputs=("tau", "dtau_dq", "dtau_dv", "dtau_da"))
    assert np.array_equal(o["tau"], tau)
    for k, x in (("dtau_dq", dq), ("dtau_dv", dv), ("dtau_da", da)):
        assert np.array_equal(o[k], x.transpose(0, 2, 1)), k
    # a subset of the outputs: the same numbers
    assert np.array_equal(r.call(STAGE, q, v, a, None, 0.0, outputs=("dtau_dv",))["dtau_dv"], dv.transpose(0, 2, 1))
    # a chain has no contacts
    io = capi.RbdIO()
    bufs = [arr(q), arr(v), arr(a), np.zeros((n, 12))]
    io.q, io.v, io.a, io.C = [b.ctypes.data for b in bufs]
    assert r.call_raw(STAGE, n, None, 0.05, io) == E_ARG
    assert capi.lib().idocp_last_error() == (b"idocp_rbd_contact_dynamics_batch: a fixed-base chain has no contacts "
                                             b"(f, contact_points and the contact outputs must be NULL)")
    io.C = None
    assert r.call_raw(IMPULSE, n, None, 0.05, io) == E_ARG
    assert capi.lib().idocp_last_error() == b"idocp_rbd_contact_dynamics_batch: a fixed-base chain has no impulse mode"


def test_facade_robot_on_the_gpu(tmp_path):
    """tests/cpp/robot_dynamics.cpp: Robot::RNEA, RNEADerivatives, computeBaumgarteResidual / Derivatives on ANYmal with two active contacts --
    the same numbers as the C ABI call, in the reference's packing (active rows only)."""
    exe = os.path.join(str(tmp_path), "robot_dynamics")
    libdir = os.path.join(ROOT, "idocp_amd", "lib")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "robot_dynamics.cpp"), "-o", exe,
                        "-L" + libdir, "-lidocp_hip", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    urdf = os.path.join(GOLDEN, "urdf", "anymal.urdf")
    r = subprocess.run([exe, urdf], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    vals = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(":")
        vals[name.strip()] = np.array([float.fromhex(x) for x in rest.split()])
    m = anymal_model()
    q, v, a, f, pts = vals["q"], vals["v"], vals["a"], vals["f"].reshape(4, 3), vals["points"].reshape(4, 3)
    mask = [int(x) for x in vals["active"]]
    assert sum(mask) == 2
    dt = float(vals["time_step"][0])
    o = Rbd(m).call(STAGE, q[None], v[None], a[None], mask, dt, f=f[None], contact_points=pts[None])
    rows = np.repeat(np.array(mask, dtype=bool), 3)
    assert np.array_equal(vals["tau"], o["tau"][0])
    for k in ("dtau_dq", "dtau_dv", "dtau_da"):
        assert np.array_equal(vals[k].reshape(NV, NV).T, o[k][0]), k          # (printed column-major)
    assert np.array_equal(vals["C"], o["C"][0][rows])
    dimf = int(rows.sum())
    for k in ("dCdq", "dCdv", "dCda"):
        assert np.array_equal(vals[k].reshape(NV, dimf).T, o[k][0][rows]), k
