"""The fixed-base solvers on revolute arms of 2 .. 8 joints other than iiwa14, on the GPU against the oracle: random chains
(random unit axes, placements, masses, inertias; some with every axis +z for the ZAX sweep) and the committed six-joint arm.
Bar: 1e-10 on the Newton direction, as for iiwa14 (tests/test_unocp_gpu.py, tests/test_unparnmpc_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from arm_chains import ARM6_URDF, arm6_model, random_arm, task_cost
from helpers import (DIR_FIELDS, SOL_FIELDS, HipUnOCP, HipUnParNMPC, OracleUnOCP, OracleUnParNMPC, P, arr, oracle, rel_err,
                     unocp_problem)
from idocp_amd import capi

pytestmark = pytest.mark.gpu
TOL = 1e-10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = tuple("new_" + f for f in ("lmd", "gmm", "a", "q", "v"))
# (nv, seed, every axis +z)
CHAINS = [(nv, 1, False) for nv in range(2, 9)] + [(6, 5, True), (3, 4, True)]


def unocp_pair(m, N, T, batch=1, q0=0.5, cost=None):
    c, cons = unocp_problem(m)
    cost = c if cost is None else cost
    o, g = OracleUnOCP(m, cost, cons, T, N), HipUnOCP(m, cost, cons, T, N, batch=batch)
    q, v = np.full(m.nv, q0), np.zeros(m.nv)
    for s in (o, g):
        s.set_solution("q", q)
        s.set_solution("v", v)
    return o, g, q, v


def oracle_rnea_derivatives(m, q, v, a):
    nv = m.nv
    d0, d1, d2 = np.zeros((nv, nv)), np.zeros((nv, nv)), np.zeros((nv, nv))
    oracle().oracle_rnea_derivatives(C.byref(m), P(arr(q)), P(arr(v)), P(arr(a)), None, 1, P(d0), P(d1), P(d2))
    return d0, d1, d2


def check_rnea_derivatives(m, n, seed):
    nv = m.nv
    rng = np.random.default_rng(seed)
    q, v, a = arr(rng.uniform(-2.5, 2.5, (n, nv))), arr(rng.uniform(-3, 3, (n, nv))), arr(rng.uniform(-5, 5, (n, nv)))
    tau, dq, dv, da = np.zeros((n, nv)), np.zeros((n, nv, nv)), np.zeros((n, nv, nv)), np.zeros((n, nv, nv))
    capi.check(capi.lib().idocp_rnea_derivatives(C.byref(m), n, P(q), P(v), P(a), P(tau), P(dq), P(dv), P(da), 0))
    t0 = np.zeros(nv)
    for i in range(n):
        oracle().oracle_rnea(C.byref(m), P(q[i]), P(v[i]), P(a[i]), None, 1, P(t0))
        d0, d1, d2 = oracle_rnea_derivatives(m, q[i], v[i], a[i])
        assert rel_err(tau[i], t0) < 1e-12, i
        assert rel_err(dq[i], d0) < 1e-12 and rel_err(dv[i], d1) < 1e-12 and rel_err(da[i], d2) < 1e-12, i


@pytest.mark.parametrize("nv,seed,zaxes", CHAINS)
def test_rnea_derivatives_vs_oracle(tmp_path, nv, seed, zaxes):
    # 37 samples: a ragged last wavefront for every chain length
    check_rnea_derivatives(random_arm(nv, seed, tmp_path, zaxes), 37, nv)


def test_rnea_derivatives_six_joint_arm():
    m = arm6_model()
    assert m.nv == 6
    check_rnea_derivatives(m, 23, 6)


@pytest.mark.parametrize("nv,seed,zaxes", CHAINS)
def test_unocp_first_iteration_parity(tmp_path, nv, seed, zaxes):
    m = random_arm(nv, seed, tmp_path, zaxes)
    o, g, q, v = unocp_pair(m, 20, 1.0)
    e_o, e_g = o.kkt_error(0.0, q, v), g.kkt_error(0.0, q, v)
    assert abs(e_g[0] - e_o) < 1e-10 * max(1.0, e_o)
    assert o.update(0.0, q, v) == 0 and g.update(0.0, q, v) == 0
    for f in DIR_FIELDS:
        assert rel_err(g.direction(f), o.direction(f)) < TOL, f
    ao, bo = o.step_sizes()
    ag, bg = g.step_sizes()
    assert abs(ag[0] - ao) < 1e-10 and abs(bg[0] - bo) < 1e-10
    for f in SOL_FIELDS:
        assert rel_err(g.solution(f), o.solution(f)) < TOL, f
    Po, so, Ko, ko = o.riccati()
    Pg, sg, Kg, kg = g.riccati()
    assert rel_err(Pg, Po) < TOL and rel_err(sg, so) < TOL and rel_err(Kg, Ko) < TOL and rel_err(kg, ko) < TOL
    sl_o, du_o = o.constraint_data()
    sl_g, du_g = g.constraint_data()
    assert rel_err(sl_g, sl_o) < TOL and rel_err(du_g, du_o) < TOL
    e_o, e_g = o.kkt_error(0.0, q, v), g.kkt_error(0.0, q, v)
    assert abs(e_g[0] - e_o) < 1e-10 * max(1.0, e_o)


def test_unocp_torque_feedback_gain_six_joint_arm():
    # du = (dID/dq + M Ka_q) dq + (dID/dv + M Ka_v) dv, with the derivatives at the iterate the update linearised (q0, 0, 0)
    m = arm6_model()
    nv = m.nv
    o, g, q, v = unocp_pair(m, 10, 0.5)
    assert o.update(0.0, q, v) == 0 and g.update(0.0, q, v) == 0
    _, _, Ko, _ = o.riccati()
    d0, d1, d2 = oracle_rnea_derivatives(m, q, np.zeros(nv), np.zeros(nv))
    for stage in (0, 4, 9):
        Kq, Kv = np.zeros((nv, nv)), np.zeros((nv, nv))
        capi.check(g.lib.idocp_unocp_get_torque_feedback_gain(g.h, 0, stage, P(Kq), P(Kv)))
        assert rel_err(Kq.T, d0 + d2 @ Ko[stage][:, :nv]) < TOL, stage
        assert rel_err(Kv.T, d1 + d2 @ Ko[stage][:, nv:]) < TOL, stage


def check_trial_points(o, g, q, v):
    """UnLineSearch's cost / violation at trial steps of the state the line search sees (direction and step sizes computed, iterate
    not yet updated), then the update completed on both sides"""
    for what in (0, 1, 2):
        assert o.stage(what, 0.0, q, v) == 0
    for kid in (0, 1, 2, 3, 4):
        g.launch(kid, q, v)
    amax = o.step_sizes()[0]
    for alpha in (0.0, 0.5 * amax, amax):
        co, vo = o.cost_and_violation(alpha)
        cg, vg = g.cost_and_violation(alpha)
        assert abs(cg[0] - co) < 1e-10 * max(1.0, abs(co)) and abs(vg[0] - vo) < 1e-10 * max(1.0, vo), (alpha, cg, co, vg, vo)
        assert cg[0] == cg[-1] and vg[0] == vg[-1]
    assert o.stage(3, 0.0, q, v) == 0
    g.launch(5, q, v)


@pytest.mark.parametrize("nv,seed", [(6, 1), (8, 1), (2, 1)])
def test_unocp_filter_line_search_parity(tmp_path, nv, seed):
    m = random_arm(nv, seed, tmp_path)
    o, g, q, v = unocp_pair(m, 20, 1.0, batch=2)
    for it in range(8):
        assert o.update(0.0, q, v, line_search=True) == 0 and g.update(0.0, q, v, line_search=True) == 0
        ao, _ = o.step_sizes()
        ag, _ = g.step_sizes()
        assert abs(ag[0] - ao) < 1e-9 and ag[0] == ag[1], (it, ag, ao)
        for f in ("q", "v", "a", "u"):
            assert rel_err(g.solution(f), o.solution(f)) < 1e-8, (it, f)


@pytest.mark.parametrize("dim", [3, 6])
def test_unocp_task_space_cost_on_the_six_joint_arm(dim):
    m = arm6_model()
    for joint in (m.njoints - 1, 3):
        cost, _ = unocp_problem(m)
        task_cost(cost, m, dim, joint=joint)
        o, g, q, v = unocp_pair(m, 20, 1.0, cost=cost)
        e_o, e_g = o.kkt_error(0.0, q, v), g.kkt_error(0.0, q, v)
        assert abs(e_g[0] - e_o) < 1e-10 * max(1.0, e_o)
        assert o.update(0.0, q, v) == 0 and g.update(0.0, q, v) == 0
        for f in DIR_FIELDS:
            assert rel_err(g.direction(f), o.direction(f)) < TOL, (joint, f)
        ao, _ = o.step_sizes()
        ag, _ = g.step_sizes()
        assert abs(ag[0] - ao) < 1e-10
        check_trial_points(o, g, q, v)      # (the task-space terms of the trial points: un_line_search_kernel, un_task_terminal_kernel)


def test_unocp_task_space_cost_on_an_eight_joint_chain(tmp_path):
    # eight joints with a task-space cost: the two-round form of the linearisation kernel
    m = random_arm(8, 1, tmp_path)
    cost, _ = unocp_problem(m)
    task_cost(cost, m, 6)
    o, g, q, v = unocp_pair(m, 20, 1.0, cost=cost)
    assert o.update(0.0, q, v) == 0 and g.update(0.0, q, v) == 0
    for f in DIR_FIELDS:
        assert rel_err(g.direction(f), o.direction(f)) < TOL, f


@pytest.mark.parametrize("nv,seed", [(6, 1), (8, 1), (3, 2)])
def test_unocp_batch_instances_are_independent(tmp_path, nv, seed):
    m = random_arm(nv, seed, tmp_path)
    cost, cons = unocp_problem(m)
    rng = np.random.default_rng(nv)
    B, N = 7, 11                              # ragged: batch * N fills no wavefront of any kernel exactly
    q0 = 0.5 + 0.3 * rng.uniform(-1, 1, (B, nv))
    v0 = 0.2 * rng.uniform(-1, 1, (B, nv))
    g = HipUnOCP(m, cost, cons, 0.55, N, batch=B)
    g.set_solution_batch("q", q0)
    g.set_solution_batch("v", v0)
    assert g.update(0.0, q0, v0) == 0
    for b in (0, 3, B - 1):
        o = OracleUnOCP(m, cost, cons, 0.55, N)
        o.set_solution("q", q0[b])
        o.set_solution("v", v0[b])
        assert o.update(0.0, q0[b], v0[b]) == 0
        for f in DIR_FIELDS:
            assert rel_err(g.direction(f, b), o.direction(f)) < TOL, (b, f)


@pytest.mark.parametrize("which", ["arm6", "random2", "random3", "random6"])
def test_unocp_converges_where_the_oracle_does(tmp_path, which):
    m = arm6_model() if which == "arm6" else random_arm(int(which[-1]), 1, tmp_path)
    o, g, q, v = unocp_pair(m, 20, 1.0, batch=2)
    for it in range(30):
        assert o.update(0.0, q, v) == 0 and g.update(0.0, q, v) == 0
        if it < 2:
            for f in DIR_FIELDS:
                assert rel_err(g.direction(f), o.direction(f)) < (TOL if it == 0 else 1e-9), (it, f)
    e_o, e_g = o.kkt_error(0.0, q, v), g.kkt_error(0.0, q, v)
    assert e_o < 1e-8 and e_g[0] < 1e-8 and e_g[1] == e_g[0], (e_o, e_g)
    for f in ("q", "v", "a", "u"):
        assert rel_err(g.solution(f), o.solution(f)) < 1e-6, f


def unparnmpc_pair(m, N, T, batch=1, q0=0.5):
    cost, cons = unocp_problem(m)
    o, g = OracleUnParNMPC(m, cost, cons, T, N), HipUnParNMPC(m, cost, cons, T, N, batch=batch)
    q, v = np.full(m.nv, q0), np.zeros(m.nv)
    for s in (o, g):
        s.set_solution("q", q)
        s.set_solution("v", v)
        s.init(0.0)
    return o, g, q, v


def compare(o, g, fields, tol, what):
    for f in fields:
        e = rel_err(g.get(f), o.get(f))
        assert e < tol, (what, f, e)


@pytest.mark.parametrize("nv,seed,zaxes", CHAINS)
def test_unparnmpc_phase_by_phase_parity(tmp_path, nv, seed, zaxes):
    m = random_arm(nv, seed, tmp_path, zaxes)
    o, g, q, v = unparnmpc_pair(m, 20, 1.0)
    assert o.stage(0, 0.0, q, v) == 0
    g.phase(0, q, v)
    g.phase(1, q, v)
    compare(o, g, NEW, TOL, "coarse update")
    for k, name in ((1, "backward serial"), (2, "backward parallel"), (3, "forward serial")):
        assert o.stage(k, 0.0, q, v) == 0
        g.phase(k + 1, q, v)
        compare(o, g, NEW, TOL, name)
    assert o.stage(4, 0.0, q, v) == 0
    g.phase(5, q, v)
    compare(o, g, NEW, TOL, "forward parallel")
    compare(o, g, tuple("d" + f for f in SOL_FIELDS), TOL, "direction")
    ao, bo = o.step_sizes()
    ag, bg = g.step_sizes()
    assert abs(ag[0] - ao) < 1e-9 and abs(bg[0] - bo) < 1e-9
    assert o.stage(5, 0.0, q, v) == 0
    g.phase(6, q, v)
    compare(o, g, SOL_FIELDS, TOL, "integrated solution")
    e_o, e_g = o.kkt_error(0.0, q, v), g.kkt_error(0.0, q, v)
    assert abs(e_g[0] - e_o) < 1e-9 * max(1.0, e_o)


@pytest.mark.parametrize("nv,seed", [(6, 1), (8, 1)])
def test_unparnmpc_ragged_batch(tmp_path, nv, seed):
    m = random_arm(nv, seed, tmp_path)
    cost, cons = unocp_problem(m)
    batch, N = 7, 5
    rng = np.random.default_rng(batch)
    q0 = 0.5 + 0.3 * rng.uniform(-1, 1, (batch, nv))
    v0 = 0.1 * rng.uniform(-1, 1, (batch, nv))
    g = HipUnParNMPC(m, cost, cons, 0.25, N, batch=batch)
    g.set_solution_batch("q", q0)
    g.set_solution_batch("v", v0)
    g.init(0.0)
    for _ in range(2):
        assert g.update(0.0, q0, v0) == 0
    for b in (0, batch - 1):
        o = OracleUnParNMPC(m, cost, cons, 0.25, N)
        o.set_solution("q", q0[b])
        o.set_solution("v", v0[b])
        o.init(0.0)
        for _ in range(2):
            assert o.update(0.0, q0[b], v0[b]) == 0
        for f in SOL_FIELDS:
            assert rel_err(g.get("d" + f, b), o.get("d" + f)) < 1e-9, (b, f)


def test_unparnmpc_two_shards_equal_the_whole_horizon_six_joints():
    """two shard handles of 10 stages of the six-joint arm on this GPU, halos of the handle's size, against one handle of 20"""
    import torch
    from parnmpc_dist import AUX_ALL, HipUnParNMPCShard

    class Shard(HipUnParNMPCShard):
        def halo_size(self, kind):
            return 1 if kind == AUX_ALL else self.lib.idocp_unparnmpc_halo_size_of(self.h, kind)

    m = arm6_model()
    nv = m.nv
    o, g, q, v = unparnmpc_pair(m, 20, 1.0)
    cost, cons = unocp_problem(m)
    lib = capi.lib()
    assert lib.idocp_unparnmpc_halo_size_of(g.h, 0) == 2 * nv and lib.idocp_unparnmpc_halo_size_of(g.h, 2) == 4 * nv * nv
    shards = [Shard(m, cost, cons, 1.0, 20, r, 2, 1, 0) for r in range(2)]
    for sh in shards:
        capi.check(lib.idocp_unocp_set_solution(sh.h, b"q", P(arr(q))))
        capi.check(lib.idocp_unocp_set_solution(sh.h, b"v", P(arr(v))))
        sh.phase("init_aux", 0.0)
    s0, s1 = shards
    s0.set_initial_state(q[None, :], v[None, :])

    def boundary():
        s1.import_(0, s0.export(0))
        s0.import_(1, s1.export(1))
        s0.import_(2, s1.export(2))

    def get(sh, name):
        out = np.zeros((11, nv))
        capi.check(lib.idocp_unocp_get_solution(sh.h, name.encode(), 0, P(out)))
        return out[:10]

    for it in range(4):
        assert g.update(0.0, q, v) == 0
        boundary()
        for sh in shards:
            sh.phase("linearize", 0.0)
        s1.phase("bwd_serial", 0.0)
        s0.import_(3, s1.export(3))
        s0.phase("bwd_serial", 0.0)
        for sh in shards:
            sh.phase("bwd_parallel", 0.0)
        s0.phase("fwd_serial", 0.0)
        s1.import_(4, s0.export(4))
        s1.phase("fwd_serial", 0.0)
        for sh in shards:
            sh.phase("fwd_parallel", 0.0)
        steps = torch.minimum(s0.local_steps(), s1.local_steps())
        ag, bg = g.step_sizes()
        assert abs(float(steps[0, 0]) - ag[0]) < 1e-12 and abs(float(steps[0, 1]) - bg[0]) < 1e-12
        for sh in shards:
            sh.set_steps(steps)
            sh.phase("integrate", 0.0)
        for name in SOL_FIELDS:
            both = np.concatenate([get(s0, name), get(s1, name)])
            assert rel_err(both, g.get(name)) < 1e-12, (it, name)


def test_six_joint_example_runs_and_converges():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "arm6_unocp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(ROOT, "examples", "arm6_unocp"), ARM6_URDF], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    init = float(re.search(r"Initial KKT error = ([-+0-9.eE]+|nan|inf)", r.stdout).group(1))
    its = [float(x) for x in re.findall(r"KKT error after iteration \d+ = ([-+0-9.eE]+|nan|inf)", r.stdout)]
    assert len(its) == 30 and "CPU time per update" in r.stdout
    # the same problem through the oracle
    m = arm6_model()
    o, _, q, v = unocp_pair(m, 20, 1.0)
    ref_init = o.kkt_error(0.0, q, v)
    assert abs(init - ref_init) < 1e-5 * max(1.0, ref_init)          # (the driver prints six significant digits)
    ref = []
    for _ in range(30):
        assert o.update(0.0, q, v) == 0
        ref.append(o.kkt_error(0.0, q, v))
    for a, b in zip(its[:3], ref[:3]):
        assert abs(a - b) < 1e-5 * max(1.0, b), (its[:3], ref[:3])
    assert its[-1] < 1e-8 and ref[-1] < 1e-8
