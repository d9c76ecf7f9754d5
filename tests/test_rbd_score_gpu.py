"""The score of a rollout on the GPU (idocp_rbd_objective_*, idocp_rbd_score_rollout; rbd_score_kernel.hip) against the numpy referee of
tests/rbd_score.py, which test_rbd_score_host.py holds to the oracle's line-search cost.  The bar is the project's bar for the rbd calls against numpy,
|gpu - referee| <= 1e-11 max(1, |referee|) per result (independent_rbd.BAR).

Trajectories are random arrays passed straight in (scoring does not ask that they come from a rollout), so violations are placed deliberately.  Shapes:
n in {1, 2, 3, 5} (an odd n ends in a workgroup with an idle wavefront), steps in {1, 2, 7} (7 + the terminal slice: two passes of the four step groups
of a chain wavefront, four of the two of a quadruped's), one case of 70 steps (a second chunk of 64 logarithms).  On the quadrupeds the base is 1.4 to 1.7
rad from its reference (the rotation angle around pi / 2)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import independent_rbd as IR
import rbd_forward as F
import rbd_policy as RP
import rbd_score as RS
from helpers import anymal_model, anymal_problem, running_problem
from idocp_amd import capi
from rbd_batch import E_ARG, E_UNSUPPORTED, DeviceArray, Rbd, random_samples
from test_other_quadrupeds_gpu import other_quadruped

pytestmark = pytest.mark.gpu
BAR = IR.BAR
NMAX, SMAX = 5, 7
DT = 0.02
CHANGING = [[1, 1, 1, 1], [1, 0, 0, 1], [0, 0, 0, 0], [0, 1, 1, 0], [1, 1, 1, 0], [0, 0, 0, 1], [1, 0, 1, 1]]
SCHEDULES = {"none": [[0, 0, 0, 0]] * SMAX, "one": [[0, 0, 1, 0]] * SMAX, "all": [[1, 1, 1, 1]] * SMAX, "changing": CHANGING}


def close(got, want):
    return abs(got - want) <= BAR * max(1.0, abs(want))


def quat_mul(a, b):
    """(x, y, z, w) of a * b"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def no_constraints():
    cons = capi.Constraints()
    capi.lib().idocp_constraints_init(C.byref(cons))
    for name, _ in capi.Constraints._fields_:
        if isinstance(getattr(cons, name), int):
            setattr(cons, name, 0)
    cons.mu = 0.7
    return cons


def all_constraints(m, cone="linearized_friction_cone"):
    cons = no_constraints()
    for name in ("joint_position_limits", "joint_velocity_limits", "joint_torque_limits", "joint_acceleration_lower_limit", "joint_acceleration_upper_limit", cone):
        setattr(cons, name, 1)
    for j in range(m.nu):
        cons.a_min[j], cons.a_max[j] = -1.0 - 0.1 * j, 0.5 + 0.1 * j
    return cons


def with_limits(m):
    """a copy of the model whose joint limits lie INSIDE the ranges the random trajectories are drawn from, so that rows of every kind are active"""
    m = capi.Model.from_buffer_copy(m)
    for j in range(m.nu):
        m.q_min[j], m.q_max[j], m.v_max[j], m.u_max[j] = -0.6 - 0.01 * j, 0.5 + 0.02 * j, 0.4 + 0.03 * j, 6.0 + j
    return m


@functools.lru_cache(maxsize=None)
def case(which, kind="constant"):
    """(model, generator's model, cost, t0, random slices for NMAX samples and SMAX steps + the terminal slice)"""
    if isinstance(which, str) and which.startswith("chain"):
        nv = int(which[5:])
        m, M = IR.chain(nv, 1)
        m = with_limits(m)
        rng = np.random.default_rng([71, nv])
        cost = capi.Cost()
        cost.set("q_ref", rng.uniform(-1, 1, nv)).set("v_ref", rng.uniform(-1, 1, nv)).set("u_ref", rng.uniform(-1, 1, nv))
        for name in ("q_weight", "v_weight", "a_weight", "u_weight", "qf_weight", "vf_weight"):
            cost.set(name, rng.uniform(0.1, 10, nv))
        q = rng.uniform(-2.5, 2.5, (SMAX + 1, NMAX, nv))
        f, t0 = None, 0.3
    else:
        if which == "anymal":
            base, rng = anymal_model(), np.random.default_rng(41)
        else:
            base, rng = other_quadruped(which)
        m = with_limits(base)
        M = IR.model_from_struct(m)
        if kind == "time_varying":
            cost, _ = running_problem(m, steps=1)
            cost.tv_t_begin, cost.tv_t_end = 1.0, 1.0 + 3.5 * DT      # steps 0, 1 before / on t_begin ... the last ones beyond t_end
            cost.v_ref[5] = 0.7
            t0 = 1.0 - DT
        else:
            cost, _ = anymal_problem(m, trotting_ref=kind == "trotting")
            t0 = 1.0 - 3.5 * DT                                     # trotting: the period boundary t = 1.0 lies inside the window
        cost.set("u_weight", np.linspace(0.01, 0.02, m.nu)).set("u_ref", np.linspace(-1.0, 1.0, m.nu))
        for c in range(4):
            for x in range(3):
                cost.f_weight[c][x] = 0.001 * (1 + c + x)
        q_tab = RS.reference_tables(M, cost, t0, DT, SMAX)[0]
        q = np.zeros((SMAX + 1, NMAX, m.nq))
        for k in range(SMAX + 1):
            for i in range(NMAX):
                d = rng.uniform(-0.9, 0.9, m.nv)
                ax = rng.normal(size=3)
                d[:3], d[3:6] = rng.uniform(-0.3, 0.3, 3), ax / np.linalg.norm(ax) * rng.uniform(1.4, 1.7)
                q[k, i] = F.RBD.integrate(M, q_tab[k], d)
        f = rng.uniform(-30, 30, (SMAX, NMAX, 4, 3))
        f[..., 2] = rng.uniform(-5, 60, (SMAX, NMAX, 4))
    x = dict(q=q, v=rng.uniform(-1, 1, (SMAX + 1, NMAX, m.nv)), u=rng.uniform(-12, 12, (SMAX, NMAX, m.nu)), a=rng.uniform(-2, 2, (SMAX, NMAX, m.nv)), f=f)
    return m, M, cost, t0, x


def window(x, n, steps, terminal, first=0):
    """the slices of a window of the case's arrays for the first n samples"""
    s = lambda a, extra: np.ascontiguousarray(a[first:first + steps + extra, :n]) if a is not None else None      # noqa: E731
    return dict(q=s(x["q"], int(terminal)), v=s(x["v"], int(terminal)), u=s(x["u"], 0), a=s(x["a"], 0), f=s(x["f"], 0))


def referee(m, M, cost, cons, t0, w, active, first=0, terminal=False, total_steps=SMAX):
    tables = RS.reference_tables(M, cost, t0, DT, total_steps)
    n = w["q"].shape[1]
    pick = lambda a, i: a[:, i] if a is not None else None      # noqa: E731
    out = [RS.reference_score(m, M, cost, cons, tables, DT, pick(w["q"], i), pick(w["v"], i), pick(w["u"], i), pick(w["a"], i), pick(w["f"], i), active,
                              first, terminal) for i in range(n)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]).T


def check(got, want, what):
    bad = [(what, i, g, w) for i, (g, w) in enumerate(zip(np.ravel(got), np.ravel(want))) if not close(g, w)]
    assert not bad, bad[:3]


# ------------------------------------------------------------------ 1. every model, size and window length, all rows switched on

@pytest.mark.parametrize("steps", [1, 2, 7])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("which", ["chain2", "chain8", "anymal", 1], ids=["chain2", "chain8", "anymal", "other1"])
def test_score_against_the_numpy_referee(which, n, steps):
    m, M, cost, t0, x = case(which)
    quad = m.ncontacts > 0
    active = CHANGING[:steps] if quad else None
    r = Rbd(m)
    for cone in ("linearized_friction_cone", "friction_cone"):
        cons = all_constraints(m, cone)
        o = RS.Objective(r, cost, cons, t0, DT, SMAX)
        for terminal in (False, True):
            w = window(x, n, steps, terminal)
            got = RS.score(r, o, active=active, terminal=terminal, **w)
            want = referee(m, M, cost, cons, t0, w, active, 0, terminal)
            print("%s n=%d steps=%d %s terminal=%d: cost %s violation %s" % (which, n, steps, cone, terminal, got[0], got[1]))
            assert (want[1] > 0).all()                     # (rows are active)
            for g, wnt, what in zip(got, want, ("cost", "violation", "stage_cost")):
                check(g, wnt, what)
            # stage_cost: folded in index order it IS the cost; not asking for it changes nothing
            seq = np.zeros(n)
            for s in got[2]:
                seq = seq + s
            assert np.array_equal(seq, got[0])
            bare = RS.score(r, o, active=active, terminal=terminal, want_stage=False, **w)
            assert bare[2] is None and np.array_equal(bare[0], got[0]) and np.array_equal(bare[1], got[1])
            only_cost = RS.score(r, o, active=active, terminal=terminal, want_stage=False, want=("cost",), **w)
            only_viol = RS.score(r, o, active=active, terminal=terminal, want_stage=False, want=("violation",), **w)
            assert only_cost[1] is None and only_viol[0] is None and np.array_equal(only_cost[0], got[0]) and np.array_equal(only_viol[1], got[1])
        o.close()
        if not quad:
            break                                          # (a chain has no cone)
    r.close()


def test_a_window_longer_than_one_chunk_of_logarithms():
    m, M, cost, t0, x = case("anymal")
    steps, n = 70, 3
    rng = np.random.default_rng(5)
    idx = rng.integers(0, SMAX, steps + 1)
    big = {k: (np.ascontiguousarray(a[idx[:steps + (k in "qv")]][:, :n]) if a is not None else None) for k, a in x.items()}
    active = [CHANGING[k % SMAX] for k in range(steps)]
    cons = all_constraints(m)
    r = Rbd(m)
    o = RS.Objective(r, cost, cons, t0, DT, steps)
    got = RS.score(r, o, active=active, terminal=True, **big)
    want = referee(m, M, cost, cons, t0, big, active, 0, True, total_steps=steps)
    for g, wnt, what in zip(got, want, ("cost", "violation", "stage_cost")):
        check(g, wnt, what)
    o.close()
    r.close()


# ------------------------------------------------------------------ 2. contact schedules; an inactive contact's f is not read

@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_contact_schedules_and_unread_forces(schedule):
    m, M, cost, t0, x = case("anymal")
    active = SCHEDULES[schedule]
    n = 3
    w = window(x, n, SMAX, False)
    mask = np.array(active, dtype=bool)
    w["f"][~mask[:, None, :].repeat(n, axis=1)] = np.nan            # the forces of every inactive contact
    assert np.isnan(w["f"]).any() or schedule == "all"
    r = Rbd(m)
    for cone in ("linearized_friction_cone", "friction_cone"):
        cons = no_constraints()
        setattr(cons, cone, 1)
        o = RS.Objective(r, cost, cons, t0, DT, SMAX)
        got = RS.score(r, o, active=active, **w)
        assert all(np.isfinite(g).all() for g in got), schedule
        want = referee(m, M, cost, cons, t0, w, active)
        for g, wnt, what in zip(got, want, ("cost", "violation", "stage_cost")):
            check(g, wnt, what)
        assert (got[1] > 0).all() or schedule == "none"
        if schedule == "none":
            assert (got[1] == 0).all()
        o.close()
    r.close()


# ------------------------------------------------------------------ 3. every constraint row on its own: inactive by a margin, active, on the bound

MU = 0.7
M_LIN = MU / math.sqrt(2.0)
# name -> (the switch, the array, (contact or None, entry), the value ON the bound given the model / bounds below, the direction that violates)
Q_MIN, Q_MAX, V_MAX, U_MAX, A_MIN, A_MAX = -0.5, 0.75, 2.0, 8.0, -3.0, 4.0
JOINT = 4                                                 # the actuated joint the row is placed on (of 12; chain: of 2 -> joint 1)
ROWS = {
    "q_min": ("joint_position_limits", "q", Q_MIN, -1), "q_max": ("joint_position_limits", "q", Q_MAX, 1),
    "v_lower": ("joint_velocity_limits", "v", -V_MAX, -1), "v_upper": ("joint_velocity_limits", "v", V_MAX, 1),
    "u_lower": ("joint_torque_limits", "u", -U_MAX, -1), "u_upper": ("joint_torque_limits", "u", U_MAX, 1),
    "a_min": ("joint_acceleration_lower_limit", "a", A_MIN, -1), "a_max": ("joint_acceleration_upper_limit", "a", A_MAX, 1),
}
FZ = 16.0


def row_case(which):
    """a model with the bounds above and one sample, two steps, strictly inside every bound"""
    if which == "anymal":
        m = capi.Model.from_buffer_copy(anymal_model())
    else:
        m = capi.Model.from_buffer_copy(IR.chain(2, 1)[0])
    for j in range(m.nu):
        m.q_min[j], m.q_max[j], m.v_max[j], m.u_max[j] = Q_MIN, Q_MAX, V_MAX, U_MAX
    M = IR.model_from_struct(m) if which == "anymal" else IR.chain(2, 1)[1]
    rng = np.random.default_rng(9)
    steps, n = 2, 1
    q = np.zeros((steps, n, m.nq))
    if m.ncontacts:
        q[..., :7] = random_samples(rng, steps)[0][:, None, :7]
    q[..., m.nq - m.nu:] = rng.uniform(-0.3, 0.5, (steps, n, m.nu))
    w = dict(q=q, v=rng.uniform(-1, 1, (steps, n, m.nv)), u=rng.uniform(-5, 5, (steps, n, m.nu)), a=rng.uniform(-2, 2, (steps, n, m.nv)),
             f=np.tile(np.array([1.0, -2.0, 40.0]), (steps, n, 4, 1)) if m.ncontacts else None)
    cost = capi.Cost()
    cost.set("q_ref", np.concatenate([[0, 0, 0.5, 0, 0, 0, 1], np.zeros(12)]) if m.ncontacts else np.zeros(m.nq))
    cost.set("q_weight", np.ones(m.nv))
    return m, M, cost, w


@pytest.mark.parametrize("row", list(ROWS))
@pytest.mark.parametrize("which", ["anymal", "chain2"])
def test_each_joint_row_inactive_active_and_on_the_bound(which, row):
    m, M, cost, w = row_case(which)
    switch, arr_name, bound, sign = ROWS[row]
    cons = no_constraints()
    setattr(cons, switch, 1)
    for j in range(m.nu):
        cons.a_min[j], cons.a_max[j] = A_MIN, A_MAX
    j = JOINT if which == "anymal" else 1
    col = (m.nq - m.nu if arr_name == "q" else (0 if arr_name == "u" else m.nv - m.nu)) + j
    active = [[1, 1, 1, 1]] * 2 if m.ncontacts else None
    r = Rbd(m)
    o = RS.Objective(r, cost, cons, 0.0, DT, 2)
    # inside by a margin: no row contributes, exactly
    _, viol, _ = RS.score(r, o, active=active, **w)
    assert viol[0] == 0.0
    # exactly on the bound: still nothing, exactly
    w[arr_name][1, 0, col] = bound
    _, viol, _ = RS.score(r, o, active=active, **w)
    assert viol[0] == 0.0, (row, viol)
    # beyond it by 0.375 (exact in binary): dt * 0.375 from this row and this step alone
    w[arr_name][1, 0, col] = bound + sign * 0.375
    _, viol, _ = RS.score(r, o, active=active, **w)
    want = referee(m, M, cost, cons, 0.0, w, active, total_steps=2)[1]
    assert close(viol[0], DT * 0.375) and close(viol[0], want[0]), (row, viol, want)
    # the other side of the same switch is far away: moving the entry inside again gives zero
    w[arr_name][1, 0, col] = bound - sign * 0.125
    assert RS.score(r, o, active=active, **w)[1][0] == 0.0
    o.close()
    r.close()


def cone_point(kind, row):
    """(f on the bound of `row` and strictly inside every other row, the unit direction that violates `row`, d row / d direction)"""
    if kind == "linearized_friction_cone":
        if row == 0:
            return np.zeros(3), np.array([0.0, 0.0, -1.0]), None         # the apex: every row is zero there; below it all five are active
        sx, axis = [(1, 0), (-1, 0), (1, 1), (-1, 1)][row - 1]
        f = np.array([0.0, 0.0, FZ])
        f[axis] = sx * M_LIN * FZ
        d = np.zeros(3)
        d[axis] = sx
        return f, d, 1.0
    if row == 0:
        return np.zeros(3), np.array([0.0, 0.0, -1.0]), None
    return np.array([MU * FZ * 0.6, MU * FZ * 0.8, FZ]), np.array([0.6, 0.8, 0.0]), None


@pytest.mark.parametrize("kind,row", [("linearized_friction_cone", k) for k in range(5)] + [("friction_cone", k) for k in range(2)])
def test_each_cone_row_inactive_active_and_on_the_bound(kind, row):
    m, M, cost, w = row_case("anymal")
    cons = no_constraints()
    setattr(cons, kind, 1)
    cons.mu = MU
    active = [[1, 1, 1, 1], [1, 1, 1, 0]]
    w["f"][1, 0, 3] = np.nan                               # (inactive at step 1)
    r = Rbd(m)
    o = RS.Objective(r, cost, cons, 0.0, DT, 2)
    assert RS.score(r, o, active=active, **w)[1][0] == 0.0      # f = (1, -2, 40): inside by a margin
    f, d, slope = cone_point(kind, row)
    w["f"][1, 0, 2] = f
    on_bound = RS.score(r, o, active=active, **w)[1][0]
    # on the bound the row is zero up to the rounding of mu / sqrt 2 times fz (1 ulp of 8: 2e-15), exactly zero at the apex
    assert 0.0 <= on_bound <= BAR and (row != 0 or on_bound == 0.0), (kind, row, on_bound)
    w["f"][1, 0, 2] = f + 0.375 * d
    viol = RS.score(r, o, active=active, **w)[1][0]
    want = referee(m, M, cost, cons, 0.0, w, active, total_steps=2)[1][0]
    assert viol > 1e-3 and close(viol, want), (kind, row, viol, want)
    if slope is not None:
        assert close(viol, DT * 0.375 * slope)              # this row alone
    w["f"][1, 0, 2] = f - 0.25 * d if row else np.array([0.0, 0.0, 1.0])
    assert RS.score(r, o, active=active, **w)[1][0] == 0.0
    o.close()
    r.close()


# ------------------------------------------------------------------ 4. reference kinds, far from the reference and very close to it

@pytest.mark.parametrize("kind", ["constant", "trotting", "time_varying"])
def test_reference_kinds(kind):
    m, M, cost, t0, x = case("anymal", kind)
    n = 3
    cons = all_constraints(m)
    r = Rbd(m)
    o = RS.Objective(r, cost, cons, t0, DT, SMAX)
    tables = RS.reference_tables(M, cost, t0, DT, SMAX)
    q_tab, v_tab = o.tables()
    assert np.abs(RP.same_rotation(q_tab, tables[0]) - tables[0]).max() < 1e-14 and np.abs(v_tab - tables[1]).max() < 1e-15
    if kind != "constant":
        assert np.abs(q_tab[-1] - q_tab[0]).max() > 1e-3
    w = window(x, n, SMAX, True)
    angles = [np.linalg.norm(F.RBD.difference(M, tables[0][k], w["q"][k, i])[3:6]) for k in range(SMAX + 1) for i in range(n)]
    assert 1.39 < min(angles) and max(angles) < 1.71
    got = RS.score(r, o, active=CHANGING, terminal=True, **w)
    want = referee(m, M, cost, cons, t0, w, CHANGING, 0, True)
    print(kind, got[0], want[0])
    for g, wnt, what in zip(got, want, ("cost", "violation", "stage_cost")):
        check(g, wnt, what)
    o.close()
    r.close()


def test_small_angle_takes_the_series_branch():
    m, M, cost, t0, x = case("anymal")
    n, steps = 2, 2
    tables = RS.reference_tables(M, cost, t0, DT, SMAX)
    w = window(x, n, steps, True)
    axis = np.array([0.6, -0.48, 0.64])
    tiny = np.concatenate([axis * math.sin(0.5e-9), [math.cos(0.5e-9)]])      # (x, y, z, w) of a rotation by 1e-9 rad
    for k in range(steps + 1):
        w["q"][k, 0] = tables[0][k]
        w["q"][k, 0, :3] += [0.3, -0.2, 0.1]
        w["q"][k, 0, 3:7] = quat_mul(tables[0][k][3:7], tiny)          # (the generator's integrate() drops a rotation this small)
        angle = np.linalg.norm(F.RBD.difference(M, tables[0][k], w["q"][k, 0])[3:6])
        assert 0.9e-9 < angle < 1.1e-9, angle
        w["q"][k, 1] = tables[0][k]                        # q == q_ref bit for bit
        w["v"][k, 1] = tables[1][k]
    cost1 = capi.Cost.from_buffer_copy(cost)
    for name in ("q_weight", "qf_weight"):
        cost1.set(name, np.concatenate([np.zeros(3), np.full(3, 1e18), np.zeros(12)]))      # the rotation rows alone, scaled to O(1)
    for name in ("v_weight", "vf_weight", "a_weight", "u_weight"):
        cost1.set(name, np.zeros(m.nv if name != "u_weight" else m.nu))
    for c in range(4):
        for k in range(3):
            cost1.f_weight[c][k] = 0.0
    r = Rbd(m)
    o = RS.Objective(r, cost1, None, t0, DT, SMAX)
    got = RS.score(r, o, active=[[1, 1, 1, 1]] * steps, terminal=True, **w)
    want = referee(m, M, cost1, None, t0, w, [[1, 1, 1, 1]] * steps, 0, True)
    print("small angle:", got[0], want[0])
    assert 0.1 < want[0][0] < 10 and want[0][1] < 1e-11
    check(got[0], want[0], "cost")
    assert got[0][1] == 0.0 and (got[1] == 0).all()
    o.close()
    r.close()


# ------------------------------------------------------------------ 5. optional arrays

def test_null_arrays_with_zero_weights_are_accepted_and_refused_otherwise():
    lib = capi.lib()
    m, M, cost, t0, x = case("anymal")
    n, steps = 2, 2
    w = window(x, n, steps, False)
    active = [[1, 1, 1, 1]] * steps
    bare = capi.Cost.from_buffer_copy(cost)
    bare.set("a_weight", np.zeros(m.nv)).set("u_weight", np.zeros(m.nu))
    for c in range(4):
        for k in range(3):
            bare.f_weight[c][k] = 0.0
    r = Rbd(m)
    o = RS.Objective(r, bare, no_constraints(), t0, DT, SMAX)
    got = RS.score(r, o, w["q"], w["v"], active=active)
    full = RS.score(r, o, active=active, **w)
    want = referee(m, M, bare, None, t0, dict(w, u=None, a=None, f=None), active)
    check(got[0], want[0], "cost")
    assert np.array_equal(got[0], full[0]) and (got[1] == 0).all()      # zero weights: the arrays add exact zeros
    o.close()
    for what, change, text in (("u", lambda c, k: c.set("u_weight", np.full(m.nu, 0.5)), "u_traj is NULL but a torque weight or the torque limits read it"),
                               ("u", lambda c, k: setattr(k, "joint_torque_limits", 1), "u_traj is NULL but a torque weight or the torque limits read it"),
                               ("a", lambda c, k: c.set("a_weight", np.full(m.nv, 0.5)), "a_traj is NULL but an acceleration weight or the acceleration limits read it"),
                               ("a", lambda c, k: setattr(k, "joint_acceleration_lower_limit", 1), "a_traj is NULL but an acceleration weight or the acceleration limits read it"),
                               ("f", lambda c, k: setattr(k, "friction_cone", 1), "f_traj is NULL but a contact-force weight or the friction cone reads it"),
                               ("f", lambda c, k: c.f_weight[1].__setitem__(2, 1.0), "f_traj is NULL but a contact-force weight or the friction cone reads it")):
        c2, k2 = capi.Cost.from_buffer_copy(bare), no_constraints()
        change(c2, k2)
        o = RS.Objective(r, c2, k2, t0, DT, SMAX)
        arrays = dict(q_traj=w["q"], v_traj=w["v"], u_traj=w["u"], a_traj=w["a"], f_traj=w["f"], cost=np.zeros(n))
        arrays[what + "_traj"] = None
        io, keep = RS.io_struct(**arrays)
        for device in (False, True):
            assert RS.score_raw(r, o, n, 0, steps, active, 0, 0, io, device=device) == E_ARG
            name = "idocp_rbd_score_rollout" + ("_device" if device else "")
            assert lib.idocp_last_error().decode() == name + ": " + text
        o.close()
    r.close()


# ------------------------------------------------------------------ 6. identities that need no referee

def device_score(r, o, w, n, steps, active, terminal, accumulate=False, start=None, first=0):
    """the device form on freshly uploaded copies; returns (cost, violation, stage_cost)"""
    slices = steps + int(terminal)
    d = {k: DeviceArray(a) for k, a in w.items() if a is not None}
    d["cost"] = DeviceArray(start[0] if start is not None else np.full(n, -777.0))
    d["violation"] = DeviceArray(start[1] if start is not None else np.full(n, -777.0))
    d["stage_cost"] = DeviceArray(np.full((slices, n), -777.0))
    io = capi.RbdScoreIO()
    for k in "qvuaf":
        if k in d:
            setattr(io, k + "_traj", d[k].ptr.value)
    for k in ("cost", "violation", "stage_cost"):
        setattr(io, k, d[k].ptr.value)
    capi.check(RS.score_raw(r, o, n, first, steps, active, terminal, accumulate, io, device=True), "idocp_rbd_score_rollout_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    out = tuple(d[k].numpy() for k in ("cost", "violation", "stage_cost"))
    for a in d.values():
        a.free()
    return out


@pytest.mark.parametrize("which", ["chain8", "anymal"])
def test_windows_launch_size_and_form_do_not_change_a_bit(which):
    m, M, cost, t0, x = case(which)
    quad = m.ncontacts > 0
    active = CHANGING if quad else None
    part = lambda a, b: active[a:b] if quad else None      # noqa: E731
    cons = all_constraints(m)
    r = Rbd(m)
    o = RS.Objective(r, cost, cons, t0, DT, SMAX)
    n = NMAX
    for terminal in (False, True):
        whole = RS.score(r, o, active=active, terminal=terminal, **window(x, n, SMAX, terminal))
        # windows of 3 + 4 with accumulate (the terminal slice belongs to the last window)
        first = RS.score(r, o, active=part(0, 3), **window(x, n, 3, False))
        second = RS.score(r, o, active=part(3, 7), first_step=3, terminal=terminal, accumulate=(first[0], first[1]), **window(x, n, 4, terminal, first=3))
        assert np.array_equal(second[0], whole[0]) and np.array_equal(second[1], whole[1]), terminal
        assert np.array_equal(np.concatenate([first[2], second[2]]), whole[2])
        # ... and of 1 + 1 + 5
        acc = (np.zeros(n), np.zeros(n))
        for a, b in ((0, 1), (1, 2), (2, 7)):
            last = b == SMAX
            res = RS.score(r, o, active=part(a, b), first_step=a, terminal=terminal and last, accumulate=acc, **window(x, n, b - a, terminal and last, first=a))
            acc = (res[0], res[1])
        assert np.array_equal(acc[0], whole[0]) and np.array_equal(acc[1], whole[1])
        # a sample alone and as sample 3 of 5
        one = {k: (np.ascontiguousarray(a[:, 3:4]) if a is not None else None) for k, a in window(x, n, SMAX, terminal).items()}
        alone = RS.score(r, o, active=active, terminal=terminal, **one)
        assert all(np.array_equal(a[..., 0], b[..., 3]) for a, b in zip(alone, whole))
        # the device form
        dev = device_score(r, o, window(x, n, SMAX, terminal), n, SMAX, active, terminal)
        assert all(np.array_equal(a, b) for a, b in zip(dev, whole))
        dev2 = device_score(r, o, window(x, n, 4, terminal, first=3), n, 4, part(3, 7), terminal, accumulate=True, start=(first[0], first[1]), first=3)
        assert np.array_equal(dev2[0], whole[0]) and np.array_equal(dev2[1], whole[1])
    o.close()
    r.close()


# ------------------------------------------------------------------ 7. non-finite input

def test_a_nan_poisons_its_own_sample_only():
    m, M, cost, t0, x = case("anymal")
    n = NMAX
    others = [0, 1, 3, 4]
    r = Rbd(m)
    o = RS.Objective(r, cost, all_constraints(m), t0, DT, SMAX)
    w = window(x, n, SMAX, True)
    clean = RS.score(r, o, active=CHANGING, terminal=True, **w)
    assert all(np.isfinite(c).all() for c in clean)
    for name, at, value in (("v", (1, 2, 4), np.nan), ("v", (1, 2, 11), np.inf), ("q", (3, 2, 5), np.nan), ("q", (SMAX, 2, 12), np.nan), ("u", (0, 2, 0), -np.inf),
                            ("a", (6, 2, 17), np.nan)):
        bad = {k: a.copy() for k, a in w.items()}
        bad[name][at] = value
        cost_, viol, _ = RS.score(r, o, active=CHANGING, terminal=True, **bad)
        assert np.isnan(cost_[2]) and np.isnan(viol[2]), (name, at)
        assert np.array_equal(cost_[others], clean[0][others]) and np.array_equal(viol[others], clean[1][others]), (name, at)
    o.close()
    # a NaN force on an active contact with only the cone switched on: max(0, NaN) must not swallow it
    bare = capi.Cost()
    bare.set("q_ref", np.array(cost.q_ref[:m.nq]))
    for cone in ("linearized_friction_cone", "friction_cone"):
        cons = no_constraints()
        setattr(cons, cone, 1)
        o = RS.Objective(r, bare, cons, t0, DT, SMAX)
        clean = RS.score(r, o, active=CHANGING, **window(x, n, SMAX, False))
        for entry in range(3):
            bad = window(x, n, SMAX, False)
            assert CHANGING[1][3] == 1
            bad["f"][1, 2, 3, entry] = np.nan
            cost_, viol, _ = RS.score(r, o, active=CHANGING, **bad)
            assert np.isnan(cost_[2]) and np.isnan(viol[2]), (cone, entry)
            assert np.array_equal(cost_[others], clean[0][others]) and np.array_equal(viol[others], clean[1][others])
        o.close()
    r.close()


# ------------------------------------------------------------------ 8. end to end: a closed-loop rollout, scored where it lies

def test_policy_rollout_scored_on_its_own_outputs():
    m, M, cost, t0, x = case("anymal", "trotting")
    n, steps, dt, ts = 3, 4, 1e-2, 0.04
    rng = np.random.default_rng(77)
    cons = all_constraints(m)
    r = Rbd(m)
    o = RS.Objective(r, cost, cons, t0, dt, steps)
    q_tab, v_tab = o.tables()
    dq, dv = o.device_tables()
    # the device tables are the host tables bit for bit
    got_q, got_v = np.empty_like(q_tab), np.empty_like(v_tab)
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    capi.check(r.lib.idocp_device_download(got_q.ctypes.data, dq, got_q.nbytes), "idocp_device_download")
    capi.check(r.lib.idocp_device_download(got_v.ctypes.data, dv, got_v.nbytes), "idocp_device_download")
    assert np.array_equal(got_q, q_tab) and np.array_equal(got_v, v_tab)
    q0 = RP.perturbed_configurations(M, rng, np.repeat(q_tab[:1], n, axis=0), angle=0.3, lin=0.05, joint=0.1)
    v0 = 0.1 * rng.uniform(-1, 1, (n, m.nv))
    pts = np.repeat(F.foot_positions(m, q0)[None], steps, axis=0)
    masks = [[1, 1, 1, 1], [1, 1, 1, 1], [1, 0, 0, 1], [1, 0, 0, 1]]
    d = dict(K=DeviceArray(RP.random_gains(rng, (steps,), m.nu, m.nv, 20.0)), u_ff=DeviceArray(rng.uniform(-5, 5, (steps, n, m.nu))), pts=DeviceArray(pts),
             q=DeviceArray(np.concatenate([q0[None], np.zeros((steps, n, m.nq))])), v=DeviceArray(np.concatenate([v0[None], np.zeros((steps, n, m.nv))])),
             u=DeviceArray(np.zeros((steps, n, m.nu))), a=DeviceArray(np.zeros((steps, n, m.nv))), f=DeviceArray(np.zeros((steps, n, 4, 3))),
             cost=DeviceArray(np.zeros(n)), violation=DeviceArray(np.zeros(n)))
    pol = capi.RbdPolicy()
    pol.u_ff, pol.K, pol.q_ref, pol.v_ref, pol.shared_gains, pol.shared_ref = d["u_ff"].ptr.value, d["K"].ptr.value, dq.value, dv.value, 1, 1
    act = (C.c_int * (4 * steps))(*[b for s in masks for b in s])
    capi.check(r.lib.idocp_rbd_rollout_policy_device(r.h, n, steps, act, ts, dt, C.byref(pol), d["pts"].ptr, d["q"].ptr, d["v"].ptr, d["u"].ptr, d["a"].ptr, d["f"].ptr, 0),
               "idocp_rbd_rollout_policy_device")
    io = capi.RbdScoreIO()
    for k in "qvuaf":
        setattr(io, k + "_traj", d[k].ptr.value)
    io.cost, io.violation = d["cost"].ptr.value, d["violation"].ptr.value
    capi.check(RS.score_raw(r, o, n, 0, steps, masks, 1, 0, io, device=True), "idocp_rbd_score_rollout_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    w = {k: d[k].numpy() for k in "qvuaf"}
    assert all(np.isfinite(a).all() for a in w.values())
    tables = RS.reference_tables(M, cost, t0, dt, steps)
    for i in range(n):
        want = RS.reference_score(m, M, cost, cons, tables, dt, w["q"][:, i], w["v"][:, i], w["u"][:, i], w["a"][:, i], w["f"][:, i], masks, 0, True)
        got = (d["cost"].numpy()[i], d["violation"].numpy()[i])
        print("sample %d: cost %.12g (%.12g) violation %.12g (%.12g)" % (i, got[0], want[0], got[1], want[1]))
        assert close(got[0], want[0]) and close(got[1], want[1]), (i, got, want[:2])
    for a in d.values():
        a.free()
    o.close()
    r.close()


# ------------------------------------------------------------------ 9. refusals

def test_refusals():
    lib = capi.lib()
    m, M, cost, t0, x = case("anymal")
    n, steps = 2, 2
    w = window(x, n, steps, False)
    active = [[1, 1, 1, 1]] * steps
    r, other = Rbd(m), Rbd(m)
    o, foreign = RS.Objective(r, cost, all_constraints(m), t0, DT, SMAX), RS.Objective(other, cost, all_constraints(m), t0, DT, SMAX)
    io, keep = RS.io_struct(q_traj=w["q"], v_traj=w["v"], u_traj=w["u"], a_traj=w["a"], f_traj=w["f"], cost=np.zeros(n), violation=np.zeros(n))

    def refused(rc, call, text, code=E_ARG):
        assert rc == code, text
        assert lib.idocp_last_error().decode() == call + ": " + text, lib.idocp_last_error()

    for device in (False, True):
        call = "idocp_rbd_score_rollout" + ("_device" if device else "")
        refused(RS.score_raw(r, foreign, n, 0, steps, active, 0, 0, io, device), call, "the objective was created on another handle")
        refused(RS.score_raw(r, o, n, SMAX - 1, steps, active, 0, 0, io, device), call, "first_step + steps must lie within the objective's %d steps" % SMAX)
        refused(RS.score_raw(r, o, n, -1, steps, active, 0, 0, io, device), call, "first_step + steps must lie within the objective's %d steps" % SMAX)
        refused(RS.score_raw(r, o, 0, 0, steps, active, 0, 0, io, device), call, "n must be positive")
        refused(RS.score_raw(r, o, -3, 0, steps, active, 0, 0, io, device), call, "n must be positive")
        refused(RS.score_raw(r, o, n, 0, 0, active, 0, 0, io, device), call, "steps must be at least 1")
        refused(RS.score_raw(r, o, n, 0, steps, active, 0, 0, None, device), call, "null handle, objective or io")
        refused(RS.score_raw(r, None, n, 0, steps, active, 0, 0, io, device), call, "null handle, objective or io")
        refused(RS.score_raw(r, o, n, 0, steps, None, 0, 0, io, device), call, "the contact status `active` is needed")
        io2, keep2 = RS.io_struct(v_traj=w["v"], u_traj=w["u"], a_traj=w["a"], f_traj=w["f"], cost=np.zeros(n))
        refused(RS.score_raw(r, o, n, 0, steps, active, 0, 0, io2, device), call, "q_traj and v_traj are needed")
    # create
    call, out = "idocp_rbd_objective_create", C.c_void_p()
    cons = all_constraints(m)
    refused(RS.create_raw(r, None, cons, t0, DT, SMAX, out), call, "null cost")
    refused(RS.create_raw(r, cost, cons, t0, DT, 0, out), call, "steps must be at least 1")
    refused(RS.create_raw(r, cost, cons, t0, -DT, SMAX, out), call, "dt must be positive and finite")
    refused(RS.create_raw(r, cost, cons, t0, math.nan, SMAX, out), call, "dt must be positive and finite")
    task = capi.Cost.from_buffer_copy(cost)
    task.task_dim = 3
    assert RS.create_raw(r, task, cons, t0, DT, SMAX, out) == E_UNSUPPORTED and "task-space cost components" in lib.idocp_last_error().decode()
    cons.contact_distance = 1
    assert RS.create_raw(r, cost, cons, t0, DT, SMAX, out) == E_UNSUPPORTED and "contact_distance" in lib.idocp_last_error().decode()
    cons.contact_distance, cons.friction_cone = 0, 1
    assert RS.create_raw(r, cost, cons, t0, DT, SMAX, out) == E_UNSUPPORTED and "together" in lib.idocp_last_error().decode()
    assert not out.value
    assert lib.idocp_rbd_objective_get_reference(o.h, SMAX + 1, None, None) == E_ARG
    # the refusals left handle and objective usable
    assert np.isfinite(RS.score(r, o, active=active, **w)[0]).all()
    # a chain takes active = NULL and f_traj = NULL, and neither the trotting nor the time-varying reference
    mc, Mc, costc, t0c, xc = case("chain2")
    rc_ = Rbd(mc)
    oc = RS.Objective(rc_, costc, None, t0c, DT, SMAX)
    wc = window(xc, n, steps, False)
    ioc, keepc = RS.io_struct(q_traj=wc["q"], v_traj=wc["v"], u_traj=wc["u"], a_traj=wc["a"], cost=np.zeros(n))
    refused(RS.score_raw(rc_, oc, n, 0, steps, active, 0, 0, ioc), "idocp_rbd_score_rollout", "a fixed-base chain has no contacts (active and f_traj must be NULL)")
    assert RS.score_raw(rc_, oc, n, 0, steps, None, 0, 0, ioc) == 0
    trot = capi.Cost.from_buffer_copy(costc)
    trot.use_trotting_ref, trot.t_period = 1, 0.5
    assert RS.create_raw(rc_, trot, None, t0c, DT, SMAX, out) == E_UNSUPPORTED
    oc.close()
    rc_.close()
    o.close()
    foreign.close()
    r.close()
    other.close()
