"""Sampling around a torque sequence on the GPU (idocp_rbd_perturb_torques, idocp_rbd_importance_weights, idocp_rbd_weighted_mean;
rbd_sample_kernel.hip) against the referee of tests/rbd_sample.py, which test_rbd_sample_host.py holds to the published Philox vectors and to the
moments of a standard normal.  The bar is the project's bar for the rbd calls against numpy, |gpu - referee| <= 1e-11 max(1, |referee|) per result
(independent_rbd.BAR), measured as test_rbd_score_gpu.py measures it.

Shapes: n in {1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 chunk + 1} around the wavefront and the chunk of the fixed-order sums; m in
{1, 12, 18, 19, 64} (one lane group per column: 256, 21, 14, 13 and 4 groups, 19 leaving idle lanes); rows in {1, 3}."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import independent_rbd as IR
import rbd_forward as F
import rbd_sample as RS
import rbd_score as RSC
from helpers import ANYMAL_Q_STANDING, anymal_contact_points, anymal_model, anymal_problem
from idocp_amd import capi
from rbd_batch import E_ARG, DeviceArray, Rbd

pytestmark = pytest.mark.gpu
BAR = IR.BAR
CHUNK = RS.CHUNK
NS = [1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
SEED = 0x1234567887654321


def check(got, want, what):
    got, want = np.ravel(got), np.ravel(want)
    bad = [(what, i, g, w) for i, (g, w) in enumerate(zip(got, want)) if not abs(g - w) <= BAR * max(1.0, abs(w))]
    assert not bad, bad[:3]


def same(a, b):
    """bit for bit, NaN included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def handle(which):
    return Rbd(anymal_model() if which == "anymal" else IR.chain(int(which[5:]), 1)[0])


def last_error():
    return capi.lib().idocp_last_error()


# ------------------------------------------------------------------ perturb

def perturb_case(nu, steps):
    rng = np.random.default_rng([3, nu, steps])
    return rng.uniform(-20, 20, (steps, nu)), rng.uniform(0.5, 3.0, nu), np.full(nu, -21.0), np.full(nu, 20.5)


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 65])
@pytest.mark.parametrize("which", ["anymal", "chain3", "chain7"])
def test_perturb_against_the_referee(which, n, steps):
    r = handle(which)
    nom, sigma, lo, hi = perturb_case(r.m.nu, steps)
    got = RS.perturb(r, n, nom, sigma, lo, hi, seed=SEED, draw=4, first_step=2)
    want = RS.reference_perturb(n, 2, nom, sigma, lo, hi, SEED, 4)
    print("%s n=%d steps=%d: max |gpu - referee| = %.3e" % (which, n, steps, np.abs(got - want).max()))
    check(got, want, "u_samples")
    assert same(got[:, 0], RS.clamp(nom, lo, hi))                       # sample 0 is the clamped nominal itself
    free = RS.perturb(r, n, nom, sigma, seed=SEED, draw=4, first_step=2)
    assert same(free[:, 0], nom)
    check(free, RS.reference_perturb(n, 2, nom, sigma, None, None, SEED, 4), "u_samples without bounds")
    if n > 1:
        assert (np.abs(free[:, 1:] - nom[:, None]) > 0).all() and np.abs(free - nom[:, None]).max() <= sigma.max() * RS.Z_MAX


@pytest.mark.parametrize("which", ["anymal", "chain3"])
def test_a_sample_depends_on_seed_draw_step_index_and_torque_alone(which):
    r = handle(which)
    nom, sigma, lo, hi = perturb_case(r.m.nu, 3)
    big = RS.perturb(r, 65, nom, sigma, lo, hi, seed=SEED, draw=1)
    small = RS.perturb(r, 2, nom, sigma, lo, hi, seed=SEED, draw=1)
    assert same(big[:, :2], small)                                      # whatever n is
    for k in range(3):                                                  # one call or window by window
        assert same(big[k:k + 1], RS.perturb(r, 65, nom[k:k + 1], sigma, lo, hi, seed=SEED, draw=1, first_step=k))
    free = RS.perturb(r, 65, nom, sigma, seed=SEED, draw=1)             # without bounds, so that no two entries meet at a bound
    for seed, draw in ((SEED, 2), (SEED + 1, 1), (SEED + (1 << 32), 1)):  # another draw, another low word, another high word of the seed
        other = RS.perturb(r, 65, nom, sigma, seed=seed, draw=draw)
        assert same(other[:, 0], free[:, 0]) and (other[:, 1:] != free[:, 1:]).all()      # every perturbed entry changes
    assert same(big, RS.perturb(r, 65, nom, sigma, lo, hi, seed=SEED, draw=1))                   # and a run repeats


def test_perturb_clamps_on_both_sides_and_the_forms_agree():
    r = handle("anymal")
    nu, n, steps = r.m.nu, 65, 3
    nom, _, _, _ = perturb_case(nu, steps)
    sigma, lo, hi = np.full(nu, 400.0), np.full(nu, -25.0), np.full(nu, 30.0)
    got = RS.perturb(r, n, nom, sigma, lo, hi, seed=7, draw=0)
    check(got, RS.reference_perturb(n, 0, nom, sigma, lo, hi, 7, 0), "clamped u_samples")
    assert (got == lo).any() and (got == hi).any() and got.min() == -25.0 and got.max() == 30.0
    only_lo = RS.perturb(r, n, nom, sigma, lo, None, seed=7, draw=0)
    only_hi = RS.perturb(r, n, nom, sigma, None, hi, seed=7, draw=0)
    assert only_lo.min() == -25.0 and only_lo.max() > 30.0 and only_hi.max() == 30.0 and only_hi.min() < -25.0
    d = {k: DeviceArray(x) for k, x in (("nom", nom), ("sigma", sigma), ("lo", lo), ("hi", hi), ("out", np.full((steps, n, nu), -777.0)))}
    capi.check(RS.perturb_raw(r, n, 0, steps, d["nom"], d["sigma"], d["lo"], d["hi"], 7, 0, d["out"], device=True), "idocp_rbd_perturb_torques_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "synchronize")
    assert same(d["out"].numpy(), got)


def test_perturb_refusals():
    r = handle("chain3")
    nu = r.m.nu
    nom, sigma, out = np.zeros((2, nu)), np.ones(nu), np.zeros((2, 4, nu))
    ok = dict(n=4, first_step=0, steps=2, u_nominal=nom, sigma=sigma, u_min=None, u_max=None, seed=1, draw=0, u_samples=out)
    name = b"idocp_rbd_perturb_torques"

    def refused(text, device=False, **change):
        assert RS.perturb_raw(r, device=device, **dict(ok, **change)) == E_ARG
        assert last_error() == name + (b"_device" if device else b"") + b": " + text, last_error()

    assert RS.perturb_raw(r, **ok) == 0
    for device in (False, True):
        refused(b"n must be positive", device, n=0)
        refused(b"steps must be at least 1", device, steps=0)
        refused(b"first_step must be non-negative, and first_step + steps must fit an int", device, first_step=-1)
        refused(b"first_step must be non-negative, and first_step + steps must fit an int", device, first_step=2 ** 31 - 2)
        for missing in ("u_nominal", "sigma", "u_samples"):
            refused(b"u_nominal, sigma and u_samples are needed", device, **{missing: None})
    for bad in (-1.0, math.nan, math.inf):
        s = sigma.copy()
        s[1] = bad
        refused(b"sigma[1] must be finite and non-negative", sigma=s)
    lo, hi = np.full(nu, -1.0), np.full(nu, 1.0)
    lo[2] = 2.0
    refused(b"u_min[2] <= u_max[2] does not hold (or a bound is NaN)", u_min=lo, u_max=hi)
    lo[2] = math.nan
    refused(b"u_min[2] <= u_max[2] does not hold (or a bound is NaN)", u_min=lo)
    hi[0] = math.nan
    refused(b"u_min[0] <= u_max[0] does not hold (or a bound is NaN)", u_max=hi)
    assert RS.perturb_raw(r, **dict(ok, sigma=np.zeros(nu))) == 0 and same(out, np.repeat(nom[:, None], 4, axis=1))      # sigma = 0 is allowed


# ------------------------------------------------------------------ weights

@functools.lru_cache(maxsize=None)
def scores(n):
    """(cost, violation, the indices of the minimum): NaN, +Inf and -Inf entries where n has room, the minimum tied at two indices, one of them the
    last sample (the last chunk)"""
    rng = np.random.default_rng([17, n])
    cost, viol = rng.uniform(2.0, 9.0, n), rng.uniform(0.0, 0.5, n)
    if n >= 63:
        cost[[3, 40]] = math.nan
        cost[7], cost[11] = math.inf, -math.inf
        viol[21] = math.nan
        viol[22] = math.inf
    ties = sorted({max(5, n - 60), n - 1}) if n >= 63 else [n - 1]      # (across two chunks where n has more than one)
    for i in ties:
        cost[i], viol[i] = 1.25, 0.125                  # s = 1.25 + 2 * 0.125, exact
    return cost, viol, ties


@pytest.mark.parametrize("n", NS)
def test_weights_against_the_referee(n):
    r = handle("anymal")
    cost, viol, ties = scores(n)
    w, stats = RS.weights(r, cost, viol, penalty=2.0, temperature=0.7)
    want_w, want_stats = RS.reference_weights(cost, viol, 2.0, 0.7)
    print("n=%d: stats %s, referee %s" % (n, stats, want_stats))
    check(w, want_w, "weights")
    check(stats, want_stats, "stats")
    s = cost + 2.0 * viol
    assert (w[~np.isfinite(s)] == 0.0).all() and not np.signbit(w).any()            # exact zeros outside F
    assert stats[0] == np.isfinite(s).sum() and stats[1] == 1.5 and stats[2] == ties[0]      # the lowest index of the tie
    assert all(w[i] == 1.0 for i in ties) and w.max() == 1.0 and stats[3] >= len(ties)
    assert 1.0 <= stats[4] <= stats[0]
    again = RS.weights(r, cost, viol, penalty=2.0, temperature=0.7)
    assert same(again[0], w) and same(again[1], stats)
    # violation = NULL is penalty = 0
    a, b = RS.weights(r, cost, None, penalty=2.0, temperature=0.7), RS.weights(r, cost, np.abs(np.nan_to_num(viol, posinf=1.0)), penalty=0.0, temperature=0.7)
    assert same(a[0], b[0]) and same(a[1], b[1])
    check(a[0], RS.reference_weights(cost, None, 0.0, 0.7)[0], "weights without violation")
    # the device form, stats in device memory
    d = {k: DeviceArray(x) for k, x in (("cost", cost), ("viol", viol), ("w", np.full(n, -777.0)), ("stats", np.full(5, -777.0)))}
    capi.check(RS.weights_raw(r, n, d["cost"], d["viol"], 2.0, 0.7, d["w"], d["stats"], device=True), "idocp_rbd_importance_weights_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "synchronize")
    assert same(d["w"].numpy(), w) and same(d["stats"].numpy(), stats)


@pytest.mark.parametrize("n", [1, 65, CHUNK + 1])
def test_weights_with_no_finite_score(n):
    r = handle("chain3")
    cost = np.array([math.nan, math.inf, -math.inf] * n)[:n]
    w, stats = RS.weights(r, cost, None, temperature=2.0)
    assert same(w, np.zeros(n)) and same(stats, np.array([0.0, math.nan, -1.0, 0.0, 0.0])), (w, stats)
    w, stats = RS.weights(r, np.ones(n), np.full(n, math.nan), penalty=1.0, temperature=2.0)
    assert same(w, np.zeros(n)) and same(stats[[0, 2, 3, 4]], np.array([0.0, -1.0, 0.0, 0.0])) and math.isnan(stats[1])


def test_weights_refusals():
    r = handle("chain3")
    cost, w, stats = np.ones(4), np.zeros(4), np.zeros(5)
    ok = dict(n=4, cost=cost, violation=None, penalty=0.0, temperature=1.0, weights=w, stats=stats)
    assert RS.weights_raw(r, **ok) == 0
    for device in (False, True):
        name = b"idocp_rbd_importance_weights" + (b"_device" if device else b"")

        def refused(text, **change):
            assert RS.weights_raw(r, device=device, **dict(ok, **change)) == E_ARG
            assert last_error() == name + b": " + text, last_error()

        refused(b"n must be positive", n=0)
        for missing in ("cost", "weights", "stats"):
            refused(b"cost, weights and stats are needed", **{missing: None})
        for bad in (0.0, -1.0, math.nan, math.inf):
            refused(b"temperature must be finite and positive", temperature=bad)
        for bad in (-1.0, math.nan, math.inf):
            refused(b"penalty must be finite and non-negative", penalty=bad)


# ------------------------------------------------------------------ weighted mean

@functools.lru_cache(maxsize=None)
def mean_case(n, m):
    """(weights with exact zeros, x [3][n][m]) and the referee's mean, computed once"""
    rng = np.random.default_rng([29, n, m])
    w = np.exp(-rng.uniform(0.0, 6.0, n))
    w[rng.uniform(size=n) < 0.2] = 0.0
    w[rng.integers(0, n)] = 1.0
    x = rng.uniform(-5.0, 5.0, (3, n, m))
    return w, x, RS.reference_mean(w, x)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m", [1, 12, 18, 19, 64])
def test_mean_against_the_referee(m, n):
    r = handle("chain3")
    w, x, want = mean_case(n, m)
    got = RS.mean(r, w, x)
    print("m=%d n=%d: max |gpu - referee| = %.3e" % (m, n, np.abs(got - want).max()))
    check(got, want, "mean, rows = 3")
    one = RS.mean(r, w, x[1:2])                                        # rows = 1: the middle row on its own
    check(one, want[1:2], "mean, rows = 1")
    assert same(one[0], got[1])                                        # a row does not depend on rows or on the call that carried it
    assert same(RS.mean(r, w, x), got)                                 # a run repeats
    d = {k: DeviceArray(a) for k, a in (("w", w), ("x", x), ("mean", np.full((3, m), -777.0)))}
    capi.check(RS.mean_raw(r, n, 3, m, d["w"], d["x"], d["mean"], device=True), "idocp_rbd_weighted_mean_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "synchronize")
    assert same(d["mean"].numpy(), got)


@pytest.mark.parametrize("n", [2, 65, CHUNK + 1])
@pytest.mark.parametrize("m", [12, 19])
def test_mean_skips_weightless_samples_and_confines_a_nan(m, n):
    r = handle("chain3")
    w, x, _ = mean_case(n, m)
    w, x = w.copy(), x.copy()
    dead = n - 1                                                       # a diverged sample: weight 0, NaN and Inf in its slices
    w[dead], w[0] = 0.0, 1.0
    zeroed = x.copy()
    zeroed[:, dead] = 0.0
    x[:, dead] = math.nan
    x[1, dead, 0] = math.inf
    got = RS.mean(r, w, x)
    assert np.isfinite(got).all() and same(got, RS.mean(r, w, zeroed))
    check(got, RS.reference_mean(w, zeroed), "mean with a skipped sample")
    hit = x.copy()                                                     # a NaN under a positive weight: its own (row, column) entry only
    hit[2, 0, m - 1] = math.nan
    bad = RS.mean(r, w, hit)
    assert math.isnan(bad[2, m - 1])
    bad[2, m - 1] = got[2, m - 1]
    assert same(bad, got)
    none = RS.mean(r, np.zeros(n), x)                                  # no weight at all: undefined, NaN everywhere
    assert np.isnan(none).all()


def test_mean_refusals():
    r = handle("chain3")
    w, x, out = np.ones(4), np.ones((2, 4, 3)), np.zeros((2, 3))
    ok = dict(n=4, rows=2, m=3, weights=w, x=x, mean=out)
    assert RS.mean_raw(r, **ok) == 0
    for device in (False, True):
        name = b"idocp_rbd_weighted_mean" + (b"_device" if device else b"")

        def refused(text, **change):
            assert RS.mean_raw(r, device=device, **dict(ok, **change)) == E_ARG
            assert last_error() == name + b": " + text, last_error()

        refused(b"n must be positive", n=0)
        refused(b"rows must be at least 1", rows=0)
        refused(b"m must be 1 .. 64 (IDOCP_RBD_MEAN_MAX_COLUMNS)", m=0)
        refused(b"m must be 1 .. 64 (IDOCP_RBD_MEAN_MAX_COLUMNS)", m=65)
        for missing in ("weights", "x", "mean"):
            refused(b"weights, x and mean are needed", **{missing: None})
    for bad in (-0.5, math.nan, math.inf):
        v = w.copy()
        v[2] = bad
        assert RS.mean_raw(r, **dict(ok, weights=v)) == E_ARG
        assert last_error() == b"idocp_rbd_weighted_mean: weights[2] must be finite and non-negative"


# ------------------------------------------------------------------ one iteration composed on the device

def test_one_refinement_iteration_on_the_device():
    """perturb, rollout_policy_device, score_rollout_device, weights, mean on the handle's stream with no synchronisation between; the new nominal
    against the referee's update from the DOWNLOADED cost, violation and u_traj (the rollout and the score have their own tests)"""
    m = anymal_model()
    r = handle("anymal")
    n, steps, dt = 65, 3, 0.02
    nq, nv, nu = m.nq, m.nv, m.nu
    cost, cons = anymal_problem(m, trotting_ref=False)
    cost.set("u_weight", np.full(nu, 0.01))
    cons.joint_position_limits = cons.joint_velocity_limits = cons.joint_torque_limits = 1
    o = RSC.Objective(r, cost, cons, 0.0, dt, steps)
    rng = np.random.default_rng(8)
    nominal = rng.uniform(-3.0, 3.0, (steps, nu))
    sigma, lo, hi = np.full(nu, 1.5), np.full(nu, -4.0), np.full(nu, 4.0)
    q_traj, v_traj = np.zeros((steps + 1, n, nq)), np.zeros((steps + 1, n, nv))
    q_traj[0] = ANYMAL_Q_STANDING
    pts = np.tile(anymal_contact_points(m).reshape(-1), (steps, n, 1))
    active = [[1, 1, 1, 1]] * steps
    d = {k: DeviceArray(x) for k, x in (("nominal", nominal), ("sigma", sigma), ("lo", lo), ("hi", hi), ("samples", np.zeros((steps, n, nu))),
                                        ("q", q_traj), ("v", v_traj), ("u", np.zeros((steps, n, nu))), ("a", np.zeros((steps, n, nv))),
                                        ("f", np.zeros((steps, n, 12))), ("pts", pts), ("cost", np.zeros(n)), ("viol", np.zeros(n)),
                                        ("w", np.zeros(n)), ("stats", np.zeros(5)), ("new", np.zeros((steps, nu))))}
    pol = capi.RbdPolicy()
    pol.u_ff = d["samples"].ptr
    io = capi.RbdScoreIO()
    for key, name in (("q_traj", "q"), ("v_traj", "v"), ("u_traj", "u"), ("a_traj", "a"), ("f_traj", "f"), ("cost", "cost"), ("violation", "viol")):
        setattr(io, key, d[name].ptr)
    lib = r.lib
    capi.check(RS.perturb_raw(r, n, 0, steps, d["nominal"], d["sigma"], d["lo"], d["hi"], SEED, 0, d["samples"], device=True), "perturb")
    capi.check(lib.idocp_rbd_rollout_policy_device(r.h, n, steps, F._act(np.asarray(active).reshape(-1)), dt, dt, C.byref(pol), d["pts"].ptr, d["q"].ptr,
                                                   d["v"].ptr, d["u"].ptr, d["a"].ptr, d["f"].ptr, 0), "rollout")
    capi.check(RSC.score_raw(r, o, n, 0, steps, active, True, False, io, device=True), "score")
    capi.check(RS.weights_raw(r, n, d["cost"], d["viol"], 10.0, 0.5, d["w"], d["stats"], device=True), "weights")
    capi.check(RS.mean_raw(r, n, steps, nu, d["w"], d["u"], d["new"], device=True), "mean")
    capi.check(lib.idocp_rbd_synchronize(r.h), "synchronize")
    c, g, u_traj = d["cost"].numpy(), d["viol"].numpy(), d["u"].numpy()
    assert np.isfinite(c).all() and np.isfinite(g).all() and c.std() > 0
    want_w, want_stats = RS.reference_weights(c, g, 10.0, 0.5)
    want = RS.reference_mean(want_w, u_traj)
    print("cost %.4g .. %.4g, stats %s" % (c.min(), c.max(), d["stats"].numpy()))
    check(d["stats"].numpy(), want_stats, "stats")
    check(d["w"].numpy(), want_w, "weights")
    check(d["new"].numpy(), want, "new nominal")
    check(u_traj, RS.reference_perturb(n, 0, nominal, sigma, lo, hi, SEED, 0), "the torques applied are the samples")
    assert np.abs(d["new"].numpy() - nominal).max() > 1e-3            # (the update moves the nominal)
    o.close()
