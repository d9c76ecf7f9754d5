"""idocp_rbd_score_al and idocp_rbd_multiplier_update on the GPU (rbd_al_kernel.hip) on the cases of test_rbd_penalty_gpu.py: n = 5, steps = 4, ANYmal
under both cone kinds and the chain of 2 joints, bounds at the medians so that rows are active.  lambda is drawn with the correct signs
(rbd_al.draw_multipliers): a third of the rows zero, a third small, a third large enough to switch on a row that its value alone leaves off --
asserted first.  sq_shifted, lambda+ and both statistics against the numpy referee at 1e-11; host and device form the same bits; n = 5 against
n = 1; one window against windows of 1 + 3 steps with accumulate; lambda_out aliasing lambda_traj; lambda = NULL and all zeros equal to
idocp_rbd_score_penalty bit for bit; a NaN in one sample's lambda stays there; the refusals of mu; multiplier_rows."""
import functools
import math

import numpy as np
import pytest

import rbd_al as AL
import rbd_penalty as PN
import rbd_score as RS
from idocp_amd import capi
from rbd_batch import E_ARG, Rbd
from test_rbd_penalty_gpu import CASES, MU, N, STEPS, T0, case, same

pytestmark = pytest.mark.gpu

BAR = 1e-11


@functools.lru_cache(maxsize=None)
def multipliers(which, cone, push=True):
    """lambda [STEPS][N][L] for the rollout of case(which, cone, push), and the referee at it"""
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone, push)
    zero = AL.reference_score_update_batch(mm, M, cons, MU, dt, None, q[:STEPS], v[:STEPS], u, a, f, active)
    L = AL.multiplier_rows(mm, M, cons)
    base = np.array([[AL.al_rows(mm, M, cons, MU, None, q[k, i], v[k, i], u[k, i], a[k, i], None if f is None else f[k, i],
                                 list(active[k]) if active is not None else [])["unshifted"] for i in range(N)] for k in range(STEPS)])
    lam = AL.draw_multipliers(np.random.default_rng([11, len(which), L]), mm, M, cons, MU, (STEPS, N), base)
    ref = AL.reference_score_update_batch(mm, M, cons, MU, dt, lam, q[:STEPS], v[:STEPS], u, a, f, active)
    return lam, ref, zero, base


def rel(x, want):
    return np.abs(x - want).max() / max(np.abs(want).max(), 1e-300)


@pytest.mark.parametrize("which,cone", CASES)
def test_score_and_update_against_the_referee(which, cone):
    mm, M, cost, cons, tables, active, pts, ts, dt, (q, v, u, a, f) = case(which, cone, True)
    lam, ref, zero, base = multipliers(which, cone)
    L = lam.shape[2]
    qs, vs = q[:STEPS], v[:STEPS]
    r = Rbd(mm)
    o = RS.Objective(r, cost, cons, T0, dt, STEPS)
    bare = RS.Objective(r, cost, None, T0, dt, STEPS)
    assert r.lib.idocp_rbd_objective_multiplier_rows(o.h) == L == {"linearized": 68, "nonlinear": 56, None: 8}[cone]
    assert r.lib.idocp_rbd_objective_multiplier_rows(bare.h) == 0 and r.lib.idocp_rbd_objective_multiplier_rows(None) == 0
    # 0. the draw: zero rows, and a row that its value alone leaves off is switched on by its multiplier
    cone_rows = np.arange(L) >= 4 * mm.nu
    off = np.where(cone_rows, base <= 0, base == 0)
    plus0 = zero["lambda_plus"]
    assert (lam == 0).any() and (off & (plus0 == 0) & (ref["lambda_plus"] != 0)).any() and (ref["lambda_plus"] == 0).any()
    assert (lam[..., 4 * mm.nu:] >= 0).all()
    # 1. against the referee
    sq = AL.score_al(r, o, MU, lam, qs, vs, u, a, f, active)
    plus, inf, ch = AL.multiplier_update(r, o, MU, lam, qs, vs, u, a, f, active)
    for name, got, want in (("sq_shifted", sq, ref["sq_shifted"]), ("lambda+", plus, ref["lambda_plus"]), ("infeasibility", inf, ref["infeasibility"]),
                            ("multiplier_change", ch, ref["multiplier_change"])):
        d = rel(got, want)
        print("%s %s %s: |gpu - referee| / |referee| %.2e (bar %.0e)" % (which, cone, name, d, BAR))
        assert np.isfinite(got).all() and d <= BAR, (which, cone, name, d)
    assert ((plus != 0) == (ref["lambda_plus"] != 0)).all()      # (the same rows are active)
    assert (inf > 0).all() and (ch > 0).all() and not same(sq, PN.score_penalty(r, o, qs, vs, u, a, f, active))
    # 2. the device form: the same bits
    assert same(AL.score_al(r, o, MU, lam, qs, vs, u, a, f, active, device=True), sq)
    dplus, dinf, dch = AL.multiplier_update(r, o, MU, lam, qs, vs, u, a, f, active, device=True)
    assert same(dplus, plus) and same(dinf, inf) and same(dch, ch)
    # 3. n = 5 against n = 1
    c = lambda x, i: None if x is None else np.ascontiguousarray(x[:, i:i + 1])      # noqa: E731
    for i in (0, 3):
        assert same(AL.score_al(r, o, MU, c(lam, i), c(qs, i), c(vs, i), c(u, i), c(a, i), c(f, i), active), sq[i:i + 1])
        one = AL.multiplier_update(r, o, MU, c(lam, i), c(qs, i), c(vs, i), c(u, i), c(a, i), c(f, i), active)
        assert same(one[0], plus[:, i:i + 1]) and same(one[1], inf[i:i + 1]) and same(one[2], ch[i:i + 1])
    # 4. one window against 1 + 3 steps with accumulate
    w = lambda x, s: None if x is None else x[s]      # noqa: E731
    a0, a1 = slice(0, 1), slice(1, STEPS)
    first = AL.score_al(r, o, MU, lam[a0], qs[a0], vs[a0], u[a0], a[a0], w(f, a0), w(active, a0))
    both = AL.score_al(r, o, MU, lam[a1], qs[a1], vs[a1], u[a1], a[a1], w(f, a1), w(active, a1), first_step=1, accumulate=first)
    assert same(both, sq) and not same(first, sq)
    p0, i0, c0 = AL.multiplier_update(r, o, MU, lam[a0], qs[a0], vs[a0], u[a0], a[a0], w(f, a0), w(active, a0))
    p1, i1, c1 = AL.multiplier_update(r, o, MU, lam[a1], qs[a1], vs[a1], u[a1], a[a1], w(f, a1), w(active, a1), first_step=1, accumulate=(i0, c0))
    assert same(np.concatenate([p0, p1]), plus) and same(i1, inf) and same(c1, ch)
    # 5. lambda_out aliasing lambda_traj, both forms
    for device in (False, True):
        got = AL.multiplier_update(r, o, MU, lam, qs, vs, u, a, f, active, device=device, in_place=True)
        assert same(got[0], plus) and same(got[1], inf) and same(got[2], ch)
    # 6. lambda = NULL and all zeros: idocp_rbd_score_penalty bit for bit
    pen = PN.score_penalty(r, o, qs, vs, u, a, f, active)
    assert np.array_equal(AL.score_al(r, o, MU, None, qs, vs, u, a, f, active), pen)
    assert np.array_equal(AL.score_al(r, o, MU, np.zeros_like(lam), qs, vs, u, a, f, active), pen)
    zplus, zinf, zch = AL.multiplier_update(r, o, MU, None, qs, vs, u, a, f, active, L=L)
    assert rel(zplus, plus0) <= BAR and rel(zinf, zero["infeasibility"]) <= BAR and same(zch, np.abs(zplus).max(axis=(0, 2)))
    # 7. a NaN in one sample's lambda poisons that sample alone
    bad = lam.copy()
    row = int(np.argmax(base[1, 4] != 0))      # (a row that is read: kinds switched on everywhere)
    bad[1, 4, row] = np.nan
    got = AL.score_al(r, o, MU, bad, qs, vs, u, a, f, active)
    assert np.isnan(got[4]) and same(got[:4], sq[:4])
    bplus, binf, bch = AL.multiplier_update(r, o, MU, bad, qs, vs, u, a, f, active)
    want = plus.copy()
    want[1, 4] = np.nan
    assert same(bplus, want) and np.isnan(binf[4]) and np.isnan(bch[4]) and same(binf[:4], inf[:4]) and same(bch[:4], ch[:4])
    # 8. mu <= 0 or not finite: IDOCP_E_ARG
    out = np.zeros(N)
    for mu in (0.0, -1.0, math.nan, math.inf):
        for call, who in ((lambda: AL.score_al_raw(r, o, N, 0, STEPS, active, 0, qs, vs, u, a, f, mu, lam, out), "idocp_rbd_score_al"),
                          (lambda: AL.update_raw(r, o, N, 0, STEPS, active, 0, qs, vs, u, a, f, mu, lam, lam.copy(), out, out), "idocp_rbd_multiplier_update")):
            rc = call()
            assert rc == E_ARG and capi.last_error().startswith(who + ": ") and "mu must be positive and finite" in capi.last_error(), (mu, capi.last_error())
    for x in (o, bare):
        x.close()
    r.close()
