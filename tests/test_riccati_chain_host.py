"""The dense KKT referee of tests/riccati_chain_cases.py on the CPU: against the committed 3-stage fixture, against the oracle's backward and forward
recursions on every chain (which settles the referee's conventions -- signs of s, xi, m, the row packing -- before a kernel is held to it), its own
float64 error, and the sensitivity of the problems it draws to the slips the GPU tests are there to catch.  No GPU."""
import json
import os

import numpy as np
import pytest

import riccati_chain_cases as rc
from helpers import ANYMAL_Q_STANDING, GOLDEN, OracleOCP, P, anymal_contact_points, anymal_model, anymal_problem, arr

REFEREE_BAR = 1e-13      # the referee's own float64 error (distance of the unrefined solve from the refined one), stage-scaled
ORACLE_BAR = 1e-12       # FP64 oracle against referee: 100 x under the bar the kernels are held to


def scaled(have, want):
    want = np.asarray(want)
    return float(np.abs(np.asarray(have) - want).max() / max(1.0, np.abs(want).max()))


def test_referee_reproduces_the_committed_three_stage_fixture():
    g = json.load(open(os.path.join(GOLDEN, "riccati_lqr.json")))
    stages = []
    for st in g["stages"]:
        d = {k: np.asarray(v) for k, v in st.items() if k != "dt"}
        d.update(kind="stage", dt=st["dt"], dimi=0)
        stages.append(d)
    stages.append(dict(kind="terminal", dt=0.0, dimi=0, Qxx=np.asarray(g["terminal"]["Qxx"]), lx=np.asarray(g["terminal"]["lx"])))
    ref = rc.solve_chain(stages)
    own = max(ref["first"].values())
    assert own <= REFEREE_BAR, ref["first"]
    # the bound: the referee's own reported float64 error plus the fixture's.  The fixture is one unrefined float64 solve of these very systems
    # (gen_golden_riccati.py), i.e. what "first" measures here, and "first" is itself held to REFEREE_BAR above: that bar stands in for it
    worst = 0.0
    for i, r in enumerate(g["riccati"]):
        for name in ("P", "s") + (("K", "k") if i < g["N"] else ()):
            err = scaled(ref[name][i], r[name])
            worst = max(worst, err)
            assert err <= own + REFEREE_BAR, (i, name, err, own)
    print("referee against riccati_lqr.json: worst %.2e (the referee's own float64 error %.2e, last correction %.1e)" % (worst, own, ref["last"]))


@pytest.fixture(scope="module")
def anymal():
    m = anymal_model()
    cost, cons = anymal_problem(m, trotting_ref=False)
    return m, cost, cons, anymal_contact_points(m)


@pytest.mark.parametrize("name", list(rc.CHAINS))
def test_oracle_recursions_equal_the_dense_kkt_solution(name, anymal):
    """Backward (P, s, K, k, M, m) and forward (dq, dv, du, dxi) recursion of the FP64 oracle against the referee, three different problems per chain;
    the referee's own error on the same problems."""
    m, cost, cons, pts = anymal
    spec, seed = rc.CHAINS[name], rc.SEEDS[name]
    o = OracleOCP(m, cost, cons, spec["N"] * rc.DT, spec["N"], max_num_impulse=spec["E"])
    rc.prepare(o, spec, m, pts, ANYMAL_Q_STANDING.copy())
    chain = rc.chain_key(rc.oracle_chain(o))
    rc.check_chain(chain, spec)
    M = len(chain)
    qs, vs = o.get_chain("q", M)[0], o.get_chain("v", M)[0]
    worst, own = {}, {}
    for inst in range(rc.BATCH):
        q0, v0, dx0 = rc.initial_state(qs, vs, seed, inst)
        stages = rc.draw_problem(chain, seed, inst)
        ref = rc.referee(chain, seed, inst, dx0)
        for key, val in ref["first"].items():
            own[key] = max(own.get(key, 0.0), val)
        assert ref["last"] <= 1e-15
        assert np.abs(ref["P"] - ref["P"].transpose(0, 2, 1)).max() <= 1e-12 * np.abs(ref["P"]).max()
        rc.inject_oracle(o, stages)
        assert o.lib.oracle_ocp_backward_riccati_only(o.h) == 0
        Pm, s, K, k = o.riccati_chain(M)
        pairs = []
        for p in range(M):
            pairs += [("P", p, Pm[p], ref["P"][p]), ("s", p, s[p], ref["s"][p])]
            if p < M - 1:
                pairs += [("K", p, K[p], ref["K"][p]), ("k", p, k[p], ref["k"][p])]
                if chain[p][0] == "impulse":
                    assert not K[p].any() and not k[p].any() and not ref["K"][p].any()
            if chain[p][3] > 0:
                Mx, mx = rc.oracle_switching_policy(o, p, chain[p][3])
                pairs += [("M", p, Mx, ref["Mxi"][p]), ("m", p, mx, ref["mxi"][p])]
        assert o.lib.oracle_ocp_forward_riccati_only(o.h, P(arr(q0)), P(arr(v0))) == 0
        dq, dv, du, dxi = (o.get_chain(f, M) for f in ("dq", "dv", "du", "dxi"))
        for p in range(M):
            pairs += [("dq", p, dq[p], ref["dq"][p]), ("dv", p, dv[p], ref["dv"][p])]
            if p < M - 1:
                pairs.append(("du", p, du[p], ref["du"][p]))
            if chain[p][3] > 0:
                pairs.append(("dxi", p, dxi[p][:chain[p][3]], ref["dxi"][p]))
        for what, p, have, want in pairs:
            err = scaled(have, want)
            worst[what] = max(worst.get(what, 0.0), err)
            assert err <= ORACLE_BAR, (name, inst, what, p, chain[p], err)
    assert max(own.values()) <= REFEREE_BAR, own
    fmt = lambda d: "  ".join("%s %.1e" % kv for kv in d.items())
    print("%s (M = %d): oracle against referee  %s\n    the referee's own float64 error  %s" % (name, M, fmt(worst), fmt(own)))


@pytest.mark.parametrize("variant", ["drop_switch", "shift_switch", "grid_dt_on_impulse"])
def test_the_problems_notice_the_slips_they_are_there_for(variant, anymal):
    """A test of the test: dropping the switching rows, shifting the rows of Phix by one against Phiu and P, or giving the impulse node the grid
    time step must move the referee's K of the carrying stage, or P in front of the event, by more than 1e-3 relative -- else a kernel with that
    slip would pass at 1e-10."""
    m, cost, cons, pts = anymal
    moved = {}
    for name in ("touchdown1", "touchdown4", "multi", "early"):
        spec, seed = rc.CHAINS[name], rc.SEEDS[name]
        o = OracleOCP(m, cost, cons, spec["N"] * rc.DT, spec["N"], max_num_impulse=spec["E"])
        rc.prepare(o, spec, m, pts, ANYMAL_Q_STANDING.copy())
        chain = rc.chain_key(rc.oracle_chain(o))
        carrying = next(p for p, c in enumerate(chain) if c[3] > 0)
        impulse = next(p for p, c in enumerate(chain) if c[0] == "impulse")
        good, bad = rc.referee(chain, seed, 0), rc.referee(chain, seed, 0, None, variant)
        rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
        if variant == "grid_dt_on_impulse":
            moved[name] = rel(bad["P"][impulse], good["P"][impulse])                 # P in front of the event: the cost-to-go AT the impulse node
        else:
            moved[name] = rel(bad["K"][carrying], good["K"][carrying])
        assert moved[name] > 1e-3, (variant, name, moved[name])
    print("%s moves the referee by  %s" % (variant, "  ".join("%s %.1e" % kv for kv in moved.items())))
