"""Both backward Riccati sweeps and the forward sweep ALONE on random LQ problems along chains with discrete events, held to the dense KKT referee
of tests/riccati_chain_cases.py -- no oracle, no recursion, no restatement in between.  The chains (riccati_chain_cases.CHAINS): plain ones of
N = 1, 2, 5 (the non-hybrid instantiations; M - 1 = 1, 2, 5 are the forward sweep's prefetch edges and both parities), touchdowns of one to four feet
at once (3, 6, 9, 12 switching rows, impulse rows to match), one chain with lift, impulse and aux nodes around a switching stage, and one whose
switching stage is chain position 0.  Three instances hold three different problems, each against its own referee.

The FUSED forward sweep (ocp_forward_expand_kernel) is not run here: it advances the velocity rows as dv+ = dv + dt (w - t) + Fv from the expansion
record (MJtJinv, MJtJinv_dIDCdqv; ocp_expand_kernel.hip, wavefront 0 of the kernel), not from Fvq, Fvv, Fvu of the kkt record, so its dq, dv, du
depend on a record these tests do not inject."""
import ctypes as C

import numpy as np
import pytest

import riccati_chain_cases as rc
from helpers import ANYMAL_Q_STANDING, HipOCP, P, anymal_contact_points, anymal_model, anymal_problem, arr, force_forms
from idocp_amd import capi

pytestmark = pytest.mark.gpu
BAR = 1e-10      # the bar of this layer (tests/test_golden_riccati.py): max |have - want| / max(1, max |want|)


def scaled(have, want):
    want = np.asarray(want)
    return float(np.abs(np.asarray(have) - want).max() / max(1.0, np.abs(want).max()))


def on_device(h, a):
    d = C.c_void_p()
    a = arr(a)
    capi.check(h.lib.idocp_device_alloc(C.byref(d), a.nbytes), "alloc")
    capi.check(h.lib.idocp_device_upload(d, a.ctypes.data, a.nbytes), "upload")
    return d


@pytest.mark.parametrize("sweep", [0, 1])
@pytest.mark.parametrize("name", list(rc.CHAINS))
def test_sweeps_alone_equal_the_dense_kkt_solution(name, sweep, monkeypatch):
    force_forms(monkeypatch, sweep=sweep, fused=0)
    spec, seed = rc.CHAINS[name], rc.SEEDS[name]
    m = anymal_model()
    cost, cons = anymal_problem(m, trotting_ref=False)
    h = HipOCP(m, cost, cons, spec["N"] * rc.DT, spec["N"], batch=rc.BATCH, max_num_impulse=spec["E"])
    rc.prepare(h, spec, m, anymal_contact_points(m), ANYMAL_Q_STANDING.copy())      # one update(): discretises, sizes every record
    chain = rc.chain_key(h.chain(0.0))
    rc.check_chain(chain, spec)
    M = len(chain)
    # the form the launch takes: the per-handle setting, and HYBRID exactly when the chain carries a switching constraint
    assert h.lib.idocp_ocp_riccati_sweep(h.h) == sweep and h.lib.idocp_ocp_fused_forward(h.h) == 0
    hybrid = any(c[3] > 0 for c in chain)
    assert hybrid == bool(spec["sw_rows"])
    refs, q0s, v0s = [], [], []
    for inst in range(rc.BATCH):
        q0, v0, dx0 = rc.initial_state(h.get_chain("q", M, inst)[0], h.get_chain("v", M, inst)[0], seed, inst)
        rc.inject_hip(h, rc.draw_problem(chain, seed, inst), inst)
        refs.append(rc.referee(chain, seed, inst, dx0))
        q0s.append(q0); v0s.append(v0)
    dq_, dv_ = on_device(h, np.stack(q0s)), on_device(h, np.stack(v0s))
    capi.check(h.lib.idocp_ocp_launch_kernel(h.h, 2, dq_, dv_), "backward sweep")
    capi.check(h.lib.idocp_ocp_launch_kernel(h.h, 3, dq_, dv_), "forward sweep")
    capi.check(h.lib.idocp_ocp_synchronize(h.h), "synchronize")
    h.lib.idocp_device_free(dq_)
    h.lib.idocp_device_free(dv_)
    worst = {}
    failures = []
    for inst, ref in enumerate(refs):
        Pm, s, K, k = h.riccati_chain(M, inst)
        dq, dv, du = (h.get_chain(f, M, inst) for f in ("dq", "dv", "du"))
        pairs = []
        for p in range(M):
            pairs += [("P", p, Pm[p], ref["P"][p]), ("s", p, s[p], ref["s"][p]), ("dq", p, dq[p], ref["dq"][p]), ("dv", p, dv[p], ref["dv"][p])]
            if p < M - 1:
                if chain[p][0] == "impulse":      # no control there: the sweep's K, k and the forward du must be zero to the bar
                    assert not ref["K"][p].any() and not ref["k"][p].any() and not ref["du"][p].any()
                pairs += [("K", p, K[p], ref["K"][p]), ("k", p, k[p], ref["k"][p]), ("du", p, du[p], ref["du"][p])]
            if chain[p][3] > 0:
                Mx, mx = rc.hip_switching_policy(h, inst, p, chain[p][3])
                pairs += [("M", p, Mx, ref["Mxi"][p]), ("m", p, mx, ref["mxi"][p])]
        for what, p, have, want in pairs:
            err = scaled(have, want)
            worst[what] = max(worst.get(what, 0.0), err)
            if not err <= BAR:
                failures.append((what, inst, p, chain[p], err))
    print("%s, S3 form %d%s (M = %d) against the dense KKT referee:  %s" % (name, sweep, " HYBRID" if hybrid else "", M,
                                                                             "  ".join("%s %.1e" % kv for kv in worst.items())))
    assert not failures, failures[:8]


def test_chain_entries_refuse_what_they_cannot_address():
    from helpers import HipParNMPC
    spec = rc.CHAINS["touchdown1"]
    m = anymal_model()
    cost, cons = anymal_problem(m, trotting_ref=False)
    pts = anymal_contact_points(m)
    h = HipOCP(m, cost, cons, spec["N"] * rc.DT, spec["N"], batch=1, max_num_impulse=spec["E"])
    rc.prepare(h, spec, m, pts, ANYMAL_Q_STANDING.copy())
    chain = rc.chain_key(h.chain(0.0))
    M = len(chain)
    carrying = next(p for p, c in enumerate(chain) if c[3] > 0)
    st = rc.draw_problem(chain, 1, 0)
    blocks = [rc._p(a) for a in rc._blocks(st[0])]
    z = P(np.zeros(NXX))
    err = lambda: h.lib.idocp_last_error().decode()
    for bad in (-1, M):
        assert h.lib.idocp_ocp_set_lqr_stage_chain(h.h, 0, bad, *blocks) == -1
        assert err() == "idocp_ocp_set_lqr_stage_chain: position out of range"
        assert h.lib.idocp_ocp_set_switching_constraint(h.h, 0, bad, 3, z, z, z) == -1
        assert err() == "idocp_ocp_set_switching_constraint: position out of range"
        assert h.lib.idocp_ocp_get_switching_policy(h.h, 0, bad, z, z) == -1
        assert err() == "idocp_ocp_get_switching_policy: position out of range"
    assert h.lib.idocp_ocp_set_lqr_stage_chain(h.h, 1, 0, *blocks) == -1
    assert err() == "idocp_ocp_set_lqr_stage_chain: instance out of range"
    assert h.lib.idocp_ocp_set_switching_constraint(h.h, 0, 0, 3, z, z, z) == -1
    assert err() == "idocp_ocp_set_switching_constraint: no switching constraint at position 0"
    assert h.lib.idocp_ocp_get_switching_policy(h.h, 0, 0, z, z) == -1
    assert err() == "idocp_ocp_get_switching_policy: no switching constraint at position 0"
    assert h.lib.idocp_ocp_set_switching_constraint(h.h, 0, carrying, 6, z, z, z) == -1
    assert err() == "idocp_ocp_set_switching_constraint: dimi 6 is not the 3 rows of the node"
    g = HipParNMPC(m, cost, cons, 5 * rc.DT, 5, batch=1)
    assert g.lib.idocp_ocp_set_lqr_stage_chain(g.h, 0, 0, *blocks) == -1
    assert err() == "idocp_ocp_set_lqr_stage_chain: a ParNMPC handle has no Riccati sweep to inject into"
    assert g.lib.idocp_ocp_set_switching_constraint(g.h, 0, 0, 3, z, z, z) == -1
    assert err() == "idocp_ocp_set_switching_constraint: a ParNMPC handle has no Riccati sweep to inject into"
    assert g.lib.idocp_ocp_get_switching_policy(g.h, 0, 0, z, z) == -1
    assert err() == "idocp_ocp_get_switching_policy: a ParNMPC handle has no Riccati sweep to inject into"


NXX = rc.NU * rc.NX      # room for the largest block a refused call could be handed
