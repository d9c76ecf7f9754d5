"""The host-side discretiser of the contact path (idocp_amd/csrc/ocp_capi.hip `discretize`: ContactSequence + OCPDiscretizer of the reference,
contact_sequence.hxx:56-333, ocp_discretizer.hxx:65-374) against the oracle's restatement, DIFFERENTIALLY on random contact sequences: random horizon,
random number of events, switching times anywhere -- beyond the horizon, a hair's breadth from a grid point, equal, decreasing --, random feet touching
down and lifting off.  Every push must be accepted or refused by both; every chain both produce must be the same chain (kinds, indices, slots,
contact rows, time steps to 1e-15), at the initial time and after the horizon has moved.  The hand-picked sequences of tests/test_hybrid_gpu.py
(trot, run, jump, pops) are points of this space.  The sequences come from tests/discretiser_fuzz.py, which tests/test_ocp_chain_host.py
runs through the host-only planner (idocp_amd/csrc/ocp_chain.hpp); here they go through the C ABI's wrappers and the upload."""
import ctypes as C

import numpy as np
import pytest

from discretiser_fuzz import forward_euler_stream, parnmpc_stream
from helpers import HipOCP, OracleOCP, P, anymal_contact_points, anymal_model, anymal_problem, arr
from idocp_amd import capi

pytestmark = pytest.mark.gpu


def chains(o, g, t, cap):
    IA = lambda: (C.c_int * cap)()
    k, i, s, d, w = IA(), IA(), IA(), IA(), IA()
    dt = np.zeros(cap)
    Mg = g.lib.idocp_ocp_get_chain(g.h, t, cap, k, i, s, P(dt), d, w)
    ko, io, so, wo, do = IA(), IA(), IA(), IA(), IA()
    tto, dto = np.zeros(cap), np.zeros(cap)
    Mo = o.lib.oracle_ocp_chain(o.h, t, ko, io, so, P(tto), P(dto), wo, do)
    cg = [(k[p], i[p], s[p], d[p], w[p] > 0, dt[p]) for p in range(max(Mg, 0))]
    co = [(ko[p], io[p], so[p], do[p], wo[p] >= 0, dto[p]) for p in range(max(Mo, 0))]
    return Mg, Mo, cg, co


def test_random_contact_sequences_discretise_like_the_oracle():
    m = anymal_model()
    cost, cons = anymal_problem(m, trotting_ref=False)
    pts = anymal_contact_points(m)
    olib = OracleOCP(m, cost, cons, 0.5, 10, max_num_impulse=1).lib
    olib.oracle_ocp_pop_back_contact_status.argtypes = [C.c_void_p]      # (helpers sets these lazily, inside its wrappers)
    olib.oracle_ocp_pop_front_contact_status.argtypes = [C.c_void_p]
    stats = dict(sequences=0, pushes=0, refused=0, chains=0, chains_refused=0, events_in_chains=0)

    class Pair:
        def create(self, trial, T, N, E):
            self.g, self.o = HipOCP(m, cost, cons, T, N, max_num_impulse=E), OracleOCP(m, cost, cons, T, N, max_num_impulse=E)
            stats["sequences"] += 1

        def status(self, active):
            for s in (self.g, self.o):
                s.set_contact_status(active, pts)

        def push(self, trial, j, nxt, time):
            g, o = self.g, self.o
            rg = g.lib.idocp_ocp_push_back_contact_status(g.h, (C.c_int * 4)(*[int(x) for x in nxt]), P(arr(pts)), time)
            ro = o.lib.oracle_ocp_push_back_contact_status(o.h, (C.c_int * 4)(*[int(x) for x in nxt]), P(arr(pts)), time)
            stats["pushes"] += 1
            assert (rg == 0) == (ro == 0), (trial, j, "push accepted by one, refused by the other", rg, ro, capi.lib().idocp_last_error())
            if rg != 0:
                stats["refused"] += 1
            return rg == 0

        def pop(self, trial, fn):
            g, o = self.g, self.o
            rg = getattr(g.lib, "idocp_ocp_%s_contact_status" % fn)(g.h)
            ro = getattr(o.lib, "oracle_ocp_%s_contact_status" % fn)(o.h)
            assert (rg == 0) == (ro == 0), (trial, fn, rg, ro)
            stats["pops"] = stats.get("pops", 0) + 1

        def chain(self, trial, t, cap):
            Mg, Mo, cg, co = chains(self.o, self.g, t, cap)
            assert (Mg > 0) == (Mo > 0), (trial, t, "discretisation accepted by one, refused by the other", Mg, Mo, capi.lib().idocp_last_error())
            if Mg <= 0:
                stats["chains_refused"] += 1
                return
            stats["chains"] += 1
            assert Mg == Mo, (trial, t, Mg, Mo)
            for p, (a, b) in enumerate(zip(cg, co)):
                assert a[:5] == b[:5] and abs(a[5] - b[5]) <= 1e-15, (trial, t, p, a, b)
            stats["events_in_chains"] += sum(1 for a in cg if a[0] in (1, 3))

    forward_euler_stream(Pair())
    print(stats)
    assert stats["chains"] > 1000 and stats["events_in_chains"] > 800 and stats["refused"] > 80 and stats["pops"] > 300, stats


def test_random_contact_sequences_discretise_like_the_oracle_parnmpc():
    """The same for ParNMPCSolver's chain (ParNMPCDiscretizer, parnmpc_discretizer.hxx: backward-Euler stages, the aux stage BEHIND its impulse, no
    terminal stage of its own -- the GPU chain ends with a placeholder)."""
    from helpers import HipParNMPC, OracleParNMPC
    m = anymal_model()
    cost, cons = anymal_problem(m, trotting_ref=False)
    pts = anymal_contact_points(m)
    KIND = {"stage": 0, "impulse": 1, "aux": 2, "lift": 3, "terminal": 4}
    stats = dict(pushes=0, refused=0, chains=0, chains_refused=0, events_in_chains=0)

    class Pair:
        def create(self, trial, T, N, E):
            self.g, self.o = HipParNMPC(m, cost, cons, T, N, max_num_impulse=E), OracleParNMPC(m, cost, cons, T, N, max_num_impulse=E)

        def status(self, active):
            for s in (self.g, self.o):
                s.set_contact_status(active, pts)

        def push(self, trial, j, nxt, time):
            g, o = self.g, self.o
            arg = (C.c_int * 4)(*[int(x) for x in nxt])
            rg = g.lib.idocp_ocp_push_back_contact_status(g.h, arg, P(arr(pts)), time)
            ro = o.lib.oracle_parnmpc_push_back_contact_status(o.h, arg, P(arr(pts)), time)
            stats["pushes"] += 1
            assert (rg == 0) == (ro == 0), (trial, j, rg, ro, capi.lib().idocp_last_error())
            if rg != 0:
                stats["refused"] += 1
            return rg == 0

        def chain(self, trial, t, cap):
            g, o = self.g, self.o
            IA = lambda: (C.c_int * cap)()
            k, i, s_, d, w = IA(), IA(), IA(), IA(), IA()
            dtg = np.zeros(cap)
            Mg = g.lib.idocp_ocp_get_chain(g.h, t, cap, k, i, s_, P(dtg), d, w)
            ko, io, so, do, lo = IA(), IA(), IA(), IA(), IA()
            tto, dto = np.zeros(cap), np.zeros(cap)
            Mo = o.lib.oracle_parnmpc_chain(o.h, t, cap, ko, io, so, P(tto), P(dto), do, lo)
            assert (Mg > 0) == (Mo > 0), (trial, t, "accepted by one, refused by the other", Mg, Mo, capi.lib().idocp_last_error())
            if Mg <= 0:
                stats["chains_refused"] += 1
                return
            stats["chains"] += 1
            assert Mg == Mo + 1 and k[Mg - 1] == KIND["terminal"], (trial, t, Mg, Mo)      # (the placeholder)
            for p in range(Mo):
                ok = ko[p] if ko[p] != KIND["terminal"] else KIND["stage"]                # (the oracle's last stage carries the terminal cost)
                assert (k[p], d[p]) == (ok, do[p]) and abs(dtg[p] - dto[p]) <= 1e-15, (trial, t, p, (k[p], d[p], dtg[p]), (ok, do[p], dto[p]))
            stats["events_in_chains"] += sum(1 for p in range(Mo) if ko[p] in (1, 3))

    parnmpc_stream(Pair())
    print(stats)
    assert stats["chains"] > 300 and stats["chains_refused"] > 100 and stats["events_in_chains"] > 200 and stats["refused"] > 30, stats
