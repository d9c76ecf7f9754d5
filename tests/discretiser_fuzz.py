"""The random contact sequences of the discretiser tests (tests/test_discretiser_fuzz_gpu.py on the device handles, tests/test_ocp_chain_host.py on
the host-only planner): random horizon, random number of events, switching times anywhere -- beyond the horizon, a hair's breadth from a grid point,
equal, decreasing --, random feet touching down and lifting off, events leaving at either end.  The streams draw from their generator in a fixed
order and hand every step to a backend:

    create(trial, T, N, E)      a new pair of solvers (or whatever the backend compares)
    status(active)              setContactStatusUniformly
    push(trial, j, nxt, time)   pushBackContactStatus; returns whether it was ACCEPTED
    pop(trial, fn)              "pop_front" | "pop_back"   (forward-Euler stream only)
    chain(trial, t, cap)        discretise at t
"""
import numpy as np


def forward_euler_stream(b, seed=2024, trials=600):
    rng = np.random.default_rng(seed)
    for trial in range(trials):
        N = int(rng.integers(6, 41))
        dt = rng.uniform(0.015, 0.06)
        T = N * dt
        E = int(rng.integers(1, 7))
        b.create(trial, T, N, E)
        active = rng.integers(0, 2, size=4)
        b.status(active)
        n_ev = int(rng.integers(0, E + 3))                   # (sometimes more than the containers hold)
        times = np.sort(rng.uniform(0.02 * T, 1.25 * T, size=n_ev))
        for j in range(n_ev):
            mode = rng.integers(0, 10)
            if mode == 0:
                times[j] = round(times[j] / dt) * dt + rng.choice([-1, 1]) * 10.0 ** rng.integers(-12, -3)      # a hair from a grid point
            elif mode == 1 and j > 0:
                times[j] = times[j - 1]                                                                       # the same instant twice
            elif mode == 2 and j > 0:
                times[j] = times[j - 1] - rng.uniform(0, 0.5 * dt)                                             # back in time
            elif mode == 3 and j > 0:
                times[j] = times[j - 1] + 10.0 ** rng.integers(-9, -3)                                        # two events in one interval
        for j in range(n_ev):
            nxt = active.copy()
            flip = rng.integers(0, 2, size=4)
            if rng.integers(0, 8) > 0 and not flip.any():
                flip[rng.integers(0, 4)] = 1                 # (now and then: no change at all -- not an event)
            nxt = np.where(flip == 1, 1 - nxt, nxt)
            if b.push(trial, j, nxt, float(times[j])):
                active = nxt
        cap = N + 1 + 3 * E + 8
        for popping in range(int(rng.integers(0, 3))):       # the receding horizon: events leave at either end (ocp_solver.cpp:187-194)
            b.pop(trial, ("pop_front", "pop_back")[int(rng.integers(0, 2))])
        for t in (0.0, float(rng.uniform(0, 0.6 * T)), float(rng.uniform(0.6 * T, 1.3 * T))):
            b.chain(trial, t, cap)


def parnmpc_stream(b, seed=77, trials=300):
    rng = np.random.default_rng(seed)
    for trial in range(trials):
        N = int(rng.integers(6, 41))
        dt = rng.uniform(0.015, 0.06)
        T = N * dt
        E = int(rng.integers(1, 6))
        b.create(trial, T, N, E)
        active = rng.integers(0, 2, size=4)
        b.status(active)
        n_ev = int(rng.integers(0, E + 2))
        times = np.sort(rng.uniform(0.02 * T, 1.2 * T, size=n_ev))
        for j in range(n_ev):
            mode = rng.integers(0, 10)
            if mode == 0:
                times[j] = round(times[j] / dt) * dt + rng.choice([-1, 1]) * 10.0 ** rng.integers(-12, -3)
            elif mode == 1 and j > 0:
                times[j] = times[j - 1] + 10.0 ** rng.integers(-9, -3)
            elif mode == 2 and j > 0:
                times[j] = times[j - 1] - rng.uniform(0, 0.5 * dt)
        for j in range(n_ev):
            flip = rng.integers(0, 2, size=4)
            if rng.integers(0, 8) > 0 and not flip.any():
                flip[rng.integers(0, 4)] = 1
            nxt = np.where(flip == 1, 1 - active, active)
            if b.push(trial, j, nxt, float(times[j])):
                active = nxt
        cap = N + 3 * E + 8
        for t in (0.0, float(rng.uniform(0, 0.6 * T))):
            b.chain(trial, t, cap)
