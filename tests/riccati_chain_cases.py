"""An INDEPENDENT referee for the Riccati sweeps along chains with discrete events: numpy only, no oracle, no recursion.

tests/golden/gen_golden_riccati.py generalised from a grid to a chain.  The input is the chain as idocp_ocp_get_chain reports it -- kind, dt, dimf
and sw_dimi per position; the discretiser is not restated -- and a seed.  From the seed every position of every instance draws its own condensed LQ
stage in the reference's block structure

    min  sum_p  1/2 [x_p; u_p]^T [Qxx Qxu; Qxu^T Quu]_p [x_p; u_p] + lx_p^T x_p + lu_p^T u_p   +   1/2 x_T^T Qf x_T + lf^T x_T
    s.t. x_{p+1} = A_p x_p + B_p u_p + Fx_p,     A = [Fqq Fqv; Fvq Fvv],  B = [0; Fvu],
         Fqq = diag(Fqq6, I),  Fqv = diag(Fqv6, dtq I)                 (floating base: only the leading 6 x 6 blocks are stored)
         Phix_p x_p + Phiu_p u_p + P_p = 0                            (positions with sw_dimi > 0: the switching constraint of the impulse ahead)

with dtq = 0 on an impulse position (kind 1), where the problem also has NO control (the column block of u is absent, and Fqv = 0), and the
reported dt everywhere else (shortened in front of an event, the remainder on an aux or lift position).

For every chain position p the DENSE KKT system of the tail problem p .. terminal is assembled -- the dynamics rows and the switching rows of the
positions that carry them -- and solved with x_p = 0 and x_p = e_j prescribed.  By the definition of the cost-to-go and of the policies,

    multiplier of the initial condition   lambda_p = P_p x_p - s_p        (split_riccati_factorizer.hxx:131-139 of the reference),
    u_p = K_p x_p + k_p,     xi_p = M_p x_p + m_p                           (:139-145)

so P, K, M are differences of columns and s, k, m come from the x_p = 0 column.  The Lagrangian carries the dynamics as  + lambda^T (d - C z),
which is the sign of gen_golden_riccati.py, and the switching constraint as  + xi^T (Phix x + Phiu u + P):  that is the reference's sign,
include/idocp/ocp/forward_switching_constraint.hxx:49-51 (lq += Phiq^T xi, lv += Phiv^T xi, la += Phia^T xi).
One further solve from a given dx_0 yields dq, dv, du of every position and dxi of the switching positions: the forward sweep's answer.

Every solve is done in float64 and then REFINED with residuals formed in numpy.longdouble until the correction is below 1e-15 of the largest entry
of the solution.  Next to the answers the referee returns the size of that last correction and, per quantity, how far the unrefined float64 solve
was from the refined one ("first"): the referee's own float64 error, in the very metric the tests use."""
import ctypes as C
import functools

import numpy as np

NV, NU = 18, 12
NX = 2 * NV
LD = np.longdouble
KINDS = ("stage", "impulse", "aux", "lift", "terminal")

# ---------------------------------------------------------------------------------------------------------------- chains
# Contact sequences on ANYmal; times in units of the grid step.  `expect`: the node kinds, the switching rows and the impulse rows the discretiser
# has to produce for the case to mean what it says (asserted by the tests on whatever the chain getter returns).
DT = 0.05


def _touchdown(feet):
    start = [0 if c in feet else 1 for c in range(4)]
    return dict(N=5, E=1, start=start, events=[([1, 1, 1, 1], 2.6)], sw_rows=[3 * len(feet)], impulse_rows=[3 * len(feet)],
                kinds=["stage", "stage", "stage", "impulse", "aux", "stage", "stage", "terminal"])


CHAINS = {
    "plain1": dict(N=1, E=0, start=[1, 1, 1, 1], events=[], sw_rows=[], impulse_rows=[], kinds=["stage", "terminal"]),
    "plain2": dict(N=2, E=0, start=[1, 1, 1, 1], events=[], sw_rows=[], impulse_rows=[], kinds=["stage"] * 2 + ["terminal"]),
    "plain5": dict(N=5, E=0, start=[1, 1, 1, 1], events=[], sw_rows=[], impulse_rows=[], kinds=["stage"] * 5 + ["terminal"]),
    "touchdown1": _touchdown([2]),
    "touchdown2": _touchdown([0, 3]),
    "touchdown3": _touchdown([0, 1, 3]),
    "touchdown4": _touchdown([0, 1, 2, 3]),      # out of flight
    # lift of two feet, their touchdown, lift of one foot: lift, impulse and aux nodes, a switching stage among plain ones, shortened steps
    "multi": dict(N=8, E=3, start=[1, 1, 1, 1], events=[([0, 1, 1, 0], 1.4), ([1, 1, 1, 1], 4.6), ([1, 0, 1, 1], 6.5)], sw_rows=[6], impulse_rows=[6],
                  kinds=["stage", "stage", "lift", "stage", "stage", "stage", "impulse", "aux", "stage", "stage", "lift", "stage", "terminal"]),
    # a touchdown in the second grid interval: the stage two steps ahead of the impulse is chain position 0
    "early": dict(N=5, E=1, start=[1, 0, 0, 1], events=[([1, 1, 1, 1], 1.5)], sw_rows=[6], impulse_rows=[6],
                  kinds=["stage", "stage", "impulse", "aux", "stage", "stage", "stage", "terminal"], sw_position=0),
}
SEEDS = {name: 7100 + 17 * i for i, name in enumerate(CHAINS)}
BATCH = 3


def apply_sequence(solver, spec, pts):
    """The contact sequence of a case on a HipOCP or OracleOCP wrapper (both spell the calls the same way)."""
    solver.set_contact_status(spec["start"], pts)
    for active, when in spec["events"]:
        solver.push_back_contact_status(active, pts, when * DT)


def chain_key(chain):
    """A chain as the referee takes it, hashable: (kind name, dt, dimf, sw_dimi) per position."""
    return tuple((c["kind"], float(c["dt"]), int(c["dimf"]), int(c["sw_dimi"])) for c in chain)


def check_chain(chain, spec):
    """The chain is the one the case was written for."""
    assert [c[0] for c in chain] == spec["kinds"], [c[0] for c in chain]
    assert [c[3] for c in chain if c[3] > 0] == spec["sw_rows"], [c[3] for c in chain]
    assert [c[2] for c in chain if c[0] == "impulse"] == spec["impulse_rows"]
    for kind, dt, _, sw in chain:
        assert (dt == 0.0) == (kind in ("impulse", "terminal")), (kind, dt)
        assert not (sw > 0 and kind == "impulse")
    if "sw_position" in spec:
        assert chain[spec["sw_position"]][3] > 0
    if spec["events"]:      # shortened steps in front of every event, the remainder behind it
        assert sum(1 for kind, dt, _, _ in chain if kind != "impulse" and kind != "terminal" and abs(dt - DT) > 1e-9) >= 2 * len(spec["events"])


# ---------------------------------------------------------------------------------------------------------------- the random problem
def spd(rng, n, lo):
    a = rng.standard_normal((n, n))
    return a @ a.T / n + lo * np.eye(n)


def draw_problem(chain, seed, instance):
    """One LQ stage per chain position, drawn for this instance alone.  Every position draws the same list of blocks (so that the stream does
    not depend on the kinds); an impulse position keeps no control blocks, the terminal position Qxx and lx only."""
    rng = np.random.default_rng([seed, instance])
    out = []
    for kind, dt, _, dimi in chain:
        Qz = spd(rng, NX + NU, 0.5)
        st = dict(kind=kind, dt=0.0 if kind == "impulse" else dt, dimi=dimi,
                  Qxx=Qz[:NX, :NX], Qxu=Qz[:NX, NX:], Quu=Qz[NX:, NX:], Fqq6=np.eye(6) + 0.05 * rng.standard_normal((6, 6)),
                  Fqv6=dt * np.eye(6) + 0.01 * rng.standard_normal((6, 6)), Fvq=0.1 * rng.standard_normal((NV, NV)),
                  Fvv=np.eye(NV) + 0.1 * rng.standard_normal((NV, NV)), Fvu=0.3 * rng.standard_normal((NV, NU)), lx=rng.standard_normal(NX),
                  lu=rng.standard_normal(NU), Fx=0.1 * rng.standard_normal(NX))
        # (drawn at every position, kept where the chain has rows) Phiu = diag(0.8 .. 1.25) x orthonormal rows: full row rank, the square case too
        Phix = 0.1 * rng.standard_normal((NU, NX))
        Qo, _ = np.linalg.qr(rng.standard_normal((NU, NU)))
        Phiu = rng.uniform(0.8, 1.25, NU)[:, None] * Qo
        Pv = 0.1 * rng.standard_normal(NU)
        if dimi > 0:
            st.update(Phix=Phix[:dimi], Phiu=Phiu[:dimi], P=Pv[:dimi])
        if kind == "impulse":
            st["Fqv6"] = np.zeros((6, 6))
            for name in ("Qxu", "Quu", "Fvu", "lu"):
                del st[name]
        if kind == "terminal":
            # the terminal cost-to-go takes Qqq and Qvv (riccati_recursion_solver.cpp:53-56): the problem has no q-v coupling there
            st["Qxx"] = st["Qxx"].copy()
            st["Qxx"][:NV, NV:] = 0.0
            st["Qxx"][NV:, :NV] = 0.0
            st = dict(kind=kind, dt=0.0, dimi=0, Qxx=st["Qxx"], lx=st["lx"])
        out.append(st)
    return out


def AB(st, impulse_dt=None):
    dt = st["dt"] if (st["kind"] != "impulse" or impulse_dt is None) else impulse_dt
    Fqq = np.eye(NV); Fqq[:6, :6] = st["Fqq6"]
    Fqv = dt * np.eye(NV); Fqv[:6, :6] = st["Fqv6"]
    A = np.block([[Fqq, Fqv], [st["Fvq"], st["Fvv"]]])
    B = np.vstack([np.zeros((NV, NU)), st["Fvu"]]) if "Fvu" in st else None
    return A, B


# ---------------------------------------------------------------------------------------------------------------- dense solves
def _refined_solve(Kmat, rhs):
    """Kmat X = rhs in float64, refined with longdouble residuals.  Returns (X refined, X of the plain float64 solve, last correction relative to
    the largest entry of X, iterations)."""
    n = Kmat.shape[0]
    Kinv = np.linalg.inv(Kmat)
    blocks = []      # the nonzero columns of each block of rows: the residual costs nnz, not n^2, longdouble products
    for r0 in range(0, n, 48):
        rows = slice(r0, min(n, r0 + 48))
        cols = np.flatnonzero(np.any(Kmat[rows] != 0.0, axis=0))
        blocks.append((rows, cols, Kmat[rows][:, cols].astype(LD)))
    rl = rhs.astype(LD)
    X0 = np.linalg.solve(Kmat, rhs)      # the plain float64 answer (LU with partial pivoting); the inverse only drives the refinement
    X = X0.astype(LD)
    last, it = np.inf, 0
    for it in range(1, 9):
        res = np.empty_like(X)
        for rows, cols, Kb in blocks:
            res[rows] = rl[rows] - Kb @ X[cols]
        dx = Kinv @ res.astype(np.float64)
        X = X + dx.astype(LD)
        last = float(np.abs(dx).max() / np.abs(X).max())
        if last <= 1e-15:
            break
    assert last <= 1e-15, ("the refinement of the dense solve stalled", last)
    return X.astype(np.float64), X0, last, it


def _tail_system(stages, p, variant):
    """Dense KKT matrix of the tail problem from position p; layout of unknowns and multipliers."""
    tail = stages[p:]
    xo, uo, off = [], [], 0
    for st in tail:
        xo.append(off); off += NX
        if "Quu" in st:
            uo.append(off); off += NU
        else:
            uo.append(None)
    nz = off
    rows, off = [("init", 0, 0)], NX      # (what, local position, first row)
    for i, st in enumerate(tail[:-1]):
        rows.append(("dyn", i, off)); off += NX
    use_sw = variant != "drop_switch"
    for i, st in enumerate(tail):
        if st["dimi"] > 0 and use_sw:
            rows.append(("sw", i, off)); off += st["dimi"]
    nc = off
    H = np.zeros((nz, nz)); g = np.zeros(nz)
    Cm = np.zeros((nc, nz)); d = np.zeros(nc); sigma = np.zeros(nc)
    for i, st in enumerate(tail):
        H[xo[i]:xo[i] + NX, xo[i]:xo[i] + NX] = st["Qxx"]
        g[xo[i]:xo[i] + NX] = st["lx"]
        if uo[i] is not None:
            H[xo[i]:xo[i] + NX, uo[i]:uo[i] + NU] = st["Qxu"]
            H[uo[i]:uo[i] + NU, xo[i]:xo[i] + NX] = st["Qxu"].T
            H[uo[i]:uo[i] + NU, uo[i]:uo[i] + NU] = st["Quu"]
            g[uo[i]:uo[i] + NU] = st["lu"]
    for what, i, r in rows:
        st = tail[i]
        if what == "init":                      # x_p = x0, Lagrangian term lambda^T (d - C z)
            Cm[r:r + NX, xo[0]:xo[0] + NX] = np.eye(NX); sigma[r:r + NX] = -1.0
        elif what == "dyn":                     # x_{i+1} - A x_i - B u_i = Fx, the same sign
            A, B = AB(st, impulse_dt=DT if variant == "grid_dt_on_impulse" else None)
            Cm[r:r + NX, xo[i + 1]:xo[i + 1] + NX] = np.eye(NX)
            Cm[r:r + NX, xo[i]:xo[i] + NX] = -A
            if uo[i] is not None:
                Cm[r:r + NX, uo[i]:uo[i] + NU] = -B
            d[r:r + NX] = st["Fx"]; sigma[r:r + NX] = -1.0
        else:                                   # Phix x + Phiu u = -P, Lagrangian term + xi^T (Phix x + Phiu u + P)
            n = st["dimi"]
            Phix = np.roll(st["Phix"], 1, axis=0) if variant == "shift_switch" else st["Phix"]
            Cm[r:r + n, xo[i]:xo[i] + NX] = Phix
            Cm[r:r + n, uo[i]:uo[i] + NU] = st["Phiu"]
            d[r:r + n] = -st["P"]; sigma[r:r + n] = 1.0
    Kmat = np.block([[H, Cm.T * sigma[None, :]], [Cm, np.zeros((nc, nc))]])      # H z + g + C^T (sigma lam) = 0 ; C z = d
    return Kmat, np.concatenate([-g, d]), nz, xo, uo, rows


def _scaled(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def solve_chain(stages, dx0=None, variant=None):
    """The referee proper, on explicit stage data (draw_problem's, or the blocks of a fixture).  Returns a dict: P [M, NX, NX], s [M, NX],
    K [M - 1, NU, NX], k [M - 1, NU] (zero rows on impulse positions, which have no control), Mxi / mxi {position: array} on switching positions;
    with dx0: dq, dv [M, NV], du [M - 1, NU], dxi {position: array}; first {quantity: worst distance of the unrefined float64 solve from the
    refined one, scaled as the tests scale}; last: the largest final correction relative to the solution."""
    M = len(stages)
    out = dict(P=np.zeros((M, NX, NX)), s=np.zeros((M, NX)), K=np.zeros((M - 1, NU, NX)), k=np.zeros((M - 1, NU)), Mxi={}, mxi={}, first={},
               last=0.0, iterations=0)
    first = out["first"]

    def note(name, plain, refined):
        first[name] = max(first.get(name, 0.0), _scaled(plain, refined))

    for p in range(M):
        Kmat, rhs0, nz, xo, uo, rows = _tail_system(stages, p, variant)
        forward = p == 0 and dx0 is not None
        rhs = np.tile(rhs0[:, None], (1, NX + 1 + (1 if forward else 0)))
        rhs[nz:nz + NX, 1:NX + 1] += np.eye(NX)
        if forward:
            rhs[nz:nz + NX, NX + 1] += np.asarray(dx0, dtype=np.float64)
        X, X0, last, it = _refined_solve(Kmat, rhs)
        out["last"] = max(out["last"], last); out["iterations"] = max(out["iterations"], it)
        sw_row = next((r for what, i, r in rows if what == "sw" and i == 0), None)

        def read(Y):
            lam = Y[nz:nz + NX]
            q = dict(P=lam[:, 1:NX + 1] - lam[:, :1], s=-lam[:, 0])
            if uo[0] is not None:
                u = Y[uo[0]:uo[0] + NU]
                q.update(K=u[:, 1:NX + 1] - u[:, :1], k=u[:, 0])
            if sw_row is not None:
                xi = Y[nz + sw_row:nz + sw_row + stages[p]["dimi"]]
                q.update(Mxi=xi[:, 1:NX + 1] - xi[:, :1], mxi=xi[:, 0])
            return q

        have, plain = read(X), read(X0)
        for name in have:
            note(name, plain[name], have[name])
            if name in ("Mxi", "mxi"):
                out[name][p] = have[name]
            else:
                out[name][p] = have[name]
        if forward:
            def fwd(Y):
                y = Y[:, NX + 1]
                f = dict(dq=np.stack([y[o:o + NV] for o in xo]), dv=np.stack([y[o + NV:o + NX] for o in xo]),
                         du=np.stack([y[o:o + NU] if o is not None else np.zeros(NU) for o in uo[:-1]]), dxi={})
                for what, i, r in rows:
                    if what == "sw":
                        f["dxi"][i] = y[nz + r:nz + r + stages[i]["dimi"]]
                return f
            f, f0 = fwd(X), fwd(X0)
            for name in ("dq", "dv", "du"):
                out[name] = f[name]
                first[name] = max(_scaled(f0[name][i], f[name][i]) for i in range(len(f[name])))
            out["dxi"] = f["dxi"]
            for i in f["dxi"]:
                note("dxi", f0["dxi"][i], f["dxi"][i])
    return out      # (P is read off as it is: its symmetry is something the tests can check, not something imposed)


@functools.lru_cache(maxsize=None)
def referee(chain, seed, instance, dx0=None, variant=None):
    """solve_chain on the problem drawn for (chain, seed, instance); chain = chain_key(...), dx0 a tuple of NX floats or None."""
    return solve_chain(draw_problem(chain, seed, instance), dx0, variant)


# ---------------------------------------------------------------------------------------------------------------- injection
def _cm(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)      # column-major


def _p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _blocks(st):
    names = ("Qxx", "Qxu", "Quu", "Fqq6", "Fqv6", "Fvq", "Fvv", "Fvu", "lx", "lu", "Fx")
    return [(_cm(st[n]) if st[n].ndim == 2 else np.ascontiguousarray(st[n], dtype=np.float64)) if n in st else None for n in names]


def inject_hip(h, stages, instance):
    """Every position of one instance (or of all: -1) into the device records of a HipOCP handle."""
    from idocp_amd import capi
    for p, st in enumerate(stages):
        keep = _blocks(st)
        capi.check(h.lib.idocp_ocp_set_lqr_stage_chain(h.h, instance, p, *[_p(a) for a in keep]), "set_lqr_stage_chain")
        if st["dimi"] > 0:
            sw = [np.ascontiguousarray(st["P"]), _cm(st["Phix"]), _cm(st["Phiu"])]
            capi.check(h.lib.idocp_ocp_set_switching_constraint(h.h, instance, p, st["dimi"], *[_p(a) for a in sw]), "set_switching_constraint")


def hip_switching_policy(h, instance, p, dimi):
    Mx, m = np.zeros((NX, dimi)), np.zeros(dimi)
    assert h.lib.idocp_ocp_get_switching_policy(h.h, instance, p, _p(Mx), _p(m)) == dimi
    return Mx.T.copy(), m


def setup_oracle(lib):
    dp = C.POINTER(C.c_double)
    lib.oracle_ocp_inject_lqr_stage_chain.argtypes = [C.c_void_p, C.c_int] + [dp] * 11
    lib.oracle_ocp_inject_switching_constraint.argtypes = [C.c_void_p, C.c_int, C.c_int] + [dp] * 3
    lib.oracle_ocp_switching_rows.argtypes = [C.c_void_p, C.c_int]
    lib.oracle_ocp_get_switching_policy.argtypes = [C.c_void_p, C.c_int, dp, dp]
    lib.oracle_ocp_forward_riccati_only.argtypes = [C.c_void_p, dp, dp]
    lib.oracle_ocp_backward_riccati_only.argtypes = [C.c_void_p]


def inject_oracle(o, stages):
    """(the oracle's backward recursion works in place: inject again before every run)"""
    setup_oracle(o.lib)
    for p, st in enumerate(stages):
        keep = _blocks(st)
        assert o.lib.oracle_ocp_inject_lqr_stage_chain(o.h, p, *[_p(a) for a in keep]) == 0
        if st["dimi"] > 0:
            sw = [np.ascontiguousarray(st["P"]), _cm(st["Phix"]), _cm(st["Phiu"])]
            assert o.lib.oracle_ocp_inject_switching_constraint(o.h, p, st["dimi"], *[_p(a) for a in sw]) == 0


def oracle_switching_policy(o, p, dimi):
    Mx, m = np.zeros((NX, dimi)), np.zeros(dimi)
    assert o.lib.oracle_ocp_get_switching_policy(o.h, p, _p(Mx), _p(m)) == dimi
    return Mx.T.copy(), m


def oracle_chain(o):
    """The oracle's chain in the form idocp_ocp_get_chain reports it: sw_dimi is the row count of the constraint the node carries."""
    setup_oracle(o.lib)
    ch = o.chain(0.0)
    for p, c in enumerate(ch):
        c["sw_dimi"] = o.lib.oracle_ocp_switching_rows(o.h, p)
    return ch


def prepare(solver, spec, model, pts, q_standing):
    """Sequence, iterate and one update() of a HipOCP or OracleOCP wrapper: discretises the chain and sizes every record."""
    apply_sequence(solver, spec, pts)
    solver.set_solution("q", q_standing)
    solver.set_solution("v", np.zeros(model.nv))
    solver.set_solution("f", [0, 0, 0.25 * (-model.total_mass * model.gravity[2])])
    solver.init_constraints(0.0)
    assert solver.update(0.0, q_standing, np.zeros(model.nv)) == 0


def initial_state(q_stored, v_stored, seed, instance):
    """q0 with the BASE POSE of the stored iterate (the Lie difference is exactly zero and no Lie formula is shared) and perturbed joints, v0
    perturbed; and the dx_0 = (0, dq_joints, dv) the referee starts from."""
    rng = np.random.default_rng([seed, instance, 99])
    q0, v0 = np.array(q_stored, dtype=np.float64), np.array(v_stored, dtype=np.float64)
    q0[7:] += rng.uniform(-0.05, 0.05, NU)
    v0 += rng.uniform(-0.1, 0.1, NV)
    dx0 = np.concatenate([np.zeros(6), q0[7:] - np.asarray(q_stored)[7:], v0 - np.asarray(v_stored)])
    return q0, v0, tuple(float(x) for x in dx0)
