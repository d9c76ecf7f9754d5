"""Shared by test_ocp_stage_terms_host.py / test_ocp_stage_terms_gpu.py: the cases the STAGE kernels of OCPSolver / ParNMPCSolver
(ocp_condense_kernel.hip, ocp_nominal_kernel.hip, ocp_rnea_kernel.hip, parnmpc_event_kernels.hip) are held on, and the referee's version of
the record a stage keeps -- MJtJinv = [M J^T; J 0]^-1, MJtJinv [dID; dC]/d(q, v), MJtJinv [ID - S^T u; C] (ContactDynamicsData,
contact_dynamics_data.hxx:8-29; read with idocp_ocp_get_contact_dynamics_chain, the active rows packed).  The referee is the numpy model
evaluated at test time (independent_rbd.py, rbd_cases.py on gen_golden_rbd.py: body-frame Newton-Euler, complex-step derivatives) with the
inverse in np.longdouble; nothing here calls the oracle or the library's arithmetic.  A plain module: the referee's answers are computed
once per (model, mask) or per chain and shared.

The conventions of the node kinds, as READ (not as returned by a kernel):

* grid stage, forward Euler: contact status and points of the phase the stage lies in -- the number of events before it
  (idocp_amd/csrc/ocp_chain.hpp:307-321; ocp_linearizer.hxx:134 contactStatus(contactPhase(i))); the rows are the Baumgarte residual at
  (q, v, a) with the time step T / N (hybrid_container.hpp:186-188; ocp_condense_kernel.hip:324), the dynamics ID(q, v, a, f) - S^T u
  (contact_dynamics.hxx:88; ocp_condense_kernel.hip:639).
* impulse stage: the contacts of the IMPULSE status -- those the event switches on, not those that already stand
  (discrete_event.hxx:57-84; ocp_chain.hpp:79-87, :324) -- no torques (ocp_chain.hpp:183).  [ImD; V] in the place of [ID; C]
  (impulse_dynamics_forward_euler_data.hxx): ImD = RNEAImpulse(q, dv), no gravity and zero velocity
  (impulse_dynamics_forward_euler.hxx:50-51; ocp_nominal_kernel.hip:37-38, :75), dImD/dv = 0; V = the LOCAL linear velocity of the
  contact frames with dV/dv = dV/ddv = J (impulse_dynamics_forward_euler.hxx:58-67).  The velocity V is taken at: v + dv on a
  forward-Euler chain (impulse_split_ocp.hxx:55 updateKinematics(s.q, s.v+s.dv); ocp_nominal_kernel.hip:122-123), v itself on a
  backward-Euler chain, where v IS the post-impact velocity (impulse_split_parnmpc.hxx:58; ocp_rnea_kernel.hip:98-100).
* aux stage, forward Euler: the phase AFTER the impulse (ocp_linearizer.hxx:191-192 contactPhaseAfterImpulse; ocp_chain.hpp:325);
  lift stage: the phase AFTER the lift (ocp_linearizer.hxx:207-208; ocp_chain.hpp:328).  Both are regular stages otherwise.
* backward Euler (ParNMPC): the chain is stage i-1, [aux k, impulse k | lift k], stage i (ocp_chain.hpp:362-366); the aux and the lift
  stage take the phase BEFORE the event (ocp_chain.hpp:390-398), the grid stage behind an event the phase after it (:400).  Stage i is
  linearised at its own (q_i, v_i, a_i, f_i, u_i).  The BWD instantiation of ocp_condense_kernel writes the same E_MJ / E_MJD / E_MJIDC
  record as the forward one (ocp_condense_kernel.hip:952-968, no BWD branch) for grid, aux and lift stages, at the iterate
  idocp_parnmpc_compute_direction is called with (it does not integrate).  The backward-Euler IMPULSE stage is not condensed that way
  (ocp_condense_kernel.hip:169 returns; impulse_dynamics_backward_euler.hxx): parnmpc_event_kernels.hip:264, :279 leave only
  Minv = (dImD/ddv)^-1 in the leading nv x nv block of E_MJ and Minv ImD in E_MJIDC, no E_MJD and no contact rows -- that kind has no
  such record; what it does leave (`backward_impulse_record`) is held to the referee all the same.
"""
import functools

import numpy as np

import independent_rbd as IR
import rbd_cases as RC
from helpers import rel_err
from rbd_batch import random_samples

BAR = 1e-11                         # the bar of this layer (test_golden_rbd_gpu.py, test_rbd_contact_sets_gpu.py)
SELF_BAR = BAR / 4                  # what the referee may differ from itself by (its float64 against its long double route)
MODELS = RC.MODELS                  # ANYmal and other_quadruped(1)
N_UNIFORM, BATCH = 2, 3             # two grid stages and the terminal one; the last workgroup of a launch is not full
TS = RC.TS                          # Baumgarte time step T / N
BACKWARD_MASKS = ((1, 1, 1, 1), (1, 0, 0, 1), (0, 0, 1, 0), (0, 0, 0, 0))
# one short event chain: N = 4, dt = 0.05; the phases have dimf 6 -> 12 -> 9 -> 3: a two-foot impulse while two feet stand, then two lifts
CHAIN_N, CHAIN_T, CHAIN_EVENTS = 4, 0.2, 3
CHAIN_PHASES = ((1, 0, 0, 1), (1, 1, 1, 1), (0, 1, 1, 1), (0, 0, 1, 0))
CHAIN_TIMES = (0.07, 0.12, 0.17)
# (kind, mask) of every chain position that has dynamics, as the conventions of the module docstring give them
FORWARD_CHAIN = (("stage", CHAIN_PHASES[0]), ("stage", CHAIN_PHASES[0]), ("impulse", (0, 1, 1, 0)), ("aux", CHAIN_PHASES[1]), ("stage", CHAIN_PHASES[1]),
                 ("lift", CHAIN_PHASES[2]), ("stage", CHAIN_PHASES[2]), ("lift", CHAIN_PHASES[3]))
BACKWARD_CHAIN = (("stage", CHAIN_PHASES[0]), ("aux", CHAIN_PHASES[0]), ("impulse", (0, 1, 1, 0)), ("stage", CHAIN_PHASES[1]), ("lift", CHAIN_PHASES[1]),
                  ("stage", CHAIN_PHASES[2]), ("lift", CHAIN_PHASES[2]), ("stage", CHAIN_PHASES[3]))
TERMS = ("M", "J", "dID/dq", "dID/dv", "dC/dq", "dC/dv", "ID - S^T u", "C")
PRODUCTS = ("MJtJinv", "MJtJinv dIDC/dqv", "MJtJinv IDC")
# The one handle with its own bar for three terms: the `stiff` hard state, Baumgarte step 1e-3.  There dC/dq = 1e6 J, the entries of the
# record MJtJinv [dID; dC]/d(q, v) grow with 1 / step^2, each is rounded to float64, and dID/dq, dID/dv, ID - S^T u come back out of it
# as sums over nv + dimf such entries: the ROUNDING OF THE RECORD alone costs eps / step^2 per entry, whoever computed it.  Their bar
# on that handle is therefore eps * nv / step^2 = 2.2e-16 * 18 * 1e6 = 4e-9 (from the number format and the shapes, not from what a
# kernel returned) -- four orders below what a wrong sign or row costs -- and the referee's own float64 record must be within a
# quarter of it like everywhere else (measured: 3.4e-10).  Everything else on that handle, and everything on every other case, is held to BAR.
STIFF_TERMS = ("dID/dq", "dID/dv", "ID - S^T u")
STIFF_BAR = float(np.finfo(np.float64).eps) * 18 / RC.STIFF_TS ** 2


def dimf_of(mask):
    return 3 * int(sum(mask))


# ------------------------------------------------------------------ the referee's record of one chain node

def referee_record(M, q, v, a, f, u, pts, time_step, mask, kind, backward=False, stiff=False):
    """The three records of one node and what they are made of, from the independent model: {name of TERMS / PRODUCTS: array [row, column]},
    "dimf", "cond" = cond(K), "bars" = {name: the bar the quantity is held to} (BAR; STIFF_BAR for STIFF_TERMS with stiff = True, which
    only the `stiff` hard handle passes) and "self" = the referee against itself: the largest of `distances`, each over a quarter of its
    bar, between the record formed in FLOAT64 from its own terms (inverse of K = [M J^T; J 0] over the active rows, two products, the
    terms taken back out of them) and the long double one -- at most 1 where the referee reproduces itself to a quarter of every bar;
    "self_distance": the largest plain distance among the quantities held to BAR.
    a is dv and f the impulse forces on an impulse node; u, pts and time_step are not used there."""
    nv = M["nv"]
    mask = tuple(int(x) for x in mask)
    if kind == "impulse":
        t = IR.terms(M, q, v, a, f, active=mask)
        rows = RC.impulse_rows(M, q, np.asarray(v) + (0.0 if backward else np.asarray(a)), mask)
        held = {"M": t["dimp_da"], "J": rows["imp_J"], "dID/dq": t["dimp_dq"], "dID/dv": np.zeros((nv, nv)), "dC/dq": rows["imp_dCdq"], "dC/dv": rows["imp_J"],
                "ID - S^T u": t["tau_impulse"], "C": rows["imp_C"]}
    else:
        t = IR.terms(M, q, v, a, f, pts, time_step, active=mask, impulse_forms=False)
        tau = t["tau"].copy()
        tau[nv - len(u):] -= u
        held = {"M": t["dtau_da"], "J": t["dCda"], "dID/dq": t["dtau_dq"], "dID/dv": t["dtau_dv"], "dC/dq": t["dCdq"], "dC/dv": t["dCdv"], "ID - S^T u": tau,
                "C": t["C"]}
    nf = held["J"].shape[0]
    assert nf == dimf_of(mask)
    K = np.block([[held["M"], held["J"].T], [held["J"], np.zeros((nf, nf))]])
    Kinv = RC.solve_longdouble(K, np.eye(nv + nf))
    D = np.block([[held["dID/dq"], held["dID/dv"]], [held["dC/dq"], held["dC/dv"]]]).astype(np.longdouble)
    r = np.concatenate([held["ID - S^T u"], held["C"]]).astype(np.longdouble)
    held.update({"MJtJinv": Kinv.astype(np.float64), "MJtJinv dIDC/dqv": (Kinv @ D).astype(np.float64), "MJtJinv IDC": (Kinv @ r).astype(np.float64),
                 "dimf": nf, "cond": float(np.linalg.cond(K))})
    own = distances(record_of(K, D.astype(np.float64), r.astype(np.float64)), held, nv)
    held["bars"] = {name: (STIFF_BAR if stiff and name in STIFF_TERMS else BAR) for name in own}
    held["self"] = max(d / (held["bars"][name] / 4) for name, (d, _) in own.items())
    held["self_distance"] = max(d for name, (d, _) in own.items() if held["bars"][name] == BAR)
    held["self_stiff"] = max([d for name, (d, _) in own.items() if held["bars"][name] != BAR] or [0.0])
    return held


def backward_impulse_record(ref):
    """what a backward-Euler impulse stage leaves on the device (module docstring), from the referee's record of that node:
    (Minv, Minv ImD) with Minv = (dImD/ddv)^-1 in long double"""
    Minv = RC.solve_longdouble(ref["M"], np.eye(ref["M"].shape[0]))
    return Minv.astype(np.float64), (Minv @ ref["ID - S^T u"].astype(np.longdouble)).astype(np.float64)


def check_referee(refs, label):
    """the referee against itself on the records of one case, over EVERY compared quantity: prints the worst self-distance and cond(K) and
    holds each quantity's self-distance to a quarter of the bar it is held to"""
    worst, cond, stiff = max(r["self_distance"] for r in refs), max(r["cond"] for r in refs), max(r["self_stiff"] for r in refs)
    print("referee %s: self-distance %.1e, cond(K) %.1e%s" % (label, worst, cond, "; %s at the stiff step %.1e (bar %.1e)" % (", ".join(STIFF_TERMS), stiff, STIFF_BAR)
                                                              if stiff else ""))
    assert max(r["self"] for r in refs) <= 1.0, (label, worst, stiff)
    return worst, cond


# ------------------------------------------------------------------ a record taken apart, and compared term by term

def unpack(MJ, MJD, MJIDC, nv):
    """One inverse of a record's MJtJinv gives M and J back, two products the derivative blocks and the residuals:
    {name of TERMS / PRODUCTS: array}, "K" = the inverse itself and "schur" = its block K[nv:, nv:] that must vanish."""
    K = np.linalg.inv(MJ)                                       # [M J^T; J 0]
    dIDC, IDC = K @ MJD, K @ MJIDC
    return {"K": K, "MJtJinv": MJ, "MJtJinv dIDC/dqv": MJD, "MJtJinv IDC": MJIDC, "M": K[:nv, :nv], "J": K[nv:, :nv], "schur": K[nv:, nv:],
            "dID/dq": dIDC[:nv, :nv], "dID/dv": dIDC[:nv, nv:], "dC/dq": dIDC[nv:, :nv], "dC/dv": dIDC[nv:, nv:], "ID - S^T u": IDC[:nv], "C": IDC[nv:]}


def record_of(K, dIDCdqv, IDC):
    """the record a float64 implementation forms from K = [M J^T; J 0], [dID; dC]/d(q, v) and [ID - S^T u; C] (the oracle in the kernel's place)"""
    MJ = np.linalg.inv(K)
    return MJ, MJ @ dIDCdqv, MJ @ IDC


def device_record(g, instance, position):
    """(dimf, MJtJinv, MJtJinv dIDC/dqv, MJtJinv IDC) of a chain position as [row, column], through idocp_ocp_get_contact_dynamics_chain"""
    from helpers import P
    from idocp_amd import capi
    nv, nmax = g.nv, g.nv + 12
    MJ, MJD, MJIDC = np.zeros(nmax * nmax), np.zeros(nmax * 2 * nv), np.zeros(nmax)
    dimf = g.lib.idocp_ocp_get_contact_dynamics_chain(g.h, instance, position, P(MJ), P(MJD), P(MJIDC))
    assert dimf >= 0, (dimf, capi.lib().idocp_last_error())
    n = nv + dimf
    return dimf, MJ[:n * n].reshape(n, n).T.copy(), MJD[:n * 2 * nv].reshape(2 * nv, n).T.copy(), MJIDC[:n].copy()      # column-major -> [row, column]


def worst_row(x, ref):
    """(helpers.rel_err of x against ref, the row it is reached in): rel_err takes a matrix row by row, a vector as a whole"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if not ref.size:
        return 0.0, -1
    err = np.abs(x - ref)
    if ref.ndim < 2:
        return rel_err(x, ref), int(err.argmax())
    scaled = err.max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))
    return rel_err(x, ref), int(scaled.argmax())


def distances(record, ref, nv):
    """{term: (distance, packed row)} of a record (MJ, MJD, MJIDC) against the referee's, the three products and the eight terms they are made
    of; "schur": the largest entry of the block of K that must vanish.  A packed row >= nv of a product is contact row (row - nv)."""
    got = unpack(*record, nv)
    out = {name: worst_row(got[name], ref[name]) for name in PRODUCTS + TERMS}
    s = np.abs(got["schur"])
    out["schur"] = (float(s.max()), int(s.max(axis=1).argmax())) if s.size else (0.0, -1)
    return out


def hold(dist, where, bars, worst=None):
    """assert every quantity of `distances` below its bar (the referee record's "bars"), naming the term and the packed row; keeps the
    largest distance per term in `worst`"""
    if worst is not None:
        for name, (d, _) in dist.items():
            worst[name] = max(worst.get(name, 0.0), d)
    bad = ["%s: %.2e at packed row %d (bar %.1e)" % (name, d, row, bars[name]) for name, (d, row) in dist.items() if not d < bars[name]]
    assert not bad, "%s -- %s" % (where, "; ".join(bad))


def summary(worst):
    return "  ".join("%s %.1e" % (name, worst[name]) for name in PRODUCTS + TERMS + ("schur",) if name in worst)


# ------------------------------------------------------------------ the uniform cases: every mask, two models, distinct iterates per stage

def uniform_inputs(which):
    """(struct, model dict, dict of the per-stage inputs) of a two-stage handle: stage i holds sample i of rbd_cases.quadruped, the terminal
    stage the configuration and velocity of sample 2; the contact points of the one phase lie a few centimetres off the feet of stage 0"""
    m, M, (q, v, a, f, pts, u) = RC.quadruped(which)
    n = N_UNIFORM
    return m, M, dict(q=q[:n + 1], v=v[:n + 1], a=a[:n], f=f[:n], u=u[:n], pts=pts[0])


@functools.lru_cache(maxsize=None)
def uniform_reference(which, mask):
    """the referee's record of the two grid stages (the same for the forward- and the backward-Euler form: a regular stage is linearised at
    its own iterate in both)"""
    _, M, s = uniform_inputs(which)
    return [referee_record(M, s["q"][i], s["v"][i], s["a"][i], s["f"][i], s["u"][i], s["pts"], TS, mask, "stage") for i in range(N_UNIFORM)]


# ------------------------------------------------------------------ the event chain: every node kind, partial contact sets

@functools.lru_cache(maxsize=None)
def chain_inputs(which):
    """(struct, model dict, dict) of the event chain: nine distinct samples (a chain has eight positions with dynamics in either form; the
    forward one a terminal stage behind them) and the contact points of each phase a few centimetres off the feet of one of the samples"""
    m, M, _ = RC.quadruped(which)
    rng = np.random.default_rng([4711, 0 if which == "anymal" else int(which) + 1])
    n = len(FORWARD_CHAIN) + 1
    q, v, a, f, _ = random_samples(rng, n)
    u = rng.uniform(-20, 20, (n, m.nu))
    pts = np.array([RC.feet(M, q[2 * k]) + rng.uniform(-0.03, 0.03, (4, 3)) for k in range(len(CHAIN_PHASES))])
    return m, M, dict(q=q, v=v, a=a, f=f, u=u, pts=pts)


def phase_of(mask, kind):
    return None if kind == "impulse" else CHAIN_PHASES.index(tuple(mask))


@functools.lru_cache(maxsize=None)
def chain_reference(which, backward):
    """the referee's record of every position of the chain that has dynamics (the backward-Euler impulse position too: the oracle keeps
    all of it, the device what backward_impulse_record makes of it)"""
    _, M, s = chain_inputs(which)
    out = []
    for p, (kind, mask) in enumerate(BACKWARD_CHAIN if backward else FORWARD_CHAIN):
        pts = None if kind == "impulse" else s["pts"][phase_of(mask, kind)]
        out.append(referee_record(M, s["q"][p], s["v"][p], s["a"][p], s["f"][p], s["u"][p], pts, CHAIN_T / CHAIN_N, mask, kind, backward))
    return out


def build_chain(g, which):
    """the contact sequence of the event chain on a solver wrapper (HipOCP / HipParNMPC or the oracle's)"""
    _, _, s = chain_inputs(which)
    g.set_contact_status(CHAIN_PHASES[0], s["pts"][0])
    for k, t in enumerate(CHAIN_TIMES):
        g.push_back_contact_status(CHAIN_PHASES[k + 1], s["pts"][k + 1], t)


# ------------------------------------------------------------------ hard states (ANYmal), one per stage of a two-stage handle

# `far` leads its pair: the points of a handle are those of its first state.  A handle has ONE Baumgarte step (T / N), so `stiff` fills
# both stages of a handle of its own and `rest` both stages of one at the normal step: five handles, every state at the step it names.
HARD_PAIRS = (("straight", "pi"), ("w_zero", "w_negative"), ("far", "fast"), ("rest", "rest"), ("stiff", "stiff"))
STIFF_PAIR = ("stiff", "stiff")
assert sorted(set(sum(HARD_PAIRS, ()))) == sorted(RC.HARD_NAMES)


def hard_state(name):
    """rbd_cases.hard_cases()[name], unchanged: no state needed softening (straight legs: cond(K) 1e3 with four, three and one foot)"""
    m, M, cases = RC.hard_cases()
    return m, M, cases[name]


def hard_time_step(pair):
    """the Baumgarte step of a handle that holds the pair: a handle has ONE (T / N), and only the stiff handle departs from TS"""
    steps = {hard_state(name)[2]["time_step"] for name in pair}
    assert len(steps) == 1 and (steps == {RC.STIFF_TS}) == (pair == STIFF_PAIR), pair
    return steps.pop()


@functools.lru_cache(maxsize=None)
def hard_reference(pair, mask):
    """the referee's record of the two stages of the handle that holds `pair`; the contact points of the one phase are those of the first
    state (a different second state is then some decimetres off: `far` in its own right)"""
    ts = hard_time_step(pair)
    first = hard_state(pair[0])[2]
    out = []
    for name in pair:
        _, M, s = hard_state(name)
        out.append(referee_record(M, s["q"], s["v"], s["a"], s["f"], s["u"], first["pts"], ts, mask, "stage", stiff=pair == STIFF_PAIR))
    return out
