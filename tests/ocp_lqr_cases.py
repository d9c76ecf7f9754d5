"""Shared by test_ocp_lqr_stage_host.py / test_ocp_lqr_stage_gpu.py: a referee for the CONDENSED LQR stage of OCPSolver -- Qxx, Qxu, Quu, A, B, lx, lu, Fx
in the layout of idocp_ocp_get_lqr_stage -- that is not the restatement (oracle/ocp.cpp) and not the kernels (ocp_condense_kernel.hip): the stage
Lagrangian of one grid stage of a forward-Euler chain written down from the mathematics, differentiated numerically, and condensed by eliminating
(da, df) with one solve of [M J^T; J 0].  Nothing here calls the oracle or the library's arithmetic; the rigid-body rows and their first derivatives are
ocp_stage_cases.referee_record (the numpy Newton-Euler model), the reference tables and the constraint rows are rbd_score's second writing of them.

The stage.  With x = (q, v), the next node (q+, v+), the previous node q-, the costates (lmd, gmm) of this node and (lmd+, gmm+) of the next:

    L = dt l(q, v, a, f, u; t) + dt sum_r c_r g_r + lmd+ . Fq + gmm+ . Fv + lmd . Fq- + gmm . Fv- + dt beta . (ID(q, v, a, f) - S^T u) + dt mu . C(q, v, a)
    l   = 1/2 |q (-) q_ref(t)|^2_Wq + 1/2 |v - v_ref(t)|^2_Wv + 1/2 |a|^2_Wa + 1/2 |u - u_ref|^2_Wu + 1/2 sum_active |f_c - f_ref,c|^2_Wf
    Fq  = (q (-) q+) + dt v          Fv  = v + dt a - v+          Fq- = (q- (-) q) + dt- v-          Fv- = v- + dt- a- - v
    g_r <= 0: the rows of rbd_score.constraint_rows; c_r = z + (z (g + s) - (s z - eps)) / s with the slack s and the dual z of the HANDLE UNDER TEST
    (get_constraint_data: they are state, not arithmetic of the stage) and eps the barrier parameter.

The gradient of L with respect to (x, u, a, f) holds every term above, beta, mu and the costates included; the passive torques are no variable (they are
fixed at zero), so nu_passive cannot enter a condensed stage -- it is set non-zero in the iterate all the same, and a kernel that let it through would be
seen.  Derivatives: the complex step wherever the function is analytic as written (the quadratic cost terms, the constraint rows), a Romberg-extrapolated
central difference for the SE(3) logarithm (`jac_difference`; its own error estimate is held below a quarter of the bar by `check_referee`).

THE HESSIAN CONVENTION, in one place: Gauss-Newton throughout.  The cost Hessian is dt J^T W J with J the Jacobian of the configuration difference and
dt W on v, a, u, f; no second derivative of the dynamics, of the Baumgarte rows or of the state equation enters; every inequality row adds
dt (z / s) grad g grad g^T, the nonlinear cone too (no z grad^2 g term).

The condensation is an elimination: the linearised [ID - S^T u; C] = 0 gives w = [da; -df] = Wx dx + Wu du + w0 with ONE long double solve of
K = [M J^T; J 0] against [-D | S^T | -r]; substituted into the quadratic model and into Fv that gives Qxx = Hxx + Wx^T Hww Wx, Qxu = Wx^T Hww Wu,
Quu = Huu + Wu^T Hww Wu, lx = gx + Wx^T (gw + Hww w0), lu = gu + Wu^T (gw + Hww w0), [A_vq A_vv] = [0 I] + dt Wx[:nv], B_v = dt Wu[:nv],
Fx_v = Fv + dt w0[:nv]; the linearised Fq row solved for the tangent step of q+ gives A_qq = -(dFq/dq+)^-1 dFq/dq, A_qv = -dt (dFq/dq+)^-1,
Fx_q = -(dFq/dq+)^-1 Fq (identity, dt I and Fq outside the 6 x 6 base block).  Every result is a Schur complement; the order of operations of the
reference's condenseContactDynamics does not appear.  beta and mu cancel in lx and lu only analytically (K^-1 K); the float64 route carries them
like a kernel does.

Conventions of the reference that the referee FOLLOWS (read in oracle/ocp.cpp against the reference's constraints_data.hpp, state_equation.hxx):
* the joint position rows exist from grid stage 2 on and the velocity rows from stage 1 on (the initial state fixes q0, v0 and q1): the cases
  therefore have N = 3 grid stages, one more than ocp_stage_cases.N_UNIFORM, so that the position barrier is reached at all;
* lx keeps the costate lmd+ in the coordinates of the un-condensed Fq row (dFq/dq^T lmd+), while A and Fx are those of the row solved for dq+.
Out of scope: the multiplier xi of the switching constraint is held at ZERO on the event chain (it is set back with the iterate after an update): the
term xi . P(q (+) ..) of the stage that carries the constraint is not written here; the impulse, aux and lift positions of an event chain cannot be reached through idocp_ocp_get_lqr_stage; the grid stages of the event
chain are held, with the chain neighbours and the time steps idocp_ocp_get_chain reports."""
import contextlib
import functools
import types

import numpy as np

import independent_rbd as IR
import ocp_stage_cases as S
import rbd_cases as RC
import rbd_score as RS
from idocp_amd.workloads import ANYMAL_Q_STANDING, anymal_problem      # (problem set-up shared with bench.py; helpers, and with it the oracle loader, is not needed here)

RBD = IR.RBD
BAR, SELF_BAR = S.BAR, S.SELF_BAR
N, BATCH, DT = 3, S.BATCH, S.TS                 # three grid stages (module docstring), dt = T / N = the Baumgarte step
CHAIN_T0 = 0.0                                 # the event chain of ocp_stage_cases is discretised at 0 (its event times are absolute)
T0 = 0.67                                       # stage times 0.67 .. 0.79: the trotting knees are mid-swing (rate 0.34 .. 0.58), inside the time-varying window
QUANTITIES = ("Qxx", "Qxu", "Quu", "A", "B", "lx", "lu", "Fx")
LD = np.longdouble
ACCEL_SLACK = 0.84                              # what every acceleration row keeps of slack right after init_constraints (`iterate`: why)
MUTATIONS = ("barrier_dt", "cost_J_identity", "cone_fz_sign", "cone_mu", "no_q_prev", "no_gmm_next_in_la", "trot_phase", "A_base_identity")


# ------------------------------------------------------------------ SE(3) x R^n: difference and its Jacobians, in any real type

def _skew(w):
    return np.array([[0 * w[0], -w[2], w[1]], [w[2], 0 * w[0], -w[0]], [-w[1], w[0], 0 * w[0]]], dtype=w.dtype)


def _coeffs(t2, T):
    """sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3 by their series below t = 0.1 (8 terms: truncation 1e-25), the closed forms above"""
    if t2 < 0.01:
        a = b = c = T(0)
        ta, tb, tc = T(1), T(1) / 2, T(1) / 6
        for k in range(8):
            a, b, c = a + ta, b + tb, c + tc
            ta, tb, tc = -ta * t2 / ((2 * k + 2) * (2 * k + 3)), -tb * t2 / ((2 * k + 3) * (2 * k + 4)), -tc * t2 / ((2 * k + 4) * (2 * k + 5))
        return a, b, c
    t = np.sqrt(t2)
    return np.sin(t) / t, (1 - np.cos(t)) / t2, (t - np.sin(t)) / (t2 * t)


def _exp(e, T):
    """(R, p) of exp of the tangent e = (linear, angular)"""
    w, K = e[3:], _skew(e[3:])
    a, b, c = _coeffs(w @ w, T)
    I = np.eye(3, dtype=T)
    return I + a * K + b * (K @ K), (I + b * K + c * (K @ K)) @ e[:3]


def _log(R, p, T):
    """the tangent (linear, angular) of the placement (R, p): the angle by atan2 (well-conditioned away from pi, where no case goes)"""
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], dtype=T) / 2
    s, c = np.sqrt(ax @ ax), (np.trace(R) - 1) / 2
    t = np.arctan2(s, c)
    w = ax * (t / s if s > 1e-8 else 1 + (t * t) / 6)
    K = _skew(w)
    _, b, cc = _coeffs(w @ w, T)
    V = np.eye(3, dtype=T) + b * K + cc * (K @ K)
    return np.concatenate([_solve(V, p[:, None], T).reshape(-1), w])


def _solve(A, B, T):
    """A^-1 B in the type T: LAPACK in float64, rbd_cases' Gaussian elimination in long double"""
    return np.linalg.solve(A, B) if T is np.float64 else RC.solve_longdouble(A, B)


def _placement(q, T):
    x, y, z, w = (T(c) for c in q[3:7])
    n = x * x + y * y + z * z + w * w
    R = np.array([[1 - 2 * (y * y + z * z) / n, 2 * (x * y - z * w) / n, 2 * (x * z + y * w) / n],
                  [2 * (x * y + z * w) / n, 1 - 2 * (x * x + z * z) / n, 2 * (y * z - x * w) / n],
                  [2 * (x * z - y * w) / n, 2 * (y * z + x * w) / n, 1 - 2 * (x * x + y * y) / n]], dtype=T)
    return R, np.array(q[:3], dtype=T)


def _base_difference(X0, X1, T, e0=None, e1=None):
    """log(X0^-1 X1) with X0, X1 moved along their own tangents e0, e1 first"""
    (R0, p0), (R1, p1) = X0, X1
    if e0 is not None:
        dR, dp = _exp(e0, T)
        R0, p0 = R0 @ dR, p0 + R0 @ dp
    if e1 is not None:
        dR, dp = _exp(e1, T)
        R1, p1 = R1 @ dR, p1 + R1 @ dp
    return _log(R0.T @ R1, R0.T @ (p1 - p0), T)


def difference(q0, q1, T=np.float64):
    """q1 (-) q0, the tangent at q0 (floating base in front, joints behind)"""
    q0, q1 = np.asarray(q0), np.asarray(q1)
    return np.concatenate([_base_difference(_placement(q0, T), _placement(q1, T), T), q1[7:].astype(T) - q0[7:].astype(T)])


def jac_difference(q0, q1, arg, T=np.float64):
    """(d (q1 (-) q0) / d q_arg in the tangent of q_arg [nv x nv], its own error estimate): -I / +I on the joints; the 6 x 6 base block by central
    differences at h, h / 2, h / 4, h / 8 Romberg-extrapolated three times (error h^8), the estimate = the last correction of the table"""
    nv = len(q0) - 1
    J = np.eye(nv, dtype=T) * (1 if arg else -1)
    J[:6, :6], worst = jac_log(_placement(np.asarray(q0), T), _placement(np.asarray(q1), T), arg, T)
    return J, worst


def jac_log(X0, X1, arg, T=np.float64):
    """(d log(X0^-1 X1) / d (the own tangent of X_arg) [6 x 6], its error estimate) of two placements (R, p): the Romberg table of `jac_difference`"""
    J = np.zeros((6, 6), dtype=T)
    h0, worst = T(0.05) if T is not np.float64 else 0.04, 0.0
    for k in range(6):
        tab = []
        for lvl in range(4):
            h = h0 / 2 ** lvl
            e = np.zeros(6, dtype=T)
            e[k] = h
            fp = _base_difference(X0, X1, T, *((None, e) if arg else (e, None)))
            fm = _base_difference(X0, X1, T, *((None, -e) if arg else (-e, None)))
            tab.append((fp - fm) / (2 * h))
        for m in range(1, 4):
            new = [(4 ** m * tab[j + 1] - tab[j]) / (4 ** m - 1) for j in range(len(tab) - 1)]
            last, tab = tab[-1], new
        J[:, k] = tab[0]
        worst = max(worst, float(np.abs(tab[0] - last).max()))
    return J, worst


def complex_step_jacobian(fun, x):
    """d fun / d x of an analytic vector function, [row, argument]"""
    x = np.asarray(x, dtype=np.float64)
    cols = []
    for k in range(x.size):
        z = x.astype(np.complex128)
        z[k] += 1e-30j
        cols.append(np.asarray(fun(z)).imag / 1e-30)
    return np.array(cols).T.reshape(-1, x.size)


# ------------------------------------------------------------------ the problem: two constraint sets, each with its cost

def problem(m, kind, t0=None):
    """(cost, cons) of a case.  "limits": anymal_problem as it is -- six joint limits, the linearised cone -- with the trotting reference; "accel": the
    nonlinear cone, the six limits and both acceleration limits, with the time-varying reference inside its window.  Both with u != u_ref, f != f_ref
    and weights spread over more than three decades (fixed seeds).  t0: the time the handle is discretised at (T0; CHAIN_T0 on the event chain, whose event
    times are absolute) -- the trotting rule starts, and the time-varying window opens, 0.17 before it."""
    t0 = T0 if t0 is None else t0
    cost, cons = anymal_problem(m, trotting_ref=kind == "limits", cone="linearized" if kind == "limits" else "nonlinear")
    rng = np.random.default_rng(91 if kind == "limits" else 92)
    nv, nu = m.nv, m.nu
    for name, n, lo, hi in (("q_weight", nv, -1, 2.5), ("v_weight", nv, -2, 1.5), ("a_weight", nv, -3, 0.5), ("u_weight", nu, -3, 0.5), ("qf_weight", nv, -1, 2.5), ("vf_weight", nv, -2, 1.5)):
        cost.set(name, 10.0 ** rng.uniform(lo, hi, n))
    cost.set("u_ref", rng.uniform(-5, 5, nu))
    for c in range(4):
        for k in range(3):
            cost.f_weight[c][k] = float(10.0 ** rng.uniform(-3.5, 0.0))
            cost.f_ref[c][k] += float(rng.uniform(-3, 3))
    if kind == "limits":
        cost.t_start = t0 - 0.17
    if kind == "accel":
        cost.use_time_varying_ref = 1
        cost.tv_t_begin, cost.tv_t_end = t0 - 0.17, t0 + 0.33
        cost.set("v_ref", rng.uniform(-0.4, 0.4, nv))
        cons.joint_acceleration_lower_limit = cons.joint_acceleration_upper_limit = 1
        for k in range(nv):
            cons.a_min[k], cons.a_max[k] = -3.0, 3.0
    return cost, cons


PROBLEMS = ("limits", "accel")


@functools.lru_cache(maxsize=None)
def iterate(which):
    """(struct, model dict, dict) of the iterate of a three-stage handle: q, v, lmd, gmm [N + 1], a, f, u, beta, mu, nu_passive [N], all distinct per
    stage, q_init / v_init = the state in front of stage 0, pts = the contact points.  The base stays within a radian or so of the reference and of
    its neighbours (the logarithm is ill-conditioned at pi); the joints lie inside their limits but for:
      one joint position / velocity / torque per stage 1e-3 INSIDE its bound (z / s spans decades right after init_constraints),
      one joint position / velocity / torque BEYOND its bound (the slack was bumped: a non-zero primal residual; z / s = 1 / barrier .. / 4),
      every acceleration at least 1 inside its bound of +-3 (ACCEL_SLACK).  Why: the entries of Wx = -K^-1 D come out of a solve and carry an absolute
      error of eps max|Wx| at the least, so Qxx = .. + Wx^T Haa Wx carries eps max|Wx|^2 max(dt z / s) absolutely, which rel_err sees in full on the
      base rows, whose scale is 1.  With no foot down max|Wx| = 223 (other_quadruped(1)), so a quarter of the bar needs dt z / s < 2.5e-12 /
      (2.2e-16 * 223^2) = 0.23, z / s < 5.7; an update may shrink a slack to 0.005 of itself (fraction to the boundary) and leaves z / s near
      barrier / s^2, so the slack must START at 0.005^-1 sqrt(1e-4 / 5.7) = 0.84 or more.  (Seen first: an acceleration 1e-3 or 1e-2 inside, or
      beyond its bound, put the float64 form of this referee 3e-11, 4.6e-12 and 1.9e-12 from its long double form on the sets with no foot down.)  The
      cases were made less extreme and the bar kept; the acceleration barrier still enters la at dt z = 4e-6 and Qaa at dt z / s, far above the bar,
      foot 0 1e-2 inside the linearised cone, foot 1 1e-2 inside the nonlinear one (and so beyond the linearised one), feet 2, 3 well inside."""
    m, M, _ = RC.quadruped(which)
    rng = np.random.default_rng([515, 0 if which == "anymal" else int(which) + 1])
    nv, nu, nq = m.nv, m.nu, m.nq
    lim = lambda name: np.array(getattr(m, name)[:nu])      # noqa: E731
    qlo, qhi = np.maximum(lim("q_min"), -3.0), np.minimum(lim("q_max"), 3.0)      # the range the other joints are SAMPLED in (the limits are +-9.4 and wider)
    vmax, umax = lim("v_max"), lim("u_max")
    step = lambda: np.concatenate([rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.4, 0.4, 3), np.zeros(nu)])      # noqa: E731
    q = [RBD.integrate(M, np.array(ANYMAL_Q_STANDING), np.concatenate([rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.5, 0.5, 3), np.zeros(nu)]))]
    for _ in range(N + 1):
        q.append(RBD.integrate(M, q[-1], step()))
    q = np.array(q)
    q[:, 7:] = qlo + rng.uniform(0.15, 0.85, (N + 2, nu)) * (qhi - qlo)
    v = np.concatenate([rng.uniform(-1, 1, (N + 2, 6)), rng.uniform(-0.7, 0.7, (N + 2, nu)) * np.minimum(vmax, 10.0)], axis=1)
    a = rng.uniform(-2, 2, (N, nv))
    u = rng.uniform(-0.7, 0.7, (N, nu)) * np.minimum(umax, 100.0)
    mu_c = 0.7
    f = np.zeros((N, 4, 3))
    for i in range(N):
        f[i, :, 2] = rng.uniform(20, 60, 4)
        f[i, :, :2] = rng.uniform(-0.3, 0.3, (4, 2)) * mu_c * f[i, :, 2:3]
        f[i, 0, :2] = (mu_c / np.sqrt(2.0) * f[i, 0, 2] - 1e-2, 0.0)
        f[i, 1, :2] = (np.sqrt(mu_c ** 2 * f[i, 1, 2] ** 2 - 1e-2), 0.0)
        j, k = (3 * i + 1) % nu, (3 * i + 5) % nu
        q[i + 1, 7 + j], q[i + 1, 7 + k] = lim("q_max")[j] - 1e-3, lim("q_min")[k] - 0.05      # (against the model's limits, not the sampling range)
        v[i + 1, 6 + j], v[i + 1, 6 + k] = -vmax[j] + 1e-3, vmax[k] + 0.05
        u[i, j], u[i, k] = umax[j] - 1e-3, -umax[k] - 0.5
    pts = RC.feet(M, q[1]) + rng.uniform(-0.03, 0.03, (4, 3))
    return m, M, dict(q=q[1:], v=v[1:], a=a, f=f, u=u, q_init=q[0], v_init=v[0], pts=pts, lmd=rng.uniform(-3, 3, (N + 1, nv)), gmm=rng.uniform(-3, 3, (N + 1, nv)),
                      beta=rng.uniform(-3, 3, (N, nv)), mu=rng.uniform(-3, 3, (N, 4, 3)), nu_passive=rng.uniform(-3, 3, (N, 6)))


SET_FIELDS = ("q", "v", "a", "f", "u", "lmd", "gmm", "beta", "mu", "nu_passive")


def stage_arrays(s, name, n=N):
    """values[nstages][dim] of a field for idocp_ocp_set_solution_stages: q v lmd gmm on the terminal stage too"""
    k = n + 1 if name in ("q", "v", "lmd", "gmm") else n
    return np.ascontiguousarray(np.asarray(s[name][:k]).reshape(k, -1))


# ------------------------------------------------------------------ the rigid-body rows of a stage, shared by every problem and barrier state

@functools.lru_cache(maxsize=None)
def rigid_body(which, mask, chain=False):
    """ocp_stage_cases.referee_record of every grid stage of the uniform handle (or of the event chain's grid stages, {position: record})"""
    if chain:
        _, M, s = chain_iterate(which)
        return {p: S.referee_record(M, s["q"][p], s["v"][p], s["a"][p], s["f"][p], s["u"][p], s["pts"][S.CHAIN_PHASES.index(tuple(mk))], S.CHAIN_T / S.CHAIN_N, mk, "stage")
                for p, (kind, mk) in enumerate(S.FORWARD_CHAIN) if kind == "stage"}
    _, M, s = iterate(which)
    return [S.referee_record(M, s["q"][i], s["v"][i], s["a"][i], s["f"][i], s["u"][i], s["pts"], DT, mask, "stage") for i in range(N)]


@functools.lru_cache(maxsize=None)
def chain_iterate(which):
    """the iterate along the event chain of ocp_stage_cases (nine positions, the terminal one last): its samples for q v a f u with the joints, the
    forces and the base moved as in `iterate`, and costates / multipliers of its own"""
    m, M, s = S.chain_inputs(which)
    _, _, it = iterate(which)
    rng = np.random.default_rng([516, 0 if which == "anymal" else int(which) + 1])
    n = len(S.FORWARD_CHAIN) + 1
    out = {k: np.array(x) for k, x in s.items()}
    for p in range(n):
        out["q"][p] = RBD.integrate(M, it["q"][p % (N + 1)], np.concatenate([rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.2, 0.2, 3), np.zeros(m.nu)]))
        out["v"][p, 6:] = it["v"][p % (N + 1), 6:]
        out["f"][p] = it["f"][p % N]
        out["u"][p] = it["u"][p % N]
    out.update(lmd=rng.uniform(-3, 3, (n, m.nv)), gmm=rng.uniform(-3, 3, (n, m.nv)), beta=rng.uniform(-3, 3, (n, m.nv)), mu=rng.uniform(-3, 3, (n, 4, 3)),
               nu_passive=rng.uniform(-3, 3, (n, 6)), xi=np.zeros((n, 12)), q_init=it["q_init"], v_init=it["v_init"])
    return m, M, out


# ------------------------------------------------------------------ the constraint rows and where the handle keeps their slack and dual

def _flags(cons, level):
    """the switches of rbd_score.constraint_rows for a grid stage: position rows from stage 2 on, velocity rows from stage 1 on (module docstring)"""
    c = types.SimpleNamespace(**{name: getattr(cons, name) for name, _ in cons._fields_})
    c.a_min, c.a_max = np.array(cons.a_min[:]), np.array(cons.a_max[:])
    c.joint_position_limits = int(bool(cons.joint_position_limits) and level >= 2)
    c.joint_velocity_limits = int(bool(cons.joint_velocity_limits) and level >= 1)
    return c


def families(cons, nu):
    """({family: slice of a stage's row of get_constraint_data}, dimc, rows per cone): the handle's record has every ENABLED component -- position,
    velocity, torque limits (lower then upper), the cone of all four feet, acceleration lower, upper -- whatever the stage or mask"""
    cr = 5 if cons.linearized_friction_cone else 2
    off, at = 0, {}
    for name, n, on in (("q", 2 * nu, cons.joint_position_limits), ("v", 2 * nu, cons.joint_velocity_limits), ("u", 2 * nu, cons.joint_torque_limits),
                        ("cone", 4 * cr, cons.linearized_friction_cone or cons.friction_cone), ("alo", nu, cons.joint_acceleration_lower_limit),
                        ("ahi", nu, cons.joint_acceleration_upper_limit), ("cd", 4, getattr(cons, "contact_distance", 0))):
        if on:
            at[name] = slice(off, off + n)
            off += n
    return at, off, cr


def row_index(cons, nu, mask, level):
    """where get_constraint_data keeps the rows of rbd_score.constraint_rows of a stage, in their order"""
    at, dimc, cr = families(cons, nu)
    c = _flags(cons, level)
    idx = []
    for name, on in (("q", c.joint_position_limits), ("v", c.joint_velocity_limits), ("u", c.joint_torque_limits), ("alo", c.joint_acceleration_lower_limit),
                     ("ahi", c.joint_acceleration_upper_limit)):
        if on:
            idx += range(at[name].start, at[name].stop)
    if "cone" in at:
        for cc, active in enumerate(mask):
            if active:
                idx += range(at["cone"].start + cr * cc, at["cone"].start + cr * (cc + 1))
    return np.array(idx, dtype=int), dimc


def check_barrier_construction(cons, nu, mask, slack, dual):
    """Right after init_constraints the barrier state is the one `iterate` was built for, family by family, read from the handle's record
    (slack, dual [N][dimc]): a row 1e-3 inside its bound (1e-2 for the cone), and a row BEYOND its bound, whose slack
    was therefore bumped into [barrier, 2 barrier) -- position rows on stage 2, velocity rows on stages 1 and 2, torque rows on every stage,
    the accelerations ACCEL_SLACK or more inside (`iterate`: why), the cone on the feet that are down (foot 0 near the linearised cone, foot 1
    near the nonlinear one and beyond the linearised one).  z / s then spans more than six decades on every stage."""
    at, _, cr = families(cons, nu)
    eps = cons.barrier
    near = lambda x, d: bool(((x > 0.9 * d) & (x < 1.1 * d)).any())      # noqa: E731
    bumped = lambda x: bool(((x >= eps) & (x < 2 * eps)).any())      # noqa: E731
    for i in range(N):
        sl = np.asarray(slack[i])
        for name, first in (("q", 2), ("v", 1), ("u", 0)):
            if name in at and i >= first:
                assert near(sl[at[name]], 1e-3) and bumped(sl[at[name]]), (name, i, sl[at[name]])
        for name in ("alo", "ahi"):
            if name in at:
                assert sl[at[name]].min() >= ACCEL_SLACK, (name, i, sl[at[name]])
        if "cone" in at:
            foot = 0 if cons.linearized_friction_cone else 1
            cone = sl[at["cone"]].reshape(4, cr)
            assert not mask[foot] or near(cone[foot], 1e-2), (i, cone[foot])
            assert not (cons.linearized_friction_cone and mask[1]) or bumped(cone[1]), (i, cone[1])
        live = sl > 0
        ratio = np.asarray(dual[i])[live] / sl[live]
        assert ratio.max() / ratio.min() > 1e6, (i, ratio.min(), ratio.max())


def _mutant_cone_rows(which):
    def rows(kind, mu, f):
        fx, fy, fz = f
        if kind == "linearized":
            mm = mu / np.sqrt(2.0)
            return [-fz, fx + mm * fz if which == "cone_fz_sign" else fx - mm * fz, -fx - mm * fz, fy - mm * fz, -fy - mm * fz]
        m2 = mu if which == "cone_mu" else mu * mu
        return [-fz, fx * fx + fy * fy + m2 * fz * fz if which == "cone_fz_sign" else fx * fx + fy * fy - m2 * fz * fz]
    return rows


@contextlib.contextmanager
def _cone_rows(mutate):
    """rbd_score.cone_rows, or for the sensitivity test a mutant in its place"""
    if mutate not in ("cone_fz_sign", "cone_mu"):
        yield
        return
    keep = RS.cone_rows
    RS.cone_rows = _mutant_cone_rows(mutate)
    try:
        yield
    finally:
        RS.cone_rows = keep


# ------------------------------------------------------------------ the referee

def reference_at(M, cost, t, mutate=None):
    """(q_ref, v_ref) of the stage time t (rbd_score.reference_tables)"""
    qt, vt = RS.reference_tables(M, cost, t, 0.0, 0)
    q_ref = qt[0]
    if mutate == "trot_phase":      # every knee offset handed to the next leg
        base = np.array(cost.q_ref[:M["nq"]])
        off = q_ref - base
        off[[9, 12, 15, 18]] = off[[18, 9, 12, 15]]
        q_ref = base + off
    return q_ref, vt[0]


def lqr_stage(m, M, cost, cons, rec, st, slack, dual, T=LD, mutate=None, ext=None):
    """The condensed stage (module docstring) as {name of QUANTITIES: float64 array}, "fd_error": the largest error estimate of the differenced
    Jacobians.  st: dict(dt, t, level, mask, q, v, a, f [4][3], u, beta, mu [4][3], q_next, v_next, q_prev, lmd, gmm, lmd_next, gmm_next); rec: the
    referee_record of the stage; slack, dual: the stage's row of get_constraint_data.  T: the real type everything is formed in.  ext: the terms with frame
    Jacobians of their own (ocp_ext_cases.ext_record: "lq" [nv] and "H" [nv][nv], dt and weights inside), added to the gradient and the Hessian of q."""
    nv, nu, nq = m.nv, m.nu, m.nq
    dt, mask = T(st["dt"]), tuple(int(x) for x in st["mask"])
    act = RC.rows_of(mask)
    nf = int(act.sum())
    c = lambda x: np.asarray(x, dtype=np.float64).astype(T)      # noqa: E731
    q, v, a, u, f = np.asarray(st["q"], dtype=np.float64), c(st["v"]), c(st["a"]), c(st["u"]), np.asarray(st["f"], dtype=np.float64).reshape(4, 3)
    fa = c(f.reshape(-1)[act])
    W = lambda name, n: c(getattr(cost, name)[:n])      # noqa: E731
    q_ref, v_ref = reference_at(M, cost, float(st["t"]), mutate)
    fd = []
    # ---- the cost: gradient and Gauss-Newton Hessian
    e = difference(q_ref, q, T)
    Jq, err = jac_difference(q_ref, q, 1, T)
    fd.append(err)
    if mutate == "cost_J_identity":
        Jq = np.eye(nv, dtype=T)
    wq, wv, wa, wu = W("q_weight", nv), W("v_weight", nv), W("a_weight", nv), W("u_weight", nu)
    wf = c(np.array([cost.f_weight[cc][:] for cc in range(4)]).reshape(-1)[act])
    f_ref = c(np.array([cost.f_ref[cc][:] for cc in range(4)]).reshape(-1)[act])
    gq, Hqq = dt * (Jq.T @ (wq * e)), dt * (Jq.T @ (wq[:, None] * Jq))
    gv, ga, gu, gf = dt * wv * (v - c(v_ref)), dt * wa * a, dt * wu * (u - W("u_ref", nu)), dt * wf * (fa - f_ref)
    hv, ha, hu, Hff = dt * wv, dt * wa, dt * wu, np.diag(dt * wf)
    Hqq, Hff = Hqq.copy(), Hff.astype(T)
    if ext is not None:
        gq, Hqq = gq + c(ext["lq"]), Hqq + c(ext["H"])
    # ---- the inequality rows: dt grad g (z + (z (g + s) - (s z - eps)) / s) and dt (z / s) grad g grad g^T
    idx, dimc = row_index(cons, nu, mask, st["level"])
    assert len(slack) == len(dual) == dimc, (len(slack), dimc)
    if idx.size:
        flags = _flags(cons, st["level"])
        model = types.SimpleNamespace(nu=nu, nv=nv, nq=nq, **{name: np.array(getattr(m, name)[:nu]) for name in ("q_min", "q_max", "v_max", "u_max")})

        def rows(z):      # z = (joint positions, joint velocities, u, joint accelerations, forces [4][3])
            qz, vz, az = (np.concatenate([np.zeros(n - nu), z[k * nu:(k + 1) * nu]]) for k, n in ((0, nq), (1, nv), (3, nv)))
            return np.array(RS.constraint_rows(model, flags, qz, vz, z[2 * nu:3 * nu], az, z[4 * nu:].reshape(4, 3), mask))

        z0 = np.concatenate([q[7:], np.asarray(st["v"])[6:], np.asarray(st["u"]), np.asarray(st["a"])[6:], f.reshape(-1)]).astype(np.float64)
        with _cone_rows(mutate):
            g = c(rows(z0))
            G = c(complex_step_jacobian(rows, z0))
        assert g.size == idx.size, (g.size, idx.size)
        s_, z_ = c(np.asarray(slack)[idx]), c(np.asarray(dual)[idx])
        assert (np.asarray(slack)[idx] > 0).all(), "a row of the stage has no slack in the handle's record"
        eps = T(cons.barrier)
        coef = dt * (z_ + (z_ * (g + s_) - (s_ * z_ - eps)) / s_)
        if mutate == "barrier_dt":      # the dt dropped from the gradient of ONE row, the one that weighs most
            coef[int(np.abs(coef).argmax())] /= dt
        grad = G.T @ coef
        Hess = G.T @ ((dt * z_ / s_)[:, None] * G)
        blocks = [slice(0, nu), slice(nu, 2 * nu), slice(2 * nu, 3 * nu), slice(3 * nu, 4 * nu)]
        gq[6:] += grad[blocks[0]]; gv[6:] += grad[blocks[1]]; gu += grad[blocks[2]]; ga[6:] += grad[blocks[3]]
        gf += grad[4 * nu:][act]
        Hqq[6:, 6:] += Hess[blocks[0], blocks[0]]
        Hvv = np.diag(hv); Hvv[6:, 6:] += Hess[blocks[1], blocks[1]]
        Huu = np.diag(hu) + Hess[blocks[2], blocks[2]]
        Haa = np.diag(ha); Haa[6:, 6:] += Hess[blocks[3], blocks[3]]
        Hff = Hff + Hess[4 * nu:, 4 * nu:][np.ix_(act, act)]
        cross = Hess.copy()      # the rows couple nothing across (q, v, u, a, f): a cross block would have no place in the model below
        for b in blocks + [slice(4 * nu, None)]:
            cross[b, b] = 0
        assert not cross.any()
    else:
        Hvv, Huu, Haa = np.diag(hv), np.diag(hu), np.diag(ha)
    # ---- the state equation and the costates
    Fq = difference(st["q_next"], q, T) + dt * v
    Fv = v + dt * a - c(st["v_next"])
    Fqq, e1 = jac_difference(st["q_next"], q, 1, T)
    Fqn, e2 = jac_difference(st["q_next"], q, 0, T)
    Fqp, e3 = jac_difference(q, st["q_prev"], 0, T)
    fd += [e1, e2, e3]
    lmd, gmm, lmd_n, gmm_n = c(st["lmd"]), c(st["gmm"]), c(st["lmd_next"]), c(st["gmm_next"])
    gq = gq + Fqq.T @ lmd_n + (0 if mutate == "no_q_prev" else Fqp.T @ lmd)
    gv = gv + dt * lmd_n + gmm_n - gmm
    ga = ga + (0 if mutate == "no_gmm_next_in_la" else dt * gmm_n)
    # ---- the dynamics and the Baumgarte rows with their multipliers
    beta, mu = c(st["beta"]), c(np.asarray(st["mu"]).reshape(-1)[act])
    Mm, J = c(rec["M"]), c(rec["J"]).reshape(nf, nv)
    dIDq, dIDv, dCq, dCv = c(rec["dID/dq"]), c(rec["dID/dv"]), c(rec["dC/dq"]).reshape(nf, nv), c(rec["dC/dv"]).reshape(nf, nv)
    gq = gq + dt * (dIDq.T @ beta + dCq.T @ mu)
    gv = gv + dt * (dIDv.T @ beta + dCv.T @ mu)
    ga = ga + dt * (Mm.T @ beta + J.T @ mu)
    gf = gf - dt * (J @ beta)                       # dID / df = -J^T
    gu = gu - dt * beta[6:]
    # ---- the elimination of w = [da; -df]
    K = np.block([[Mm, J.T], [J, np.zeros((nf, nf), dtype=T)]])
    D = np.block([[dIDq, dIDv], [dCq, dCv]])
    St = np.zeros((nv + nf, nu), dtype=T)
    St[6:nv] = np.eye(nu, dtype=T)
    r = np.concatenate([c(rec["ID - S^T u"]), c(rec["C"])])
    rhs = np.concatenate([-D, St, -r[:, None]], axis=1)
    sol = _solve(K, rhs, T)
    Wx, Wu, w0 = sol[:, :2 * nv], sol[:, 2 * nv:2 * nv + nu], sol[:, -1]
    Hww = np.block([[Haa, np.zeros((nv, nf), dtype=T)], [np.zeros((nf, nv), dtype=T), Hff]])
    gw = np.concatenate([ga, -gf]) + Hww @ w0
    Hxx = np.block([[Hqq, np.zeros((nv, nv), dtype=T)], [np.zeros((nv, nv), dtype=T), Hvv]])
    out = {"Qxx": Hxx + Wx.T @ Hww @ Wx, "Qxu": Wx.T @ Hww @ Wu, "Quu": Huu + Wu.T @ Hww @ Wu,
           "lx": np.concatenate([gq, gv]) + Wx.T @ gw, "lu": gu + Wu.T @ gw}
    # ---- the two rows of the state equation solved for the next node's step
    base = _solve(Fqn, np.concatenate([Fqq, dt * np.eye(nv, dtype=T), Fq[:, None]], axis=1), T)
    Aqq, Aqv, Fxq = -base[:, :nv], -base[:, nv:2 * nv], -base[:, -1]
    if mutate == "A_base_identity":
        Aqq = np.eye(nv, dtype=T)
    Av = dt * Wx[:nv]
    Av[:, nv:] += np.eye(nv, dtype=T)
    out["A"] = np.block([[Aqq, Aqv], [Av[:, :nv], Av[:, nv:]]])
    out["B"] = np.concatenate([np.zeros((nv, nu), dtype=T), dt * Wu[:nv]])
    out["Fx"] = np.concatenate([Fxq, Fv + dt * w0[:nv]])
    out = {k: np.asarray(x, dtype=np.float64) for k, x in out.items()}
    out["fd_error"] = max(fd)
    return out


def terminal_stage(m, M, cost, st, T=LD, ext=None):
    """(Hessian, gradient) of the terminal node: 1/2 |q (-) q_ref|^2_Wqf + 1/2 |v - v_ref|^2_Wvf + lmd . Fq- + gmm . Fv-, Gauss-Newton; st: dict(t, q, v,
    q_prev, lmd, gmm)"""
    nv = m.nv
    c = lambda x: np.asarray(x, dtype=np.float64).astype(T)      # noqa: E731
    q_ref, v_ref = reference_at(M, cost, float(st["t"]))
    e = difference(q_ref, st["q"], T)
    Jq, e0 = jac_difference(q_ref, st["q"], 1, T)
    Fqp, e1 = jac_difference(st["q"], st["q_prev"], 0, T)
    wq, wv = c(cost.qf_weight[:nv]), c(cost.vf_weight[:nv])
    H = np.zeros((2 * nv, 2 * nv), dtype=T)
    H[:nv, :nv] = Jq.T @ (wq[:, None] * Jq)
    H[nv:, nv:] = np.diag(wv)
    g = np.concatenate([Jq.T @ (wq * e) + Fqp.T @ c(st["lmd"]), wv * (c(st["v"]) - c(v_ref)) - c(st["gmm"])])
    if ext is not None:      # (ocp_ext_cases.ext_record of the terminal node)
        H[:nv, :nv] += c(ext["H"])
        g[:nv] += c(ext["lq"])
    return H.astype(np.float64), g.astype(np.float64), max(e0, e1)


# ------------------------------------------------------------------ what a stage is made of, and the comparison

def uniform_stage(s, i, mask, t0=T0, dt=DT):
    """st of lqr_stage for grid stage i of the uniform handle with the iterate s (`iterate`); the state in front of stage 0 is s["q_init"]"""
    return dict(dt=dt, t=t0 + i * dt, level=i, mask=mask, q=s["q"][i], v=s["v"][i], a=s["a"][i], f=s["f"][i], u=s["u"][i], beta=s["beta"][i], mu=s["mu"][i],
                q_next=s["q"][i + 1], v_next=s["v"][i + 1], q_prev=s["q"][i - 1] if i else s["q_init"], lmd=s["lmd"][i], gmm=s["gmm"][i],
                lmd_next=s["lmd"][i + 1], gmm_next=s["gmm"][i + 1])


def distances(got, ref):
    """{quantity: (helpers.rel_err, worst row)}; of Qxx the upper triangle only (the block below it is written by the sweep)"""
    out = {}
    for name, g in zip(QUANTITIES, got):
        r = ref[name]
        if name == "Qxx":
            g, r = np.triu(g), np.triu(r)
        out[name] = S.worst_row(np.asarray(g), r)
    return out


def hold(dist, where, worst=None, bar=BAR):
    if worst is not None:
        for name, (d, _) in dist.items():
            worst[name] = max(worst.get(name, 0.0), d)
    bad = ["%s: %.2e at row %d (bar %.1e)" % (name, d, row, bar) for name, (d, row) in dist.items() if not d < bar]
    assert not bad, "%s -- %s" % (where, "; ".join(bad))


def check_referee(ref64, refld, label):
    """the referee against itself: its float64 stage against its long double one, every quantity within a quarter of the bar, and the error estimate of
    the differenced Jacobians (long double route) below a quarter of the bar; prints both like ocp_stage_cases.check_referee"""
    d = {name: S.worst_row(ref64[name], refld[name])[0] for name in QUANTITIES}
    worst = max(d.values())
    print("referee %s: self-distance %.1e (%s), difference-quotient error %.1e" % (label, worst, max(d, key=d.get), refld["fd_error"]))
    assert worst <= SELF_BAR and refld["fd_error"] <= SELF_BAR, (label, d, refld["fd_error"])
    return worst


def terminal_reference(which, kind, T=LD):
    """ocp_lqr_cases.terminal_stage of the uniform handle's terminal node"""
    m, M, s = iterate(which)
    cost, _ = problem(m, kind)
    return terminal_stage(m, M, cost, dict(t=T0 + N * DT, q=s["q"][N], v=s["v"][N], q_prev=s["q"][N - 1], lmd=s["lmd"][N], gmm=s["gmm"][N]), T)


def hold_terminal(which, kind, Pn, sn, label):
    """P[N] and s[N] of a Riccati record against the terminal cost's Hessian and MINUS its gradient; the referee against itself first"""
    H, g, err = terminal_reference(which, kind)
    H64, g64, _ = terminal_reference(which, kind, np.float64)
    self_d = max(S.worst_row(H64, H)[0], S.worst_row(g64, g)[0])
    assert self_d <= SELF_BAR and err <= SELF_BAR, (label, self_d, err)
    d = {"P[N]": S.worst_row(Pn, H), "s[N]": S.worst_row(sn, -g)}
    print("%s terminal: P[N] %.1e  s[N] %.1e  (referee against itself %.1e)" % (label, d["P[N]"][0], d["s[N]"][0], self_d))
    hold(d, label + ", terminal stage")


def summary(worst):
    return "  ".join("%s %.1e" % (name, worst[name]) for name in QUANTITIES if name in worst)
