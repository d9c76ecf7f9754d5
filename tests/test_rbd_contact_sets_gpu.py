"""The quadruped kernels of the rigid-body API (rbd_batch_kernel.hip behind idocp_rbd_contact_dynamics_batch, rbd_forward_kernel.hip behind
idocp_rbd_forward_dynamics_batch / idocp_rbd_rollout) and the forward chain kernel on every contact set, on hard states and at every position
of a batch.  Both quadruped kernels pack the rows of the active contacts through a table and run the in-register Cholesky routines of
dev_dense.hpp at the runtime size dimf = 3 x (active contacts): 12, 9, 6, 3 and 0 are all here, with every choice of the contacts.

The referee is the numpy model evaluated at test time (rbd_cases.py on independent_rbd.py / rbd_forward.py / gen_golden_rbd.py), the bar
independent_rbd.BAR = 1e-11 under helpers.rel_err; test_rbd_contact_sets_host.py holds the referee's own error on these very cases below 1e-13.
The position tests compare a large tiled batch with the small refereed call bit for bit: a sample's answer depends on neither its index nor
its neighbours."""

import numpy as np
import pytest

import independent_rbd as IR
import rbd_cases as RC
import rbd_forward as F
from helpers import anymal_model, rel_err
from idocp_amd import capi
from rbd_batch import ALL_OUTPUTS, IMPULSE, STAGE, DeviceArray, Rbd, packed_mjtjinv, random_samples
from rbd_cases import DT, TS, mask_id, rows_of, tiled

pytestmark = pytest.mark.gpu
BAR = IR.BAR
NBIG = 131                  # 65 full workgroups and one with a single live wavefront: every sample in both wavefront slots

all_masks = pytest.mark.parametrize("mask", RC.ALL_MASKS, ids=[mask_id(x) for x in RC.ALL_MASKS])
hard_masks = pytest.mark.parametrize("mask", RC.HARD_MASKS, ids=[mask_id(x) for x in RC.HARD_MASKS])
hard_names = pytest.mark.parametrize("name", RC.HARD_NAMES)
modes = pytest.mark.parametrize("mode", [STAGE, IMPULSE], ids=["stage", "impulse"])
position_masks = pytest.mark.parametrize("mask", [(1, 1, 1, 0), (0, 1, 0, 1)], ids=["1110", "0101"])


def report(label, errs):
    print(label, {k: "%.2e" % e for k, e in errs.items()})
    bad = {k: e for k, e in errs.items() if not e < BAR}
    assert not bad, (label, bad)


# ------------------------------------------------------------------ the inverse side: idocp_rbd_contact_dynamics_batch

def check_inverse(label, o, refs, mask, mode, nv):
    """every output of one call against rbd_cases.inverse_terms of its samples"""
    rows = rows_of(mask)
    dimf, errs = int(rows.sum()), {}
    for k, kref in (RC.STAGE_HELD if mode == STAGE else RC.IMPULSE_HELD).items():
        x = o[k]
        if k in RC.CONTACT_OUTPUTS:
            assert (x[:, ~rows] == 0).all(), (label, k)             # the rows of an inactive contact: exactly zero
            x = x[:, rows]
        elif k == "MJtJinv":
            assert (x[:, (nv + dimf) ** 2:] == 0).all(), label     # idocp_hip.h: behind the packed block the slot is zero in the host form
            x = np.array([packed_mjtjinv(s, nv, dimf) for s in x])
        errs[k] = RC.dist(x, IR.stack(refs, kref))
    if mode == IMPULSE:
        assert (o["dtau_dv"] == 0).all(), label                     # (the impulse dynamics see no velocity)
    report(label, errs)


@modes
@all_masks
@pytest.mark.parametrize("which", RC.MODELS, ids=[str(x) for x in RC.MODELS])
def test_inverse_on_every_contact_set(which, mask, mode):
    m, _, (q, v, a, f, pts, _) = RC.quadruped(which)
    r = Rbd(m)
    o = r.call(mode, q, v, a, mask, TS if mode == STAGE else 0.0, f=f, contact_points=pts)
    check_inverse("%s %s mode %d:" % (which, mask_id(mask), mode), o, RC.inverse_reference(which, mask), mask, mode, m.nv)
    r.close()


@hard_masks
@hard_names
def test_inverse_on_the_hard_states(name, mask):
    m, _, cases = RC.hard_cases()
    s = cases[name]
    one = lambda x: np.asarray(x)[None]      # noqa: E731
    r = Rbd(m)
    for mode in (STAGE, IMPULSE):
        o = r.call(mode, one(s["q"]), one(s["v"]), one(s["a"]), mask, s["time_step"] if mode == STAGE else 0.0, f=one(s["f"]), contact_points=one(s["pts"]))
        check_inverse("%s %s mode %d:" % (name, mask_id(mask), mode), o, [RC.hard_inverse_reference(name, mask)], mask, mode, m.nv)
    r.close()


@modes
@position_masks
def test_inverse_at_every_position_of_the_batch(mask, mode):
    """n = 131 tiled from the 3 refereed samples: every copy bit for bit the n = 3 call"""
    m, _, (q, v, a, f, pts, _) = RC.quadruped("anymal")
    r = Rbd(m)
    ts = TS if mode == STAGE else 0.0
    small = r.call(mode, q, v, a, mask, ts, f=f, contact_points=pts)
    big = r.call(mode, *(tiled(x, NBIG) for x in (q, v, a)), mask, ts, f=tiled(f, NBIG), contact_points=tiled(pts, NBIG))
    for k in ALL_OUTPUTS:
        assert np.isfinite(small[k]).all(), k
        assert np.array_equal(big[k], tiled(small[k], NBIG)), (k, np.argwhere(big[k] != tiled(small[k], NBIG))[:3])
    r.close()


# ------------------------------------------------------------------ the forward side: idocp_rbd_forward_dynamics_batch, idocp_rbd_rollout

# The round trip through the inverse call is held as test_rbd_forward_dynamics_gpu.py holds it: tau under rel_err against [0; u], |C| and
# the impulse |tau| to BAR itself.  One figure of one hard state cannot be: C of the STAGE call at time_step = 1e-3.  The zero that comes back is
# a sum of terms, FP64 carries it to a few ulp of the largest, and there b = C(q, v, 0) reaches 2.9e4 (1 / time_step^2 = 1e6 times the
# centimetres the contact points are off).  On the MI355X |C| comes back as 5.7e-11 / 9.6e-11 / 2.2e-11 (masks 1111 / 1110 / 0010), 3e-15 of
# |b|; so that one figure is held to BAR x max(1, |b|), b taken from the referee -- what helpers.rel_err does with a quantity that has
# entries of its own.  Everything else stays on the bars above, v x 20 included (there |tau - S^T u| = 8.2e-12 and |C| = 5.7e-12 come back).
SCALED_C = ("stiff",)


def term_scale(*terms):
    return max([1.0] + [float(np.abs(t).max()) for t in terms if np.size(t)])


@hard_masks
@hard_names
def test_forward_on_the_hard_states(name, mask):
    m, M, cases = RC.hard_cases()
    s = cases[name]
    q, v, u, pts, ts = s["q"], s["v"], s["u"], s["pts"], s["time_step"]
    stage, imp = RC.hard_forward_terms(name)
    rows, on = rows_of(mask), np.array(mask, dtype=bool)
    one = lambda x: np.asarray(x)[None]      # noqa: E731
    r = Rbd(m)
    # STAGE
    o = F.forward(r, STAGE, one(q), one(v), one(u), mask, ts, DT, contact_points=one(pts))
    a_ref, f_ref = F.solve_terms(stage, u, mask)
    qn, vn = F.euler_step(M, q, v, o["a"][0], DT)
    errs = {"a": rel_err(o["a"][0], a_ref), "f": rel_err(o["f"][0], f_ref), "q_next": rel_err(o["q_next"][0], qn), "v_next": rel_err(o["v_next"][0], vn)}
    back = r.call(STAGE, one(q), one(v), o["a"], mask, ts, f=o["f"], contact_points=one(pts), outputs=("tau", "C"))
    tau = np.concatenate([np.zeros(6), u])
    errs["tau"] = rel_err(back["tau"][0], tau)
    errs["C"] = float(np.abs(back["C"][0][rows]).max()) if rows.any() else 0.0
    if name in SCALED_C:
        print("%s %s STAGE round trip: |C| %.2e, |b| %.2e" % (name, mask_id(mask), errs["C"], term_scale(stage["b"][rows])))
        errs["C"] = errs["C"] / term_scale(stage["b"][rows])
    report("%s %s STAGE (|a| %.0f, |f| %.0f):" % (name, mask_id(mask), np.abs(a_ref).max(), np.abs(f_ref).max()), errs)
    assert (o["f"][0][~on] == 0).all()
    # the step stays on the side of the input quaternion (w = 0, w < 0 included) and on the unit sphere
    assert np.dot(o["q_next"][0][3:7], q[3:7]) > 0 and abs(np.linalg.norm(o["q_next"][0][3:7]) - 1) <= 1e-15
    if name == "rest":
        # u = NULL is u = 0: the same bits, and so the same referee
        null = F.forward(r, STAGE, one(q), one(v), None, mask, ts, DT, contact_points=one(pts))
        for k in F.FD_OUTPUTS:
            assert np.array_equal(null[k], o[k]), k
    # IMPULSE
    o = F.forward(r, IMPULSE, one(q), one(v), one(u), mask, 0.0, DT)
    dv_ref, l_ref = F.solve_terms(imp, None, mask)
    errs = {"dv": rel_err(o["a"][0], dv_ref), "lambda": rel_err(o["f"][0], l_ref), "v_next": rel_err(o["v_next"][0], v + o["a"][0])}
    back = r.call(IMPULSE, one(q), one(v), o["a"], mask, 0.0, f=o["f"], outputs=("tau", "C"))
    errs["tau"] = float(np.abs(back["tau"][0]).max())
    errs["C"] = float(np.abs(back["C"][0][rows]).max()) if rows.any() else 0.0
    report("%s %s IMPULSE:" % (name, mask_id(mask)), errs)
    assert (o["f"][0][~on] == 0).all() and (o["q_next"][0] == q).all()
    r.close()


@modes
@position_masks
def test_forward_at_every_position_of_the_batch(mask, mode):
    """n = 131 tiled from the 5 samples test_rbd_forward_dynamics_gpu.py referees on every mask: bit for bit the n = 5 call"""
    from test_rbd_forward_dynamics_gpu import quadruped
    m, _, (q, v, u, pts), _, _ = quadruped("anymal")
    r = Rbd(m)
    ts = TS if mode == STAGE else 0.0
    small = F.forward(r, mode, q, v, u, mask, ts, DT, contact_points=pts)
    big = F.forward(r, mode, tiled(q, NBIG), tiled(v, NBIG), tiled(u, NBIG), mask, ts, DT, contact_points=tiled(pts, NBIG))
    for k in F.FD_OUTPUTS:
        assert np.isfinite(small[k]).all(), k
        assert np.array_equal(big[k], tiled(small[k], NBIG)), (k, np.argwhere(big[k] != tiled(small[k], NBIG))[:3])
    r.close()


CHAINS = [("arm2_1", 2, 1, False), ("arm6", 0, 0, False), ("arm8_1", 8, 1, False)]


@pytest.mark.parametrize("n", [64, 65, 128, 130])
@pytest.mark.parametrize("nv,seed,zaxes", [c[1:] for c in CHAINS], ids=[c[0] for c in CHAINS])
def test_chains_at_every_position_of_the_batch(nv, seed, zaxes, n):
    """rbd_forward_chain_kernel runs one lane per sample, 64 per block: one full block, one sample into the second, two full blocks (the last
    lane of the last block is a sample; n = 128 is the case that catches a block stride of 63 in place of 64, which leaves sample 127 to no
    lane while 64, 65 and 130 still pass -- keep it) and a third, partly filled block -- tiled from the 5 samples and torques of
    test_rbd_forward_dynamics_gpu.test_chains, which holds the n = 5 answers to the model.  Through device pointers, into buffers that hold
    NaN: a sample no lane took stays NaN, whatever an earlier launch left in the handle's own staging."""
    assert (nv, seed, zaxes) in [c[1:] for c in IR.chain_cases()] + [(0, 0, False)]
    m, _ = IR.chain(nv, seed, zaxes)
    (q, v, _), _ = IR.chain_samples(nv, seed, zaxes)
    u = np.random.default_rng([41, nv, seed]).uniform(-10, 10, (2, q.shape[0], m.nv))[0]
    r = Rbd(m)
    small = F.forward(r, STAGE, q, v, u, None, 0.0, DT)
    dev = {"q": DeviceArray(tiled(q, n)), "v": DeviceArray(tiled(v, n)), "u": DeviceArray(tiled(u, n))}
    dev.update({k: DeviceArray(np.full((n, m.nv), np.nan)) for k in ("a", "q_next", "v_next")})
    io = capi.RbdFdIO()
    for k, x in dev.items():
        setattr(io, k, x.ptr.value)
    capi.check(F.forward_raw(r, STAGE, n, None, 0.0, DT, io, device=True), "idocp_rbd_forward_dynamics_batch_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    for k in ("a", "q_next", "v_next"):
        big = dev[k].numpy()
        assert np.isfinite(small[k]).all(), k
        assert np.array_equal(big, tiled(small[k], n)), (k, np.argwhere(big != tiled(small[k], n))[:3])
    for x in dev.values():
        x.free()
    r.close()


@modes
def test_the_step_in_place(mode):
    """idocp_hip.h: q_next may be the very pointer q and v_next the very pointer v (the rollout's touchdown impulse relies on it for v).  The
    device form with q_next = q, v_next = v gives the bits of the call with separate outputs."""
    from test_rbd_forward_dynamics_gpu import N, quadruped
    m, _, (q, v, u, pts), _, _ = quadruped("anymal")
    mask = (1, 1, 1, 0)
    ts = TS if mode == STAGE else 0.0
    r = Rbd(m)
    apart = F.forward(r, mode, q, v, u, mask, ts, DT, contact_points=pts)
    assert all(np.isfinite(x).all() for x in apart.values())
    if mode == STAGE:
        assert not np.array_equal(apart["q_next"], q) and not np.array_equal(apart["v_next"], v)      # (there is a step to take)
    dev = {"q": DeviceArray(q), "v": DeviceArray(v), "u": DeviceArray(u), "contact_points": DeviceArray(pts),
           "a": DeviceArray(np.zeros((N, m.nv))), "f": DeviceArray(np.zeros((N, 4, 3)))}
    io = capi.RbdFdIO()
    for k, x in dev.items():
        setattr(io, k, x.ptr.value)
    io.q_next, io.v_next = dev["q"].ptr.value, dev["v"].ptr.value
    capi.check(F.forward_raw(r, mode, N, mask, ts, DT, io, device=True), "idocp_rbd_forward_dynamics_batch_device")
    capi.check(r.lib.idocp_rbd_synchronize(r.h), "idocp_rbd_synchronize")
    for k, name in (("a", "a"), ("f", "f"), ("q", "q_next"), ("v", "v_next")):
        assert np.array_equal(dev[k].numpy(), apart[name]), name
    for x in dev.values():
        x.free()
    r.close()


SCHEDULE = ([1, 1, 1, 1], [0, 0, 0, 1], [0, 0, 0, 1], [1, 1, 1, 1], [0, 1, 1, 0], [0, 1, 1, 0])


def test_rollout_with_odd_touchdowns():
    """the touchdown in front of step 3 lands three feet at once (an impulse with 9 rows), the change of status in front of step 4 lands
    none; every step and the impulse are refereed at the GPU's own state, as test_rollout_over_a_contact_schedule does it"""
    m = anymal_model()
    M = IR.model_from_struct(m)
    n, steps = 2, len(SCHEDULE)
    rng = np.random.default_rng(19)
    q0, v0 = random_samples(rng, n)[:2]
    v0 = 0.3 * v0
    u = rng.uniform(-20, 20, (steps, n, m.nu))
    pts = np.repeat((F.foot_positions(m, q0) + rng.uniform(-0.02, 0.02, (n, 4, 3)))[None], steps, axis=0)
    r = Rbd(m)
    qt, vt, at, ft = F.rollout(r, q0, v0, u, SCHEDULE, TS, DT, pts, impulse=True)
    assert all(np.isfinite(x).all() for x in (qt, vt, at, ft))
    q, v = q0.copy(), v0.copy()
    jumps = {}
    for k in range(steps):
        new = [int(b and not a) for a, b in zip(SCHEDULE[k - 1], SCHEDULE[k])] if k else [0] * 4
        if any(new):
            imp = F.forward(r, IMPULSE, q, v, None, new, 0.0, DT)
            jumps[k] = (new, q.copy(), v.copy(), imp)
            v = imp["v_next"]
        assert (qt[k] == q).all() and (vt[k] == v).all(), k
        o = F.forward(r, STAGE, q, v, u[k], SCHEDULE[k], TS, DT, contact_points=pts[k])
        assert (at[k] == o["a"]).all() and (ft[k] == o["f"]).all(), k
        ref = [F.reference(M, q[i], v[i], u[k][i], SCHEDULE[k], pts[k][i], TS) for i in range(n)]
        step = [F.euler_step(M, q[i], v[i], o["a"][i], DT) for i in range(n)]
        errs = {"a": rel_err(o["a"], np.array([x[0] for x in ref])), "f": rel_err(o["f"].reshape(n, -1), np.array([x[1].reshape(-1) for x in ref])),
                "q_next": rel_err(o["q_next"], np.array([x[0] for x in step])), "v_next": rel_err(o["v_next"], np.array([x[1] for x in step]))}
        report("rollout step %d %s:" % (k, mask_id(SCHEDULE[k])), errs)
        q, v = o["q_next"], o["v_next"]
    assert (qt[steps] == q).all() and (vt[steps] == v).all()
    # one touchdown, in front of step 3, on contacts 0, 1 and 2; none in front of step 4 (contacts only leave there)
    assert list(jumps) == [3] and jumps[3][0] == [1, 1, 1, 0]
    new, q_pre, v_pre, imp = jumps[3]
    ref = [F.reference(M, q_pre[i], v_pre[i], None, new, impulse=True) for i in range(n)]
    errs = {"dv": rel_err(imp["a"], np.array([x[0] for x in ref])), "lambda": rel_err(imp["f"].reshape(n, -1), np.array([x[1].reshape(-1) for x in ref]))}
    report("touchdown impulse on three contacts:", errs)
    assert np.abs(imp["a"]).max() > 1e-3 and (imp["f"][:, 3] == 0).all() and np.abs(imp["f"][:, :3]).min(axis=2).max() > 0
    # without the touchdown impulse the velocity does not jump
    vn = F.rollout(r, q0, v0, u, SCHEDULE, TS, DT, pts, impulse=False)[1]
    assert (vn[:3] == vt[:3]).all() and not (vn[3] == vt[3]).all()
    r.close()
