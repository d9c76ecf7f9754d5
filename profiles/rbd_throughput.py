"""Throughput of the batched rigid-body API (idocp_rbd_contact_dynamics_batch_device and idocp_rbd_forward_dynamics_batch_device): ANYmal, four active contacts,
device pointers, n = 122 880 samples per launch by default (the stage count of the headline step: 1 024 instances x 120 stages).  Every launch is
bracketed by HIP events on the handle's stream after warm-up launches; prints one JSON line with the median / min / max ms per launch and the
samples per second of each output selection.  The fd_* rows are the forward dynamics: stage mode (a and f out) and impulse mode (dv and lambda out),
without and with the Euler step; stage_da_mjtjinv is what a caller needed for the same answer before that call existed.  The policy_* rows are the
feedback policy alone (idocp_rbd_feedback_torques_batch_device) with one gain block and reference shared by all samples and with one per sample;
fd_step_closed_loop is one step of idocp_rbd_rollout_policy_device (policy launch + forward launch with the Euler step, per-sample gains), to be
read against fd_stage_a_f_step.  The score_* rows are idocp_rbd_score_rollout_device on a window of 1 and of 16 steps (terminal slice included): every
weight, the joint limits and the linearized cone (score_sK_all_linearized) or the FrictionCone (score_sK_all_cone), and the cost alone
(score_sK_cost_only); score_sK_copy is a device-to-device copy of exactly the bytes the call reads, timed in the same run, and each score row carries
its ratio to that copy.  The sample_* rows are the sampling calls on 16 steps of the 12 torques: sample_perturb (idocp_rbd_perturb_torques_device writes
u_samples [16][n][12]), sample_mean (idocp_rbd_weighted_mean_device reads an array of that shape) -- both read against sample_copy, a device-to-device
copy of that array -- and sample_weights (idocp_rbd_importance_weights_device: cost and violation in, weights out) against sample_weights_copy, a copy of
those three arrays.  The fdd_* rows are the forward-dynamics derivatives (fdd_rows has their description).  The kin_* rows are idocp_rbd_contact_kinematics_batch_device: kin_points (q in, points out) and kin_all (q and v in, all four
outputs), each against kin_*_copy, a device-to-device copy of the bytes the call reads and writes.  rollout is idocp_rbd_rollout_device over
ROLLOUT_STEPS open-loop steps with every contact active and no touchdown impulse, rollout_footholds the same schedule through
idocp_rbd_rollout_footholds_device (one latch launch more per step); both carry ms_per_step.  The lqr_* rows are idocp_rbd_lqr_backward_device over
16 steps (lqr_rows has their description); run with fdd_linearize_s16 they also carry their ratio to the linearisation that feeds them.  The grad_*,
ilqr_accept and ilqr_iterate rows are the cost gradients, the acceptance step and one whole iLQR iteration (ilqr_rows has their description).
The penalty_* rows are the gn_* rows under constraints with the penalty calls (gn_rows with penalty=True has their setting).
The al_* rows are the augmented-Lagrangian calls in the same setting, next to them (al_rows has their description).
The gn_* rows are the cost linearisation with residual rows, the backward pass with G^T G and one full-cost iteration (gn_rows has their
description).

    python profiles/rbd_throughput.py [--n 122880] [--launches 20] [--warmup 5] [--rows name,name,...]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idocp_amd import capi  # noqa: E402
from idocp_amd.workloads import ANYMAL_Q_STANDING, anymal_model  # noqa: E402

SELECTIONS = (("stage_all", capi.RBD_STAGE, capi.RbdIO.OUTPUTS),
              ("stage_no_mjtjinv", capi.RBD_STAGE, capi.RbdIO.OUTPUTS[:-1]),
              ("stage_da_mjtjinv", capi.RBD_STAGE, ("tau", "dtau_da", "C", "dCda", "MJtJinv")),
              ("stage_tau_C", capi.RBD_STAGE, ("tau", "C")),
              ("impulse_all", capi.RBD_IMPULSE, capi.RbdIO.OUTPUTS))

FD_SELECTIONS = (("fd_stage_a_f", capi.RBD_STAGE, ("a", "f")),
                 ("fd_stage_a_f_step", capi.RBD_STAGE, ("a", "f", "q_next", "v_next")),
                 ("fd_impulse_dv_lambda", capi.RBD_IMPULSE, ("a", "f")),
                 ("fd_impulse_dv_lambda_step", capi.RBD_IMPULSE, ("a", "f", "q_next", "v_next")))

POLICY_ROWS = ("policy_shared", "policy_per_sample", "fd_step_closed_loop")
SCORE_STEPS = (1, 16)
SCORE_KINDS = ("copy", "all_linearized", "all_cone", "cost_only")
SCORE_ROWS = tuple("score_s%d_%s" % (s, k) for s in SCORE_STEPS for k in SCORE_KINDS)
SAMPLE_STEPS = 16
SAMPLE_ROWS = ("sample_copy", "sample_perturb", "sample_mean", "sample_weights_copy", "sample_weights")
KIN_ROWS = ("kin_points_copy", "kin_points", "kin_all_copy", "kin_all", "rollout", "rollout_footholds")
ROLLOUT_STEPS = 4


def kin_rows(wanted, lib, rt, h, stream, m, n, host, measure, res):
    """the kin_* rows and the two rollouts"""
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    nv, nq, nu, nf, steps = m.nv, m.nq, m.nu, 3 * m.ncontacts, ROLLOUT_STEPS
    sizes = {"q": nq, "v": nv, "points": nf, "rotation": 3 * nf, "velocity": nf, "jacobian": nf * nv}
    dev = {}
    for key, size in list(sizes.items()) + [("copy", sum(sizes.values())), ("q_traj", (steps + 1) * nq), ("v_traj", (steps + 1) * nv), ("u", steps * nu),
                                             ("pts", steps * nf), ("a_traj", steps * nv), ("f_traj", steps * nf)]:
        dev[key] = C.c_void_p()
        capi.check(lib.idocp_device_alloc(C.byref(dev[key]), 8 * n * size), "alloc")
    for key, x in (("q", host["q"]), ("v", host["v"]), ("q_traj", host["q"]), ("v_traj", 0.1 * host["v"])):
        x = np.ascontiguousarray(x)
        capi.check(lib.idocp_device_upload(dev[key], x.ctypes.data, x.nbytes), "upload")
    u = np.zeros((steps, n, nu))
    capi.check(lib.idocp_device_upload(dev["u"], u.ctypes.data, u.nbytes), "upload")
    feet = np.zeros((n, nf))
    kin = capi.RbdKinIO()
    kin.q, kin.points = dev["q"], dev["points"]
    capi.check(lib.idocp_rbd_contact_kinematics_batch_device(h, n, C.byref(kin)), "kinematics")      # every plant stands on its own feet
    capi.check(lib.idocp_rbd_synchronize(h), "synchronize")
    capi.check(lib.idocp_device_download(feet.ctypes.data, dev["points"], feet.nbytes), "download")
    pts = np.ascontiguousarray(np.repeat(feet[None], steps, axis=0))
    capi.check(lib.idocp_device_upload(dev["pts"], pts.ctypes.data, pts.nbytes), "upload")
    selections = {"kin_points": ("q", "points"), "kin_all": ("q", "v", "points", "rotation", "velocity", "jacobian")}

    def copy(keys):
        at = 0
        for key in keys:      # the very bytes the call reads and writes, array by array
            assert rt.hipMemcpyAsync(C.c_void_p(dev["copy"].value + at), dev[key], 8 * n * sizes[key], 3, stream) == 0
            at += 8 * n * sizes[key]

    for name, keys in selections.items():
        io = capi.RbdKinIO()
        for key in keys:
            setattr(io, key, dev[key])
        nbytes = 8 * n * sum(sizes[key] for key in keys)
        for row, launch in ((name + "_copy", lambda: copy(keys)),
                            (name, lambda: capi.check(lib.idocp_rbd_contact_kinematics_batch_device(h, n, C.byref(io)), name))):
            if wanted and row not in wanted:
                continue
            measure(row, launch)
            res[row]["bytes"] = nbytes
            res[row]["GB_per_s"] = round(nbytes / res[row]["ms_median"] / 1e6, 1)
        if name in res and name + "_copy" in res:
            res[name]["ratio_to_copy"] = round(res[name]["ms_median"] / res[name + "_copy"]["ms_median"], 3)
    active = (C.c_int * (4 * steps))(*([1] * (4 * steps)))
    fio = capi.RbdFootholdRollout()
    fio.u, fio.contact_points, fio.q_traj, fio.v_traj, fio.a_traj, fio.f_traj = dev["u"], dev["pts"], dev["q_traj"], dev["v_traj"], dev["a_traj"], dev["f_traj"]
    launches = {
        "rollout": lambda: capi.check(lib.idocp_rbd_rollout_device(h, n, steps, active, 0.05, 0.01, dev["u"], dev["pts"], dev["q_traj"], dev["v_traj"],
                                                                   dev["a_traj"], dev["f_traj"], 0), "rollout"),
        "rollout_footholds": lambda: capi.check(lib.idocp_rbd_rollout_footholds_device(h, n, steps, active, 0.05, 0.01, C.byref(fio), 0, 0), "rollout_footholds"),
    }
    for row, launch in launches.items():
        if wanted and row not in wanted:
            continue
        measure(row, launch)
        res[row]["steps"] = steps
        res[row]["ms_per_step"] = round(res[row]["ms_median"] / steps, 4)
    if "rollout" in res and "rollout_footholds" in res:
        res["rollout_footholds"]["ratio_to_rollout"] = round(res["rollout_footholds"]["ms_median"] / res["rollout"]["ms_median"], 3)
        res["rollout_footholds"]["latch_ms_per_step"] = round((res["rollout_footholds"]["ms_median"] - res["rollout"]["ms_median"]) / steps, 4)
    out = np.zeros((n, nf * nv))
    capi.check(lib.idocp_device_download(out.ctypes.data, dev["jacobian"], out.nbytes), "download")
    if "kin_all" in res:
        res["kin_finite"] = bool(np.isfinite(out).all())
    for d in dev.values():
        lib.idocp_device_free(d)


def sample_rows(wanted, lib, rt, h, stream, m, n, measure, res):
    """the sample_* rows; the weights come from random scores, so that the mean multiplies rather than skips"""
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    nu, steps = m.nu, SAMPLE_STEPS
    rng = np.random.default_rng(1)
    host = {"nominal": rng.uniform(-20, 20, (steps, nu)), "sigma": np.full(nu, 2.0), "cost": rng.uniform(1, 5, n), "violation": rng.uniform(0, 1, n)}
    dev = {}
    for key, x in host.items():
        dev[key] = C.c_void_p()
        capi.check(lib.idocp_device_alloc(C.byref(dev[key]), x.nbytes), "alloc")
        capi.check(lib.idocp_device_upload(dev[key], x.ctypes.data, x.nbytes), "upload")
    big = 8 * steps * n * nu
    for key, size in (("samples", big), ("copy", big), ("weights", 8 * n), ("small_copy", 3 * 8 * n), ("stats", 8 * capi.RBD_WEIGHT_STATS), ("mean", 8 * steps * nu)):
        dev[key] = C.c_void_p()
        capi.check(lib.idocp_device_alloc(C.byref(dev[key]), size), "alloc")

    def small_copy():
        for at, key in enumerate(("cost", "violation", "weights")):
            assert rt.hipMemcpyAsync(C.c_void_p(dev["small_copy"].value + at * 8 * n), dev[key], 8 * n, 3, stream) == 0

    launches = {
        "sample_copy": lambda: rt.hipMemcpyAsync(dev["copy"], dev["samples"], big, 3, stream),
        "sample_perturb": lambda: capi.check(lib.idocp_rbd_perturb_torques_device(h, n, 0, steps, dev["nominal"], dev["sigma"], None, None, 7, 1, dev["samples"]), "perturb"),
        "sample_weights_copy": small_copy,
        "sample_weights": lambda: capi.check(lib.idocp_rbd_importance_weights_device(h, n, dev["cost"], dev["violation"], 10.0, 1.0, dev["weights"], dev["stats"]), "weights"),
        "sample_mean": lambda: capi.check(lib.idocp_rbd_weighted_mean_device(h, n, steps, nu, dev["weights"], dev["samples"], dev["mean"]), "mean"),
    }
    launches["sample_perturb"]()                           # whatever rows are asked for, the mean has samples and weights to read
    launches["sample_weights"]()
    for name in ("sample_copy", "sample_perturb", "sample_weights_copy", "sample_weights", "sample_mean"):
        if wanted and name not in wanted:
            continue
        measure(name, launches[name])
        nbytes = 3 * 8 * n if "weights" in name else big
        res[name]["bytes"] = nbytes
        res[name]["GB_per_s"] = round(nbytes / res[name]["ms_median"] / 1e6, 1)
    for name, base in (("sample_perturb", "sample_copy"), ("sample_mean", "sample_copy"), ("sample_weights", "sample_weights_copy")):
        if name in res and base in res:
            res[name]["ratio_to_copy"] = round(res[name]["ms_median"] / res[base]["ms_median"], 3)
    out, stats = np.zeros((steps, nu)), np.zeros(capi.RBD_WEIGHT_STATS)
    capi.check(lib.idocp_device_download(out.ctypes.data, dev["mean"], out.nbytes), "download")
    capi.check(lib.idocp_device_download(stats.ctypes.data, dev["stats"], stats.nbytes), "download")
    if "sample_mean" in res:
        res["sample_mean_finite"] = bool(np.isfinite(out).all())
        res["sample_mean_max_shift"] = float(np.abs(out - host["nominal"]).max())      # (the mean of n perturbations stays near the nominal)
    res["sample_stats"] = [float(x) for x in stats]
    for d in dev.values():
        lib.idocp_device_free(d)


def score_rows(args, wanted, lib, rt, h, stream, m, n, host, measure, res):
    """the score_* rows: the slices of one step repeated over the window (what is read is what matters, not what it holds)"""
    from idocp_amd.workloads import anymal_problem
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    nv, nq, nu, nf = m.nv, m.nq, m.nu, 3 * m.ncontacts
    cost, cons = anymal_problem(m, trotting_ref=False)
    cost.set("u_weight", np.full(nu, 0.01))
    objectives = {}
    for kind in SCORE_KINDS[1:]:
        k = capi.Constraints.from_buffer_copy(cons)
        k.linearized_friction_cone, k.friction_cone = int(kind == "all_linearized"), int(kind == "all_cone")
        if kind != "cost_only":
            k.joint_position_limits = k.joint_velocity_limits = k.joint_torque_limits = 1
        objectives[kind] = C.c_void_p()
        capi.check(lib.idocp_rbd_objective_create(h, C.byref(cost), C.byref(k) if kind != "cost_only" else None, 0.0, 0.01, max(SCORE_STEPS), C.byref(objectives[kind])),
                   "idocp_rbd_objective_create")
    for steps in SCORE_STEPS:
        names = ["score_s%d_%s" % (steps, kind) for kind in SCORE_KINDS]
        if wanted and not set(names) & set(wanted):
            continue
        arrays = {"q_traj": (host["q"], steps + 1), "v_traj": (host["v"], steps + 1), "u_traj": (host["u"], steps), "a_traj": (host["a"], steps), "f_traj": (host["f"], steps)}
        dev, nbytes = {}, 0
        for key, (x, slices) in arrays.items():
            x = np.ascontiguousarray(x)
            dev[key] = C.c_void_p()
            capi.check(lib.idocp_device_alloc(C.byref(dev[key]), x.nbytes * slices), "alloc")
            for s in range(slices):
                capi.check(lib.idocp_device_upload(C.c_void_p(dev[key].value + s * x.nbytes), x.ctypes.data, x.nbytes), "upload")
            nbytes += x.nbytes * slices
        for key, size in (("cost", 8 * n), ("violation", 8 * n), ("copy", nbytes)):
            dev[key] = C.c_void_p()
            capi.check(lib.idocp_device_alloc(C.byref(dev[key]), size), "alloc")
        active = (C.c_int * (4 * steps))(*([1] * (4 * steps)))
        io = capi.RbdScoreIO()
        for key in capi.RbdScoreIO.INPUTS + ("cost", "violation"):
            setattr(io, key, dev[key])

        def copy():
            at = 0
            for key, (x, slices) in arrays.items():      # the very bytes the call reads, array by array
                size = np.ascontiguousarray(x).nbytes * slices
                assert rt.hipMemcpyAsync(C.c_void_p(dev["copy"].value + at), dev[key], size, 3, stream) == 0
                at += size

        for name, kind in zip(names, SCORE_KINDS):
            if wanted and name not in wanted:
                continue
            if kind == "copy":
                measure(name, copy)
            else:
                measure(name, lambda: capi.check(lib.idocp_rbd_score_rollout_device(h, objectives[kind], n, 0, steps, active, 1, 0, C.byref(io)), name))
            res[name]["input_bytes"] = nbytes
            res[name]["GB_per_s"] = round(nbytes / res[name]["ms_median"] / 1e6, 1)
        for name in names[1:]:
            if name in res and names[0] in res:
                res[name]["ratio_to_copy"] = round(res[name]["ms_median"] / res[names[0]]["ms_median"], 3)
        out = np.zeros((2, n))
        capi.check(lib.idocp_device_download(out[0].ctypes.data, dev["cost"], 8 * n), "download")
        capi.check(lib.idocp_device_download(out[1].ctypes.data, dev["violation"], 8 * n), "download")
        res["score_s%d_finite" % steps] = bool(np.isfinite(out).all())
        for d in dev.values():
            lib.idocp_device_free(d)
    for o in objectives.values():
        lib.idocp_rbd_objective_destroy(o)


FDD_ROWS = ("fdd_fd_stage_a_f", "fdd_batch_scratch", "fdd_all", "fdd_A_B", "fdd_all_but_A", "fdd_fd_impulse", "fdd_batch_impulse_scratch", "fdd_impulse_all",
            "fdd_linearize_s16")
FDD_STEPS = 16


def fdd_rows(wanted, lib, h, m, n, dev, active, measure, res):
    """the fdd_* rows: idocp_rbd_forward_dynamics_derivatives_batch_device with every output and with A, B alone, beside the two launches it is
    made of in the SAME run -- the forward call (a, f out) and the inverse call with the five scratch outputs -- and a 16-step
    idocp_rbd_linearize_rollout_device on the same slices repeated (no touchdown: the status is constant).  fdd_ratio_*: the whole call over
    the sum of its two existing launches; what is above 1 is the new kernel.  Three rows take the new kernel's serial sections apart: fdd_all_but_A
    skips the lane-0 retraction Jacobians (they run for A alone); the IMPULSE call (fdd_impulse_all beside fdd_fd_impulse and
    fdd_batch_impulse_scratch) has neither them nor the 36-lane correction sweep, only the product loop and the stores."""
    nv, nq, nu, nf, nx = m.nv, m.nq, m.nu, 3 * m.ncontacts, 2 * m.nv
    own = {}

    def room(name, doubles):
        own[name] = C.c_void_p()
        capi.check(lib.idocp_device_alloc(C.byref(own[name]), 8 * doubles), "alloc")
        return own[name]

    def want(name):
        return not wanted or name in wanted

    fd = capi.RbdFdIO()
    for k in capi.RbdFdIO.INPUTS:
        setattr(fd, k, dev[k])
    fd.a, fd.f = dev["fd_a"], dev["fd_f"]
    if want("fdd_fd_stage_a_f"):
        measure("fdd_fd_stage_a_f", lambda: capi.check(lib.idocp_rbd_forward_dynamics_batch_device(h, capi.RBD_STAGE, n, active, 0.05, 0.01, C.byref(fd)), "fd"))
    if want("fdd_batch_scratch"):
        io = capi.RbdIO()
        for k in capi.RbdIO.INPUTS + ("dtau_dq", "dtau_dv", "dCdq", "dCdv", "MJtJinv"):
            setattr(io, k, dev[k])
        measure("fdd_batch_scratch", lambda: capi.check(lib.idocp_rbd_contact_dynamics_batch_device(h, capi.RBD_STAGE, n, active, 0.05, C.byref(io)), "batch"))
    sizes = {"a": nv, "f": nf, "da_dq": nv * nv, "da_dv": nv * nv, "da_du": nv * nu, "df_dq": nf * nv, "df_dv": nf * nv, "df_du": nf * nu, "A": nx * nx, "B": nx * nu}
    if want("fdd_fd_impulse"):
        fi = capi.RbdFdIO()
        fi.q, fi.v, fi.a, fi.f = dev["q"], dev["v"], dev["fd_a"], dev["fd_f"]
        measure("fdd_fd_impulse", lambda: capi.check(lib.idocp_rbd_forward_dynamics_batch_device(h, capi.RBD_IMPULSE, n, active, 0.05, 0.01, C.byref(fi)), "fd"))
    if want("fdd_batch_impulse_scratch"):
        bi = capi.RbdIO()
        for k in ("q", "v", "a", "f", "dtau_dq", "dtau_dv", "dCdq", "dCdv", "MJtJinv"):
            setattr(bi, k, dev[k])
        measure("fdd_batch_impulse_scratch", lambda: capi.check(lib.idocp_rbd_contact_dynamics_batch_device(h, capi.RBD_IMPULSE, n, active, 0.05, C.byref(bi)), "batch"))
    no_torque = tuple(k for k in capi.RbdFddIO.OUTPUTS if k not in ("da_du", "df_du", "B"))
    for name, mode, outputs in (("fdd_all", capi.RBD_STAGE, capi.RbdFddIO.OUTPUTS), ("fdd_A_B", capi.RBD_STAGE, ("A", "B")),
                                ("fdd_all_but_A", capi.RBD_STAGE, tuple(k for k in capi.RbdFddIO.OUTPUTS if k != "A")),
                                ("fdd_impulse_all", capi.RBD_IMPULSE, no_torque)):
        if not want(name):
            continue
        io = capi.RbdFddIO()
        for k in ("q", "v") if mode == capi.RBD_IMPULSE else capi.RbdFddIO.INPUTS:
            setattr(io, k, dev[k])
        for k in outputs:
            setattr(io, k, own[k] if k in own else room(k, sizes[k] * n))
        measure(name, lambda io=io, mode=mode: capi.check(lib.idocp_rbd_forward_dynamics_derivatives_batch_device(h, mode, n, active, 0.05, 0.01, C.byref(io)), name))
    if want("fdd_linearize_s16"):
        S = FDD_STEPS
        slices = {"q": (S + 1, nq), "v": (S + 1, nv), "u": (S, nu), "contact_points": (S, nf)}
        traj = {}
        for k, (count, width) in slices.items():
            traj[k] = room("traj_" + k, count * n * width)
            for i in range(count):
                capi.check(lib.idocp_device_copy(C.c_void_p(traj[k].value + 8 * i * n * width), dev[k], 8 * n * width), "copy")
        At, Bt = room("A_traj", S * n * nx * nx), room("B_traj", S * n * nx * nu)
        act = (C.c_int * (4 * S))(*([1] * (4 * S)))
        measure("fdd_linearize_s16", lambda: capi.check(lib.idocp_rbd_linearize_rollout_device(h, n, S, act, 0.05, 0.01, traj["u"], traj["contact_points"], traj["q"],
                                                                                                 traj["v"], At, Bt, 1), "linearize"))
    parts = [res.get("fdd_fd_stage_a_f"), res.get("fdd_batch_scratch")]
    if all(parts):
        both = sum(x["ms_median"] for x in parts)
        for name in ("fdd_all", "fdd_A_B"):
            if name in res:
                res["fdd_ratio_" + name[4:]] = round(res[name]["ms_median"] / both, 3)
        if "fdd_all_but_A" in res:
            res["fdd_ratio_all_but_A"] = round(res["fdd_all_but_A"]["ms_median"] / both, 3)
        if "fdd_linearize_s16" in res:
            res["fdd_ratio_linearize_per_step"] = round(res["fdd_linearize_s16"]["ms_median"] / FDD_STEPS / both, 3)
    parts = [res.get("fdd_fd_impulse"), res.get("fdd_batch_impulse_scratch")]
    if all(parts) and "fdd_impulse_all" in res:
        res["fdd_ratio_impulse_all"] = round(res["fdd_impulse_all"]["ms_median"] / sum(x["ms_median"] for x in parts), 3)
    for d in own.values():
        lib.idocp_device_free(d)


LQR_ROWS = ("lqr_gains_copy", "lqr_gains", "lqr_gains_ilqr_copy", "lqr_gains_ilqr")
LQR_STEPS = 16
LQR_FLOP_PER_STEP = 2.7e5      # per sample and step on the quadruped: P A, A^T (P A), B^T (P A), Qux^T K and the small rest


def lqr_rows(wanted, lib, rt, h, stream, m, n, measure, res):
    """the lqr_* rows: idocp_rbd_lqr_backward_device over 16 steps of A = I + 0.1 N(0, 1), B = 0.1 N(0, 1) (one block of 1 024 samples repeated
    over the batch and the steps) -- lqr_gains writes K_traj and status alone, lqr_gains_ilqr takes the gradients and writes every output --, each
    against a device-to-device copy of the bytes it reads and writes, and with the FP64 rate it reaches on the 2.7e5 FLOP per sample and step."""
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    nx, nu, S, block = 2 * m.nv, m.nu, LQR_STEPS, min(n, 1024)
    rng = np.random.default_rng(5)
    sizes = {"A_traj": S * n * nx * nx, "B_traj": S * n * nx * nu, "lx_traj": (S + 1) * n * nx, "lu_traj": S * n * nu, "K_traj": S * n * nx * nu,
             "k_traj": S * n * nu, "P0": n * nx * nx, "p0": n * nx, "expected": 2 * n, "status": (n + 1) // 2, "x_weight": nx, "u_weight": nu, "xf_weight": nx}
    dev = {}
    for key, size in list(sizes.items()) + [("copy", sum(sizes.values()))]:
        dev[key] = C.c_void_p()
        capi.check(lib.idocp_device_alloc(C.byref(dev[key]), 8 * size), "alloc")
    for key, x in (("x_weight", rng.uniform(0.5, 2, nx)), ("u_weight", rng.uniform(0.5, 2, nu)), ("xf_weight", rng.uniform(0.5, 2, nx))):
        capi.check(lib.idocp_device_upload(dev[key], x.ctypes.data, x.nbytes), "upload")
    for key, width, x in (("A_traj", nx * nx, np.eye(nx) + 0.1 * rng.normal(size=(block, nx, nx))), ("B_traj", nx * nu, 0.1 * rng.normal(size=(block, nu, nx))),
                          ("lx_traj", nx, rng.normal(size=(block, nx))), ("lu_traj", nu, rng.normal(size=(block, nu)))):
        x = np.ascontiguousarray(x)
        capi.check(lib.idocp_device_upload(dev[key], x.ctypes.data, x.nbytes), "upload")
        at, total = block * width, sizes[key]
        while at < total:      # (doubling: the filled front copied behind itself)
            count = min(at, total - at)
            capi.check(lib.idocp_device_copy(C.c_void_p(dev[key].value + 8 * at), dev[key], 8 * count), "copy")
            at += count
    selections = {"lqr_gains": ("A_traj", "B_traj", "K_traj", "status"), "lqr_gains_ilqr": tuple(k for k in sizes if not k.endswith("weight"))}
    for name, keys in selections.items():
        io = capi.RbdLqrIO()
        for key in keys + ("x_weight", "u_weight", "xf_weight"):
            setattr(io, key, dev[key])
        io.regularization = 0.1
        nbytes = 8 * sum(sizes[key] for key in keys)

        def copy(keys=keys):
            at = 0
            for key in keys:      # the very bytes the call reads and writes, array by array
                assert rt.hipMemcpyAsync(C.c_void_p(dev["copy"].value + at), dev[key], 8 * sizes[key], 3, stream) == 0
                at += 8 * sizes[key]

        for row, launch in ((name + "_copy", copy), (name, lambda io=io: capi.check(lib.idocp_rbd_lqr_backward_device(h, n, S, C.byref(io)), "lqr"))):
            if wanted and row not in wanted:
                continue
            measure(row, launch)
            res[row].update({"steps": S, "bytes": nbytes, "GB_per_s": round(nbytes / res[row]["ms_median"] / 1e6, 1)})
        if name in res:
            res[name]["ms_per_step"] = round(res[name]["ms_median"] / S, 4)
            res[name]["fp64_TFLOP_per_s"] = round(LQR_FLOP_PER_STEP * n * S / res[name]["ms_median"] / 1e9, 2)
            if name + "_copy" in res:
                res[name]["ratio_to_copy"] = round(res[name]["ms_median"] / res[name + "_copy"]["ms_median"], 3)
            if "fdd_linearize_s16" in res:      # the call that produces its input, same shapes, same run
                res[name]["ratio_to_linearize"] = round(res[name]["ms_median"] / res["fdd_linearize_s16"]["ms_median"], 3)
    status = np.zeros((n + 1) // 2)
    capi.check(lib.idocp_rbd_synchronize(h), "synchronize")
    capi.check(lib.idocp_device_download(status.ctypes.data, dev["status"], status.nbytes), "download")
    res["lqr_all_solved"] = bool((status.view(np.int32)[:n] == -1).all())
    for d in dev.values():
        lib.idocp_device_free(d)

ILQR_ROWS = ("grad_s16_copy", "grad_s16", "ilqr_accept_copy", "ilqr_accept", "ilqr_iterate")
ILQR_STEPS = 16


def ilqr_rows(wanted, lib, rt, h, stream, m, n, measure, res):
    """the grad_*, ilqr_accept and ilqr_iterate rows on 16 steps of ANYmal standing on four feet: grad_s16 is idocp_rbd_objective_gradients_device
    (q, v, u in, lx with the terminal slice and lu out), ilqr_accept is idocp_rbd_ilqr_accept_device with EVERY sample accepted (done is cleared in
    front of each launch, so q, v, u, a, f are copied in full), each against a device-to-device copy of the bytes the call moves; ilqr_iterate is one
    idocp_rbd_ilqr_iterate_device with two trial rounds about a rollout of zero torques, to be read against fdd_linearize_s16 and lqr_gains_ilqr."""
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rt.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    nq, nv, nu, nf, S = m.nq, m.nv, m.nu, 3 * m.ncontacts, ILQR_STEPS
    rng = np.random.default_rng(11)
    cost = capi.Cost()
    cost.set("q_ref", ANYMAL_Q_STANDING).set("q_weight", np.full(nv, 10.0)).set("v_weight", np.full(nv, 1.0)).set("u_weight", np.full(nu, 1e-3))
    cost.set("qf_weight", np.full(nv, 10.0)).set("vf_weight", np.full(nv, 1.0)).set("a_weight", np.zeros(nv))
    for c in range(4):
        for x in range(3):
            cost.f_weight[c][x] = 0.0
    o = C.c_void_p()
    capi.check(lib.idocp_rbd_objective_create(h, C.byref(cost), None, 0.0, 0.01, S, C.byref(o)), "objective")
    want_iterate = not wanted or "ilqr_iterate" in wanted
    sizes = {"q": (S + 1) * n * nq, "v": (S + 1) * n * nv, "u": S * n * nu, "a": S * n * nv, "f": S * n * nf, "lx": (S + 1) * n * 2 * nv, "lu": S * n * nu,
             "tq": (S + 1) * n * nq, "tv": (S + 1) * n * nv, "tu": S * n * nu, "ta": S * n * nv, "tf": S * n * nf, "pts": S * n * nf,
             "cost": n, "viol": n, "tcost": n, "tviol": n, "expected": 2 * n, "alpha": n, "alpha_accepted": n, "done": (n + 1) // 2, "status": (n + 1) // 2}
    sizes["copy"] = 2 * sum(sizes[k] for k in ("q", "v", "u", "a", "f"))
    if want_iterate:
        sizes["work"] = lib.idocp_rbd_ilqr_workspace_bytes(h, n, S) // 8
    dev = {}
    for key, size in sizes.items():
        dev[key] = C.c_void_p()
        capi.check(lib.idocp_device_alloc(C.byref(dev[key]), 8 * size), "alloc")
        assert rt.hipMemsetAsync(dev[key], 0, 8 * size, stream) == 0
    q0 = np.tile(ANYMAL_Q_STANDING, (n, 1))
    q0[:, 7:] += rng.uniform(-0.02, 0.02, (n, nv - 6))
    feet = np.zeros(nf)
    capi.check(lib.idocp_model_contact_positions(C.byref(m), np.ascontiguousarray(ANYMAL_Q_STANDING).ctypes.data, feet.ctypes.data), "feet")
    pts = np.ascontiguousarray(np.broadcast_to(feet, (S, n, nf)))
    ones = np.ones(n)
    for key, x in (("q", q0), ("tq", q0), ("pts", pts), ("alpha", ones)):
        capi.check(lib.idocp_device_upload(dev[key], x.ctypes.data, x.nbytes), "upload")
    act = (C.c_int * (4 * S))(*([1] * (4 * S)))
    ts, dt = 0.05, 0.01
    # a real rollout (zero torques) in the current arrays and in the trial arrays, and its score
    for pre in ("", "t"):
        capi.check(lib.idocp_rbd_rollout_device(h, n, S, act, ts, dt, dev[pre + "u"], dev["pts"], dev[pre + "q"], dev[pre + "v"], dev[pre + "a"], dev[pre + "f"], 0), "rollout")
    sc = capi.RbdScoreIO()
    sc.q_traj, sc.v_traj, sc.u_traj, sc.a_traj, sc.f_traj, sc.cost, sc.violation = dev["q"], dev["v"], dev["u"], dev["a"], dev["f"], dev["cost"], dev["viol"]
    capi.check(lib.idocp_rbd_score_rollout_device(h, o, n, 0, S, act, 1, 0, C.byref(sc)), "score")
    assert rt.hipMemcpyAsync(dev["tcost"], dev["cost"], 8 * n, 3, stream) == 0

    def copier(keys):
        def copy():
            at = 0
            for key in keys:
                assert rt.hipMemcpyAsync(C.c_void_p(dev["copy"].value + at), dev[key], 8 * sizes[key], 3, stream) == 0
                at += 8 * sizes[key]
        return copy

    g = capi.RbdGradientIO()
    g.q_traj, g.v_traj, g.u_traj, g.lx_traj, g.lu_traj = dev["q"], dev["v"], dev["u"], dev["lx"], dev["lu"]
    grad_keys = ("q", "v", "u", "lx", "lu")
    acc = capi.RbdIlqrAcceptIO()
    for field, key in (("q_traj", "q"), ("v_traj", "v"), ("u_traj", "u"), ("a_traj", "a"), ("f_traj", "f"), ("cost", "cost"), ("violation", "viol"),
                       ("trial_q", "tq"), ("trial_v", "tv"), ("trial_u", "tu"), ("trial_a", "ta"), ("trial_f", "tf"), ("trial_cost", "tcost"),
                       ("trial_violation", "tviol"), ("expected", "expected"), ("alpha", "alpha"), ("done", "done"), ("alpha_accepted", "alpha_accepted")):
        setattr(acc, field, dev[key])
    acc.penalty, acc.armijo, acc.shrink, acc.alpha_min = 0.0, 1e-4, 0.5, 1e-3
    acc_keys = ("q", "v", "u", "a", "f", "tq", "tv", "tu", "ta", "tf")      # (read the trial, write the current: a copy of the same bytes reads and writes both)

    def accept():
        assert rt.hipMemsetAsync(dev["done"], 0, 8 * sizes["done"], stream) == 0      # every sample is accepted again: merit_trial == merit, expected = 0
        capi.check(lib.idocp_rbd_ilqr_accept_device(h, n, S, C.byref(acc)), "accept")

    plan = (("grad_s16_copy", copier(grad_keys), grad_keys), ("grad_s16", lambda: capi.check(lib.idocp_rbd_objective_gradients_device(h, o, n, 0, S, 1, C.byref(g)), "gradients"), grad_keys),
            ("ilqr_accept_copy", copier(("tq", "tv", "tu", "ta", "tf")), acc_keys), ("ilqr_accept", accept, acc_keys))
    for row, launch, keys in plan:
        if wanted and row not in wanted:
            continue
        measure(row, launch)
        nbytes = 8 * sum(sizes[k] for k in keys)
        res[row].update({"steps": S, "bytes": nbytes, "GB_per_s": round(nbytes / res[row]["ms_median"] / 1e6, 1)})
    for name in ("grad_s16", "ilqr_accept"):
        if name in res and name + "_copy" in res:
            res[name]["ratio_to_copy"] = round(res[name]["ms_median"] / res[name + "_copy"]["ms_median"], 3)
    if want_iterate:
        io = capi.RbdIlqrIO()
        for field, key in (("q_traj", "q"), ("v_traj", "v"), ("u_traj", "u"), ("a_traj", "a"), ("f_traj", "f"), ("cost", "cost"), ("violation", "viol"),
                           ("alpha_accepted", "alpha_accepted"), ("lqr_status", "status"), ("expected", "expected"), ("workspace", "work")):
            setattr(io, field, dev[key])
        io.regularization, io.armijo, io.shrink, io.alpha_min, io.penalty, io.trials = 1e-6, 1e-4, 0.5, 1e-3, 0.0, 2
        measure("ilqr_iterate", lambda: capi.check(lib.idocp_rbd_ilqr_iterate_device(h, o, n, S, act, ts, dt, dev["pts"], C.byref(io), 0), "iterate"))
        res["ilqr_iterate"].update({"steps": S, "trials": 2})
        status = np.zeros((n + 1) // 2)
        capi.check(lib.idocp_rbd_synchronize(h), "synchronize")
        capi.check(lib.idocp_device_download(status.ctypes.data, dev["status"], status.nbytes), "download")
        res["ilqr_all_solved"] = bool((status.view(np.int32)[:n] == -1).all())
        for part in ("fdd_linearize_s16", "lqr_gains_ilqr"):
            if part in res:
                res["ilqr_iterate"]["share_" + part] = round(res[part]["ms_median"] / res["ilqr_iterate"]["ms_median"], 3)
    capi.check(lib.idocp_rbd_synchronize(h), "synchronize")
    lib.idocp_rbd_objective_destroy(o)
    for d in dev.values():
        lib.idocp_device_free(d)


GN_ROWS = ("gn_linearize_s16", "gn_residual_pass_copy", "gn_lqr_backward", "gn_iterate")
PENALTY_ROWS = ("penalty_linearize_s16", "penalty_residual_pass_copy", "penalty_lqr_backward", "penalty_iterate")
AL_ROWS = ("al_score", "al_score_copy", "al_update", "al_update_copy", "al_linearize_s16", "al_iterate")
GN_STEPS = 16
GN_RESIDUAL_DOUBLES = 1470 + 48 + 1536 + 32 + 48      # per quadruped sample and launch of rbd_residual_kernel: a, f and the six blocks in; lx, lu in; G, rho, lx, lu out
GN_PASS = ((256 << 20) // 8) // (1470 + 8) // 2 * 2      # samples per pass of the cost linearisation (ResidualPlan of rbd_capi.hip)


def gn_rows(wanted, lib, rt, h, stream, m, n, measure, res, penalty=False):
    """the gn_* rows on 16 steps of ANYmal standing on four feet under the ANYmal workload's own cost (a_weight and f_weight set, u_weight zero),
    about a rollout of zero torques: gn_linearize_s16 is idocp_rbd_linearize_rollout_cost_device with every output (read it against
    fdd_linearize_s16); gn_residual_pass_copy is a device-to-device copy of the bytes ONE launch of rbd_residual_kernel touches (a pass of GN_PASS
    samples; the kernel's own time comes from a kernel trace of the gn_linearize_s16 row); gn_lqr_backward is idocp_rbd_lqr_backward_gn_device on what
    the linearisation wrote, every output (read it against lqr_gains_ilqr); gn_iterate is one idocp_rbd_ilqr_iterate_gn_device with two trial rounds
    (read it against ilqr_iterate).
    penalty: the penalty_* rows instead -- the same setting under constraints (every joint limit of the model, an acceleration box of +- 5, the
    LinearizedFrictionCone with mu = 0.7) and mu = 10: idocp_rbd_linearize_rollout_penalty_device with all seven outputs (read it against
    gn_linearize_s16), the copy of the bytes one launch of the penalty form touches (G and rho twice as wide, D more), idocp_rbd_lqr_backward_gn_diag_device
    at R + Rc = 64 rows (against gn_lqr_backward at 32) and idocp_rbd_ilqr_iterate_penalty_device (against gn_iterate)."""
    P = "penalty_" if penalty else "gn_"
    from idocp_amd.workloads import anymal_problem
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rt.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    nq, nv, nu, nf, S = m.nq, m.nv, m.nu, 3 * m.ncontacts, GN_STEPS
    nx, nz = 2 * nv, 2 * nv + nu
    rng = np.random.default_rng(13)
    cost = anymal_problem(m, trotting_ref=False)[0]
    ts, dt = 0.05, 0.01
    o = C.c_void_p()
    cons = None
    if penalty:
        cons = capi.Constraints()
        cons.joint_position_limits = cons.joint_velocity_limits = cons.joint_torque_limits = cons.linearized_friction_cone = 1
        cons.joint_acceleration_lower_limit = cons.joint_acceleration_upper_limit = 1
        cons.mu = 0.7
        for j in range(nu):
            cons.a_min[j], cons.a_max[j] = -5.0, 5.0
    capi.check(lib.idocp_rbd_objective_create(h, C.byref(cost), C.byref(cons) if penalty else None, 0.0, dt, S, C.byref(o)), "objective")
    Rc = lib.idocp_rbd_objective_constraint_rows(o) if penalty else 0
    R = lib.idocp_rbd_objective_residual_rows(o) + Rc
    MU = 10.0
    want_iterate = not wanted or P + "iterate" in wanted or (penalty and "al_iterate" in wanted)
    sizes = {"q": (S + 1) * n * nq, "v": (S + 1) * n * nv, "u": S * n * nu, "a": S * n * nv, "f": S * n * nf, "pts": S * n * nf,
             "A": S * n * nx * nx, "B": S * n * nx * nu, "G": S * n * R * nz, "rho": S * n * R, "lx": (S + 1) * n * nx, "lu": S * n * nu,
             "K": S * n * nx * nu, "k": S * n * nu, "P0": n * nx * nx, "p0": n * nx, "wx": nx, "wu": nu, "wxf": nx,
             "cost": n, "viol": n, "expected": 2 * n, "alpha_accepted": n, "status": (n + 1) // 2}
    if penalty:
        sizes["D"] = S * n * nz
    if want_iterate:
        sizes["work"] = (lib.idocp_rbd_ilqr_penalty_workspace_bytes(h, o, n, S) if penalty else lib.idocp_rbd_ilqr_gn_workspace_bytes(h, n, S)) // 8
    dev = {}
    for key, size in sizes.items():
        dev[key] = C.c_void_p()
        capi.check(lib.idocp_device_alloc(C.byref(dev[key]), 8 * size), "alloc")
        assert rt.hipMemsetAsync(dev[key], 0, 8 * size, stream) == 0
    q0 = np.tile(ANYMAL_Q_STANDING, (n, 1))
    q0[:, 7:] += rng.uniform(-0.02, 0.02, (n, nv - 6))
    feet = np.zeros(nf)
    capi.check(lib.idocp_model_contact_positions(C.byref(m), np.ascontiguousarray(ANYMAL_Q_STANDING).ctypes.data, feet.ctypes.data), "feet")
    pts = np.ascontiguousarray(np.broadcast_to(feet, (S, n, nf)))
    W = lambda name, k: np.array(getattr(cost, name)[:k])      # noqa: E731
    for key, x in (("q", q0), ("pts", pts), ("wx", dt * np.concatenate([W("q_weight", nv), W("v_weight", nv)])), ("wu", dt * W("u_weight", nu)),
                   ("wxf", np.concatenate([W("qf_weight", nv), W("vf_weight", nv)]))):
        x = np.ascontiguousarray(x)
        capi.check(lib.idocp_device_upload(dev[key], x.ctypes.data, x.nbytes), "upload")
    act = (C.c_int * (4 * S))(*([1] * (4 * S)))
    capi.check(lib.idocp_rbd_rollout_device(h, n, S, act, ts, dt, dev["u"], dev["pts"], dev["q"], dev["v"], dev["a"], dev["f"], 0), "rollout")
    sc = capi.RbdScoreIO()
    sc.q_traj, sc.v_traj, sc.u_traj, sc.a_traj, sc.f_traj, sc.cost, sc.violation = dev["q"], dev["v"], dev["u"], dev["a"], dev["f"], dev["cost"], dev["viol"]
    capi.check(lib.idocp_rbd_score_rollout_device(h, o, n, 0, S, act, 1, 0, C.byref(sc)), "score")
    if penalty:      # (`violation` of the iteration holds sq_violation)
        capi.check(lib.idocp_rbd_score_penalty_device(h, o, n, 0, S, act, 0, dev["q"], dev["v"], dev["u"], dev["a"], dev["f"], dev["viol"]), "score_penalty")

    lin = capi.RbdPenaltyLinearizationIO() if penalty else capi.RbdCostLinearizationIO()
    lin.A_traj, lin.B_traj, lin.G_traj, lin.rho_traj, lin.lx_traj, lin.lu_traj = dev["A"], dev["B"], dev["G"], dev["rho"], dev["lx"], dev["lu"]
    if penalty:
        lin.D_traj = dev["D"]
        linearize = lambda: capi.check(lib.idocp_rbd_linearize_rollout_penalty_device(h, o, n, S, act, ts, dt, dev["u"], dev["pts"], dev["q"], dev["v"], C.byref(lin), MU, 0), "linearize_penalty")  # noqa: E731
    else:
        linearize = lambda: capi.check(lib.idocp_rbd_linearize_rollout_cost_device(h, o, n, S, act, ts, dt, dev["u"], dev["pts"], dev["q"], dev["v"], C.byref(lin), 0), "linearize_cost")  # noqa: E731
    linearize()      # (gn_lqr_backward reads what it wrote, whether or not its own row is asked for)
    lqr = capi.RbdLqrIO()
    for field, key in (("A_traj", "A"), ("B_traj", "B"), ("x_weight", "wx"), ("u_weight", "wu"), ("xf_weight", "wxf"), ("lx_traj", "lx"), ("lu_traj", "lu"),
                       ("K_traj", "K"), ("k_traj", "k"), ("P0", "P0"), ("p0", "p0"), ("expected", "expected"), ("status", "status")):
        setattr(lqr, field, dev[key])
    lqr.regularization = 1e-6
    pass_samples = min(n, GN_PASS)
    pass_bytes = 8 * (GN_RESIDUAL_DOUBLES + Rc * (nz + 1) + nz + nq + nv + nu) * pass_samples      # (penalty: the wider G and rho, D out, q, v, u in)

    def pass_copy():
        assert rt.hipMemcpyAsync(dev["A"], dev["G"], pass_bytes, 3, stream) == 0

    if penalty:
        backward = lambda: capi.check(lib.idocp_rbd_lqr_backward_gn_diag_device(h, n, S, C.byref(lqr), R, dev["G"], dev["D"]), "lqr_gn_diag")  # noqa: E731
    else:
        backward = lambda: capi.check(lib.idocp_rbd_lqr_backward_gn_device(h, n, S, C.byref(lqr), R, dev["G"]), "lqr_gn")  # noqa: E731
    plan = ((P + "lqr_backward", backward),
            (P + "residual_pass_copy", pass_copy), (P + "linearize_s16", linearize))      # (the copy overwrites the front of A: the linearisation runs after it)
    for row, launch in plan:
        if wanted and row not in wanted:
            continue
        measure(row, launch)
        res[row]["steps"] = S
        if row == P + "lqr_backward":
            status = np.zeros((n + 1) // 2)
            capi.check(lib.idocp_rbd_synchronize(h), "synchronize")
            capi.check(lib.idocp_device_download(status.ctypes.data, dev["status"], status.nbytes), "download")
            res[P + "lqr_all_solved"] = bool((status.view(np.int32)[:n] == -1).all())
            res[row].update({"g_rows": R, "ms_per_step": round(res[row]["ms_median"] / S, 4)})
            for other in ("lqr_gains_ilqr", "gn_lqr_backward"):
                if other in res and other != row:
                    res[row]["ratio_to_" + other] = round(res[row]["ms_median"] / res[other]["ms_median"], 3)
        if row == P + "residual_pass_copy":
            res[row].update({"samples": pass_samples, "bytes": pass_bytes, "GB_per_s": round(pass_bytes / res[row]["ms_median"] / 1e6, 1),
                             "residual_launches_per_linearisation": S * -(-n // pass_samples)})
        if row == P + "linearize_s16":
            res[row].update({"G_traj_bytes": 8 * sizes["G"], "passes_per_step": -(-n // pass_samples)})
            for other in ("fdd_linearize_s16", "gn_linearize_s16"):
                if other in res and other != row:
                    res[row]["ratio_to_" + other] = round(res[row]["ms_median"] / res[other]["ms_median"], 3)
    if want_iterate and (not wanted or P + "iterate" in wanted):
        io = capi.RbdIlqrIO()
        for field, key in (("q_traj", "q"), ("v_traj", "v"), ("u_traj", "u"), ("a_traj", "a"), ("f_traj", "f"), ("cost", "cost"), ("violation", "viol"),
                           ("alpha_accepted", "alpha_accepted"), ("lqr_status", "status"), ("expected", "expected"), ("workspace", "work")):
            setattr(io, field, dev[key])
        io.regularization, io.armijo, io.shrink, io.alpha_min, io.penalty, io.trials = 1e-6, 1e-4, 0.5, 1e-3, MU if penalty else 0.0, 2
        iterate = lib.idocp_rbd_ilqr_iterate_penalty_device if penalty else lib.idocp_rbd_ilqr_iterate_gn_device
        measure(P + "iterate", lambda: capi.check(iterate(h, o, n, S, act, ts, dt, dev["pts"], C.byref(io), 0), "iterate"))
        res[P + "iterate"].update({"steps": S, "trials": 2, "workspace_bytes": 8 * sizes["work"]})
        status = np.zeros((n + 1) // 2)
        capi.check(lib.idocp_rbd_synchronize(h), "synchronize")
        capi.check(lib.idocp_device_download(status.ctypes.data, dev["status"], status.nbytes), "download")
        res[P + "iterate_all_solved"] = bool((status.view(np.int32)[:n] == -1).all())
        for other in ("ilqr_iterate", "gn_iterate"):
            if other in res and other != P + "iterate":
                res[P + "iterate"]["ratio_to_" + other] = round(res[P + "iterate"]["ms_median"] / res[other]["ms_median"], 3)
    if penalty and (not wanted or set(wanted) & set(AL_ROWS)):
        al_rows(wanted, lib, rt, h, stream, o, n, S, act, ts, dt, MU, dev, lin, sizes, measure, res)
    capi.check(lib.idocp_rbd_synchronize(h), "synchronize")
    lib.idocp_rbd_objective_destroy(o)
    for d in dev.values():
        lib.idocp_device_free(d)


def al_rows(wanted, lib, rt, h, stream, o, n, S, act, ts, dt, MU, dev, lin, sizes, measure, res):
    """the al_* rows, in the setting and on the buffers of the penalty_* rows (read each against the penalty_* row of the same run), multipliers
    [S][n][L] as one idocp_rbd_ilqr_al_update_device from zero leaves them: al_score is idocp_rbd_score_al_device and al_update
    idocp_rbd_multiplier_update_device in place with both statistics, over all S steps; al_score_copy / al_update_copy a device-to-device copy of the
    bytes each touches (the q, v, u, a, f slices and the multipliers in; the multipliers out for the update), capped at the size of A_traj;
    al_linearize_s16 is idocp_rbd_linearize_rollout_al_device with all seven outputs; al_iterate one idocp_rbd_ilqr_iterate_al_device with two
    trial rounds."""
    L = lib.idocp_rbd_objective_multiplier_rows(o)
    for key, size in (("lam", S * n * L), ("inf", n), ("change", n), ("sq", n)):
        dev[key] = C.c_void_p()
        capi.check(lib.idocp_device_alloc(C.byref(dev[key]), 8 * size), "alloc")
        assert rt.hipMemsetAsync(dev[key], 0, 8 * size, stream) == 0
    traj = (dev["q"], dev["v"], dev["u"], dev["a"], dev["f"])
    capi.check(lib.idocp_rbd_ilqr_al_update_device(h, o, n, S, act, *traj, MU, MU, dev["lam"], dev["viol"], dev["inf"], dev["change"]), "al_update")
    per_slice = (sizes["q"] + sizes["v"]) // (S + 1)
    read = 8 * (sizes["u"] + sizes["a"] + sizes["f"] + S * per_slice + S * n * L)
    cap = 8 * min(sizes["A"], sizes["G"])

    def copy(nbytes):
        assert rt.hipMemcpyAsync(dev["A"], dev["G"], min(nbytes, cap), 3, stream) == 0

    plan = (("al_score", lambda: capi.check(lib.idocp_rbd_score_al_device(h, o, n, 0, S, act, 0, *traj, MU, dev["lam"], dev["sq"]), "score_al"), 0),
            ("al_score_copy", lambda: copy(read), read),
            ("al_update", lambda: capi.check(lib.idocp_rbd_multiplier_update_device(h, o, n, 0, S, act, 0, *traj, MU, dev["lam"], dev["lam"], dev["inf"], dev["change"]),
                                             "multiplier_update"), 0),
            ("al_update_copy", lambda: copy(read + 8 * S * n * L), read + 8 * S * n * L),
            ("al_linearize_s16", lambda: capi.check(lib.idocp_rbd_linearize_rollout_al_device(h, o, n, S, act, ts, dt, dev["u"], dev["pts"], dev["q"], dev["v"], C.byref(lin),
                                                                                            MU, dev["lam"], 0), "linearize_al"), 0))
    for row, launch, nbytes in plan:
        if wanted and row not in wanted:
            continue
        measure(row, launch)
        res[row].update({"steps": S, "multiplier_rows": L})
        if nbytes:
            res[row].update({"bytes": min(nbytes, cap), "GB_per_s": round(min(nbytes, cap) / res[row]["ms_median"] / 1e6, 1)})
        if row == "al_linearize_s16" and "penalty_linearize_s16" in res:
            res[row]["ratio_to_penalty_linearize_s16"] = round(res[row]["ms_median"] / res["penalty_linearize_s16"]["ms_median"], 3)
    if (not wanted or "al_iterate" in wanted) and "work" in dev:
        io = capi.RbdIlqrIO()
        for field, key in (("q_traj", "q"), ("v_traj", "v"), ("u_traj", "u"), ("a_traj", "a"), ("f_traj", "f"), ("cost", "cost"), ("violation", "viol"),
                           ("alpha_accepted", "alpha_accepted"), ("lqr_status", "status"), ("expected", "expected"), ("workspace", "work")):
            setattr(io, field, dev[key])
        io.regularization, io.armijo, io.shrink, io.alpha_min, io.penalty, io.trials = 1e-6, 1e-4, 0.5, 1e-3, MU, 2
        measure("al_iterate", lambda: capi.check(lib.idocp_rbd_ilqr_iterate_al_device(h, o, n, S, act, ts, dt, dev["pts"], C.byref(io), dev["lam"], 0), "iterate_al"))
        res["al_iterate"].update({"steps": S, "trials": 2})
        if "penalty_iterate" in res:
            res["al_iterate"]["ratio_to_penalty_iterate"] = round(res["al_iterate"]["ms_median"] / res["penalty_iterate"]["ms_median"], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=122880)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", default="", help="comma-separated row names (default: all)")
    args = ap.parse_args()
    wanted = [x for x in args.rows.split(",") if x]
    n, lib, rt = args.n, capi.lib(), C.CDLL("libamdhip64.so")
    rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    rt.hipEventSynchronize.argtypes = [C.c_void_p]
    rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    m = anymal_model()
    nv, nq, nf = m.nv, m.nq, 3 * m.ncontacts
    h = C.c_void_p()
    capi.check(lib.idocp_rbd_create(C.byref(m), 0, C.byref(h)), "idocp_rbd_create")
    lib.idocp_rbd_stream.restype = C.c_void_p
    stream = C.c_void_p(lib.idocp_rbd_stream(h))
    rng = np.random.default_rng(0)
    q = np.tile(ANYMAL_Q_STANDING, (n, 1))
    q[:, 7:] += rng.uniform(-0.3, 0.3, (n, nv - 6))
    quat = q[:, 3:7] + rng.normal(scale=0.2, size=(n, 4))
    q[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    host = {"q": q, "v": rng.uniform(-1, 1, (n, nv)), "a": rng.uniform(-2, 2, (n, nv)), "f": rng.uniform(-30, 30, (n, nf)),
            "contact_points": rng.uniform(-0.5, 0.5, (n, nf))}
    sizes = {"tau": nv, "dtau_dq": nv * nv, "dtau_dv": nv * nv, "dtau_da": nv * nv, "C": nf, "dCdq": nf * nv, "dCdv": nf * nv, "dCda": nf * nv,
             "MJtJinv": (nv + nf) ** 2}
    host["u"] = rng.uniform(-20, 20, (n, m.nu))
    if not wanted or set(wanted) & set(POLICY_ROWS):
        nk = m.nu * 2 * nv
        host["K"] = rng.uniform(-1, 1, (n, nk))
        host["q_ref"] = np.tile(ANYMAL_Q_STANDING, (n, 1))
        host["v_ref"] = np.zeros((n, nv))
        host["q_traj"] = np.concatenate([q[None], np.zeros((1, n, nq))])
        host["v_traj"] = np.concatenate([host["v"][None], np.zeros((1, n, nv))])
        host["u_out"] = np.zeros((n, m.nu))
    fd_sizes = {"fd_a": nv, "fd_f": nf, "fd_q_next": nq, "fd_v_next": nv}
    sizes.update(fd_sizes)
    dev = {}
    for k, x in host.items():
        dev[k] = C.c_void_p()
        x = np.ascontiguousarray(x)
        capi.check(lib.idocp_device_alloc(C.byref(dev[k]), x.nbytes), "alloc")
        capi.check(lib.idocp_device_upload(dev[k], x.ctypes.data, x.nbytes), "upload")
    for k, sz in sizes.items():
        dev[k] = C.c_void_p()
        capi.check(lib.idocp_device_alloc(C.byref(dev[k]), 8 * sz * n), "alloc")
    active = (C.c_int * 4)(1, 1, 1, 1)
    events = []
    for _ in range(args.launches + 1):
        e = C.c_void_p()
        assert rt.hipEventCreate(C.byref(e)) == 0
        events.append(e)
    res = {"n": n, "launches": args.launches, "warmup": args.warmup}

    def measure(name, launch):
        for _ in range(args.warmup):
            launch()
        capi.check(lib.idocp_rbd_synchronize(h), "synchronize")
        assert rt.hipEventRecord(events[0], stream) == 0
        for i in range(args.launches):
            launch()
            assert rt.hipEventRecord(events[i + 1], stream) == 0
        assert rt.hipEventSynchronize(events[-1]) == 0
        ms = []
        for i in range(args.launches):
            t = C.c_float()
            assert rt.hipEventElapsedTime(C.byref(t), events[i], events[i + 1]) == 0
            ms.append(t.value)
        med = float(np.median(ms))
        res[name] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "samples_per_s": round(n / med * 1e3)}

    for name, mode, outputs in SELECTIONS + FD_SELECTIONS + tuple((x, None, ()) for x in POLICY_ROWS):
        if wanted and name not in wanted:
            continue
        if name in POLICY_ROWS:
            pol = capi.RbdPolicy()
            pol.u_ff, pol.K, pol.q_ref, pol.v_ref = dev["u"], dev["K"], dev["q_ref"], dev["v_ref"]
            pol.shared_gains = pol.shared_ref = int(name == "policy_shared")
            if name == "fd_step_closed_loop":
                launch = lambda: capi.check(lib.idocp_rbd_rollout_policy_device(h, n, 1, active, 0.05, 0.01, C.byref(pol), dev["contact_points"], dev["q_traj"],  # noqa: E731
                                                                                dev["v_traj"], dev["u_out"], dev["fd_a"], dev["fd_f"], 0), name)
            else:
                launch = lambda: capi.check(lib.idocp_rbd_feedback_torques_batch_device(h, n, dev["q"], dev["v"], C.byref(pol), dev["u_out"]), name)  # noqa: E731
        elif name.startswith("fd_"):
            io = capi.RbdFdIO()
            for k in capi.RbdFdIO.INPUTS:
                setattr(io, k, dev[k])
            for k in outputs:
                setattr(io, k, dev["fd_" + k])
            launch = lambda: capi.check(lib.idocp_rbd_forward_dynamics_batch_device(h, mode, n, active, 0.05, 0.01, C.byref(io)), name)  # noqa: E731
        else:
            io = capi.RbdIO()
            for k in capi.RbdIO.INPUTS + tuple(outputs):
                setattr(io, k, dev[k])
            launch = lambda: capi.check(lib.idocp_rbd_contact_dynamics_batch_device(h, mode, n, active, 0.05, C.byref(io)), name)  # noqa: E731
        measure(name, launch)
    if not wanted or set(wanted) & set(SCORE_ROWS):
        score_rows(args, wanted, lib, rt, h, stream, m, n, host, measure, res)
    if not wanted or set(wanted) & set(SAMPLE_ROWS):
        sample_rows(wanted, lib, rt, h, stream, m, n, measure, res)
    if not wanted or set(wanted) & set(KIN_ROWS):
        kin_rows(wanted, lib, rt, h, stream, m, n, host, measure, res)
    if not wanted or set(wanted) & set(FDD_ROWS):
        fdd_rows(wanted, lib, h, m, n, dev, active, measure, res)
    if not wanted or set(wanted) & set(LQR_ROWS):
        lqr_rows(wanted, lib, rt, h, stream, m, n, measure, res)
    if not wanted or set(wanted) & set(ILQR_ROWS):
        ilqr_rows(wanted, lib, rt, h, stream, m, n, measure, res)
    if not wanted or set(wanted) & set(GN_ROWS):
        gn_rows(wanted, lib, rt, h, stream, m, n, measure, res)
    if not wanted or set(wanted) & set(PENALTY_ROWS + AL_ROWS):
        gn_rows(wanted, lib, rt, h, stream, m, n, measure, res, penalty=True)
    ran = [k for k in res if isinstance(res[k], dict)]
    for key, src, width, rows in (("tau_finite", "tau", nv, ("stage_", "impulse_")), ("fd_a_finite", "fd_a", nv, ("fd_",)),
                                  ("policy_u_finite", "u_out", m.nu, ("policy_", "fd_step_closed_loop"))):
        if any(x.startswith(rows) for x in ran):
            out = np.zeros((n, width))
            capi.check(lib.idocp_device_download(out.ctypes.data, dev[src], out.nbytes), "download")
            res[key] = bool(np.isfinite(out).all())
    for d in dev.values():
        lib.idocp_device_free(d)
    lib.idocp_rbd_destroy(h)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
