"""Shared by test_rbd_sample_gpu.py / test_rbd_sample_host.py: the sampling calls of the idocp_rbd_* handle (idocp_rbd_perturb_torques,
idocp_rbd_importance_weights, idocp_rbd_weighted_mean; include/idocp_hip.h) on numpy arrays, and their referee -- Philox4x32-10 in Python's integer
arithmetic, the word-to-uniform conversion and Box-Muller as the header states them, the weights and the mean with math.fsum."""
import math

import numpy as np

from idocp_amd import capi

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
CHUNK = capi.RBD_REDUCE_CHUNK
Z_MAX = math.sqrt(106.0 * math.log(2.0))


# ------------------------------------------------------------------ the referee

def philox4x32_10(counter, key):
    """ten rounds on four 32-bit counter words under two key words, every value a Python int"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniforms(r):
    """(u1 in (0, 1), u2 in [0, 1)) of the four output words; both are exact doubles"""
    a, b = (r[1] << 32 | r[0]) >> 12, (r[3] << 32 | r[2]) >> 11
    return (a + 0.5) * 2.0 ** -52, b * 2.0 ** -53


def words(seed, draw, step, i, pair):
    return philox4x32_10((i, step, pair, draw), (seed & MASK, seed >> 32))


def z(seed, draw, step, i, j):
    """the standard normal of torque j of sample i at a step; exactly 0 for sample 0"""
    if i == 0:
        return 0.0
    u1, u2 = uniforms(words(seed, draw, step, i, j // 2))
    rho = math.sqrt(-2.0 * math.log(u1))
    return rho * (math.sin(2.0 * math.pi * u2) if j % 2 else math.cos(2.0 * math.pi * u2))


def clamp(u, u_min, u_max):
    if u_min is not None:
        u = np.maximum(u, u_min)
    if u_max is not None:
        u = np.minimum(u, u_max)
    return u


def reference_perturb(n, first_step, u_nominal, sigma, u_min, u_max, seed, draw):
    u_nominal = np.asarray(u_nominal, dtype=np.float64)
    steps, nu = u_nominal.shape
    noise = np.array([[[z(seed, draw, first_step + k, i, j) for j in range(nu)] for i in range(n)] for k in range(steps)])
    return clamp(u_nominal[:, None, :] + np.asarray(sigma)[None, None, :] * noise, u_min, u_max)


def reference_weights(cost, violation, penalty, temperature):
    """(weights, stats) with the sums by math.fsum"""
    s = np.asarray(cost, dtype=np.float64) + (penalty * np.asarray(violation, dtype=np.float64) if violation is not None else 0.0)
    finite = np.isfinite(s)
    w = np.zeros(len(s))
    if not finite.any():
        return w, np.array([0.0, math.nan, -1.0, 0.0, 0.0])
    s_min = s[finite].min()
    at = int(np.flatnonzero(finite & (s == s_min))[0])
    w[finite] = np.exp(-(s[finite] - s_min) / temperature)
    W, W2 = math.fsum(w), math.fsum(w * w)
    return w, np.array([float(finite.sum()), s_min, float(at), W, W * W / W2])


def reference_mean(weights, x):
    """x [rows][n][m]; a sample of weight 0 is skipped; the sums by math.fsum"""
    weights, x = np.asarray(weights, dtype=np.float64), np.asarray(x, dtype=np.float64)
    rows, _, m = x.shape
    on = weights != 0.0
    W = math.fsum(weights[on])
    out = np.full((rows, m), math.nan)
    if W == 0.0:
        return out
    for r in range(rows):
        for c in range(m):
            col = x[r, on, c]
            out[r, c] = math.fsum(weights[on] * col) / W if np.isfinite(col).all() else (weights[on] * col).sum() / W
    return out


# ------------------------------------------------------------------ the calls

def _ptr(x):
    if x is None:
        return None
    return x.ptr if hasattr(x, "ptr") else x.ctypes.data


def _f64(x):
    return np.ascontiguousarray(x, dtype=np.float64) if x is not None else None


def perturb_raw(r, n, first_step, steps, u_nominal, sigma, u_min, u_max, seed, draw, u_samples, device=False):
    """numpy arrays (host form) or DeviceArrays (device form); None is NULL"""
    fn = r.lib.idocp_rbd_perturb_torques_device if device else r.lib.idocp_rbd_perturb_torques
    return fn(r.h, n, first_step, steps, _ptr(u_nominal), _ptr(sigma), _ptr(u_min), _ptr(u_max), seed, draw, _ptr(u_samples))


def weights_raw(r, n, cost, violation, penalty, temperature, weights, stats, device=False):
    fn = r.lib.idocp_rbd_importance_weights_device if device else r.lib.idocp_rbd_importance_weights
    return fn(r.h, n, _ptr(cost), _ptr(violation), penalty, temperature, _ptr(weights), _ptr(stats))


def mean_raw(r, n, rows, m, weights, x, mean, device=False):
    fn = r.lib.idocp_rbd_weighted_mean_device if device else r.lib.idocp_rbd_weighted_mean
    return fn(r.h, n, rows, m, _ptr(weights), _ptr(x), _ptr(mean))


def perturb(r, n, u_nominal, sigma, u_min=None, u_max=None, seed=0, draw=0, first_step=0):
    """host form; u_nominal [steps][nu]; returns u_samples [steps][n][nu]"""
    u_nominal, sigma, u_min, u_max = _f64(u_nominal), _f64(sigma), _f64(u_min), _f64(u_max)
    out = np.full((u_nominal.shape[0], n, u_nominal.shape[1]), -777.0)
    capi.check(perturb_raw(r, n, first_step, u_nominal.shape[0], u_nominal, sigma, u_min, u_max, seed, draw, out), "idocp_rbd_perturb_torques")
    return out


def weights(r, cost, violation=None, penalty=0.0, temperature=1.0):
    """host form; returns (weights [n], stats [5])"""
    cost, violation = _f64(cost), _f64(violation)
    w, stats = np.full(len(cost), -777.0), np.full(capi.RBD_WEIGHT_STATS, -777.0)
    capi.check(weights_raw(r, len(cost), cost, violation, penalty, temperature, w, stats), "idocp_rbd_importance_weights")
    return w, stats


def mean(r, w, x):
    """host form; x [rows][n][m]; returns mean [rows][m]"""
    w, x = _f64(w), _f64(x)
    rows, n, m = x.shape
    out = np.full((rows, m), -777.0)
    capi.check(mean_raw(r, n, rows, m, w, x, out), "idocp_rbd_weighted_mean")
    return out
