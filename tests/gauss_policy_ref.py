"""Numpy restatement of the stochastic actor head (csrc/policy_gauss.hip: cadm_policy_sample, cadm_imagine_sampled) -- test
infrastructure shared by tests/test_gauss_policy_ref.py (CPU) and tests/test_gpu_gauss_policy.py, built on tests/policy_ref.py's pieces.

A SAC actor is an MLP D -> h_1 .. h_L -> 2 A whose last layer's columns [0, A) are the mean mu and [A, 2 A) the raw log-std l (torch's
chunk(2, -1)).  `z32` / `z64` are the 2 A sums of the last layer by the kernel's float32 chain (policy_ref.emulate32 without squash or
clip: every column is its own chain, so the kernel's two A-wide layers give the same sums) and in float64; `sample32` walks the
arithmetic of include/cadm_hip.h ("Stochastic actor head") operation for operation in float32, `sample64` restates it in float64 on the
same float32 weights and the same draws; `xi` are the draws from oracle/philox.py under stream word 8; `bars` are the per-row error
bounds the GPU test holds the kernel to, derived from the project's two existing bars (1e-5 of scale for an fp32 chain, 4e-6 per unit
of Box-Muller radius for a device draw) on the reference's own values."""
import numpy as np

import policy_ref as pref
from oracle import philox

F = np.float32
STREAM_POLICY_SAMPLE = 8      # csrc/common.h CADM_STREAM_POLICY_SAMPLE
LN2 = F(0.6931472)
HALF_LOG_2PI = F(0.9189385)
BOUNDS = ("clamp", "tanh")


def split(layers, A):
    """(the mode actor's layers: the mean columns of the last layer; W_ls [h_L, A]; b_ls [A]) of a SAC actor's layers"""
    W, b = layers[-1]
    assert W.shape[1] == 2 * A and b.shape == (2 * A,)
    return list(layers[:-1]) + [(np.ascontiguousarray(W[:, :A]), np.ascontiguousarray(b[:A]))], np.ascontiguousarray(W[:, A:]), \
        np.ascontiguousarray(b[A:])


def actor(D, hidden, A, act, x, lo, hi, seed=0, mean=None, std=None):
    """He-initialised layers of D -> hidden -> 2 A whose log-std columns are mapped affinely ON THE REFERENCE so that, over the states x,
    the 20 % quantile of the raw l sits on lo and the 80 % quantile on hi: a fifth of the l beyond either bound, three fifths inside
    (the tests assert the shares they need with `shares`)"""
    layers = pref.he_policy(D, hidden, 2 * A, seed, 0.5)
    W, b = layers[-1]
    l = pref._z64(np.asarray(x, F).astype(np.float64), layers, act, mean, std)[..., A:]
    q_lo, q_hi = np.quantile(l, 0.2), np.quantile(l, 0.8)
    s = (hi - lo) / max(float(q_hi - q_lo), 1e-12)
    W, b = W.copy(), b.copy()
    W[:, A:] = (W[:, A:].astype(np.float64) * s).astype(F)
    b[A:] = (b[A:].astype(np.float64) * s + (lo - s * float(q_lo))).astype(F)
    return list(layers[:-1]) + [(W, b)]


def shares(l, lo, hi):
    """(share of l below lo, share above hi, share strictly inside)"""
    l = np.asarray(l, np.float64)
    return float((l < lo).mean()), float((l > hi).mean()), float(((l > lo) & (l < hi)).mean())


def z64(states, layers, act, mean=None, std=None):
    """the 2 A sums [..., 2 A] of the last layer in float64; a state with a non-finite value is read as zeros (its row is the fallback)"""
    x = np.asarray(states, F).astype(np.float64)
    bad = ~np.isfinite(x).all(axis=-1)
    return pref._z64(np.where(bad[..., None], 0.0, x), layers, act, mean, std)


def z32(states, layers, act, mean=None, std=None):
    """the same sums by the kernel's float32 chain"""
    return pref.emulate32(states, layers, act, "none", -np.inf, np.inf, mean, std)


def _draw(seed, call, rows, t, A):
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1)
    ng = (A + 3) // 4
    u = np.empty((rows.shape[0], 4 * ng), F)
    for g in range(ng):
        r = philox.philox4x32_10(philox._ctr(rows, np.uint32(t), np.uint32(g), np.uint32(STREAM_POLICY_SAMPLE)), philox._key(seed, call, rows.shape))
        for w in range(4):
            u[:, 4 * g + w] = philox.u01(r[..., w])
    return u


def xi(seed, call, rows, t, A):
    """the draws [R, A] float32 of rows `rows` (their Philox row numbers q) at step t: Philox4x32-10 keyed (seed, call), counter (q, t, g,
    8); one call serves dims 4 g .. 4 g + 3, words (0, 1) through Box-Muller to dims 4 g and 4 g + 1, words (2, 3) to 4 g + 2 and 4 g + 3"""
    u = _draw(seed, call, rows, t, A)
    out = np.empty_like(u)
    out[:, 0::2], out[:, 1::2] = philox.box_muller(u[:, 0::2], u[:, 1::2])
    return out[:, :A]


def xi_radius(seed, call, rows, t, A):
    """the Box-Muller radius sqrt(-2 ln u1) [R, A] float64 behind every draw of `xi`"""
    u = _draw(seed, call, rows, t, A).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u[:, 0::2]))
    return np.repeat(r, 2, axis=-1)[:, :A]


def _mid_half(lb, ub):
    return F(0.5) * (F(ub) + F(lb)), F(0.5) * (F(ub) - F(lb))


def sample64(z, xi_, squash, bound, lo, hi, lb=-1.0, ub=1.0):
    """float64 restatement on the 2 A sums z [R, 2 A] and the draws xi_ [R, A] -> dict(act, logp, mode, u, ls, sig, term): the bounds,
    mid and half are the float32 numbers the kernel reads, the arithmetic is float64"""
    z, e = np.asarray(z, np.float64), np.asarray(xi_, np.float64)
    A = e.shape[-1]
    mu, l = z[..., :A], z[..., A:]
    lo, hi, lb, ub = (float(F(v)) for v in (lo, hi, lb, ub))
    mid, half = (float(v) for v in _mid_half(lb, ub))
    ls = np.clip(l, lo, hi) if bound == "clamp" else lo + 0.5 * (hi - lo) * (np.tanh(l) + 1.0)
    sig = np.exp(ls)
    u = mu + sig * e
    if squash == "tanh":
        a = mid + half * np.tanh(u)
        x = -2.0 * u
        J = np.log(half) + 2.0 * (np.log(2.0) - u - (np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))))
        mode = mid + half * np.tanh(mu)
    else:
        a, J, mode = u, 0.0, mu
    term = -0.5 * e * e - ls - 0.5 * np.log(2.0 * np.pi) - J
    return dict(act=np.clip(a, lb, ub), logp=term.sum(axis=-1), mode=np.clip(mode, lb, ub), u=u, ls=ls, sig=sig, term=term)


def sample32(z, xi_, squash, bound, lo, hi, lb=-1.0, ub=1.0):
    """the kernel's float32 arithmetic, every operation rounded on its own, on the float32 sums z [R, 2 A] and draws xi_ [R, A] ->
    dict(act, logp, mode) float32; logp sums term_d in ascending d from term_0"""
    z, e = np.asarray(z, F), np.asarray(xi_, F)
    A = e.shape[-1]
    mu, l = z[..., :A], z[..., A:]
    lo, hi, lb, ub = F(lo), F(hi), F(lb), F(ub)
    mid, half = _mid_half(lb, ub)
    with np.errstate(all="ignore"):
        ls = np.minimum(np.maximum(l, lo), hi) if bound == "clamp" else lo + (F(0.5) * (hi - lo)) * (np.tanh(l) + F(1))
        sig = np.exp(ls)
        u = mu + sig * e
        if squash == "tanh":
            a = mid + half * np.tanh(u)
            x = F(-2) * u
            sp = np.maximum(x, F(0)) + np.log1p(np.exp(-np.abs(x)))
            J = np.log(half) + F(2) * ((LN2 - u) - sp)
        else:
            a, J = u, np.zeros_like(u)
        a = np.minimum(np.maximum(a, lb), ub)
        term = (((F(-0.5) * e) * e - ls) - HALF_LOG_2PI) - J
        logp = term[..., 0]
        for d in range(1, A):
            logp = logp + term[..., d]
        mode = np.minimum(np.maximum(pref.squash32(mu, squash, lb, ub), lb), ub)
    for v in (ls, sig, u, a, term, logp, mode):
        assert v.dtype == F
    return dict(act=a, logp=logp, mode=mode)


def bars(z, ref, xi_, radius, squash, bound, lo, hi, lb=-1.0, ub=1.0):
    """(bar on |act - ref| [R, A], bar on |logp - ref| [R]) from the reference's own values z [R, 2 A] float64, ref = sample64(..), the
    draws and their radii:
      the chain          e_z    = 1e-5 * max(1, max |z|) over the row's 2 A sums          (the project's bar for an fp32 chain)
      a device draw      del_d  = 4e-6 * max(1, r_d / 2)                                  (the bar the policy's noise is held to)
      the log-std        e_ls   = e_z (clamp: 1-Lipschitz);  0.5 (hi - lo) e_z (tanh: |d ls / d l| <= 0.5 (hi - lo))
      the pre-squash     e_u,d  = e_z + sig_d (|xi_d| e_ls + del_d)                      (d sig = sig d ls)
      act                half * e_u,d + 1e-5 (ub - lb)       half = 1 without a squash  (|d tanh| <= 1; the squash's own rounding)
      logp               sum_d (|xi_d| del_d + e_ls + 2 e_u,d) + 1e-5 max(1, |logp|)     (|d J / d u| = 2 |tanh u| <= 2)"""
    z, e, r = np.asarray(z, np.float64), np.abs(np.asarray(xi_, np.float64)), np.asarray(radius, np.float64)
    e_z = 1e-5 * np.maximum(1.0, np.abs(z).max(axis=-1, keepdims=True))
    dl = 4e-6 * np.maximum(1.0, r / 2.0)
    e_ls = e_z if bound == "clamp" else 0.5 * (float(F(hi)) - float(F(lo))) * e_z
    e_u = e_z + ref["sig"] * (e * e_ls + dl)
    half = float(_mid_half(lb, ub)[1]) if squash == "tanh" else 1.0
    act_bar = half * e_u + 1e-5 * (float(F(ub)) - float(F(lb)))
    logp_bar = (e * dl + e_ls + 2.0 * e_u).sum(axis=-1) + 1e-5 * np.maximum(1.0, np.abs(ref["logp"]))
    return act_bar, logp_bar
