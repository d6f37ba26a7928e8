"""Numpy restatement of the log-density of given actions (csrc/policy_logp.hip: cadm_policy_logp, cadm_policy_logp_returns) -- test
infrastructure shared by tests/test_policy_logp_ref.py (CPU) and tests/test_gpu_policy_logp.py, built on tests/gauss_policy_ref.py's
pieces: the actor is that file's SAC actor, `z32` / `z64` its 2 A sums of the last layer.

`y32` is the kernel's normalised action, float32 operation for operation (one subtraction, one correctly rounded division, the clamp at
YMAX).  `logp32` walks include/cadm_hip.h ("Log-density of given actions") in float32; `logp64` restates it in float64 -- from the
float64 y of the action, or, handed `y32`'s result, FROM THAT y: the inverse squash is ill-conditioned at the bounds (d u / d y = 1 /
(1 - y^2), 5e5 at YMAX), so a float64 reference that formed y on its own would differ from the kernel by the float32 rounding of y times
that factor, which is an error of the INPUT and not of the kernel.  `bars` are the per-row bounds the GPU test holds the kernel to.

Derivation of `bars` (float64 reference continued from the kernel's y; e_* are absolute error bounds of the float32 quantity):
  the chain                e_z   = 1e-5 max(1, max |z|) over the row's 2 A sums: the project's bar of an fp32 chain, on mu_d and l_d
  the log-std              e_ls  = e_z (clamp, 1-Lipschitz) | 0.5 (hi - lo) e_z (tanh): gauss_policy_ref.bars'
  a transcendental result  1e-5 max(1, |v|) on every elementwise result v of log1pf, logf, expf (the project's bar again; the libm
                           functions are good to a few ulp, 1e-7 relative, so this is generous and it is the same everywhere)
  lp, lm                   e_lp = 1e-5 max(1, |lp|),  e_lm = 1e-5 max(1, |lm|)          (their argument y is exact: see above)
  u = 0.5 (lp - lm)        e_u   = 0.5 (e_lp + e_lm);   no squash: u = a exactly, e_u = 0
  J = log(half) + lp + lm  e_J   = e_lp + e_lm + 1e-5 max(1, |log half|);   no squash, or space "pre_squash": J is not used, e_J = 0
  xi = (u - mu) exp(-ls)   e_xi  = (e_u + e_z) / sig + |xi| e_ls + |xi| 1e-5 max(1, sig)
                           the first two terms are the issue's: the numerator's error over sig, and d exp(-ls) = -exp(-ls) d ls.  The
                           third is expf's own result error, |u - mu| * 1e-5 max(1, 1 / sig) = |xi| 1e-5 max(sig, 1), which the rule
                           for a transcendental result asks for and the issue's line left out.
  g = -0.5 xi^2 - ls - c   e_g   = |xi| e_xi + e_ls
  logp = sum_d (g_d - J_d) bar   = sum_d (|xi_d| e_xi,d + e_ls + e_J,d) + 1e-5 max(1, |logp|)    (the A adds and the terms' own roundings)

`roundtrip_bars` is the bound of the round trip logp(sample's action) against the sampler's own logp, per ELEMENT (row, dim): `bars`'
element plus what the float32 rounding of the sampled action costs.  The sampler stores a = fl(mid + half * fl(tanh u)): two roundings,
each at most 2^-24 max(|a|, half) (and tanhf's own few ulp, inside the 4 2^-24 taken here), so y is off by e_y = 4 * 2^-24 * max(|a|,
half) / half + 2^-24 (the division), u by e_y / (1 - y^2), J by 2 |y| e_y / (1 - y^2), and xi by the former over sig.  The sampler's own
term is held to gauss_policy_ref's elementwise rule 1e-5 max(1, |term|)."""
import numpy as np

import gauss_policy_ref as gref

F = np.float32
YMAX = F(0.999999)            # include/cadm_hip.h CADM_LOGP_YMAX
HALF_LOG_2PI = F(0.9189385)
SPACES = ("action", "pre_squash")


def _mid_half(lb, ub):
    return gref._mid_half(lb, ub)


def y32(act, lb=-1.0, ub=1.0):
    """the kernel's y [R, A] float32: (a - mid) / half, clamped to +-YMAX"""
    mid, half = _mid_half(lb, ub)
    with np.errstate(all="ignore"):
        y = (np.asarray(act, F) - mid) / half
        y = np.minimum(np.maximum(y, -YMAX), YMAX)
    assert y.dtype == F
    return y


def _log_std64(l, bound, lo, hi):
    return np.clip(l, lo, hi) if bound == "clamp" else lo + 0.5 * (hi - lo) * (np.tanh(l) + 1.0)


def logp64(z, act, squash, bound, lo, hi, lb=-1.0, ub=1.0, space="action", y=None):
    """float64 restatement on the 2 A sums z [R, 2 A] and the actions act [R, A] -> dict(logp [R], term, u, xi, ls, sig, lp, lm, J, y):
    the bounds, mid, half and YMAX are the float32 numbers the kernel reads, the arithmetic is float64.  y: None, y is formed in float64
    from act; else the kernel's float32 y (`y32`), and the reference continues from it.  A row whose action holds a non-finite value has
    logp NaN."""
    z, a = np.asarray(z, np.float64), np.asarray(act, F).astype(np.float64)
    A = a.shape[-1]
    mu, l = z[..., :A], z[..., A:]
    lo, hi, lb, ub = (float(F(v)) for v in (lo, hi, lb, ub))
    mid, half = (float(v) for v in _mid_half(lb, ub))
    ls = _log_std64(l, bound, lo, hi)
    sig = np.exp(ls)
    with np.errstate(all="ignore"):
        if squash == "tanh":
            yy = np.clip((a - mid) / half, -float(YMAX), float(YMAX)) if y is None else np.asarray(y, np.float64)
            lp, lm = np.log1p(yy), np.log1p(-yy)
            u = 0.5 * (lp - lm)
            J = np.log(half) + (lp + lm)
        else:
            yy, u = a, a
            lp = lm = J = np.zeros_like(a)
        xi = (u - mu) * np.exp(-ls)
        g = -0.5 * xi * xi - ls - 0.5 * np.log(2.0 * np.pi)
        term = g - J if space == "action" else g
        logp = term.sum(axis=-1)
    logp = np.where(np.isfinite(a).all(axis=-1), logp, np.nan)
    return dict(logp=logp, term=term, u=u, xi=xi, ls=ls, sig=sig, lp=lp, lm=lm, J=J, y=yy)


def logp32(z, act, squash, bound, lo, hi, lb=-1.0, ub=1.0, space="action"):
    """the kernel's float32 arithmetic, every operation rounded on its own, on the float32 sums z [R, 2 A] and actions act [R, A] ->
    dict(logp [R], term [R, A]) float32; logp sums term_d in ascending d from term_0; NaN for a row with a non-finite action"""
    z, a = np.asarray(z, F), np.asarray(act, F)
    A = a.shape[-1]
    mu, l = z[..., :A], z[..., A:]
    lo, hi, lb, ub = F(lo), F(hi), F(lb), F(ub)
    mid, half = _mid_half(lb, ub)
    with np.errstate(all="ignore"):
        ls = np.minimum(np.maximum(l, lo), hi) if bound == "clamp" else lo + (F(0.5) * (hi - lo)) * (np.tanh(l) + F(1))
        if squash == "tanh":
            y = y32(a, lb, ub)
            lp, lm = np.log1p(y), np.log1p(-y)
            u = F(0.5) * (lp - lm)
            J = np.log(half) + (lp + lm)
        else:
            u, J = a, np.zeros_like(a)
        xi = (u - mu) * np.exp(-ls)
        g = ((F(-0.5) * xi) * xi - ls) - HALF_LOG_2PI
        term = g - J if space == "action" else g
        logp = term[..., 0]
        for d in range(1, A):
            logp = logp + term[..., d]
        logp = np.where(np.isfinite(a).all(axis=-1), logp, F(np.nan))
    for v in (ls, u, xi, g, term, logp):
        assert v.dtype == F
    return dict(logp=logp, term=term)


def _elements(z, ref, squash, bound, lo, hi, lb, ub, space):
    """(e_term [R, A] = |xi| e_xi + e_ls + e_J, e_u, e_J) of the derivation above"""
    z = np.asarray(z, np.float64)
    e_z = 1e-5 * np.maximum(1.0, np.abs(z).max(axis=-1, keepdims=True))
    e_ls = e_z if bound == "clamp" else 0.5 * (float(F(hi)) - float(F(lo))) * e_z
    axi, sig = np.abs(ref["xi"]), ref["sig"]
    if squash == "tanh":
        e_lp = 1e-5 * np.maximum(1.0, np.abs(ref["lp"]))
        e_lm = 1e-5 * np.maximum(1.0, np.abs(ref["lm"]))
        e_u = 0.5 * (e_lp + e_lm)
        half = float(_mid_half(lb, ub)[1])
        e_J = e_lp + e_lm + 1e-5 * max(1.0, abs(np.log(half))) if space == "action" else np.zeros_like(e_u)
    else:
        e_u = np.zeros_like(axi)
        e_J = np.zeros_like(axi)
    e_xi = (e_u + e_z) / sig + axi * e_ls + axi * 1e-5 * np.maximum(1.0, sig)
    return axi * e_xi + e_ls + e_J, e_z, e_ls


def bars(z, ref, squash, bound, lo, hi, lb=-1.0, ub=1.0, space="action"):
    """bar on |logp - ref["logp"]| [R] from the reference's own values: z [R, 2 A] float64 and ref = logp64(.., y=y32(act)) (see the
    module docstring for the derivation)"""
    e_term, _, _ = _elements(z, ref, squash, bound, lo, hi, lb, ub, space)
    with np.errstate(invalid="ignore"):
        return e_term.sum(axis=-1) + 1e-5 * np.maximum(1.0, np.abs(ref["logp"]))


def roundtrip_bars(z, ref, act, squash, bound, lo, hi, lb=-1.0, ub=1.0):
    """bar on |term(sample's action) - the sampler's own term| per element [R, A] (space "action"): `bars`' element, the sampler's own
    1e-5 max(1, |term|), and the float32 rounding of the stored action taken through the inverse squash (module docstring)"""
    e_term, e_z, e_ls = _elements(z, ref, squash, bound, lo, hi, lb, ub, "action")
    own = 2e-5 * np.maximum(1.0, np.abs(ref["term"]))
    if squash != "tanh":
        # u = a + rounding of the sampler's mu + sig xi: 2^-24 |a| on u, over sig on xi
        e_in = 2.0 ** -24 * np.abs(np.asarray(act, np.float64))
        return e_term + own + np.abs(ref["xi"]) * e_in / ref["sig"]
    half = float(_mid_half(lb, ub)[1])
    a = np.abs(np.asarray(act, np.float64))
    e_y = 4.0 * 2.0 ** -24 * np.maximum(a, half) / half + 2.0 ** -24
    inv = 1.0 / (1.0 - ref["y"] ** 2)
    e_u_in = e_y * inv
    return e_term + own + np.abs(ref["xi"]) * e_u_in / ref["sig"] + 2.0 * np.abs(ref["y"]) * e_y * inv


def step_sum32(steps, first, weight, rows, disc=None):
    """cadm_policy_logp_returns' second launch in numpy float32: steps [H, m, n, p] (NaN where not counted), first [m, n, p] int or None,
    rows [m, n, p] -> (S, rows + weight * S): S = ((0 + lp_0) + lp_1) + .. over t <= first, with disc [H + 1]: S = S + disc[t] * lp_t;
    one multiply, then one add"""
    steps, rows = np.asarray(steps, F), np.asarray(rows, F)
    H = steps.shape[0]
    last = np.full(rows.shape, H - 1) if first is None else np.minimum(np.asarray(first), H - 1)
    S = np.zeros(rows.shape, F)
    with np.errstate(all="ignore"):
        for t in range(H):
            term = steps[t] if disc is None else F(disc[t]) * steps[t]
            S = np.where(t <= last, S + term, S).astype(F)
        out = rows + F(weight) * S
    assert S.dtype == F and out.dtype == F
    return S, out
