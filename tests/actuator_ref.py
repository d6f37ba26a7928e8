"""Numpy restatement of the actuator model (include/cadm_hip.h, cadm_actuate_actions), written from the definition: the sequences in
float32 -- every operation of a chain is one float32 operation, so they are reproducible bit for bit --, the cost in float64 from those
float32 sequences.  For tests/test_actuator_ref.py (CPU) and tests/test_gpu_actuator.py."""
import numpy as np

F = np.float32


def clip(x, lo, hi):
    """min(max(x, lo), hi) by comparisons: a NaN x stays NaN, a zero keeps its sign unless a bound replaces it"""
    v = np.where(x < lo, lo, x)
    return np.where(v > hi, hi, v).astype(F)


def actuate(seqs, delay, rate_limit, rate_w, prev=None, prefix=None, lb=-1.0, ub=1.0):
    """seqs [m,n,H,A] float32 -> (actuated copy [m,n,H,A] float32, cost [m,n] float64, S [m,n] float64: the sum of |w (y - last)^2| the
    cost was added up from).  rate_limit / rate_w [A]; prev [m,A] / prefix [m,delay,A], NaN = absent, None = all NaN."""
    u = np.array(seqs, dtype=F, copy=True)
    m, n, H, A = u.shape
    dl, w = np.broadcast_to(np.asarray(rate_limit, F), (A,)), np.broadcast_to(np.asarray(rate_w, F), (A,))
    last = np.full((m, A), np.nan, F) if prev is None else np.asarray(prev, F)
    last = np.broadcast_to(last[:, None, :], (m, n, A)).copy()
    pre = np.full((m, delay, A), np.nan, F) if prefix is None else np.asarray(prefix, F)
    cost = np.zeros((m, n, A), np.float64)
    lb, ub = F(lb), F(ub)
    for t in range(H):
        x = u[:, :, t]
        pin = np.broadcast_to(pre[:, None, t], (m, n, A)) if t < delay else np.full((m, n, A), np.nan, F)
        known = ~np.isnan(last)
        with np.errstate(invalid="ignore"):
            lim = clip(clip(x, (last - dl).astype(F), (last + dl).astype(F)), lb, ub)
        y = np.where(~np.isnan(pin), pin, np.where(np.isfinite(dl)[None, None] & known, lim, x)).astype(F)
        with np.errstate(invalid="ignore"):
            e = y.astype(np.float64) - last.astype(np.float64)
        cost += np.where(known, w.astype(np.float64) * e * e, 0.0)
        u[:, :, t] = y
        last = y
    return u, cost.sum(axis=-1), np.abs(cost).sum(axis=-1)


def cost_f32(actuated, rate_w, prev=None):
    """The kernel's cost chain emulated in float32 on ACTUATED sequences [m,n,H,A]: per dim c += w * ((y - last) * (y - last)), one
    rounding each, then ((c_0 + c_1) + c_2) + ... in ascending dim order."""
    y = np.asarray(actuated, F)
    m, n, H, A = y.shape
    w = np.broadcast_to(np.asarray(rate_w, F), (A,))
    last = np.full((m, A), np.nan, F) if prev is None else np.asarray(prev, F)
    last = np.broadcast_to(last[:, None, :], (m, n, A)).copy()
    c = np.zeros((m, n, A), F)
    for t in range(H):
        known = ~np.isnan(last)
        with np.errstate(invalid="ignore"):
            e = (y[:, :, t] - last).astype(F)
            sq = (e * e).astype(F)
            c = np.where(known, (c + (w * sq).astype(F)).astype(F), c)
        last = y[:, :, t]
    s = c[..., 0]
    for a in range(1, A):
        s = (s + c[..., a]).astype(F)
    return s


def bound(S, H, A):
    """|float32 cost - float64 cost| <= 2 (H + A + 2) 2^-24 S, S the sum of the terms' magnitudes (the terms are non-negative: S is the
    cost itself).  Counted as tests/test_gpu_tracking.py counts: one rounding each for the difference, the square and the product of a
    term w (y - last)^2, one per add -- H per dim's chain, each at most u = 2^-24 of a partial sum <= S_a, and A - 1 to combine the
    dims, each at most u S: (3 + H + A - 1) u S.  Doubled for slack: that covers the difference's rounding counting twice once it is
    squared (a first-order total of (H + A + 3) u S) and the second-order terms."""
    return 2.0 * (H + A + 2) * 2.0 ** -24 * np.asarray(S, np.float64)


def window_ok(plan, rate_limit, prev=None, lb=-1.0, ub=1.0, free=None):
    """The exact float32 check a feasible sequence passes at every step: last - delta <= y <= last + delta with the two bounds rounded
    once each, or y on the box bound the window lies beyond; steps whose `last` is NaN, dims without a limit and steps where `free`
    [m,H,A] is False (pinned) are not checked.  plan [m,H,A] -> bool [m,H,A]."""
    y = np.asarray(plan, F)
    m, H, A = y.shape
    dl = np.broadcast_to(np.asarray(rate_limit, F), (A,))
    last = np.concatenate([(np.full((m, 1, A), np.nan, F) if prev is None else np.asarray(prev, F)[:, None]), y[:, :-1]], axis=1)
    with np.errstate(invalid="ignore"):
        lo, hi = (last - dl).astype(F), (last + dl).astype(F)
        ok = ((y >= lo) & (y <= hi)) | ((y == F(ub)) & (lo > F(ub))) | ((y == F(lb)) & (hi < F(lb)))
    ok |= np.isnan(last) | ~np.isfinite(dl)[None, None]
    if free is not None:
        ok |= ~np.asarray(free, bool)
    return ok


def make_case(m, n, H, A, delay, seed=0, nan_env=None, outside=False):
    """(seqs [m,n,H,A] in [-1, 1], rate_limit [A] finite on even dims and +inf on odd ones, rate_w [A] zero on every third dim,
    prev [m,A], prefix [m,delay,A] with scattered NaNs).  nan_env: an env whose prev is all NaN; outside: env 0's prev lies outside
    the box."""
    rng = np.random.default_rng(seed)
    seqs = rng.uniform(-1.0, 1.0, (m, n, H, A)).astype(F)
    dl = np.where(np.arange(A) % 2 == 0, rng.uniform(0.05, 0.6, A), np.inf).astype(F)
    w = np.where(np.arange(A) % 3 == 0, 0.0, rng.uniform(0.1, 3.0, A)).astype(F)
    prev = rng.uniform(-1.0, 1.0, (m, A)).astype(F)
    if outside:
        prev[0] = np.where(np.arange(A) % 2 == 0, 1.75, -2.5).astype(F)
    if nan_env is not None:
        prev[nan_env] = np.nan
    prefix = rng.uniform(-1.0, 1.0, (m, delay, A)).astype(F)
    prefix[rng.uniform(size=prefix.shape) < 0.3] = np.nan
    return seqs, dl, w, prev, prefix
