"""Calibration statistics of the particles (csrc/calibration.hip), restated on the host -- test infrastructure shared by
tests/test_calibration_ref.py (CPU) and tests/test_gpu_calibration.py.

stats64            the statistics in float64; every comparison (ranks, ties, degenerate) on the float32 values, so the integers are exact
kernel_bound       the per-entry absolute bar of crps / z2 / nll against stats64, from the kernel header's rounding chains and fp64 magnitudes
ROWS, WT           the rows of horizon_ref.SHAPES the kernel test runs, and this kernel's tile width on each

WT is worked out by hand from the kernel header's LDS rule -- WT (4 D (p + 3) + 8) + D (2 p + E + 1) + 8 D + 32 <= 49152, WT the
largest power of two <= 16 -- and is never taken from the code under test:
    row 0   p  20 E 5 D 45:   4148 B / window + 2462;   8 x = 35646 (16 x = 68830 does not fit)
    row 3   p 130 E 5 D 45:  23948 B / window + 12362;  1 x = 36310 (2 x = 60258 does not fit)
    rows 5, 6, 7, 8, 10: at most 1352 B / window + 1040: 16 x fits."""
import numpy as np

from horizon_ref import SHAPES, U, make_mask, row_inputs  # noqa: F401  (re-exported to the tests)

ROWS = (0, 3, 5, 6, 7, 8, 10)
WT = {0: 8, 3: 1, 5: 16, 6: 16, 7: 16, 8: 16, 10: 16}
INTS = ("rank_hist", "rank_hist_member", "ties", "degenerate", "count", "diverged")
SUMS = ("crps", "z2", "nll")
LOGF_ULP = 2           # OCML documents logf at 1 ulp; the bar assumes 2 (an ulp is at most 2 u relative)
LOG_2PI = float(np.log(2.0 * np.pi))


def gamma(n):
    """n roundings compounded: n u / (1 - n u)"""
    return n * U / (1.0 - n * U)


def _terms(traj, truth, mask, e):
    """Per (step, window, dim), in float64 from the float32 inputs: what stats64 sums and kernel_bound weighs."""
    f, m, p, d = traj.shape
    valid = (np.cumprod(mask != 0, axis=1) > 0).T                                  # [F,m] prefix rule
    finite = np.isfinite(traj).all(axis=(2, 3))
    x32 = np.where(np.isfinite(traj), traj, np.float32(0)).astype(np.float32)
    y32 = np.ascontiguousarray(np.transpose(truth.astype(np.float32), (1, 0, 2)))  # [F,m,D]
    x, y = x32.astype(np.float64), y32.astype(np.float64)
    xs = np.sort(x, axis=2)
    w = (2.0 * np.arange(p) - p + 1.0)[None, None, :, None]
    t = dict(use=valid & finite, diverged=valid & ~finite, x32=x32, y32=y32, x=x, y=y)
    t["a"] = np.abs(x - y[:, :, None, :]).mean(2)                                  # (1/p) sum |x_j - y|
    t["b"] = np.maximum((w * xs).sum(2), 0.0) / float(p * p)                      # (1/(2 p^2)) sum_j sum_k |x_j - x_k|, via the order statistics
    t["xbar"], t["v"] = x.mean(2), x.var(2)
    t["deg"] = x32.max(2) == x32.min(2)                                            # biased variance exactly 0: the particles coincide
    return t


def stats64(traj, truth, mask, e):
    """traj [F,m,p,D], truth [m,F,D], mask [m,F] (float32) -> the kernel's sums and counts: integers exact, floats in float64."""
    f, m, p, d = traj.shape
    pe = p // e
    t = _terms(traj, truth, mask, e)
    use = t["use"][:, :, None]                                                     # [F,m,1]
    rank = (t["x32"] < t["y32"][:, :, None, :]).sum(2)                             # [F,m,D]
    rank_m = (t["x32"].reshape(f, m, e, pe, d) < t["y32"][:, :, None, None, :]).sum(3)      # [F,m,E,D]
    hist = np.stack([(use & (rank == r)).sum(1) for r in range(p + 1)], axis=-1)   # [F,D,p+1]
    hist_m = np.stack([(use[..., None] & (rank_m == r)).sum(1) for r in range(pe + 1)], axis=-1)       # [F,E,D,pe+1]
    tie = (t["x32"] == t["y32"][:, :, None, :]).any(2)
    live = use & ~t["deg"]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(live, (t["xbar"] - t["y"]) ** 2 / t["v"], 0.0)
        nl = np.where(live, 0.5 * (LOG_2PI + np.log(t["v"]) + z), 0.0)
    return dict(rank_hist=hist, rank_hist_member=np.transpose(hist_m, (1, 0, 2, 3)), ties=(use & tie).sum(1), degenerate=(use & t["deg"]).sum(1),
                crps=(use * (t["a"] - t["b"])).sum(1), z2=z.sum(1), nll=nl.sum(1), count=t["use"].sum(1), diverged=t["diverged"].sum(1))


def kernel_bound(traj, truth, mask, e, wt):
    """Per-entry absolute bar of the kernel's crps / z2 / nll sums against stats64, first order in u with the chains compounded
    (gamma), every magnitude from float64 -- nothing here comes from a measured error.  Per counted window, from the kernel header:
        A = (1/p) sum |x_j - y|            p + 2 roundings of non-negative terms:           dA = gamma(p + 2) A
        B = pair term                      2 p + 1:                                         dB = gamma(2 p + 1) B
        crps_i = A - B                     dA + dB + u (A + B): the bar scales with A + B, the ABSOLUTE terms, not with their difference
        xbar - y                           the member sums, the total and the division leave md = mean(x_j - x0) with
                                           em = gamma(p / E + E + 2) mean |x_j - x0|; x0 + md and - y round once more each:
                                           delta = em + u |xbar| + u |xbar - y|
        v                                  every deviation dv_j = (x_j - x0) - md is off by eta_j = u |x_j - x0| + u |dv_j| + em;
                                           the square, p adds and the division: dv = mean(2 |dv_j| eta_j + eta_j^2) + gamma(p + 2) v
        z2_i = (xbar - y)^2 / v            at most zhi = (|xbar - y| + delta)^2 / (v - dv) (1 + gamma(3)) (the upper deviation is the larger
                                           one): dz = zhi - z2_i; infinite where dv reaches v (no such window in the tests)
        nll_i = 0.5 ((log 2 pi + log v) + z2_i)   logf: LOGF_ULP ulp = 2 LOGF_ULP u |log v|, plus what dv does to it, - log(1 - dv / v);
                                           two adds of terms of either sign, u (|log 2 pi + log v| + |log 2 pi + log v| + zhi); the halving is exact:
                                           dn = 0.5 (all of that + dz)
    Over the windows the running sum rounds acc = 64 / WT + WT + (blocks - 1) times, each time by at most u x the sum of the ABSOLUTE
    computed terms (nll's change sign): bar = sum_i d_i + gamma(acc) sum_i (|term_i| + d_i)."""
    f, m, p, d = traj.shape
    pe = p // e
    t = _terms(traj, truth, mask, e)
    use = t["use"][:, :, None]
    live = use & ~t["deg"]
    acc = gamma(64 // wt + wt + (m + 63) // 64 - 1)
    a, b, x, y = t["a"], t["b"], t["x"], t["y"]
    dc = gamma(p + 2) * a + gamma(2 * p + 1) * b + U * (a + b)
    crps = (use * (dc + acc * (np.abs(a - b) + dc))).sum(1)
    x0 = x[:, :, :1]
    dt = np.abs(t["xbar"] - y)
    em = gamma(pe + e + 2) * np.abs(x - x0).mean(2)
    delta = em + U * np.abs(t["xbar"]) + U * dt
    dev = np.abs(x - t["xbar"][:, :, None, :])
    eta = U * np.abs(x - x0) + U * dev + em[:, :, None, :]
    v = t["v"]
    dv = (2 * dev * eta + eta ** 2).mean(2) + gamma(p + 2) * v
    with np.errstate(divide="ignore", invalid="ignore"):
        room = np.where(live & (v > dv), v - dv, np.nan)                           # NaN -> an infinite bar below
        z = dt ** 2 / v
        zhi = (dt + delta) ** 2 / room * (1 + gamma(3))
        dz = zhi - z
        lv = LOG_2PI + np.log(v)
        dn = 0.5 * (2 * LOGF_ULP * U * np.abs(np.log(v)) - np.log1p(-dv / v) + U * (2 * np.abs(lv) + zhi) + dz)
        nl = np.abs(0.5 * (lv + z))
        zb = np.where(live, np.nan_to_num(dz + acc * zhi, nan=np.inf), 0.0).sum(1)
        nb = np.where(live, np.nan_to_num(dn + acc * (nl + dn), nan=np.inf), 0.0).sum(1)
    return dict(crps=crps, z2=zb, nll=nb)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over crps, z2 and nll; an entry whose bound is 0 must be exact."""
    worst = 0.0
    for k in SUMS:
        diff = np.abs(got[k].astype(np.float64) - ref[k])
        zero = bound[k] == 0
        assert (diff[zero] == 0).all(), "%s: an entry with bound 0 is not exact" % k
        if (~zero).any():
            worst = max(worst, float((diff[~zero] / bound[k][~zero]).max()))
    return worst
