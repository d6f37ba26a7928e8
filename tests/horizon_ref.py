"""Open-loop prediction error along the horizon (csrc/horizon.hip), restated on the host -- test infrastructure shared by
tests/test_horizon_ref.py (CPU), tests/test_gpu_horizon.py, tests/test_gpu_horizon_envelope.py and tests/test_gpu_context_stats.py.

stats64            the statistics in float64 (what every kernel test compares with)
restate32          the kernel's documented reduction order in numpy float32 (the CPU test's stand-in for the kernel)
kernel_bound       the per-entry absolute bar of the statistics kernel against stats64
oracle_bound       the project's 1e-5 trajectory bar propagated through the statistics (the composite against the oracle's trajectory)
SHAPES             the statistics kernel's tile widths and edges, one row each

The WT column of SHAPES is worked out by hand from the kernel's LDS budget -- 4 D (p + 2 + E) + 16 bytes per window, WT windows
+ 32 bytes within 48 KiB, WT the largest power of two <= 16 -- and is never taken from the code under test:
    p  20 D 45:   4876 B / window,  8 x = 39008 (16 x = 78016 does not fit)
    p  60 D 45:  12076 B,           4 x = 48304 (+ 32 = 48336 <= 49152)
    p  80 D 64:  22288 B,           2 x = 44576
    p 130 D 45:  24676 B,           2 x = 49352 does not fit: 1
    p 180 D 64:  47888 B,           1 x + 32 = 47920;  p = 185: 49168 B does not fit at all
    every other row: below 3072 B / window, 16 x fits."""
import numpy as np

E, RTOL = 5, 4e-6      # the ensemble of the model tests; a statistic is a chain of fewer than 64 fp32 roundings of non-negative terms: 64 * 2^-24
U = 2.0 ** -24         # fp32 unit roundoff

SHAPES = [   # p, E, D, m, F, WT, mask ("mixed": make_mask; "valid": all windows valid), what the row reaches
    dict(p=20, E=5, D=45, m=150, F=2, WT=8, mask="mixed", what="slim humanoid at the reference's p"),
    dict(p=60, E=5, D=45, m=130, F=2, WT=4, mask="mixed", what="16 tile rounds per block; ragged last tile of 2"),
    dict(p=80, E=5, D=64, m=70, F=2, WT=2, mask="mixed", what="D at its limit"),
    dict(p=130, E=5, D=45, m=70, F=2, WT=1, mask="mixed", what="64 rounds; pD = 5850 = 2 (mod 4): tiles alternate aligned / unaligned"),
    dict(p=180, E=5, D=64, m=3, F=1, WT=1, mask="valid", what="last p that fits at D = 64"),
    dict(p=1, E=1, D=3, m=131, F=3, WT=16, mask="mixed", what="cfg1-like: spread exactly 0, se_member[0] bitwise se"),
    dict(p=5, E=5, D=1, m=65, F=3, WT=16, mask="mixed", what="PE = 1, D = 1, pD odd"),
    dict(p=9, E=9, D=28, m=63, F=2, WT=16, mask="mixed", what="E > 8; one block short of full"),
    dict(p=6, E=2, D=4, m=641, F=2, WT=16, mask="mixed", what="11 blocks: stage 2's chain"),
    dict(p=12, E=3, D=17, m=5, F=100, WT=16, mask="valid", what="m < WT; grid.y = 100"),
    dict(p=10, E=5, D=18, m=1, F=4, WT=16, mask="valid", what="one window"),
]
INVARIANT_ROWS = (1, 3, 4, 5, 7)      # WT = 4, WT = 1 (both), p = 1, E = 9: the bitwise invariants run on these
NONFINITE_ROWS = (3, 6)               # WT = 1 and p = 5, D = 1: non-finite values on every load path
IDS = ["p%d-E%d-D%d-m%d-F%d-WT%d" % (r["p"], r["E"], r["D"], r["m"], r["F"], r["WT"]) for r in SHAPES]


def make_mask(n, f):
    """All-valid windows, prefixes of every length, window 5 all-invalid, window 9 with a hole (its last step but one: (1, 1, 0, 1) at
    f = 4, (1, 0, 1) at f = 3, (0, 1) at f = 2) -- each wherever n and f allow."""
    mask = np.ones((n, f), np.float32)
    for i in range(20, n, 3):
        mask[i, (i // 3) % f + 1:] = 0.0
    if n > 5:
        mask[5] = 0.0
    if n > 9 and f >= 2:
        mask[9] = 1.0
        mask[9, f - 2] = 0.0
    return mask


def row_mask(row):
    return make_mask(row["m"], row["F"]) if row["mask"] == "mixed" else np.ones((row["m"], row["F"]), np.float32)


def row_inputs(row, seed=3):
    """(traj [F,m,p,D], truth [m,F,D]) float32: traj normal x per-dim scale in [0.5, 3] + per-dim offset of order 1, truth independent
    normal x 2 (tests/test_gpu_horizon.py's test_statistics_kernel_odd_dim): no entry of a statistic is a difference of nearly equal
    numbers by design, though a single window's mean may land near its truth."""
    f, m, p, d = row["F"], row["m"], row["p"], row["D"]
    rng = np.random.default_rng(seed)
    traj = (rng.standard_normal((f, m, p, d)) * rng.uniform(0.5, 3.0, d) + rng.standard_normal(d)).astype(np.float32)
    truth = (rng.standard_normal((m, f, d)) * 2.0).astype(np.float32)
    return traj, truth


def chain(row):
    """The kernel header's own count of fp32 roundings behind a statistic: p / E + E + 7 + 64 / WT + WT + (blocks - 1)."""
    return row["p"] // row["E"] + row["E"] + 7 + 64 // row["WT"] + row["WT"] + ((row["m"] + 63) // 64 - 1)


def stats64(traj, truth, mask, e):
    """The statistics restated in float64: traj [F,m,p,D], truth [m,F,D], mask [m,F] -> sums and counts."""
    f, m, p, d = traj.shape
    valid = (np.cumprod(mask != 0, axis=1) > 0).T                                  # [F,m] prefix rule
    finite = np.isfinite(traj).all(axis=(2, 3))
    use = valid & finite
    x = np.where(np.isfinite(traj), traj, 0.0).astype(np.float64)
    y = np.transpose(truth.astype(np.float64), (1, 0, 2))                          # [F,m,D]
    mem = x.reshape(f, m, e, p // e, d).mean(3)                                    # [F,m,E,D]
    u = use[:, :, None]
    return dict(se=(u * (x.mean(2) - y) ** 2).sum(1), spread=(u * x.var(2)).sum(1),
                se_member=np.transpose((u[..., None] * (mem - y[:, :, None, :]) ** 2).sum(1), (1, 0, 2)),
                count=use.sum(1), diverged=(valid & ~finite).sum(1))


def kernel_bound(traj, truth, mask, e, chain):
    """Per-entry absolute bar of the statistics kernel against stats64.  A purely relative bar is wrong where few windows are counted:
    a window whose mean lands near its truth contributes (xbar - y)^2 from a difference that cancelled, and the rounding of xbar and
    of the subtraction -- delta = 3 u (max_j |x_j| + |y|) per (step, window, dim) -- does not shrink with it.  With ref = stats64:
        se         chain u ref + sum over the counted windows of 2 |xbar - y| delta + delta^2      (se_member: per member, its own particles)
        spread     chain u ref      (its terms are differences relative to particle 0: nothing cancels against the truth)
    `chain`: the kernel header's count of roundings (chain(row))."""
    f, m, p, d = traj.shape
    ref = stats64(traj, truth, mask, e)
    use = ((np.cumprod(mask != 0, axis=1) > 0).T & np.isfinite(traj).all(axis=(2, 3)))[:, :, None]          # [F,m,1]
    x = np.where(np.isfinite(traj), traj, 0.0).astype(np.float64)
    y = np.transpose(truth.astype(np.float64), (1, 0, 2))
    dl = 3 * U * (np.abs(x).max(2) + np.abs(y))
    se = chain * U * ref["se"] + (use * (2 * np.abs(x.mean(2) - y) * dl + dl ** 2)).sum(1)
    xm = x.reshape(f, m, e, p // e, d)
    ym = y[:, :, None, :]
    dm = 3 * U * (np.abs(xm).max(3) + np.abs(ym))
    sem = chain * U * ref["se_member"] + np.transpose((use[..., None] * (2 * np.abs(xm.mean(3) - ym) * dm + dm ** 2)).sum(1), (1, 0, 2))
    return dict(se=se, spread=chain * U * ref["spread"], se_member=sem)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over se, spread and se_member; an entry whose bound is 0 must be exact."""
    worst = 0.0
    for k in ("se", "spread", "se_member"):
        diff = np.abs(got[k].astype(np.float64) - ref[k])
        zero = bound[k] == 0
        assert (diff[zero] == 0).all(), "%s: an entry with bound 0 is not exact" % k
        if (~zero).any():
            worst = max(worst, float((diff[~zero] / bound[k][~zero]).max()))
    return worst


def restate32(traj, truth, mask, e, wt):
    """The kernel's documented order in numpy float32: everything relative to particle 0; members, then the total; the variance in a
    second pass; window w adds into slot w % WT in window order; slots added in slot order; blocks of 64 windows added in block order.
    (No fused multiply-add, numpy's division: the kernel's own roundings differ from these by less than the bar, not by nothing.)"""
    f32 = np.float32
    f, m, p, d = traj.shape
    pe = p // e
    valid = (np.cumprod(mask != 0, axis=1) > 0).T
    finite = np.isfinite(traj).all(axis=(2, 3))
    use = valid & finite
    x = np.where(np.isfinite(traj), traj, 0.0).astype(f32)
    y = np.transpose(truth.astype(f32), (1, 0, 2))
    x0 = x[:, :, 0]
    tot = np.zeros((f, m, d), f32)
    terms = np.zeros((f, m, 2 + e, d), f32)                  # per window: se, spread, se_member[e]
    for k in range(e):
        s = np.zeros((f, m, d), f32)
        for j in range(pe):
            s = s + (x[:, :, k * pe + j] - x0)
        tot = tot + s
        dm = (x0 + s / f32(pe)) - y
        terms[:, :, 2 + k] = dm * dm
    md = tot / f32(p)
    var = np.zeros((f, m, d), f32)
    for j in range(p):
        dv = (x[:, :, j] - x0) - md
        var = var + dv * dv
    dt = (x0 + md) - y
    terms[:, :, 0] = dt * dt
    terms[:, :, 1] = var / f32(p)
    total = np.zeros((f, 2 + e, d), f32)
    for b0 in range(0, m, 64):
        acc = np.zeros((wt, f, 2 + e, d), f32)
        for w in range(b0, min(b0 + 64, m)):
            sel = use[:, w][:, None, None]
            acc[w % wt] = np.where(sel, acc[w % wt] + terms[:, w], acc[w % wt])
        part = np.zeros((f, 2 + e, d), f32)
        for slot in range(wt):
            part = part + acc[slot]
        total = total + part
    assert total.dtype == f32
    return dict(se=total[:, 0], spread=total[:, 1], se_member=np.transpose(total[:, 2:], (1, 0, 2)), count=use.sum(1),
                diverged=(valid & ~finite).sum(1))


def oracle_bound(t_ref, truth, mask, e):
    """The project's trajectory bar (helpers.assert_close: every value within delta = 1e-5 * max(|x_ref|, rms(x_ref[h]))) propagated
    through the statistics, per entry, from the oracle's values: a mean of values moves by at most the mean of their deltas, so
        |d se| <= sum_i 2 |xbar_i - y_i| dbar_i + dbar_i^2          (likewise per member)
        |d var_i| <= 1/p sum_j 2 |x_ij - xbar_i| (d_ij + dbar_i) + (d_ij + dbar_i)^2
    plus the kernel's own rounding (RTOL of the statistic, test 1)."""
    f, m, p, d = t_ref.shape
    x = t_ref.astype(np.float64)
    rms = np.sqrt((x ** 2).mean(axis=(1, 2, 3), keepdims=True))
    dl = 1e-5 * np.maximum(np.abs(x), rms)
    y = np.transpose(truth.astype(np.float64), (1, 0, 2))
    u = ((np.cumprod(mask != 0, axis=1) > 0).T)[:, :, None]
    xb, db = x.mean(2), dl.mean(2)
    se = (u * (2 * np.abs(xb - y) * db + db ** 2)).sum(1)
    dj = dl + db[:, :, None, :]
    spread = (u * (2 * np.abs(x - xb[:, :, None, :]) * dj + dj ** 2).mean(2)).sum(1)
    xm, dm = x.reshape(f, m, e, p // e, d).mean(3), dl.reshape(f, m, e, p // e, d).mean(3)
    sem = np.transpose((u[..., None] * (2 * np.abs(xm - y[:, :, None, :]) * dm + dm ** 2)).sum(1), (1, 0, 2))
    return dict(se=se, spread=spread, se_member=sem)


def check_against_oracle(case, comp, what, e=E):
    ref = stats64(case.t_ref, case.truth, case.mask, e)
    bound = oracle_bound(case.t_ref, case.truth, case.mask, e)
    np.testing.assert_array_equal(comp["count"], ref["count"])
    assert comp["diverged"].sum() == 0
    for k in ("se", "spread", "se_member"):
        lim = bound[k] + RTOL * np.abs(ref[k])
        diff = np.abs(comp[k] - ref[k])
        print("%s %s: worst |diff| / bound %.3f (worst relative %.2e)" % (what, k, (diff / lim).max(), (diff / np.abs(ref[k])).max()))
        assert (diff <= lim).all(), "%s %s: %d entries outside the propagated trajectory bar, worst |diff| / bound %.3f" % (
            what, k, (diff > lim).sum(), (diff / lim).max())
