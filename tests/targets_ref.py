"""numpy restatement of csrc/imagine_targets.hip (include/cadm_hip.h "Value-expansion targets"), operation for operation, with the
dtype as a parameter: float32 is the kernel's twin (every numpy operation on float32 arrays is rounded on its own, and numpy's float32
division is correctly rounded, as `__fdiv_rn` is), float64 the yardstick.  The parameters are rounded to float32 first in either case,
as the library receives them.  Rows are vectorised; the chains along t, h and j are loops in the kernel's order."""
import numpy as np


def _prm(v, T):
    return T(np.float32(v))


def make_inputs(m, n, k, seed, plant=True):
    """Seeded inputs [k,m,n] / [k+1,m,n] of the issue's generator -- rewards ~ N(0, 3), bootstraps ~ N(0, 30), disagreement ~ |N(0, 1)|, a
    third of the rows ended early, half of those terminated -- as float32 / uint8 arrays the way `imagine` lays them out."""
    rng = np.random.default_rng(seed)
    rew = (3.0 * rng.standard_normal((k, m, n))).astype(np.float32)
    boot = (30.0 * rng.standard_normal((k + 1, m, n))).astype(np.float32)
    dis = np.abs(rng.standard_normal((k, m, n))).astype(np.float32)
    end = np.where(rng.random((m, n)) < 1.0 / 3.0, rng.integers(0, k + 1, (m, n)), k)          # the valid steps of a row
    term = (rng.random((m, n)) < 0.5) & (end < k) & (end >= 1)
    t = np.arange(k)[:, None, None]
    valid = (t < end[None]).astype(np.uint8)
    done = ((t == end[None] - 1) & term[None]).astype(np.uint8)
    rew = np.where(valid > 0, rew, np.float32(0)).astype(np.float32)                            # imagine: rew 0 and u 0 behind a row's end
    dis = np.where(valid > 0, dis, np.float32(0)).astype(np.float32)
    return dict(rew=rew, valid=valid, done=done, disagreement=dis, boot=boot)


def targets(rew, valid, done, disagreement, boot, gamma, lam=0.95, penalty=0.0, max_disagreement=None, var_floor=None, dtype=np.float32):
    """-> dict of lambda_return, nstep [k,m,n] `dtype`, nstep_ok, used [k,m,n] uint8, L [m,n], term [m,n] and, with var_floor, steve [m],
    steve_weight, steve_mean, steve_var [k,m] `dtype`, steve_count [k,m] int32, steve_fallback [m] uint8."""
    T = dtype
    rew, dis, boot = np.asarray(rew, T), np.asarray(disagreement, T), np.asarray(boot, T)
    valid, done = np.asarray(valid) != 0, np.asarray(done) != 0
    k, m, n = rew.shape
    assert boot.shape == (k + 1, m, n) and valid.shape == done.shape == dis.shape == rew.shape
    g, l_, beta = _prm(gamma, T), _prm(lam, T), _prm(penalty, T)
    oml = T(np.float32(1.0) - np.float32(lam))            # 1.0f - lambda, computed once in float32 on the host
    maxd = T(np.inf) if max_disagreement is None else _prm(max_disagreement, T)
    zero = np.zeros((m, n), T)
    with np.errstate(all="ignore"):
        alive = np.ones((m, n), bool)
        L = np.zeros((m, n), np.int64)
        for t in range(k):
            alive = alive & valid[t] & ~(dis[t] > maxd)
            L += alive
        ii, jj = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
        term = (L >= 1) & done[np.maximum(L - 1, 0), ii, jj]
        rt = rew if beta == 0 else rew - beta * dis
        # the n-step targets of the start state
        nstep, ok, used = np.zeros((k, m, n), T), np.zeros((k, m, n), np.uint8), np.zeros((k, m, n), np.uint8)
        acc, disc, x = zero.copy(), T(1), zero.copy()
        for h in range(1, k + 1):
            live = h <= L
            acc = np.where(live, acc + disc * rt[h - 1], acc)
            disc = disc * g
            x = np.where(live, np.where((h == L) & term, acc, acc + disc * boot[h]), x)
            good = (live | term) & np.isfinite(x)
            nstep[h - 1] = np.where(good, x, T(0))
            ok[h - 1] = good
            used[h - 1] = live
        # the lambda-return of every used step
        lam_ret, G = np.zeros((k, m, n), T), zero.copy()
        for t in range(k - 1, -1, -1):
            last = np.where(term, rt[t], rt[t] + g * boot[t + 1])
            inner = rt[t] + g * (oml * boot[t + 1] + l_ * G)
            G = np.where(t == L - 1, last, np.where(t < L - 1, inner, G))
            lam_ret[t] = np.where(t < L, G, T(0))
        out = dict(lambda_return=lam_ret, nstep=nstep, nstep_ok=ok, used=used, L=L, term=term)
        if var_floor is None:
            return out
        floor = _prm(var_floor, T)
        mean, var = np.zeros((k, m), T), np.zeros((k, m), T)
        count, w = np.zeros((k, m), np.int32), np.zeros((k, m), T)
        for h in range(k):
            c, s = np.zeros((m,), np.int32), np.zeros((m,), T)
            for j in range(n):
                o = ok[h, :, j] > 0
                c = c + o
                s = np.where(o, s + nstep[h, :, j], s)
            cf = np.maximum(c, 1).astype(T)
            mu = np.where(c > 0, s / cf, T(0))
            ss = np.zeros((m,), T)
            for j in range(n):
                d = nstep[h, :, j] - mu
                ss = np.where(ok[h, :, j] > 0, ss + d * d, ss)
            va = np.where(c > 0, ss / cf, T(0))
            mean[h], var[h], count[h] = mu, va, c
            w[h] = np.where(c >= 2, T(1) / (va + floor), T(0))
        W, S = np.zeros((m,), T), np.zeros((m,), T)
        for h in range(k):
            W = W + w[h]
            S = S + w[h] * mean[h]
        any_ = W > 0
        Wd = np.where(any_, W, T(1))
        out.update(steve=np.where(any_, S / Wd, boot[0, :, 0]).astype(T), steve_weight=np.where(any_[None], w / Wd[None], T(0)).astype(T),
                   steve_mean=mean, steve_var=var, steve_count=count, steve_fallback=(~any_).astype(np.uint8))
    return out


# ---------------------------------------------------------------------------------------------------------------------- the kernel's shapes
# What tests/test_gpu_imagine_targets.py launches and tests/test_targets_ref.py shows, on the CPU, to reach every branch of the arithmetic.
THREADS, LDS_BUDGET = 256, 48 * 1024      # csrc/imagine_targets.hip TGT_THREADS, TGT_LDS_BUDGET


def lds_bytes(G, n, k):
    """csrc/imagine_targets.hip tgt_lds_bytes: a tile of G n k floats and as many flag bytes, padded to 4 elements, and 2 G k floats"""
    tile = (G * n * k + 3) & ~3
    return 4 * tile + tile + 2 * G * k * 4


def group(m, n, k):
    """csrc/imagine_targets.hip tgt_group: the start states a workgroup of the STEVE form owns -- as many as give it 256 rows, at least
    one, at most m, fewer where the tile would not fit 48 KiB (0: not even one's)"""
    G = min(max(THREADS // n, 1), m)
    while G > 0 and lds_bytes(G, n, k) > LDS_BUDGET:
        G -= 1
    return G


# (m, n, k, with the STEVE outputs) -> the group the host takes, the start states of its workgroups
SHAPES = [(1, 2, 1, True), (3, 4, 5, True), (17, 3, 7, True), (2, 33, 4, True), (5, 2, 64, True), (130, 3, 2, True), (300, 1, 3, False),
          (1, 700, 20, False),
          (20, 16, 64, True),      # G = 8, cut from 16 by the budget: cap = G n = 128 under a cut G; groups of 8, 8, 4
          (9, 100, 20, True),      # G = 2: cap = 200, a partial last group of 1
          (3, 300, 4, True)]       # G = 1, n > 256: the row loop's second pass while it writes the tile
GROUPS = {(20, 16, 64): (8, [8, 8, 4]), (9, 100, 20): (2, [2, 2, 2, 2, 1]), (3, 300, 4): (1, [1, 1, 1])}
# gamma, lam, penalty, max_disagreement: no penalty and no bound (a +inf disagreement is used and never multiplied); both; a bound alone
MAXD, FLOOR = 1.5, 1e-2
CONFIGS = [(0.97, 0.9, 0.0, None), (0.99, 0.5, 0.7, MAXD), (1.0, 1.0, 0.0, MAXD)]
N_FEATURES = 7


def plant_row(x, f, i, j, k):
    """one special case on row (i, j); the row is fully valid with small disagreements unless the case says otherwise"""
    x["valid"][:, i, j], x["done"][:, i, j] = 1, 0
    x["disagreement"][:, i, j] = np.minimum(x["disagreement"][:, i, j], np.float32(1.0))
    e = max(1, k // 2)
    if f == 0:                                    # L = 0
        x["valid"][:, i, j] = 0
    elif f == 1:                                  # L = k
        pass
    elif f == 2:                                  # terminated at the last used step
        x["valid"][e:, i, j] = 0
        x["done"][e - 1, i, j] = 1
    elif f == 3:                                  # diverged: the row ends without a done
        x["valid"][k // 2:, i, j] = 0
    elif f == 4:                                  # cut by max_disagreement at the last step
        x["disagreement"][k - 1, i, j] = 3.0
    elif f == 5:                                  # a +inf disagreement
        x["disagreement"][k // 2, i, j] = np.inf
    elif f == 6:                                  # a NaN bootstrap behind the start state
        x["boot"][1:, i, j] = np.nan


def variant(m, n, k, v):
    """variant v of the seeded inputs of a shape: row r carries special case (v + r) % 7, so over 7 variants every case lands on row 0 of
    even the smallest shape; in variants 7 and 8 the last start state keeps one live branch (no horizon has two targets: the fallback),
    or one full and one diverged branch (the longer horizons have one target: weight 0)"""
    x = make_inputs(m, n, k, 100 * v + m + n + k)
    for r in range(min(m * n, N_FEATURES)):
        plant_row(x, (v + r) % N_FEATURES, r // n, r % n, k)
    if v >= 7 and n >= 2:
        i = m - 1
        x["valid"][:, i, :], x["done"][:, i, :] = 0, 0
        plant_row(x, 1, i, 0, k)
        if v == 8:
            plant_row(x, 3, i, 1, k)
    return x


def branches(x, cfg, want, steve):
    """the branches of the arithmetic that occurred on inputs x under cfg, read off the restatement's outputs `want`, as a set of names;
    asserts what holds on every input: no NaN target without a NaN bootstrap, no n-step target from one"""
    k, m, n = x["rew"].shape
    L, term, valid = want["L"], want["term"], x["valid"]
    ii, jj = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    nxt = valid[np.minimum(L, k - 1), ii, jj] > 0                 # is the step behind the used ones a valid one?
    seen = {name for name, hit in (
        ("L=0", (L == 0).any()), ("L=k", (L == k).any()), ("terminated", (term & (L >= 1)).any()),
        ("diverged", ((L < k) & ~term & ~nxt).any()), ("truncated", ((L < k) & nxt).any()),
        ("inf-unpenalised", cfg[2] == 0.0 and (np.isinf(x["disagreement"]) & (want["used"] > 0)).any()),
        ("nan-boot", np.isnan(want["lambda_return"]).any())) if hit}
    nan_rows = np.isnan(x["boot"]).any(axis=0)
    assert not np.isnan(want["lambda_return"][:, ~nan_rows]).any() and not np.isnan(want["nstep"]).any()
    assert (want["nstep_ok"][:, nan_rows & (L == k) & ~term] == 0).all()
    if steve:
        w, cnt = want["steve_weight"], want["steve_count"]
        if ((w == 0) & (cnt < 2) & (w.sum(axis=0) > 0)[None]).any():
            seen.add("weight-0")
        if want["steve_fallback"].any():
            seen.add("fallback")
    return seen


def needed(k, steve):
    """the branches a shape must show over its variants and configs"""
    need = {"L=0", "L=k", "terminated", "diverged", "truncated", "inf-unpenalised", "nan-boot"}
    if steve:
        need |= {"fallback"} | ({"weight-0"} if k >= 2 else set())
    return need
