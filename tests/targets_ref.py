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
