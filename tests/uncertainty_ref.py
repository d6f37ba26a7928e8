"""Numpy restatement of the uncertainty cost of the opt-in planner (csrc/uncertainty.hip: cadm_uncertainty_cost) -- test infrastructure.

`cost` states the quantity in float64; `emulate32` walks the kernel's float32 chain operation for operation (include/cadm_hip.h,
"Pricing model uncertainty"); `bound` says how far the two may lie apart, derived, not measured:
  per variance          bv = 4 (p + 4) 2^-24 R^2,  R = max_j |x_j - x_0|      (tests/test_gpu_forecast.py's bound of this chain)
  per step, form var    B_t = sum_d w_d bv_d + (n_w + 1) 2^-24 u_t,  n_w the number of weighted dims (a product and an add per dim)
  per step, form std    min(B_t / sqrt(u_t), sqrt(B_t)) + 2^-24 sqrt(u_t)     (|sqrt a - sqrt b| <= |a - b| / sqrt b and <= sqrt |a - b|)
  cost                  sum_t B_t + H 2^-24 sum_t u_t  over the counted steps  (one rounding per add of the chain)
The cap is a minimum with a constant, which moves two numbers no further apart: the bounds hold with it."""
import numpy as np

F = np.float32
EPS = 2.0 ** -24
KINDS = ("epistemic", "total")
FORMS = ("var", "std")


def weights(w, D):
    """w (None, a number or [D]) as the float32 values the kernel multiplies by, [D]"""
    out = np.empty((D,), F)
    out[:] = 1.0 if w is None else np.asarray(w, F)
    return out


def counted(first, H, m, n):
    """[m,n,H] bool: step t counts iff t <= min_j first[mi,c,j] (every step without `first`)"""
    if first is None:
        return np.ones((m, n, H), bool)
    return np.arange(H)[None, None, :] <= np.asarray(first).min(axis=2)[:, :, None]


def variance(traj, E, kind):
    """v [m,n,H,D] float64: the biased variance over the particles ("total") or of the E member means ("epistemic")"""
    H, m, n, p, D = traj.shape
    x = np.transpose(traj.astype(F), (1, 2, 0, 3, 4)).astype(np.float64)      # [m,n,H,p,D]
    with np.errstate(all="ignore"):
        if kind == "total":
            return x.var(axis=3)
        return x.reshape(m, n, H, E, p // E, D).mean(axis=4).var(axis=3)


def cost(traj, E, kind, w=None, form="var", cap=None, first=None):
    """(step [m,n,H], cost [m,n], B [m,n,H], S [m,n]) in float64: the step costs, the cost over the counted steps, the bound of a
    step cost and the counted sum of the step costs (what `bound` scales the chain's roundings by).  Dims with w == 0 are not read; a
    step that is not counted contributes nothing, whatever it holds."""
    H, m, n, p, D = traj.shape
    w = weights(w, D).astype(np.float64)
    on = np.flatnonzero(w > 0)
    sub = np.ascontiguousarray(traj[..., on])
    v = variance(sub, E, kind)
    x = np.transpose(sub.astype(F), (1, 2, 0, 3, 4)).astype(np.float64)
    with np.errstate(all="ignore"):
        R = np.abs(x - x[:, :, :, :1]).max(axis=3)                               # [m,n,H,n_w]
        u = (v * w[on]).sum(axis=-1)
        B = (w[on] * 4 * (p + 4) * EPS * R * R).sum(axis=-1) + (len(on) + 1) * EPS * u
        if form == "std":
            s = np.sqrt(u)
            B = np.minimum(np.where(s > 0, B / np.where(s > 0, s, 1.0), np.inf), np.sqrt(B)) + EPS * s
            u = s
        if cap is not None:
            u = np.minimum(u, float(F(cap)))      # (np.minimum hands a NaN on)
    on_t = counted(first, H, m, n)
    return u, np.where(on_t, u, 0.0).sum(axis=2), B, np.where(on_t, np.abs(u), 0.0).sum(axis=2)


def bound(B, S, H, first=None):
    """the cost's bound [m,n] from `cost`'s B and S"""
    m, n, _ = B.shape
    return np.where(counted(first, H, m, n), B, 0.0).sum(axis=2) + H * EPS * S


def emulate32(traj, E, kind, w=None, form="var", cap=None, first=None):
    """(step [m,n,H], cost [m,n]) float32 by the kernel's chain: every operation rounded to float32, nothing fused, in its order"""
    H, m, n, p, D = traj.shape
    q = p // E
    w = weights(w, D)
    x = np.transpose(traj.astype(F), (1, 2, 0, 3, 4))                            # [m,n,H,p,D]
    x0 = x[:, :, :, 0]
    with np.errstate(all="ignore"):
        def member_sum(e):
            s = np.zeros(x0.shape, F)
            for j in range(q):
                s = s + (x[:, :, :, e * q + j] - x0)
            return s
        tot = np.zeros(x0.shape, F)
        for e in range(E):
            tot = tot + member_sum(e)
        md = tot / F(p)
        acc = np.zeros(x0.shape, F)
        if kind == "total":
            for j in range(p):
                dv = (x[:, :, :, j] - x0) - md
                acc = acc + dv * dv
            v = acc / F(p)
        else:
            for e in range(E):
                de = member_sum(e) / F(q) - md
                acc = acc + de * de
            v = acc / F(E)
        assert v.dtype == F
        u = None
        for d in range(D):
            if w[d] > 0:
                term = w[d] * v[..., d]
                u = term if u is None else u + term
        if form == "std":
            u = np.sqrt(u)
        if cap is not None:
            u = np.where(u > F(cap), F(cap), u)
        on_t = counted(first, H, m, n)
        c = np.zeros((m, n), F)
        for t in range(H):
            c = np.where(on_t[:, :, t], c + u[:, :, t], c)
    assert u.dtype == F and c.dtype == F
    return u, c


def make_w(style, D, seed=0):
    """broadcast: None; per-dim: U(0.2, 3) with every third dim 0; one-hot: a single 1"""
    rng = np.random.default_rng(seed)
    if style == "broadcast":
        return None
    if style == "per-dim":
        w = rng.uniform(0.2, 3.0, D).astype(F)
        w[::3] = 0.0
        return w
    w = np.zeros((D,), F)
    w[int(style.split("-")[-1]) % D] = 1.0
    return w
