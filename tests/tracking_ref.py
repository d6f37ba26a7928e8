"""Numpy restatement of the planner's run-time tracking targets (cadm_amd/csrc/tracking.hip, `cadm_tracking_returns`) -- test
infrastructure, in float64, one obvious loop nest.

terms: a list of dict(dim=d, kind="square" | "abs" | "huber", w=..., delta=...) (kind defaults to "square", w to 1); w and delta are
rounded to float32 first, as the library receives them.  Step t of env mi is compared with targets[mi, clamp(offset[mi] + t, 0, T - 1), k];
a NaN target skips its (step, term); with `first`, steps t > first[row] are not counted.  A row with nothing counted keeps its input
value (the caller compares its bits).  Also returned: S, the per-row sum of |w c| over the counted (step, term) pairs, the scale of the
float32 chain's rounding error, and `counted`, how many pairs that were."""
import numpy as np


def cost_term(kind, e, delta):
    """c(e) of one term, float64"""
    if kind == "square":
        return e * e
    if kind == "abs":
        return np.abs(e)
    ae = np.abs(e)
    return np.where(ae <= delta, 0.5 * e * e, delta * (ae - 0.5 * delta))


def target_rows(T, H, offset):
    """[H] the row of an env's reference every step is held against"""
    return np.clip(int(offset) + np.arange(H), 0, T - 1)


def tracking(traj, rows, terms, targets, offset=None, first=None):
    """traj [H,m,n,p,D], rows [m,n,p], targets [m,T,K] (or [m,K]) -> (rows' float64 [m,n,p], cost float64, S float64, counted int [m,n,p])"""
    H, m, n, p, _ = traj.shape
    targets = np.asarray(targets, np.float32)
    if targets.ndim == 2:
        targets = targets[:, None]
    T = targets.shape[1]
    offset = np.zeros(m, np.int64) if offset is None else np.asarray(offset, np.int64)
    cost, S, counted = np.zeros((m, n, p)), np.zeros((m, n, p)), np.zeros((m, n, p), np.int64)
    with np.errstate(all="ignore"):
        for mi in range(m):
            tr = target_rows(T, H, offset[mi])
            for t in range(H):
                live = np.ones((n, p), bool) if first is None else t <= np.asarray(first)[mi]
                for k, c in enumerate(terms):
                    g = targets[mi, tr[t], k]
                    if np.isnan(g):
                        continue
                    w = float(np.float32(c.get("w", 1.0)))
                    delta = float(np.float32(c["delta"])) if c.get("kind") == "huber" else None
                    e = traj[t, mi, :, :, c["dim"]].astype(np.float64) - float(g)
                    wc = w * cost_term(c.get("kind", "square"), e, delta)
                    cost[mi] += np.where(live, wc, 0.0)
                    S[mi] += np.where(live, np.abs(wc), 0.0)
                    counted[mi] += live
        out = np.where(counted > 0, np.asarray(rows, np.float64) - cost, np.asarray(rows, np.float64))
    return out, cost, S, counted


def brute_force(traj, rows, terms, targets, offset=None, first=None):
    """The same by plain loops over (env, sequence, particle, step, term) on python floats: (rows', cost, S, counted)."""
    H, m, n, p, _ = traj.shape
    targets = np.asarray(targets, np.float32)
    if targets.ndim == 2:
        targets = targets[:, None]
    T = targets.shape[1]
    out, cost = np.array(rows, np.float64), np.zeros((m, n, p))
    S, counted = np.zeros((m, n, p)), np.zeros((m, n, p), np.int64)
    for mi in range(m):
        off = 0 if offset is None else int(offset[mi])
        for ni in range(n):
            for j in range(p):
                total = s = 0.0
                cnt = 0
                for t in range(H):
                    if first is not None and t > int(first[mi, ni, j]):
                        break
                    row = min(max(off + t, 0), T - 1)
                    for k, c in enumerate(terms):
                        g = float(targets[mi, row, k])
                        if g != g:
                            continue
                        e = float(traj[t, mi, ni, j, c["dim"]]) - g
                        kind, w = c.get("kind", "square"), float(np.float32(c.get("w", 1.0)))
                        if kind == "square":
                            v = e * e
                        elif kind == "abs":
                            v = abs(e)
                        else:
                            d = float(np.float32(c["delta"]))
                            v = 0.5 * e * e if abs(e) <= d else d * (abs(e) - 0.5 * d)
                        total += w * v
                        s += abs(w * v)
                        cnt += 1
                cost[mi, ni, j], S[mi, ni, j], counted[mi, ni, j] = total, s, cnt
                if cnt:
                    out[mi, ni, j] = float(rows[mi, ni, j]) - total
    return out, cost, S, counted


def float32_chain(traj, rows, terms, targets, offset=None, first=None):
    """The kernel's own chain emulated in float32 (every operation rounded, steps in order, k ascending): (rows' float32, cost float32)."""
    H, m, n, p, _ = traj.shape
    f = np.float32
    targets = np.asarray(targets, f)
    if targets.ndim == 2:
        targets = targets[:, None]
    T = targets.shape[1]
    offset = np.zeros(m, np.int64) if offset is None else np.asarray(offset, np.int64)
    cost, counted = np.zeros((m, n, p), f), np.zeros((m, n, p), bool)
    with np.errstate(all="ignore"):
        for mi in range(m):
            tr = target_rows(T, H, offset[mi])
            for t in range(H):
                live = np.ones((n, p), bool) if first is None else t <= np.asarray(first)[mi]
                for k, c in enumerate(terms):
                    g = targets[mi, tr[t], k]
                    if np.isnan(g):
                        continue
                    e = (traj[t, mi, :, :, c["dim"]].astype(f) - g).astype(f)
                    kind, w = c.get("kind", "square"), f(c.get("w", 1.0))
                    if kind == "square":
                        v = (e * e).astype(f)
                    elif kind == "abs":
                        v = np.abs(e)
                    else:
                        d = f(c["delta"])
                        v = np.where(np.abs(e) <= d, (f(0.5) * e * e).astype(f), (d * (np.abs(e) - f(0.5) * d).astype(f)).astype(f))
                    cost[mi] = np.where(live, (cost[mi] + (w * v).astype(f)).astype(f), cost[mi])
                    counted[mi] |= live
        r = np.asarray(rows, f)
        return np.where(counted, (r - cost).astype(f), r), cost


KINDS = ("square", "abs", "huber")
SHAPES = {      # name: (H, m, n, p, D, A, offsets) -- the geometries of tests/test_gpu_constraints.py's engines; offsets per env: see make_case
    "hopper-240": (3, 4, 12, 5, 11, 3, (-2, 1, 0, None)),      # 240 rows = 3 full workgroups + 48; 60 rows per env: workgroups span envs
    "hopper-45": (3, 1, 9, 5, 11, 3, (1,)),                    # fewer rows than a workgroup; 495 floats per step: odd steps are not 16-byte aligned
    "halfcheetah-320": (8, 4, 4, 20, 18, 6, (None, 3, 0, -1)),
    # off the geometries above (tests/test_gpu_terms_envelope.py's engines)
    "slim-150": (3, 2, 5, 15, 45, 17, (-2, 1)),               # 64 + 64 + 22 rows, tiles of 64 x 45 floats: an odd D, spans aligned at even steps only
    "wide-100": (3, 2, 5, 10, 48, 24, (1, None)),             # the declared envelope's corner: tiles of 64 x 48 floats
    "pend-135": (5, 3, 9, 5, 3, 1, (-1, 2, None)),            # D = 3: a tile of 192 floats, fewer than the workgroup has threads
    # n p = 1: one env per row, so workgroup 0 holds 64 envs, each with its own offset and target rows, and workgroup 1 holds 6
    "p1-70": (5, 70, 1, 1, 18, 6, tuple((7 * i) % 13 - 4 for i in range(70))),
    # n p = 3: 90 rows, three per env; the first workgroup ends inside env 21
    "p1-90": (5, 30, 3, 1, 18, 6, tuple((5 * i) % 13 - 4 for i in range(30))),
    "long-130": (40, 2, 13, 5, 18, 6, (-3, 5)),               # H = 40: 64 + 64 + 2 rows
}
ALL_NAN_ENV = 2      # of the shapes with m = 4: every target NaN


def make_case(shape, K, T, kinds=KINDS, seed=0, dims=None):
    """(traj, rows, terms, targets [m,T,K], offset [m] int32) on `behind_rollout.synth_traj`: K terms on random dims with the given kinds
    in turn, w in [0.1, 2], Huber deltas in [0.5, 2] (both sides of delta occur: the errors are of order 1 to 3); targets of the dims' own
    scale; an offset None stands for T + 1 (beyond the reference); a fifth of every env's T K targets NaN, and -- shapes with m = 4 --
    every target of env ALL_NAN_ENV.  `dims`: the dims of the first terms, in place of the drawn ones (the draws stay what they are)."""
    from behind_rollout import synth_traj
    H, m, n, p, D, A, offs = SHAPES[shape]
    rng = np.random.default_rng([seed, K, T, len(shape)])
    traj, _, _ = synth_traj(int(rng.integers(1 << 30)), H, m, n, p, D, A)
    rows = (10.0 * rng.standard_normal((m, n, p))).astype(np.float32)
    dims_drawn = rng.integers(0, D, K)
    if dims is not None:
        dims_drawn[:min(K, len(dims))] = list(dims)[:K]
    dims = dims_drawn
    terms = []
    for k in range(K):
        c = dict(dim=int(dims[k]), kind=kinds[k % len(kinds)], w=float(np.float32(rng.uniform(0.1, 2.0))))
        if c["kind"] == "huber":
            c["delta"] = float(np.float32(rng.uniform(0.5, 2.0)))
        terms.append(c)
    mu = traj.reshape(-1, D).mean(axis=0)[dims]
    targets = (mu + rng.standard_normal((m, T, K))).astype(np.float32)
    for mi in range(m):
        targets[mi].reshape(-1)[rng.choice(T * K, int(round(0.2 * T * K)), replace=False)] = np.nan
    if m == 4:
        targets[ALL_NAN_ENV] = np.nan
    offset = np.array([T + 1 if o is None else o for o in offs], np.int32)
    return traj, rows, terms, targets, offset


def bound(S, ref, H, K):
    """|out - ref| <= (H K + 4) 2^-23 S + 2^-24 |ref| per row: one rounding each for e, c and w c, one per add of the chain and the final
    subtraction, doubled for slack.  ref None: the bound of the cost alone, without the last term."""
    b = (H * K + 4) * 2.0 ** -23 * S
    return b if ref is None else b + 2.0 ** -24 * np.abs(ref)
