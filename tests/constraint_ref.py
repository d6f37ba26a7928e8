"""Numpy restatement of the planner's state constraints (cadm_amd/csrc/constrain.hip, `cadm_constrain_returns`) -- test infrastructure.

constraints: a list of dict(dim=d, lo=..., hi=...), a missing side being -inf / +inf.  A post-step state traj[t] is healthy iff
lo < x[d] < hi for every entry, compared in FLOAT32 (the bounds rounded to float32 first, as the library receives them); NaN and
+-inf fail the comparisons and violate.  Counters are integers.  `penalty` rows are float32: rows - w * count, a float32 product
and a float32 difference.  `terminate` rows are float64: the partial sum r_0 + ... + r_tau of `forecast_ref.step_rewards` (the env's
own closure on float32 arrays) minus w; rows without a violation keep their input value in both modes."""
import numpy as np

from forecast_ref import step_rewards


def bounds(constraints):
    """[(dim, lo, hi)] with the bounds as float32"""
    return [(int(c["dim"]), np.float32(-np.inf if c.get("lo") is None else c["lo"]), np.float32(np.inf if c.get("hi") is None else c["hi"]))
            for c in constraints]


def violation_mask(traj, constraints):
    """traj [H,m,n,p,D] -> [H,m,n,p] bool: the post-step state of step t violates"""
    x = np.asarray(traj, np.float32)
    bad = np.zeros(x.shape[:-1], bool)
    with np.errstate(invalid="ignore"):
        for d, lo, hi in bounds(constraints):
            bad |= ~((x[..., d] > lo) & (x[..., d] < hi))
    return bad


def counters(traj, constraints):
    """(first_violation, violations), both [m,n,p] int32: the first violating step (H: none) and the number of violating steps"""
    bad = violation_mask(traj, constraints)
    H = bad.shape[0]
    return np.where(bad.any(axis=0), bad.argmax(axis=0), H).astype(np.int32), bad.sum(axis=0).astype(np.int32)


def penalty_rows(rows, violations, weight):
    """float32: rows - w * (float)violations where there is a violation, else rows untouched"""
    r = np.asarray(rows, np.float32)
    with np.errstate(all="ignore"):
        pen = (np.float32(weight) * violations.astype(np.float32)).astype(np.float32)
        return np.where(violations > 0, (r - pen).astype(np.float32), r)


def terminate_rows(env, traj, obs, actions, rows, first, weight):
    """float64 [m,n,p]: (r_0 + ... + r_tau) - w for a row that first violates at tau < H, else rows.  Step rewards after tau are
    never added: whatever traj holds there does not matter."""
    H = traj.shape[0]
    with np.errstate(all="ignore"):
        r = step_rewards(env, traj, obs, actions).astype(np.float64)                # [m,n,H,p]
        part = np.cumsum(np.moveaxis(r, 2, 0), axis=0)                              # [H,m,n,p]: r_0 + ... + r_t
    tau = np.minimum(first, H - 1).astype(np.int64)
    cut = np.take_along_axis(part, tau[None], axis=0)[0] - float(np.float32(weight))
    return np.where(first < H, cut, np.asarray(rows, np.float64))


def brute_force(traj, constraints, rows, weight, step_reward=None):
    """The same by plain loops over (env, sequence, particle, step) on python floats: (first, violations, penalty rows float32,
    terminate rows float64 -- None without step_reward [m,n,H,p])."""
    H, m, n, p, D = traj.shape
    cons = bounds(constraints)
    first, viol = np.full((m, n, p), H, np.int32), np.zeros((m, n, p), np.int32)
    pen = np.array(rows, np.float32)
    term = None if step_reward is None else np.array(rows, np.float64)
    for mi in range(m):
        for ni in range(n):
            for j in range(p):
                total, cut = 0.0, None
                for t in range(H):
                    x = traj[t, mi, ni, j]
                    healthy = all(bool(np.float32(x[d]) > lo) and bool(np.float32(x[d]) < hi) for d, lo, hi in cons)
                    if step_reward is not None and cut is None:
                        total += float(step_reward[mi, ni, t, j])
                    if not healthy:
                        viol[mi, ni, j] += 1
                        if first[mi, ni, j] == H:
                            first[mi, ni, j] = t
                            cut = total
                if viol[mi, ni, j]:
                    pen[mi, ni, j] = np.float32(rows[mi, ni, j]) - np.float32(np.float32(weight) * np.float32(viol[mi, ni, j]))
                    if term is not None:
                        term[mi, ni, j] = cut - float(np.float32(weight))
    return first, viol, pen, term
