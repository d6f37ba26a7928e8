"""Numpy restatement of the planner's discount over the horizon (cadm_amd/csrc/discount.hip, `cadm_set_discount`, and what every stage
behind the rollout makes of the table) -- test infrastructure.  Each function wraps one of the existing restatements and takes the
table `disc` [H + 1] float32; with all weights 1 it reproduces the function it wraps bit for bit (tests/test_discount_ref.py).

float32 functions (`penalty_rows`, `tracking32`, `step_sum`, `uncertainty_cost32`, `actuator_cost32`, `terminal_update`) walk the kernels'
chains operation for operation: every product and every add is one float32 rounding, nothing fused.  float64 functions
(`env_returns`, `terminate_rows`) are the references the bounded comparisons are held against; `env_bound` is their bound."""
import numpy as np

import actuator_ref
import constraint_ref
import reward_ref
import uncertainty_ref
import value_ref
from forecast_ref import reward_bound, step_rewards
from tracking_ref import target_rows

F = np.float32


def weights(gamma, H):
    """disc [H + 1] float32: (float)pow((double)(float)gamma, (double)t), disc[0] = 1 exactly"""
    out = np.power(np.float64(np.float32(gamma)), np.arange(H + 1, dtype=np.float64)).astype(F)
    out[0] = F(1.0)
    return out


def counted_weight(disc, first, H):
    """float64: the sum of disc[t] over the counted steps t <= min(first, H - 1) of every row, by the cumulative sum"""
    part = np.cumsum(np.asarray(disc, np.float64)[:H])
    return part[np.minimum(np.asarray(first), H - 1)]


def geometric(gamma, k):
    """the closed form of 1 + g + .. + g^(k - 1) in float64, g the float32 gamma"""
    g = float(np.float32(gamma))
    return np.asarray(k, np.float64) if g == 1.0 else (1.0 - g ** np.asarray(k, np.float64)) / (1.0 - g)


# ---------------------------------------------------------------------------------------------- the env's own return
def env_returns(env, traj, obs, actions, disc, rows=None):
    """(returns float64 [m,n,p], step rewards float64 [m,n,H,p]): sum_t float64(disc[t]) * r_t, r_t the env's own closure on float32
    arrays widened to float64 (as `constraint_ref.terminate_rows` takes them).  rows: where it holds a NaN the return is that NaN."""
    H = traj.shape[0]
    with np.errstate(all="ignore"):
        r = step_rewards(env, traj, obs, actions).astype(np.float64)               # [m,n,H,p]
        ret = (r * np.asarray(disc, np.float64)[:H][None, None, :, None]).sum(axis=2)
    if rows is not None:
        ret = np.where(np.isnan(rows), np.asarray(rows, np.float64), ret)
    return ret, r


def env_bound(terms_env, traj, obs, actions, disc, r, first=None):
    """[m,n,p]: (steps) * max_t (b_t + 2^-23 |disc[t] r_t|) over the counted steps t <= min(first, H - 1) (all H without `first`), b_t
    `forecast_ref.reward_bound`; r: `env_returns`' float64 step rewards.  See tests/test_gpu_discount.py for the derivation."""
    H = traj.shape[0]
    with np.errstate(all="ignore"):
        b = reward_bound(terms_env, traj, obs, actions)                            # [m,n,H,p]
        per = b + 2.0 ** -23 * np.abs(np.asarray(disc, np.float64)[:H][None, None, :, None] * r)
    per = np.moveaxis(per, 2, 0)                                                   # [H,m,n,p]
    if first is None:
        return H * per.max(axis=0)
    tau = np.minimum(np.asarray(first), H - 1)
    upto = np.where(np.arange(H)[:, None, None, None] <= tau[None], per, 0.0)      # steps behind tau are not read: theirs may be NaN
    return (tau + 1) * upto.max(axis=0)


# ---------------------------------------------------------------------------------------------- constraints
def penalty_rows(rows, bad, weight, disc):
    """float32: pen = pen + disc[t] on the violating steps in ascending t from 0.0f, then rows - w * pen where there is a violation,
    else rows untouched.  bad [H,m,n,p] bool: `constraint_ref.violation_mask`."""
    r = np.asarray(rows, F)
    d = np.asarray(disc, F)
    pen = np.zeros(r.shape, F)
    with np.errstate(all="ignore"):
        for t in range(bad.shape[0]):
            pen = np.where(bad[t], pen + d[t], pen)
            assert pen.dtype == F
        wp = F(weight) * pen
        out = r - wp
    assert wp.dtype == F and out.dtype == F
    return np.where(bad.any(axis=0), out, r)


def terminate_rows(env, traj, obs, actions, rows, first, weight, disc):
    """float64 [m,n,p]: (disc[0] r_0 + ... + disc[tau] r_tau) - w disc[tau] for a row that first violates at tau < H, else rows"""
    H = traj.shape[0]
    d = np.asarray(disc, np.float64)[:H]
    with np.errstate(all="ignore"):
        r = step_rewards(env, traj, obs, actions).astype(np.float64)                # [m,n,H,p]
        part = np.cumsum(np.moveaxis(r, 2, 0) * d[:, None, None, None], axis=0)     # [H,m,n,p]
    tau = np.minimum(first, H - 1).astype(np.int64)
    cut = np.take_along_axis(part, tau[None], axis=0)[0] - float(np.float32(weight)) * d[tau]
    return np.where(first < H, cut, np.asarray(rows, np.float64))


# ---------------------------------------------------------------------------------------------- tracking
def tracking32(traj, rows, terms, targets, disc, offset=None, first=None):
    """`tracking_ref.float32_chain` with cost = cost + disc[t] * (w_k c): (rows' float32, cost float32)"""
    H, m, n, p, _ = traj.shape
    d = np.asarray(disc, F)
    targets = np.asarray(targets, F)
    if targets.ndim == 2:
        targets = targets[:, None]
    T = targets.shape[1]
    offset = np.zeros(m, np.int64) if offset is None else np.asarray(offset, np.int64)
    cost, counted = np.zeros((m, n, p), F), np.zeros((m, n, p), bool)
    with np.errstate(all="ignore"):
        for mi in range(m):
            tr = target_rows(T, H, offset[mi])
            for t in range(H):
                live = np.ones((n, p), bool) if first is None else t <= np.asarray(first)[mi]
                for k, c in enumerate(terms):
                    g = targets[mi, tr[t], k]
                    if np.isnan(g):
                        continue
                    e = (traj[t, mi, :, :, c["dim"]].astype(F) - g).astype(F)
                    kind, w = c.get("kind", "square"), F(c.get("w", 1.0))
                    if kind == "square":
                        v = (e * e).astype(F)
                    elif kind == "abs":
                        v = np.abs(e)
                    else:
                        dl = F(c["delta"])
                        v = np.where(np.abs(e) <= dl, (F(0.5) * e * e).astype(F), (dl * (np.abs(e) - F(0.5) * dl).astype(F)).astype(F))
                    term = (d[t] * (w * v).astype(F)).astype(F)
                    cost[mi] = np.where(live, (cost[mi] + term).astype(F), cost[mi])
                    counted[mi] |= live
        r = np.asarray(rows, F)
        return np.where(counted, (r - cost).astype(F), r), cost


# ---------------------------------------------------------------------------------------------- learned reward
def step_sum(r, disc, first=None):
    """`reward_ref.step_sum` with S = S + disc[t] * r_t, from the step rewards' float32 bits r [H,m,n,p]"""
    r = np.asarray(r, F)
    d = np.asarray(disc, F)
    live = reward_ref.counted(r.shape[0], r.shape[1:], first)
    S = np.zeros(r.shape[1:], F)
    with np.errstate(all="ignore"):
        for t in range(r.shape[0]):
            S = np.where(live[t], S + d[t] * r[t], S)
            assert S.dtype == F
    return S


# ---------------------------------------------------------------------------------------------- uncertainty
def uncertainty_cost32(step, disc, first=None):
    """the cost chain of `uncertainty_ref.emulate32` with c = c + disc[t] * u_t, from the step costs' float32 bits step [m,n,H]"""
    u = np.asarray(step, F)
    d = np.asarray(disc, F)
    m, n, H = u.shape
    on_t = uncertainty_ref.counted(first, H, m, n)
    c = np.zeros((m, n), F)
    with np.errstate(all="ignore"):
        for t in range(H):
            c = np.where(on_t[:, :, t], c + d[t] * u[:, :, t], c)
    assert c.dtype == F
    return c


# ---------------------------------------------------------------------------------------------- actuator
def actuator_cost32(actuated, rate_w, disc, prev=None):
    """`actuator_ref.cost_f32` with c += disc[t] * (w * ((y - last) * (y - last))) on ACTUATED sequences [m,n,H,A]"""
    y = np.asarray(actuated, F)
    d = np.asarray(disc, F)
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
            c = np.where(known, (c + (d[t] * (w * sq).astype(F)).astype(F)).astype(F), c)
        last = y[:, :, t]
    s = c[..., 0]
    for a in range(1, A):
        s = (s + c[..., a]).astype(F)
    return s


# ---------------------------------------------------------------------------------------------- terminal value / terminal Q
def terminal_weight(weight, disc):
    """float32(weight * disc[H]): the one product the launcher forms on the host"""
    return F(F(weight) * np.asarray(disc, F)[-1])


def terminal_update(rows, v, weight, disc, first=None, H=None):
    """`value_ref.update` under the effective weight: float32(rows + float32(weight_eff * v)); a row cut by `first` keeps its bits"""
    return value_ref.update(rows, v, terminal_weight(weight, disc), first, H)


__all__ = ["weights", "counted_weight", "geometric", "env_returns", "env_bound", "penalty_rows", "terminate_rows", "tracking32", "step_sum",
           "uncertainty_cost32", "actuator_cost32", "terminal_weight", "terminal_update", "actuator_ref", "constraint_ref"]
