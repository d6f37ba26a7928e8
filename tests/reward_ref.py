"""Numpy restatement of the learned reward of the opt-in planner (csrc/reward.hip: cadm_reward_eval, cadm_reward_returns) -- test
infrastructure shared by tests/test_reward_ref.py (CPU) and tests/test_gpu_reward.py.

The definition is include/cadm_hip.h, "Learned reward".  `gather_inputs` builds the net's input of every (step, row) from the three
sources; `reward64` states R in float64 and `emulate32` walks the kernel's float32 chain -- both are `value_ref`'s layer walks on the
concatenated input, because the chain is the value net's; `step_sum` and `update` are the step sum and the row update from R's own float32
bits (plain float32 adds in ascending t over the counted steps, then one multiply and one add); `brute_force` says the same with plain
loops."""
import numpy as np

import value_ref as vref

F = np.float32
INPUTS = ("next_obs", "obs_act", "obs_act_next_obs")


def input_dims(inputs, D, A):
    return {"next_obs": D, "obs_act": D + A, "obs_act_next_obs": 2 * D + A}[inputs]


def gather_inputs(traj, obs, actions, inputs):
    """x [H,m,n,p,K] float32: for step t of row (mi, ni, j) the concatenation `inputs` selects of s_t (obs[mi] for t = 0, else
    traj[t-1,mi,ni,j]), a_t = actions[mi,ni,t] (shared by the p particles) and s_{t+1} = traj[t,mi,ni,j]"""
    traj, obs, actions = np.asarray(traj, F), np.asarray(obs, F), np.asarray(actions, F)
    H, m, n, p, D = traj.shape
    A = actions.shape[-1]
    assert obs.shape == (m, D) and actions.shape == (m, n, H, A)
    s = np.concatenate([np.broadcast_to(obs[None, :, None, None, :], (1, m, n, p, D)), traj[:-1]], axis=0)
    a = np.broadcast_to(np.moveaxis(actions, 2, 0)[:, :, :, None, :], (H, m, n, p, A))
    parts = {"next_obs": [traj], "obs_act": [s, a], "obs_act_next_obs": [s, a, traj]}[inputs]
    return np.ascontiguousarray(np.concatenate(parts, axis=-1))


def reward64(x, layers, act, mean=None, std=None):
    """R [...] in float64 of concatenated inputs x [..., K]; NaN for an input with a non-finite value"""
    return vref.value(x, layers, act, mean, std)


def emulate32(x, layers, act, mean=None, std=None):
    """R [...] float32 by the kernel's chain (`value_ref.emulate32`'s layer walk on the concatenated input)"""
    return vref.emulate32(x, layers, act, mean, std)


def counted(H, shape, first=None):
    """[H, *shape] bool: step t of a row counts when t <= first[row] (every step without `first`)"""
    t = np.arange(H).reshape((H,) + (1,) * len(shape))
    return np.ones((H,) + tuple(shape), bool) if first is None else t <= np.asarray(first)[None]


def step_sum(r, first=None):
    """S [m,n,p] float32 from the step rewards' float32 bits r [H,m,n,p]: ((0 + r_0) + r_1) + .. in ascending t over the counted steps"""
    r = np.asarray(r, F)
    live = counted(r.shape[0], r.shape[1:], first)
    S = np.zeros(r.shape[1:], F)
    with np.errstate(all="ignore"):
        for t in range(r.shape[0]):
            S = np.where(live[t], S + r[t], S)
            assert S.dtype == F
    return S


def update(rows, S, weight):
    """rows' float32: float32(rows + float32(weight * S)), one multiply, then one add"""
    rows, S = np.asarray(rows, F), np.asarray(S, F)
    with np.errstate(all="ignore"):
        ws = F(weight) * S
        out = rows + ws
    assert ws.dtype == F and out.dtype == F
    return out


def masked_steps(r, first=None):
    """what `step_out` holds: r with NaN in the steps that are not counted"""
    r = np.asarray(r, F)
    return np.where(counted(r.shape[0], r.shape[1:], first), r, F(np.nan)).astype(F)


def brute_force(traj, obs, actions, rows, layers, act, inputs, weight, mean=None, std=None, first=None):
    """(rows', S, steps) with plain loops: every counted (t, row) gathered and evaluated on its own through `emulate32`, summed in order"""
    traj, obs, actions = np.asarray(traj, F), np.asarray(obs, F), np.asarray(actions, F)
    H, m, n, p, D = traj.shape
    out, S, steps = np.zeros((m, n, p), F), np.zeros((m, n, p), F), np.full((H, m, n, p), np.nan, F)
    with np.errstate(all="ignore"):
        for mi in range(m):
            for ni in range(n):
                for j in range(p):
                    s = F(0)
                    for t in range(H):
                        if first is not None and t > int(first[mi, ni, j]):
                            break
                        prev = obs[mi] if t == 0 else traj[t - 1, mi, ni, j]
                        x = {"next_obs": [traj[t, mi, ni, j]], "obs_act": [prev, actions[mi, ni, t]],
                             "obs_act_next_obs": [prev, actions[mi, ni, t], traj[t, mi, ni, j]]}[inputs]
                        r = emulate32(np.concatenate(x)[None], layers, act, mean, std)[0]
                        steps[t, mi, ni, j] = r
                        s = F(s + r)
                    S[mi, ni, j] = s
                    out[mi, ni, j] = F(F(rows[mi, ni, j]) + F(F(weight) * s))
    return out, S, steps


def he_net(K, hidden, seed=0, out_scale=1.0):
    return vref.he_net(K, hidden, seed, out_scale)
