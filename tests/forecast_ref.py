"""Float64 restatement of the plan forecast (csrc/forecast.hip: cadm_forecast_stats) from a recorded trajectory -- test infrastructure.

States are reduced in float64.  Step rewards come from the env's own closure (`EnvDecl.reward`, or the oracle env's `reward`) on
FLOAT32 arrays: threshold terms (inside / outside) then compare the same float32 numbers the kernel compares; their statistics are
taken in float64.  `reward_bound` says how far a float32 evaluation of a step reward may lie from its float64 value, per env kind."""
import numpy as np

from cadm_amd.env_spec import EnvDecl, restate


def pre_post(traj, obs):
    """traj [H,m,n,p,D], obs [m,D] -> (pre, post) [m,n,H,p,D] float32: the state before / after every step."""
    H, m, n, p, D = traj.shape
    post = np.ascontiguousarray(np.transpose(traj.astype(np.float32), (1, 2, 0, 3, 4)))
    first = np.broadcast_to(obs.astype(np.float32)[:, None, None, None, :], (m, n, 1, p, D))
    return np.concatenate([first, post[:, :, :-1]], axis=2), post


def step_rewards(env, traj, obs, actions):
    """Per-particle step rewards [m,n,H,p] in float32, by the env's closure on float32 arrays."""
    pre, post = pre_post(traj, obs)
    m, n, H, p, _ = pre.shape
    act = np.broadcast_to(actions.astype(np.float32)[:, :, :, None, :], (m, n, H, p, actions.shape[-1]))
    with np.errstate(all="ignore"):
        return np.asarray(env.reward(pre, act, post), np.float32)


def reward_terms(env, traj, obs, actions):
    """(T, S): the number of additive terms of the step reward -- the declared terms, the control cost, the bonus -- and the sum of
    their absolute values per (m, n, H, p), in float64.  `env`: an EnvDecl, or the name of a built-in kind that restates as one."""
    spec = env if isinstance(env, EnvDecl) else restate(env)
    pre, post = pre_post(traj, obs)
    pre, post = pre.astype(np.float64), post.astype(np.float64)
    S = np.zeros(pre.shape[:-1])
    for kind, d, when, w, lo, hi in spec.terms:
        S += np.abs(spec._term(kind, (pre if when == "obs" else post)[..., d], w, lo, hi))
    T = len(spec.terms)
    if spec.ctrl_cost != 0.0:
        S += np.abs(spec.ctrl_cost) * np.sum(np.square(actions.astype(np.float64)), axis=-1)[:, :, :, None]
        T += 1
    if spec.bonus != 0.0:
        S += np.abs(spec.bonus)
        T += 1
    return T, S


def pendulum_angle(pre):
    """float64 normalised angle of pre-step states [..., 3]: ((atan2(y, x) + pi) floormod 2 pi) - pi, in [-pi, pi)."""
    x = np.asarray(pre, np.float64)
    return np.mod(np.arctan2(x[..., 1], x[..., 0]) + np.pi, 2.0 * np.pi) - np.pi


def reward_bound(env, traj, obs, actions):
    """b [m,n,H,p]: how far a float32 evaluation of the step reward may lie from its float64 value, for any continuous kind.
    halfcheetah, ant, slim_humanoid and an EnvDecl: (T + 3) 2^-23 S of `reward_terms`.
    pendulum: 6 2^-23 S + 4 |tn| 2^-20 with S = tn^2 + 0.1 thetadot^2 + 0.001 clip(a, +-2)^2 and tn the float64 normalised angle of
    the pre-step state.  The second term is the angle's own rounding, which enters through tn^2 (d tn^2 = 2 |tn| d tn, on both of two
    compared sides): atan2f within 2 ulp at |theta| <= pi (2^-21), the addition of pi (2^-22), the final subtraction (2^-23), below
    2^-20 together.  The float32 pi cancels between the addition and the subtraction; the branch cut does not matter, the cost reads
    tn^2, which is continuous across it."""
    if env != "pendulum":
        T, S = reward_terms(env, traj, obs, actions)
        return (T + 3) * 2.0 ** -23 * S
    pre, _ = pre_post(traj, obs)
    tn = pendulum_angle(pre)
    tq = np.clip(actions.astype(np.float64)[..., 0], -2.0, 2.0)[:, :, :, None]
    S = tn ** 2 + 0.1 * pre[..., 2].astype(np.float64) ** 2 + 0.001 * tq ** 2
    return 6 * 2.0 ** -23 * S + 4 * np.abs(tn) * 2.0 ** -20


def diverged_step(traj):
    """[m,n] int32: the first step at which any of a sequence's p * D values is non-finite, H if there is none."""
    H = traj.shape[0]
    bad = ~np.isfinite(traj).all(axis=(3, 4))                    # [H,m,n]
    return np.where(bad.any(axis=0), bad.argmax(axis=0), H).astype(np.int32)


def forecast_ref(traj, obs, actions, E, band_k=1, rewards=None):
    """Every statistic of cadm_forecast_stats in float64 (lo / hi: float32, they are order statistics).  traj [H,m,n,p,D], obs [m,D],
    actions [m,n,H,A]; rewards: `step_rewards` of the env ([m,n,H,p] float32), or None to leave the reward outputs out.
    Statistics at and after a sequence's diverged_step are NaN, and so are its returns."""
    H, m, n, p, D = traj.shape
    pe = p // E
    div = diverged_step(traj)
    x32 = np.transpose(traj.astype(np.float32), (1, 2, 0, 3, 4))                 # [m,n,H,p,D]
    dead = np.arange(H)[None, None, :] >= div[:, :, None]                        # [m,n,H]
    with np.errstate(all="ignore"):
        x = np.where(dead[..., None, None], 0.0, x32.astype(np.float64))
        xm = x.reshape(m, n, H, E, pe, D)
        srt = np.sort(np.where(dead[..., None, None], np.float32(0), x32), axis=3)
        out = dict(mean=x.mean(3), member_mean=np.moveaxis(xm.mean(4), 3, 0), var_total=x.var(3), var_epistemic=xm.mean(4).var(3),
                   var_aleatoric=xm.var(4).mean(3), lo=srt[:, :, :, band_k - 1], hi=srt[:, :, :, p - band_k])
        if rewards is not None:
            r = np.where(dead[..., None], 0.0, rewards.astype(np.float64))       # [m,n,H,p]
            rm = r.reshape(m, n, H, E, pe)
            out.update(reward_mean=r.mean(3), reward_var=r.var(3), reward_member=np.moveaxis(rm.mean(4), 3, 0), returns=r.sum(2))
    for k, v in out.items():
        v = v.astype(np.float32 if k in ("lo", "hi") else np.float64)
        if k == "returns":
            v[div < H] = np.nan
        elif k in ("member_mean", "reward_member"):
            v[:, dead] = np.nan
        else:
            v[dead] = np.nan
        out[k] = v
    out["diverged_step"] = div
    return out


def brute_force(traj, E, band_k=1):
    """The state statistics by plain loops over (env, sequence, step, dim) on python floats: what `forecast_ref` vectorises."""
    H, m, n, p, D = traj.shape
    pe = p // E
    z = lambda *s: np.full(s, np.nan)
    out = dict(mean=z(m, n, H, D), member_mean=z(E, m, n, H, D), var_total=z(m, n, H, D), var_epistemic=z(m, n, H, D),
               var_aleatoric=z(m, n, H, D), lo=z(m, n, H, D), hi=z(m, n, H, D))
    for mi in range(m):
        for ni in range(n):
            for t in range(H):
                if not np.isfinite(traj[:t + 1, mi, ni]).all():      # this step or an earlier one holds a non-finite value
                    continue
                for d in range(D):
                    v = [float(traj[t, mi, ni, j, d]) for j in range(p)]
                    mu = sum(v) / p
                    mem = [sum(v[e * pe:(e + 1) * pe]) / pe for e in range(E)]
                    out["mean"][mi, ni, t, d] = mu
                    out["var_total"][mi, ni, t, d] = sum((a - mu) ** 2 for a in v) / p
                    out["var_epistemic"][mi, ni, t, d] = sum((a - mu) ** 2 for a in mem) / E
                    out["var_aleatoric"][mi, ni, t, d] = sum(sum((a - mem[e]) ** 2 for a in v[e * pe:(e + 1) * pe]) / pe for e in range(E)) / E
                    for e in range(E):
                        out["member_mean"][e, mi, ni, t, d] = mem[e]
                    s = sorted(v)
                    out["lo"][mi, ni, t, d], out["hi"][mi, ni, t, d] = s[band_k - 1], s[p - band_k]
    return out
