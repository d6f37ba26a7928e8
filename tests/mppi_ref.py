"""numpy restatement of the MPPI update (csrc/mppi.hip, include/cadm_hip.h "MPPI update") and of the planner loop that uses it
(`cadm_mppi_plan`).  Generic over the dtype of its inputs; the tests use float64.  Test infrastructure only."""
import numpy as np

import icem_ref
from oracle import nets as onets
from oracle import planner as oplanner


def mppi_weights(cand, temperature, relative=False):
    """cand [n] -> (weights [n], any finite).  Non-finite returns weigh 0; the best finite one weighs 1."""
    dt = cand.dtype.type
    fin = np.isfinite(cand)
    w = np.zeros(cand.shape, cand.dtype)
    if not fin.any():
        return w, False
    rmax, rmin = cand[fin].max(), cand[fin].min()
    lam = dt(temperature) * (rmax - rmin) if relative else dt(temperature)
    if relative and lam == 0:
        w[fin] = 1
    else:
        with np.errstate(over="ignore", under="ignore", divide="ignore"):
            w[fin] = np.exp((cand[fin] - rmax) / lam)
    return w, True


def mppi_update(mean, var, actions, cand, temperature, relative=False, alpha=0.1, lower=-1.0, upper=1.0):
    """mean / var [m,H,A], actions [m,n,H,A], cand [m,n] -> (new mean, new var, plan = clip(new mean)); an env without a finite
    return keeps its mean / var."""
    dt = mean.dtype.type
    new_mean, new_var = mean.copy(), var.copy()
    for mi in range(mean.shape[0]):
        w, any_finite = mppi_weights(cand[mi], temperature, relative)
        if not any_finite:
            continue
        W = w.sum()
        mu = np.tensordot(w, actions[mi], axes=(0, 0)) / W
        d = actions[mi] - mu[None]
        v = np.tensordot(w, d * d, axes=(0, 0)) / W
        new_mean[mi] = mean[mi] * dt(alpha) + (dt(1) - dt(alpha)) * mu
        new_var[mi] = var[mi] * dt(alpha) + (dt(1) - dt(alpha)) * v
    return new_mean, new_var, np.clip(new_mean, dt(lower), dt(upper))


def top_elites(cand, num_elites):
    """[m,n] -> [m,num_elites] candidate ids by return, descending, ties to the lower index (the elite selection of csrc/cem.hip)."""
    return np.stack([np.argsort(-c, kind="stable")[:num_elites] for c in cand]).astype(np.int64)


def mppi_loop(o, E, p, n, iters, num_elites, temperature=1.0, relative=False, noise_beta=0.0, K=0, decay=1.0, return_best=False,
              add_mean_last=False, z=None, xi=None, carry=None, carry_valid=None, alpha=0.1, lower=-1.0, upper=1.0, deterministic=True):
    """`icem_ref.icem_loop` with the MPPI update in place of the elite refit: the same samplers, candidate schedule, carried elites
    (still the top `num_elites` by return), mean candidate and best plan.  Returns (plan, info, carry, carry_valid)."""
    dt = o["obs"].dtype.type
    mean, var = o["init_mean"].copy(), o["init_var"].copy()
    m, H, A = mean.shape
    D = o["obs"].shape[1]
    ctx = None if o["cp"] is None else onets.context_forward(o["cp"], o["cp_obs"], o["cp_act"], o["st"])
    best_ret, best_seq = np.full(m, np.nan, dt), np.full((m, H, A), np.nan, dt)
    kept, info = None, []
    for it in range(iters):
        last = it + 1 == iters
        ni = icem_ref.n_candidates(n, decay, it, num_elites, K)
        if noise_beta > 0:
            actions = icem_ref.colored_actions(mean, var, xi[it], noise_beta, lower, upper).astype(dt)
        else:
            actions = oplanner.sample_actions(mean, var, z[it].astype(dt), lower, upper).astype(dt)
        assert actions.shape == (m, ni, H, A)
        if K > 0 and it == 0 and carry is not None:
            for mi in range(m):
                if carry_valid[mi]:
                    actions[mi, :K, :H - 1] = carry[mi, :, 1:]
        elif K > 0 and it > 0:
            actions[:, :K] = kept
        if last and add_mean_last:
            actions[:, K] = np.clip(mean, dt(lower), dt(upper))
        T = None if ctx is None else oplanner.context_table_indexed(ctx, it)
        rets = oplanner.rollout_indexed(o["env"], o["ff"], o["st"], o["obs"], T, actions, np.zeros((H, m, ni, p, D), dt), E, p, deterministic)
        cand = oplanner.particle_mean(rets)
        idx = top_elites(cand, num_elites)
        mean, var, _ = mppi_update(mean, var, actions, cand, temperature, relative, alpha, lower, upper)
        icem_ref.track_best(cand, actions, best_ret, best_seq)
        if K > 0:
            kept = np.take_along_axis(actions, idx[:, :K, None, None], axis=1)
        info.append(dict(actions=actions, cand=cand, elites=idx, kept=kept, mean=mean.copy(), var=var.copy()))
    if K > 0:
        carry, carry_valid = kept.copy(), np.ones(m, np.int32)
    plan = best_seq if return_best else np.clip(mean, dt(lower), dt(upper))
    return plan, info, carry, carry_valid
