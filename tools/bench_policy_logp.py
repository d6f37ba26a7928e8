#!/usr/bin/env python3
"""The actor's log-density of given actions (csrc/policy_logp.hip): what its planner stage costs next to the learned reward's on the same
rows, what `cadm_policy_logp` costs next to `cadm_policy_sample`, and what `cem_policy_logp` adds to a get_action call.

Stage time: device events around BATCH back-to-back calls of `cadm_policy_logp_returns` (both launches: the chain over the H m n p
(step, row) pairs and the step sum) on one stream, per call, on the trajectories of one planner iteration at the headline sizes (m = 1,
p = 20, H = 30, halfcheetah: 120 000 rows at 200 candidates) with a (256, 256) relu actor; median of ROUNDS rounds with the fastest and
slowest.  Next to it, timed in the same run: `cadm_reward_returns` with a (256, 256) relu net on "obs_act" inputs.
Row time: `cadm_policy_logp` on 4096 rows next to `cadm_policy_sample` on the same states, the same way.
Call time: `get_action` (numpy in, numpy out, one env, cfg2 sizes: halfcheetah, 4 x 200 swish, ensemble 5, 20 particles, H = 30,
5 iterations, 50 elites, 200 candidates) with `cem_noise_beta=1.0` alone against the same plus `cem_policy_logp` on a (256, 256) actor:
two models taking turns call by call, CALLS timed calls each after WARMUP, median with min .. 90th percentile.  Host clock around calls
that end in a stream synchronisation.
Writes a markdown table (--out, default stdout only).  Nothing is asserted.  Needs a GPU: there is no fallback."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd._lib import ptr
from cadm_amd.engine import HipEngine
from cadm_amd.synth import make_engine

HIDDEN = (256, 256)
HEAD = dict(kind="gaussian", log_std_bounds=(-5.0, 2.0))


def he_net(K, hidden, N, seed):
    rng = np.random.default_rng(seed)
    dims = [K] + list(hidden) + [N]
    return [((rng.standard_normal((dims[l], dims[l + 1])) * np.sqrt(2.0 / dims[l])).astype(np.float32),
             (0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32)) for l in range(len(dims) - 1)]


def timed(fn, batch, rounds):
    """(median, min, max) microseconds per call of `fn` over `rounds` rounds of `batch` back-to-back calls (round 0 warms up)"""
    dev = []
    for r in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if r > 0:
            dev.append(e0.elapsed_time(e1) * 1e3 / batch)
    return float(np.median(dev)), min(dev), max(dev)


def set_actor(eng, seed=1):
    layers = he_net(eng.D, HIDDEN, 2 * eng.A, seed)
    mean_layers, W_ls, b_ls = hplanner.split_gaussian_layers(layers, eng.A)
    eng.set_policy_net(HipEngine.policy_params(HIDDEN, "relu", "tanh", 1, 0.0), mean_layers)
    eng.set_policy_head(hplanner.policy_head_params(HEAD, has_actor=True), W_ls, b_ls)
    return layers


def device_times(eng, n, batch, rounds):
    """[(what, rows, (median, min, max))]"""
    H, p, D, A = eng.H, eng.p, eng.D, eng.A
    lib, ctx = eng.lib, eng._ctx
    z = lambda *s: torch.empty(s, dtype=torch.float32, device=eng.device)
    traj, obs, actions = z(H, 1, n, p, D).normal_(), z(1, D).normal_(), z(1, n, H, A).uniform_(-1.0, 1.0)
    rows = z(1, n, p).zero_()
    ws = torch.empty((lib.cadm_policy_logp_workspace_bytes(ctx, 1, n),), dtype=torch.uint8, device=eng.device)
    set_actor(eng)

    def check(rc, who):
        if rc != 0:
            raise RuntimeError("%s failed: %s" % (who, lib.cadm_last_error().decode()))

    out = []
    lp = HipEngine.policy_logp_params(0.0, "action")      # (weight 0: the rows stay finite over the repeated calls)
    stage = lambda: lib.cadm_policy_logp_returns(ctx, lp, ptr(traj), ptr(obs), ptr(actions), None, 1, n, ptr(rows), ptr(rows), None, None, ptr(ws),
                                                 eng.stream)
    check(stage(), "cadm_policy_logp_returns")
    out.append(("`cadm_policy_logp_returns`, (256, 256) relu actor, A = %d" % A, H * n * p, timed(stage, batch, rounds)))
    rp = HipEngine.reward_params("obs_act", HIDDEN, "relu", 0.0)
    eng.set_reward_net(rp, he_net(D + A, HIDDEN, 1, 2))
    reward = lambda: lib.cadm_reward_returns(ctx, rp, ptr(traj), ptr(obs), ptr(actions), None, 1, n, ptr(rows), ptr(rows), None, None, ptr(ws),
                                             eng.stream)
    check(reward(), "cadm_reward_returns")
    out.append(("`cadm_reward_returns`, (256, 256) relu net, obs_act", H * n * p, timed(reward, batch, rounds)))
    R = 4096
    x, a, logp, mode = z(R, D).normal_(), z(R, A).uniform_(-1.0, 1.0), z(R), z(R, A)
    one = lambda: lib.cadm_policy_logp(ctx, ptr(x), ptr(a), R, 0, ptr(logp), eng.stream)
    check(one(), "cadm_policy_logp")
    out.append(("`cadm_policy_logp`", R, timed(one, batch, rounds)))
    smp = lambda: lib.cadm_policy_sample(ctx, ptr(x), R, 0, 0, 1, 2, ptr(a), ptr(logp), ptr(mode), eng.stream)
    check(smp(), "cadm_policy_sample")
    out.append(("`cadm_policy_sample`", R, timed(smp, batch, rounds)))
    return out


def call_times(n, calls, warmup):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import make_env_spec
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=30, seed=0, trained_like=True)
    st = prob["stats"]
    nz = {k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")}
    term = dict(weight=0.01, space="action", policy=dict(hidden_sizes=HIDDEN, activation="relu", squash="tanh"))
    settings = [("cem_noise_beta=1.0", dict(cem_noise_beta=1.0)),
                ("+ cem_policy_logp, (256, 256) relu actor", dict(cem_noise_beta=1.0, cem_policy_logp=term, policy_head=HEAD))]
    models = []
    for name, kw in settings:
        model = MLPEnsembleCEMDynamicsModel("dyn", make_env_spec("halfcheetah"), hidden_sizes=(200,) * 4, hidden_nonlinearity="swish", n_forwards=30,
                                            n_candidates=n, ensemble_size=5, n_particles=20, use_cem=True, normalize_input=True, seed=7, **kw)
        model.engine.set_net("context_model", prob["cp"])
        model.engine.set_net("ff_model", prob["ff"])
        model.set_normalization(nz)
        if "cem_policy_logp" in kw:
            model.set_policy(he_net(model.obs_space_dims, HIDDEN, 2 * prob["A"], 1))
        models.append((name, model))
    A = prob["A"]
    var = np.full((1, 30, A), 0.25)
    state = {name: np.zeros((1, 30, A)) for name, _ in models}
    res = {name: [] for name, _ in models}
    for i in range(warmup + calls):
        for name, model in models:
            t0 = time.perf_counter()
            plan = model.get_action(prob["obs"], prob["cp_obs"], prob["cp_act"], state[name], var)
            dt = (time.perf_counter() - t0) * 1e3
            state[name] = np.concatenate([plan[:, 1:], np.zeros((1, 1, A))], axis=1)      # the samplers' warm start
            if i >= warmup:
                res[name].append(dt)
    return {k: (float(np.median(v)), min(v), float(np.percentile(v, 90))) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100, help="calls between the two events")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200, help="timed get_action calls per model")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_logp.py measures on a GPU; none is visible")
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=30, seed=0)
    eng = make_engine(prob, p=20)
    lines = ["# The actor's log-density: its stage, its row call and what it adds to a call (tools/bench_policy_logp.py)", "",
             "Build %s, %s.  Device events around %d back-to-back calls, per call, median of %d rounds (fastest - slowest); H = 30, m = 1, "
             "n = 200, p = 20, D = 18, A = 6.  Nothing here is a bar." % (eng.lib.cadm_build_id().decode(), torch.cuda.get_device_name(eng.device),
                                                                        a.batch, a.rounds), "",
             "| call | rows | us | (min - max) |", "|---|---|---|---|"]
    for what, rows, (med, lo, hi) in device_times(eng, 200, a.batch, a.rounds):
        lines.append("| %s | %d | %.1f | %.1f - %.1f |" % (what, rows, med, lo, hi))
    eng.close()
    c = call_times(200, a.calls, a.warmup)
    keys = list(c)
    lines += ["", "`get_action` (cfg2 sizes, m = 1, n = 200, 5 iterations), two models taking turns call by call, %d calls after %d, median (min .. "
              "90th percentile), host clock:" % (a.calls, a.warmup), "", "| model | ms / get_action | (min .. p90) | against the row above |",
              "|---|---|---|---|"]
    for i, name in enumerate(keys):
        med, lo, p90 = c[name]
        lines.append("| %s | %.3f | %.3f .. %.3f | %s |" % (name, med, lo, p90, "" if i == 0 else "%+.3f ms" % (med - c[keys[i - 1]][0])))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
