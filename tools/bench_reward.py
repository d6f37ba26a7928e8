#!/usr/bin/env python3
"""The learned reward of the opt-in planner (csrc/reward.hip): what its stage costs against the value kernel on the same rows, and what
it adds to a get_action call.

Stage time: device events around BATCH back-to-back calls of `cadm_reward_returns` (both launches: the GEMM chain over the H m n p
(step, row) pairs and the step sum) on one stream, per call, on the trajectories of one planner iteration at the headline sizes (m = 1,
p = 20, H = 30, halfcheetah: 120 000 rows at 200 candidates, 1 200 000 at 2 000) for (128, 128) and (256, 256) relu nets and all three
`inputs`; median of ROUNDS rounds with the fastest and slowest.  Yardstick, timed in the same run: `cadm_value_eval` on the same number of
rows with the same hidden sizes, on an already registered value net.  Bar: the stage takes no longer than that time x (the reward net's
multiply-adds per row / the value net's) x 1.10.
Call time: `get_action` (numpy in, numpy out, one env, cfg2 sizes: halfcheetah, 4 x 200 swish, ensemble 5, 20 particles, H = 30,
5 iterations, 50 elites, 200 candidates) with `cem_noise_beta=1.0` alone against the same plus `cem_reward_net` (128, 128): two models
taking turns call by call, CALLS timed calls each after WARMUP, median with min .. 90th percentile.  Host clock around calls that end in
a stream synchronisation.
Writes a markdown table (--out, default stdout only).  Needs a GPU: there is no fallback."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cadm_amd import synth
from cadm_amd._lib import ptr
from cadm_amd.engine import HipEngine
from cadm_amd.synth import make_engine

NETS = [("128 x 2", (128, 128)), ("256 x 2", (256, 256))]
INPUTS = ("next_obs", "obs_act", "obs_act_next_obs")


def he_net(K, hidden, seed):
    rng = np.random.default_rng(seed)
    dims = [K] + list(hidden) + [1]
    return [((rng.standard_normal((dims[l], dims[l + 1])) * np.sqrt(2.0 / dims[l])).astype(np.float32),
             (0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32)) for l in range(len(dims) - 1)]


def macs(K, hidden):
    dims = [K] + list(hidden) + [1]
    return sum(dims[l] * dims[l + 1] for l in range(len(dims) - 1))


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


def stage_times(eng, n, batch, rounds):
    """rows of the table: (net, inputs, K, stage (median, min, max), value (median, min, max), MAC ratio)"""
    H, p, D, A = eng.H, eng.p, eng.D, eng.A
    R = H * n * p
    z = lambda *s: torch.empty(s, dtype=torch.float32, device=eng.device)
    traj, obs, actions = z(H, 1, n, p, D).normal_(), z(1, D).normal_(), z(1, n, H, A).uniform_(-1.0, 1.0)
    rows, states, v = z(1, n, p).uniform_(-30.0, 30.0), z(R, D).normal_(), z(R)
    ws = torch.empty((eng.lib.cadm_reward_workspace_bytes(eng._ctx, 1, n),), dtype=torch.uint8, device=eng.device)
    lib, ctx = eng.lib, eng._ctx
    out = []

    def check(rc, who):
        if rc != 0:
            raise RuntimeError("%s failed: %s" % (who, lib.cadm_last_error().decode()))

    for name, hidden in NETS:
        eng.set_value_net(HipEngine.value_params(hidden, "relu", 1.0), he_net(D, hidden, 1))
        check(lib.cadm_value_eval(ctx, ptr(states), R, ptr(v), eng.stream), "cadm_value_eval")
        val = timed(lambda: lib.cadm_value_eval(ctx, ptr(states), R, ptr(v), eng.stream), batch, rounds)
        for inputs in INPUTS:
            K = HipEngine.reward_input_dims(inputs, D, A)
            prm = HipEngine.reward_params(inputs, hidden, "relu", 1.0)
            eng.set_reward_net(prm, he_net(K, hidden, 2))
            call = lambda: lib.cadm_reward_returns(ctx, prm, ptr(traj), ptr(obs), ptr(actions), None, 1, n, ptr(rows), ptr(rows), None, None,
                                                   ptr(ws), eng.stream)
            check(call(), "cadm_reward_returns")
            rows.uniform_(-30.0, 30.0)
            out.append((name, inputs, K, timed(call, batch, rounds), val, macs(K, hidden) / macs(D, hidden)))
    return out


def call_times(n, calls, warmup):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import make_env_spec
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=30, seed=0, trained_like=True)
    st = prob["stats"]
    nz = {k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")}
    rn = dict(inputs="obs_act_next_obs", hidden_sizes=(128, 128), activation="relu", weight=1.0)
    settings = [("cem_noise_beta=1.0", dict(cem_noise_beta=1.0)), ("+ cem_reward_net (128, 128) relu, obs_act_next_obs", dict(cem_noise_beta=1.0, cem_reward_net=rn))]
    models = []
    for name, kw in settings:
        model = MLPEnsembleCEMDynamicsModel("dyn", make_env_spec("halfcheetah"), hidden_sizes=(200,) * 4, hidden_nonlinearity="swish", n_forwards=30,
                                            n_candidates=n, ensemble_size=5, n_particles=20, use_cem=True, normalize_input=True, seed=7, **kw)
        model.engine.set_net("context_model", prob["cp"])
        model.engine.set_net("ff_model", prob["ff"])
        model.set_normalization(nz)
        if "cem_reward_net" in kw:
            model.set_reward_net(he_net(2 * model.obs_space_dims + prob["A"], (128, 128), 2))
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
        raise SystemExit("bench_reward.py measures on a GPU; none is visible")
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=30, seed=0)
    eng = make_engine(prob, p=20)
    lines = ["# The learned reward's stage and what it adds to a call (tools/bench_reward.py)", "",
             "Build %s, %s.  Stage: device events around %d back-to-back calls of `cadm_reward_returns` (the GEMM launch and the step sum), "
             "per call, median of %d rounds (fastest - slowest); H = 30, m = 1, p = 20, D = 18, A = 6, relu.  Yardstick: `cadm_value_eval` "
             "on the same number of rows (H m n p) with the same hidden sizes, timed the same way in the same run.  Bar: stage <= yardstick x "
             "(multiply-adds per row of the reward net / of the value net) x 1.10." % (eng.lib.cadm_build_id().decode(),
                                                                                        torch.cuda.get_device_name(eng.device), a.batch, a.rounds), "",
             "| net | inputs | K | candidates | rows | stage us | (min - max) | value_eval us | (min - max) | MAC ratio | bar us | stage / bar | "
             "stage / (value x ratio) |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    missed = []
    for n in (200, 2000):
        for name, inputs, K, (med, lo, hi), (vmed, vlo, vhi), ratio in stage_times(eng, n, a.batch, a.rounds):
            bar = vmed * ratio * 1.10
            lines.append("| %s | %s | %d | %d | %d | %.1f | %.1f - %.1f | %.1f | %.1f - %.1f | %.3f | %.1f | %.2f%s | %.2f |"
                         % (name, inputs, K, n, eng.H * n * eng.p, med, lo, hi, vmed, vlo, vhi, ratio, bar, med / bar,
                            "" if med <= bar else " MISSED", med / (vmed * ratio)))
            if med > bar:
                missed.append((name, inputs, n))
    lines += ["", "The bar is %s." % ("met in every row" if not missed else "MISSED in: " + ", ".join("%s %s n=%d" % x for x in missed))]
    eng.close()
    c = call_times(200, a.calls, a.warmup)
    keys = list(c)
    lines += ["", "`get_action` (cfg2 sizes, m = 1, n = 200, 5 iterations), two models taking turns call by call, %d calls after %d, median (min .. "
              "90th percentile):" % (a.calls, a.warmup), "", "| model | ms / get_action | (min .. p90) | against the row above |", "|---|---|---|---|"]
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
