#!/usr/bin/env python3
"""The policy prior of the opt-in planner (csrc/policy.hip): what the proposal roll costs, and what it adds to a get_action call.

Sizes: the headline geometry (halfcheetah with context, 4 x 200 swish, ensemble 5, 20 particles, H = 30, 5 iterations, 50 elites, one
env, 200 candidates), a (256, 256) relu policy with a tanh squash, P = 24 proposals, noise_std = 0.3.
One policy step: device events around BATCH back-to-back calls of `cadm_policy_eval` on the P rows of one env (one launch of
policy_step_kernel at p = 1) and on P * 20 rows (the roll's reads of a step, as rows), per call; median of ROUNDS rounds with the fastest
and slowest.  The roll: the same around `cadm_policy_propose` (H policy steps and H - 1 one-step rollouts: 2 H - 1 launches).
Call time: `get_action` (numpy in, numpy out) with `cem_noise_beta=1.0` alone against the same plus `cem_policy_prior`: two models taking
turns call by call, CALLS timed calls each after WARMUP, median with min .. 90th percentile.  Host clock around calls that end in a
stream synchronisation.
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

HIDDEN, P, NOISE, H, N = (256, 256), 24, 0.3, 30, 200


def he_policy(D, hidden, A, seed):
    rng = np.random.default_rng(seed)
    dims = [D] + list(hidden) + [A]
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


def roll_times(batch, rounds):
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=H, seed=0, trained_like=True)
    eng = make_engine(prob, p=20)
    lib, ctx = eng.lib, eng._ctx
    prm = HipEngine.policy_params(HIDDEN, "relu", "tanh", P, NOISE)
    eng.set_policy_net(prm, he_policy(eng.D, HIDDEN, eng.A, 1))
    obs = eng._t(prob["obs"])
    ctx_vec = eng.context_forward(prob["cp_obs"], prob["cp_act"])
    seqs = eng.policy_propose(prm, obs, ctx_vec, seed=1, call=1)      # (builds the workspace, checks the rollout)
    assert torch.isfinite(seqs).all()
    ws = eng._policy_ws
    out = []
    for rows in (P, P * eng.p):
        x = torch.empty((rows, eng.D), dtype=torch.float32, device=eng.device).normal_()
        a = torch.empty((rows, eng.A), dtype=torch.float32, device=eng.device)
        out.append(("one policy step, %d rows (`cadm_policy_eval`)" % rows,
                    timed(lambda: lib.cadm_policy_eval(ctx, ptr(x), rows, ptr(a), eng.stream), batch, rounds)))
    out.append(("the roll, %d launches (`cadm_policy_propose`)" % (2 * H - 1),
                timed(lambda: lib.cadm_policy_propose(ctx, prm, ptr(obs), ptr(ctx_vec), 1, 1, 1, ptr(seqs), None, ptr(ws), eng.stream),
                      max(batch // 10, 1), rounds)))
    bid, dev = eng.lib.cadm_build_id().decode(), torch.cuda.get_device_name(eng.device)
    eng.close()
    return out, bid, dev


def call_times(calls, warmup):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import make_env_spec
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=H, seed=0, trained_like=True)
    st = prob["stats"]
    nz = {k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")}
    pp = dict(hidden_sizes=HIDDEN, activation="relu", squash="tanh", n_samples=P, noise_std=NOISE)
    settings = [("cem_noise_beta=1.0", dict(cem_noise_beta=1.0)),
                ("+ cem_policy_prior (256, 256) relu, %d proposals" % P, dict(cem_noise_beta=1.0, cem_policy_prior=pp))]
    models = []
    for name, kw in settings:
        model = MLPEnsembleCEMDynamicsModel("dyn", make_env_spec("halfcheetah"), hidden_sizes=(200,) * 4, hidden_nonlinearity="swish", n_forwards=H,
                                            n_candidates=N, ensemble_size=5, n_particles=20, use_cem=True, normalize_input=True, seed=7, **kw)
        model.engine.set_net("context_model", prob["cp"])
        model.engine.set_net("ff_model", prob["ff"])
        model.set_normalization(nz)
        if "cem_policy_prior" in kw:
            model.set_policy(he_policy(model.obs_space_dims, HIDDEN, prob["A"], 1))
        models.append((name, model))
    A = prob["A"]
    var = np.full((1, H, A), 0.25)
    state = {name: np.zeros((1, H, A)) for name, _ in models}
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
    ap.add_argument("--batch", type=int, default=200, help="calls between the two events (a tenth of it for the roll)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200, help="timed get_action calls per model")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy.py measures on a GPU; none is visible")
    rows, bid, dev = roll_times(a.batch, a.rounds)
    lines = ["# The policy prior's roll and what it adds to a call (tools/bench_policy.py)", "",
             "Build %s, %s.  Device events around back-to-back calls on one stream, per call, median of %d rounds (fastest - slowest); halfcheetah "
             "with context, m = 1, p = 20, H = %d, D = 18, A = 6, a (256, 256) relu policy, tanh squash, P = %d, noise_std = %g."
             % (bid, dev, a.rounds, H, P, NOISE), "", "| what | us | (min - max) |", "|---|---|---|"]
    for name, (med, lo, hi) in rows:
        lines.append("| %s | %.1f | %.1f - %.1f |" % (name, med, lo, hi))
    c = call_times(a.calls, a.warmup)
    keys = list(c)
    lines += ["", "`get_action` (m = 1, n = %d, 5 iterations), two models taking turns call by call, %d calls after %d, median (min .. 90th "
              "percentile):" % (N, a.calls, a.warmup), "", "| model | ms / get_action | (min .. p90) | against the row above |", "|---|---|---|---|"]
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
