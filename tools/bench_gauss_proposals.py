#!/usr/bin/env python3
"""Proposals of the policy prior drawn from the actor's Gaussian head (csrc/policy_gauss.hip's roll flavour behind
`cadm_set_policy_proposals`): what the proposal roll costs under either source, and what the source does to an opt-in `get_action`.

Sizes: the headline model (halfcheetah with context, 4 x 200 swish, ensemble 5, p = 20 particles, H = 30), a (256, 256) relu actor with
a tanh squash whose last layer has 2 A outputs, log-std bounds (-5, 2) clamped, P = 24 proposals, at m = 1 and m = 10 envs.  The noise
route perturbs with noise_std = 0.3; the head route draws at std_scale = 1.
Measured: `cadm_policy_propose` (H policy steps, H - 1 one-step rollouts) under NOISE and under HEAD -- device events around BATCH
back-to-back calls on one stream, per call, median of ROUNDS rounds with the fastest and the slowest -- and `get_action` of the opt-in
planner with the prior (200 candidates, 5 iterations), two models taking turns call by call, host clock around calls that end in a
stream synchronisation: median of CALLS calls after WARMUP with the fastest and the 90th percentile.
With --parent DIR (a built checkout of the parent commit) `bench.py --gpus 1` runs on this tree and on that one, taking turns, each in
a fresh process, who goes first alternating: the default path launches nothing new, so the two sets must lie inside each other's spread.
Writes a markdown file (--out, default profiles/gauss_proposals.md).  Needs a GPU: there is no fallback."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from bench_gauss_policy import he_actor, headline, timed      # (tools/: the actor, `bench.py` in a tree, device events around a batch)
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd._lib import ptr
from cadm_amd.engine import HipEngine
from cadm_amd.synth import make_engine

HIDDEN, NOISE, P, H, N = (256, 256), 0.3, 24, 30, 200
HEAD = dict(kind="gaussian", log_std_bounds=(-5.0, 2.0), log_std_bound="clamp")


def roll(m, batch, rounds):
    """[(name, (median, min, max) us)] of `cadm_policy_propose` at m envs under either source, the build id and the device"""
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=m, H=H, seed=0, trained_like=True)
    eng = make_engine(prob, p=20)
    lib, ctx = eng.lib, eng._ctx
    mean_layers, W_ls, b_ls = hplanner.split_gaussian_layers(he_actor(eng.D, HIDDEN, eng.A, 1), eng.A)
    eng.set_policy_net(HipEngine.policy_params(HIDDEN, "relu", "tanh", 1, 0.0), mean_layers)
    eng.set_policy_head(hplanner.policy_head_params(HEAD, has_actor=True), W_ls, b_ls)
    obs, ctx_vec = eng._t(prob["obs"]), eng.context_forward(prob["cp_obs"], prob["cp_act"])
    out = []
    for source, noise in (("noise", NOISE), ("head", 0.0)):
        prm = HipEngine.policy_params(HIDDEN, "relu", "tanh", P, noise)
        eng.set_policy_proposals(source, 1.0)
        seqs = eng.policy_propose(prm, obs, ctx_vec, seed=1, call=1)      # (checks the route, sizes the workspace, builds nothing later)
        assert bool(torch.isfinite(seqs).all()) and not bool((seqs[:, 1] == seqs[:, 0]).all())
        ws = eng._policy_ws
        out.append(("`cadm_policy_propose`, m = %d, %s" % (m, "NOISE, noise_std = %g" % NOISE if source == "noise" else "HEAD, std_scale = 1"),
                    timed(lambda: lib.cadm_policy_propose(ctx, prm, ptr(obs), ptr(ctx_vec), m, 1, 1, ptr(seqs), None, ptr(ws), eng.stream),
                          batch, rounds)))
    bid, dev = lib.cadm_build_id().decode(), torch.cuda.get_device_name(eng.device)
    eng.close()
    return out, bid, dev


def call_times(m, calls, warmup):
    """{name: (median, min, 90th percentile) ms} of `get_action` with the prior under either source, two models taking turns"""
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import make_env_spec
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=m, H=H, seed=0, trained_like=True)
    st = prob["stats"]
    nz = {k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")}
    pp = dict(hidden_sizes=HIDDEN, activation="relu", squash="tanh", n_samples=P)
    settings = [("proposals=\"noise\", noise_std=%g" % NOISE, dict(pp, noise_std=NOISE)), ("proposals=\"head\", std_scale=1", dict(pp, proposals="head"))]
    models = []
    for name, prior in settings:
        model = MLPEnsembleCEMDynamicsModel("dyn", make_env_spec("halfcheetah"), hidden_sizes=(200,) * 4, hidden_nonlinearity="swish", n_forwards=H,
                                            n_candidates=N, ensemble_size=5, n_particles=20, use_cem=True, normalize_input=True, seed=7,
                                            cem_noise_beta=1.0, cem_policy_prior=prior, policy_head=HEAD)
        model.engine.set_net("context_model", prob["cp"])
        model.engine.set_net("ff_model", prob["ff"])
        model.set_normalization(nz)
        model.set_policy(he_actor(model.obs_space_dims, HIDDEN, prob["A"], 1))
        models.append((name, model))
    A = prob["A"]
    var = np.full((m, H, A), 0.25)
    state = {name: np.zeros((m, H, A)) for name, _ in models}
    res = {name: [] for name, _ in models}
    for i in range(warmup + calls):
        for name, model in models:
            t0 = time.perf_counter()
            plan = model.get_action(prob["obs"], prob["cp_obs"], prob["cp_act"], state[name], var)
            dt = (time.perf_counter() - t0) * 1e3
            state[name] = np.concatenate([plan[:, 1:], np.zeros((m, 1, A))], axis=1)      # the samplers' warm start
            if i >= warmup:
                res[name].append(dt)
    return {k: (float(np.median(v)), min(v), float(np.percentile(v, 90))) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20, help="`cadm_policy_propose` calls between the two events")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100, help="timed get_action calls per model")
    ap.add_argument("--call-warmup", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py's headline there and here, taking turns")
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauss_proposals.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gauss_proposals.py measures on a GPU; none is visible")
    lines = ["# Proposals drawn from the head: the roll and get_action under either source (tools/bench_gauss_proposals.py)", ""]
    for m in (1, 10):
        res, bid, dev = roll(m, a.batch, a.rounds)
        if m == 1:
            lines += ["Build %s, %s.  ONE run on ONE box.  Halfcheetah with context, E = 5, p = 20, H = %d, D = 18, A = 6, a (256, 256) relu actor "
                      "with 2 A outputs, log-std clamped to (-5, 2), P = %d proposals per env.  The roll: device events around %d back-to-back "
                      "calls on one stream, per call, median of %d rounds (fastest - slowest); %d policy steps and %d one-step rollouts per call."
                      % (bid, dev, H, P, a.batch, a.rounds, H, H - 1), ""]
        lines += ["## m = %d (%d rows per policy step)" % (m, m * P), "", "| what | us | (min - max) |", "|---|---|---|"]
        for name, (med, lo, hi) in res:
            lines.append("| %s | %.1f | %.1f - %.1f |" % (name, med, lo, hi))
        (n_med, n_lo, n_hi), (h_med, h_lo, h_hi) = res[0][1], res[1][1]
        lines += ["", "HEAD costs %.3f x NOISE (%+.1f us per roll, %+.2f us per policy step); the two spreads %s." %
                  (h_med / n_med, h_med - n_med, (h_med - n_med) / H, "overlap" if h_lo <= n_hi and n_lo <= h_hi else "do not overlap"), ""]
        c = call_times(m, a.calls, a.call_warmup)
        lines += ["`get_action` of the opt-in planner with the prior (n = %d, 5 iterations, cem_noise_beta = 1), two models taking turns call by "
                  "call, %d calls after %d, median (min .. 90th percentile):" % (N, a.calls, a.call_warmup), "",
                  "| cem_policy_prior | ms / get_action | (min .. p90) |", "|---|---|---|"]
        for name, (med, lo, p90) in c.items():
            lines.append("| %s | %.3f | %.3f .. %.3f |" % (name, med, lo, p90))
        lines.append("")
    if a.parent:
        here, there = [], []
        for turn in range(a.turns):      # (who goes first alternates: a process that follows another may find the card in another state)
            for tree in ((ROOT, a.parent) if turn % 2 == 0 else (a.parent, ROOT)):
                ms, bid = headline(os.path.abspath(tree), a.steps, a.warmup)
                if tree is ROOT:
                    here.append(ms)
                    bid_here = bid
                else:
                    there.append(ms)
                    bid_parent = bid
        inside = min(here) <= max(there) and min(there) <= max(here)
        lines += ["## bench.py's headline, this tree and the parent commit taking turns", "",
                  "`bench.py --gpus 1 --steps %d --warmup %d`, ms per get_action, %d turns each, a fresh process per run, in the order this, "
                  "parent, parent, this, this, ..  The default path launches nothing new; the two sets %s." %
                  (a.steps, a.warmup, a.turns, "lie inside each other's spread" if inside else "do NOT overlap"), "",
                  "| tree | build | ms per get_action, by turn | median |", "|---|---|---|---|",
                  "| this | %s | %s | %.4f |" % (bid_here, ", ".join("%.4f" % v for v in here), float(np.median(here))),
                  "| parent | %s | %s | %.4f |" % (bid_parent, ", ".join("%.4f" % v for v in there), float(np.median(there))), ""]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
