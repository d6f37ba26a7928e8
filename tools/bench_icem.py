#!/usr/bin/env python3
"""The opt-in iCEM planner next to the default CEM at cfg2 sizes (halfcheetah, 4 x 200 swish, ensemble 5, 20 particles, H = 30):

  * latency of `get_action` (numpy in, numpy out, warm-started like the samplers) with default kwargs and with the iCEM kwargs;
  * planner quality ON THE MODEL ITSELF (no simulator): trained-like synthetic weights, 20 start states, one plan per start and
    setting, every plan re-scored by ONE common rollout with fixed noise.

python tools/bench_icem.py [--calls 200] [--md profiles/icem_planner.md]   -- prints a markdown table (and writes it with --md)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cadm_amd import synth
from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
from cadm_amd.envs import EnvSpec

ICEM = dict(cem_noise_beta=2.0, cem_keep_elites=15, cem_decay=1.25)
H, A, D, Hh = 30, 6, 18, 10


def make_model(prob, n, **kw):
    model = MLPEnsembleCEMDynamicsModel("dyn", EnvSpec("halfcheetah"), n_candidates=n, n_particles=20, ensemble_size=5, use_cem=True,
                                        n_forwards=H, seed=1, **kw)
    model.engine.set_net("context_model", prob["cp"])
    model.engine.set_net("ff_model", prob["ff"])
    st = prob["stats"]
    model.set_normalization({k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")})
    return model


def latency(model, prob, calls):
    obs, cpo, cpa = prob["obs"][:1], prob["cp_obs"][:1], prob["cp_act"][:1]
    mean, var = np.zeros((1, H, A)), np.full((1, H, A), 0.25)
    for _ in range(10):
        model.get_action(obs, cpo, cpa, mean, var)
    best = float("inf")
    for _ in range(3):
        model.reset_plan_carry()
        mean = np.zeros((1, H, A))
        t0 = time.perf_counter()
        for _ in range(calls):
            plan = model.get_action(obs, cpo, cpa, mean, var)
            mean = np.concatenate([plan[:, 1:], np.zeros((1, 1, A))], axis=1)
        best = min(best, (time.perf_counter() - t0) / calls)
    return best * 1e3


def rescore(scorer, prob, plan):
    """Model-predicted return of every start's plan under one common rollout: the scorer's engine, fixed (seed, call, it)."""
    eng = scorer.engine
    ctx = eng.context_forward(prob["cp_obs"], prob["cp_act"])
    rows = eng.rollout_returns(prob["obs"], ctx, np.ascontiguousarray(plan[:, None]), seed=12345, call=1, it=0)
    return rows.mean(dim=(1, 2)).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--starts", type=int, default=20)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=args.starts, H=H, seed=11, trained_like=True)
    lines = ["| setting | n | ms / get_action (m = 1) | model-predicted return, mean over %d starts | s.e.m. |" % args.starts, "|---|---|---|---|---|"]
    settings = [("default CEM", 200, {}), ("iCEM beta=2 K=15 decay=1.25", 200, ICEM), ("iCEM beta=2 K=15 decay=1.25", 100, ICEM),
                ("iCEM beta=2 K=15 decay=1.25, return best", 100, dict(ICEM, cem_return="best")), ("iCEM beta=2 K=15 decay=1.25", 50, ICEM)]
    scorer = make_model(prob, 200)
    scorer._push_stats()
    mean, var = np.zeros((args.starts, H, A)), np.full((args.starts, H, A), 0.25)
    for name, n, kw in settings:
        model = make_model(prob, n, **kw)
        ms = latency(model, prob, args.calls)
        model.reset_plan_carry()
        model._call = 0
        plan = model.get_action(prob["obs"], prob["cp_obs"], prob["cp_act"], mean, var)
        ret = rescore(scorer, prob, plan)
        lines.append("| %s | %d | %.3f | %.3f | %.3f |" % (name, n, ms, ret.mean(), ret.std(ddof=1) / np.sqrt(len(ret))))
        model.engine.close()
    torch.cuda.synchronize()
    out = "\n".join(lines)
    print(out)
    if args.md:
        with open(args.md, "w") as f:
            f.write(HEADER + out + "\n" + FOOTER)


HEADER = """# iCEM planner next to the default CEM (tools/bench_icem.py)

cfg2 sizes: halfcheetah, 4 x 200 swish, ensemble 5, 20 particles, H = 30, 5 CEM iterations, 50 elites; trained-like synthetic weights
(cadm_amd/synth.py).  Latency: `get_action`, numpy in / numpy out, one env, warm-started like the samplers, best of 3 runs.
Quality: one plan per start state and setting from a zero warm start; every plan re-scored by one common rollout of the same model
with fixed noise.  With decay 1.25 the five iterations roll out 200, 160, 128, 102, 100 candidates of n = 200 (never fewer than
2 x 50 elites): n = 100 and n = 50 stay at 100 and 50.

"""
FOOTER = """
The return is what the MODEL predicts for the plan: it shows whether fewer candidates hold the planner's own objective.  Closed-loop
quality on a real environment is unmeasured (no simulator here), and no threshold was fixed in advance.

The iCEM route is the stepwise sequence of launches per iteration (sample, inject, [mean candidate], rollout, particle mean, refit,
track-best, keep) against the default route's fused refit + sample kernel and staged host call: what its latency carries beyond
the rollouts is those small launches and a stream synchronisation instead of the staged call's completion flags.  Candidates to fuse,
not fused in this change: inject + mean candidate into the sampler; particle mean + track-best + keep into the refit kernel.
"""


if __name__ == "__main__":
    main()
