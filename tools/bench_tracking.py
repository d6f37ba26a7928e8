#!/usr/bin/env python3
"""Tracking targets in the opt-in planner (csrc/tracking.hip): the kernel's own time next to the constraint kernel's, and what
tracking costs a `get_action`.

Kernel time: device events around --batch back-to-back launches at the bench headline geometry (halfcheetah, E = 5, p = 20, H = 30,
m = 1; traj [30, 1, n, 20, 18]) for n = 200 and n = 2000, per launch; the median round with the fastest and slowest:
  (a) `cadm_tracking_returns` with K = 1 and K = 16 terms (square / abs / huber in turn, a constant goal, no NaN: every pair is counted);
  (b) `cadm_constrain_returns` in penalty mode with two never-binding constraints at the same shape: it reads the same bytes once.
      The constraint kernel is whatever the loaded library holds; run this tool in a checkout of another commit to time that commit's.
Call time: (c) `get_action` (numpy in, numpy out, one env, n = 200, 5 iterations, 50 elites) three ways in one process, the models
taking turns call by call: cem_noise_beta=1.0 alone; with a never-binding penalty constraint (it already pays for recording the
trajectories); with cem_tracking (K = 2, targets that are all NaN plan the same actions, so the three differ by the features' cost
alone -- the kernel still runs its whole chain of loads).  Host clock around calls that end in a stream synchronisation; the median over
--calls calls after --warmup.
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

NEVER = [dict(dim=0, lo=-3e38, hi=3e38), dict(dim=8, lo=-3e38, hi=3e38)]
KINDS = ("square", "abs", "huber")
H, N, P, D, A = 30, 200, 20, 18, 6


def call_times(calls, warmup):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import make_env_spec
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=H, seed=0, trained_like=True)
    st = prob["stats"]
    nz = {k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")}
    settings = [("cem_noise_beta=1.0", {}),
                ("+ never-binding constraint, penalty", dict(cem_constraints=NEVER, cem_constraint_mode="penalty", cem_constraint_weight=1.0)),
                ("+ cem_tracking, K = 2, all-NaN targets", dict(cem_tracking=[dict(dim=0, w=1.0), dict(dim=8, kind="huber", w=1.0, delta=1.0)]))]
    models = []
    for name, kw in settings:
        model = MLPEnsembleCEMDynamicsModel("dyn", make_env_spec("halfcheetah"), hidden_sizes=(200,) * 4, hidden_nonlinearity="swish", n_forwards=H,
                                            n_candidates=N, ensemble_size=5, n_particles=P, use_cem=True, normalize_input=True, seed=7,
                                            cem_noise_beta=1.0, **kw)
        model.engine.set_net("context_model", prob["cp"])
        model.engine.set_net("ff_model", prob["ff"])
        model.set_normalization(nz)
        if "cem_tracking" in kw:
            model.set_targets(np.full((1, H, 2), np.nan))
        models.append((name, model))
    var = np.full((1, H, A), 0.25)
    state = {name: np.zeros((1, H, A)) for name, _ in models}
    res = {name: [] for name, _ in models}
    for i in range(warmup + calls):
        plans = []
        for name, model in models:
            t0 = time.perf_counter()
            plan = model.get_action(prob["obs"], prob["cp_obs"], prob["cp_act"], state[name], var)
            dt = time.perf_counter() - t0
            if i >= warmup:
                res[name].append(dt * 1e3)
            state[name] = np.concatenate([plan[:, 1:], np.zeros((1, 1, A))], axis=1)      # the samplers' warm start
            plans.append(plan)
        if not all(np.array_equal(plans[0], q) for q in plans[1:]):
            raise RuntimeError("call %d: a never-binding constraint or all-NaN targets changed the plan" % i)
    return {k: (float(np.median(v)), min(v), float(np.percentile(v, 90))) for k, v in res.items()}, models[1][1].engine


def _time(launch, batch, rounds, lib):
    times = []
    for r in range(rounds + 1):                      # (round 0 warms the kernel up and is dropped)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(batch):
            rc = launch()
        e1.record()
        torch.cuda.synchronize()
        if rc != 0:
            raise RuntimeError("launch failed: %s" % lib.cadm_last_error().decode())
        if r > 0:
            times.append(e0.elapsed_time(e1) * 1e3 / batch)
    return float(np.median(times)), min(times), max(times)


def kernel_times(eng, n, batch, rounds):
    """{name: (median, min, max)} in microseconds per launch at traj [H, 1, n, P, D]"""
    traj = torch.empty((H, 1, n, P, D), dtype=torch.float32, device=eng.device).normal_()
    rows = torch.empty((1, n, P), dtype=torch.float32, device=eng.device).uniform_(-30.0, 30.0)
    out = torch.empty_like(rows)
    lib, ctx = eng.lib, eng._ctx
    res = {}
    for K in (1, 16):
        terms = [dict(dim=(5 * k) % D, kind=KINDS[k % 3], w=1.0, **(dict(delta=1.0) if k % 3 == 2 else {})) for k in range(K)]
        prm = HipEngine.track_params(terms)
        targets = torch.zeros((1, 1, K), dtype=torch.float32, device=eng.device)
        res["cadm_tracking_returns, K = %d" % K] = _time(
            lambda: lib.cadm_tracking_returns(ctx, prm, ptr(traj), ptr(targets), 1, None, None, ptr(rows), 1, n, ptr(out), None, eng.stream),
            batch, rounds, lib)
    cprm = HipEngine.constraint_params(NEVER, "penalty", 1.0)
    res["cadm_constrain_returns, penalty"] = _time(
        lambda: lib.cadm_constrain_returns(ctx, cprm, ptr(traj), None, None, ptr(rows), 1, n, ptr(out), None, None, eng.stream), batch, rounds, lib)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed get_action calls per model")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=100, help="kernel launches between the two events")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tracking.py measures on a GPU; none is visible")
    c, eng = call_times(a.calls, a.warmup)
    base = c["cem_noise_beta=1.0"][0]
    lines = ["# Tracking targets: the kernel's time and the cost per call (tools/bench_tracking.py)", "",
             "Build %s, %s.  `get_action` at the bench headline sizes (m = 1, n = %d, p = %d, H = %d), the three models taking turns call by "
             "call; %d calls after %d warm-up calls." % (eng.lib.cadm_build_id().decode(), torch.cuda.get_device_name(eng.device), N, P, H, a.calls,
                                                          a.warmup), "",
             "| get_action | median ms | min | p90 | x plain |", "|---|---|---|---|---|"]
    for name, (med, lo, p90) in c.items():
        lines.append("| %s | %.3f | %.3f | %.3f | %.3f |" % (name, med, lo, p90, med / base))
    for n in (N, 10 * N):
        k = kernel_times(eng, n, a.batch, a.rounds)
        ref = k["cadm_constrain_returns, penalty"][0]
        lines += ["", "Kernels alone at traj [%d, 1, %d, %d, %d] (%.1f MB): device events around %d back-to-back launches, per launch, median "
                  "of %d rounds:" % (H, n, P, D, H * n * P * D * 4 / 1e6, a.batch, a.rounds), "",
                  "| kernel | us / launch | (min - max) | x constrain |", "|---|---|---|---|"]
        for name, (med, lo, hi) in k.items():
            lines.append("| %s | %.2f | %.2f - %.2f | %.2f |" % (name, med, lo, hi, med / ref))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
