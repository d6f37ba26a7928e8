#!/usr/bin/env python3
"""The uncertainty cost of the opt-in planner (csrc/uncertainty.hip): the two kernels' own time next to the tracking kernel's on the same
trajectories, and what the term costs a `get_action`.

Call time: (a) `get_action` (numpy in, numpy out, one env, n = 200, 5 iterations, 50 elites) two ways in one process, the models taking
turns call by call: cem_noise_beta=1.0 alone; with cem_uncertainty (epistemic, every dim, lambda 0.5).  The model with the term records
every rollout's trajectories and adds two launches per CEM iteration (the step costs, and the cut + sum + cand -= lambda cost); it plans
other actions than the plain model, on rollouts of the same size.  Host clock around calls that end in a stream synchronisation; the
median over --calls calls after --warmup.
Kernel time: (b) device events around --batch back-to-back calls of `cadm_uncertainty_cost` with a step_out (its two launches: what the
loop enqueues, less the subtraction) on trajectories [30, 1, n, 20, 18] for n = 200 and n = 2000, per call, both kinds; the median round
with the fastest and slowest; (c) the same without a step_out (the one kernel that walks the steps); (d) `cadm_tracking_returns` of the
same build with K = 1 on the SAME buffer in the same run: the same bytes, read once, behind an H-step chain of loads.
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

H, N, P, A, D = 30, 200, 20, 6, 18
UNC = dict(cem_uncertainty=dict(kind="epistemic", weight=0.5))


def call_times(calls, warmup):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import make_env_spec
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=H, seed=0, trained_like=True)
    st = prob["stats"]
    nz = {k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")}
    settings = [("cem_noise_beta=1.0", {}), ("+ cem_uncertainty epistemic, lambda 0.5", UNC)]
    models = []
    for name, kw in settings:
        model = MLPEnsembleCEMDynamicsModel("dyn", make_env_spec("halfcheetah"), hidden_sizes=(200,) * 4, hidden_nonlinearity="swish", n_forwards=H,
                                            n_candidates=N, ensemble_size=5, n_particles=P, use_cem=True, normalize_input=True, seed=7,
                                            cem_noise_beta=1.0, **kw)
        model.engine.set_net("context_model", prob["cp"])
        model.engine.set_net("ff_model", prob["ff"])
        model.set_normalization(nz)
        models.append((name, model))
    var = np.full((1, H, A), 0.25)
    state = {name: np.zeros((1, H, A)) for name, _ in models}
    res = {name: [] for name, _ in models}
    for i in range(warmup + calls):
        for name, model in models:
            t0 = time.perf_counter()
            plan = model.get_action(prob["obs"], prob["cp_obs"], prob["cp_act"], state[name], var)
            dt = time.perf_counter() - t0
            if i >= warmup:
                res[name].append(dt * 1e3)
            if not np.isfinite(plan).all():
                raise RuntimeError("call %d of %r: the plan is not finite" % (i, name))
            state[name] = np.concatenate([plan[:, 1:], np.zeros((1, 1, A))], axis=1)      # the samplers' warm start
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
    """{name: (median, min, max)} in microseconds per call on traj [H, 1, n, P, D]"""
    traj = torch.randn((H, 1, n, P, D), dtype=torch.float32, device=eng.device)
    rows = torch.zeros((1, n, P), dtype=torch.float32, device=eng.device)
    out = torch.empty_like(rows)
    step = torch.empty((1, n, H), dtype=torch.float32, device=eng.device)
    cost = torch.empty((1, n), dtype=torch.float32, device=eng.device)
    targets = torch.zeros((1, 1, 1), dtype=torch.float32, device=eng.device)
    lib, ctx = eng.lib, eng._ctx
    track = HipEngine.track_params([dict(dim=0, kind="square", w=1.0)])
    res = {}
    for kind in ("epistemic", "total"):
        unc = HipEngine.uncertainty_params(kind, 0.5, obs_dim=D)
        res["cadm_uncertainty_cost, %s: steps + apply" % kind] = _time(
            lambda: lib.cadm_uncertainty_cost(ctx, unc, ptr(traj), None, 1, n, ptr(step), ptr(cost), eng.stream), batch, rounds, lib)
        res["cadm_uncertainty_cost, %s: no step_out (one walking kernel)" % kind] = _time(
            lambda: lib.cadm_uncertainty_cost(ctx, unc, ptr(traj), None, 1, n, None, ptr(cost), eng.stream), batch, rounds, lib)
    res["cadm_tracking_returns, K = 1"] = _time(
        lambda: lib.cadm_tracking_returns(ctx, track, ptr(traj), ptr(targets), 1, None, None, ptr(rows), 1, n, ptr(out), None, eng.stream),
        batch, rounds, lib)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed get_action calls per model")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=100, help="kernel calls between the two events")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_uncertainty.py measures on a GPU; none is visible")
    c, eng = call_times(a.calls, a.warmup)
    base = c["cem_noise_beta=1.0"][0]
    lines = ["# Uncertainty cost: the kernels' time and the cost per call (tools/bench_uncertainty.py)", "",
             "Build %s, %s.  `get_action` at cfg2 sizes (m = 1, n = %d, p = %d, H = %d), the two models taking turns call by call; %d calls "
             "after %d warm-up calls.  The model with the term records every rollout's trajectories and adds two launches per CEM iteration "
             "(the step costs; the cut, the sum and cand -= lambda cost); it plans other actions than the plain model, on rollouts of the same size."
             % (eng.lib.cadm_build_id().decode(), torch.cuda.get_device_name(eng.device), N, P, H, a.calls, a.warmup), "",
             "| get_action | median ms | min | p90 | x plain |", "|---|---|---|---|---|"]
    for name, (med, lo, p90) in c.items():
        lines.append("| %s | %.3f | %.3f | %.3f | %.3f |" % (name, med, lo, p90, med / base))
    for n in (N, 10 * N):
        k = kernel_times(eng, n, a.batch, a.rounds)
        ref = k["cadm_tracking_returns, K = 1"][0]
        nbytes = H * n * P * D * 4
        lines += ["", "Kernels alone on trajectories [%d, 1, %d, %d, %d] (%.2f MB, read once by each): device events around %d back-to-back calls, "
                  "per call, median of %d rounds:" % (H, n, P, D, nbytes / 1e6, a.batch, a.rounds), "",
                  "| call | us / call | (min - max) | x tracking | GB/s of traj |", "|---|---|---|---|---|"]
        for name, (med, lo, hi) in k.items():
            lines.append("| %s | %.2f | %.2f - %.2f | %.2f | %.0f |" % (name, med, lo, hi, med / ref, nbytes / med / 1e3))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
