#!/usr/bin/env python3
"""The actuator model of the opt-in planner (csrc/actuator.hip): the actuate kernel's own time next to the knot kernel's, and what the
model costs a `get_action`.

Call time: (a) `get_action` (numpy in, numpy out, one env, n = 200, 5 iterations, 50 elites) two ways in one process, the models taking
turns call by call: cem_noise_beta=1.0 alone; with cem_action_delay=2, a rate limit and a rate cost on every dim.  The actuated model adds
per CEM iteration one actuate launch and one cand -= cost launch, and per call the plan's last pass, its copy to the host buffer and the
state's advance; it plans other actions than the plain model, on rollouts of the same size.  Host clock around calls that end in a
stream synchronisation; the median over --calls calls after --warmup.
Kernel time: (b) device events around --batch back-to-back launches of `cadm_actuate_actions` (delay 2, every dim limited and priced,
the cost written) on [1, n, 30, 6] for n = 200 and n = 2000, per launch; the median round with the fastest and slowest;
(c) `cadm_shape_actions` of the same build (spacing 3, hold, phase 1) at the same sizes beside it: the same traffic.
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

H, N, P, A = 30, 200, 20, 6
ACT = dict(cem_action_delay=2, cem_action_rate_limit=0.25, cem_action_rate_cost=0.1)


def call_times(calls, warmup):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import make_env_spec
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=H, seed=0, trained_like=True)
    st = prob["stats"]
    nz = {k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")}
    settings = [("cem_noise_beta=1.0", {}), ("+ delay 2, rate limit 0.25, rate cost 0.1", ACT)]
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
    """{name: (median, min, max)} in microseconds per launch on seqs [1, n, H, A]"""
    seqs = torch.empty((1, n, H, A), dtype=torch.float32, device=eng.device).uniform_(-1.0, 1.0)
    prev = torch.zeros((1, A), dtype=torch.float32, device=eng.device)
    prefix = torch.zeros((1, 2, A), dtype=torch.float32, device=eng.device)
    cost = torch.empty((1, n), dtype=torch.float32, device=eng.device)
    phase = torch.ones((1,), dtype=torch.int32, device=eng.device)
    lib, ctx = eng.lib, eng._ctx
    act = HipEngine.actuator_params(2, 0.25, 0.1, action_dim=A, horizon=H)
    knots = HipEngine.knot_params(3, "hold")
    res = {}
    res["cadm_actuate_actions"] = _time(lambda: lib.cadm_actuate_actions(ctx, act, ptr(prev), ptr(prefix), 1, n, ptr(seqs), ptr(cost), eng.stream),
                                        batch, rounds, lib)
    res["cadm_shape_actions, hold"] = _time(lambda: lib.cadm_shape_actions(ctx, knots, ptr(phase), 1, n, ptr(seqs), eng.stream), batch, rounds, lib)
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
        raise SystemExit("bench_actuator.py measures on a GPU; none is visible")
    c, eng = call_times(a.calls, a.warmup)
    base = c["cem_noise_beta=1.0"][0]
    lines = ["# Actuator model: the kernel's time and the cost per call (tools/bench_actuator.py)", "",
             "Build %s, %s.  `get_action` at cfg2 sizes (m = 1, n = %d, p = %d, H = %d), the two models taking turns call by call; %d calls "
             "after %d warm-up calls.  The actuated model adds two launches per CEM iteration (actuate, cand -= cost) and three per call (the "
             "plan's last pass, its copy out, the state's advance); it plans other actions than the plain model, on rollouts of the same size."
             % (eng.lib.cadm_build_id().decode(), torch.cuda.get_device_name(eng.device), N, P, H, a.calls, a.warmup), "",
             "| get_action | median ms | min | p90 | x plain |", "|---|---|---|---|---|"]
    for name, (med, lo, p90) in c.items():
        lines.append("| %s | %.3f | %.3f | %.3f | %.3f |" % (name, med, lo, p90, med / base))
    for n in (N, 10 * N):
        k = kernel_times(eng, n, a.batch, a.rounds)
        ref = k["cadm_shape_actions, hold"][0]
        lines += ["", "Kernels alone on [1, %d, %d, %d] floats (%.0f KB): device events around %d back-to-back launches, per launch, median of "
                  "%d rounds:" % (n, H, A, n * H * A * 4 / 1e3, a.batch, a.rounds), "",
                  "| kernel | us / launch | (min - max) | x shape |", "|---|---|---|---|"]
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
