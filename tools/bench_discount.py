#!/usr/bin/env python3
"""The discount over the horizon of the opt-in planner (csrc/discount.hip): the env-return kernel's own time next to the constraint
kernel's, and what a discount costs a `get_action`.

Call time: (a) `get_action` (numpy in, numpy out, one env, n = 200, 5 iterations, 50 elites) through the class with a terminal value
(one hidden layer of 64), two ways in one process, the models taking turns call by call: cem_discount=1.0 (no table: the loop of the
terminal value alone) and cem_discount=0.99.  The discounted model adds one launch per CEM iteration, `cadm_discount_returns` behind
the rollout; both record trajectories (the terminal value reads them).  Host clock around calls that end in a stream synchronisation;
the median over --calls calls after --warmup.
Kernel time: (b) device events around --batch back-to-back launches of `cadm_discount_returns` on traj [30, 1, 200, 20, 18] (4000 rows),
per launch; the median round with the fastest and slowest; (c) the yardstick, in the same run: `cadm_constrain_returns` in TERMINATE mode
on the same trajectories with no table set -- the launch every earlier build makes -- under bounds nothing violates and with the
violation counts asked for, so that no row and no workgroup stops early: the same loads and the same reward chain, plus its tests.
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
GAMMA = 0.99
VALUE = dict(hidden_sizes=(64,), activation="relu", weight=1.0)


def value_net(rng):
    return [((rng.standard_normal((D, 64)) * np.sqrt(2.0 / D)).astype(np.float32), np.zeros(64, np.float32)),
            ((rng.standard_normal((64, 1)) * np.sqrt(2.0 / 64)).astype(np.float32), np.zeros(1, np.float32))]


def call_times(calls, warmup):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import make_env_spec
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=H, seed=0, trained_like=True)
    st = prob["stats"]
    nz = {k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")}
    settings = [("terminal value, cem_discount=1.0", 1.0), ("terminal value, cem_discount=%g" % GAMMA, GAMMA)]
    models = []
    for name, gamma in settings:
        model = MLPEnsembleCEMDynamicsModel("dyn", make_env_spec("halfcheetah"), hidden_sizes=(200,) * 4, hidden_nonlinearity="swish", n_forwards=H,
                                            n_candidates=N, ensemble_size=5, n_particles=P, use_cem=True, normalize_input=True, seed=7,
                                            cem_terminal_value=VALUE, cem_discount=gamma)
        model.engine.set_net("context_model", prob["cp"])
        model.engine.set_net("ff_model", prob["ff"])
        model.set_normalization(nz)
        model.set_terminal_value(value_net(np.random.default_rng(1)))
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
    return {k: (float(np.median(v)), min(v), float(np.percentile(v, 90))) for k, v in res.items()}, models[0][1].engine, models[1][1].engine


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


def kernel_times(plain, disc, n, batch, rounds):
    """{name: (median, min, max)} in microseconds per launch on traj [H, 1, n, P, D]: the constraint kernel on the engine without a
    table, the discount kernel on the engine with one"""
    dev = plain.device
    g = torch.Generator(device="cpu").manual_seed(3)
    traj = torch.randn((H, 1, n, P, D), generator=g).to(dev)
    obs = torch.randn((1, D), generator=g).to(dev)
    acts = (torch.rand((1, n, H, A), generator=g) * 2 - 1).to(dev)
    rows = torch.randn((1, n, P), generator=g).to(dev)
    out = torch.empty_like(rows)
    first = torch.empty((1, n, P), dtype=torch.int32, device=dev)
    viol = torch.empty((1, n, P), dtype=torch.int32, device=dev)
    never = HipEngine.constraint_params([dict(dim=0, lo=-3e38, hi=3e38), dict(dim=5, lo=-3e38, hi=3e38)], "terminate", 1.0)
    res = {}
    res["cadm_constrain_returns, terminate, no table"] = _time(
        lambda: plain.lib.cadm_constrain_returns(plain._ctx, never, ptr(traj), ptr(obs), ptr(acts), ptr(rows), 1, n, ptr(out), ptr(first), ptr(viol),
                                                 plain.stream), batch, rounds, plain.lib)
    torch.cuda.synchronize()
    if int(viol.abs().max()) != 0 or int((first != H).sum()) != 0:
        raise RuntimeError("the yardstick's constraints must not bind")
    res["cadm_discount_returns"] = _time(
        lambda: disc.lib.cadm_discount_returns(disc._ctx, ptr(traj), ptr(obs), ptr(acts), 1, n, ptr(rows), ptr(out), None, disc.stream),
        batch, rounds, disc.lib)
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
        raise SystemExit("bench_discount.py measures on a GPU; none is visible")
    c, plain, disc = call_times(a.calls, a.warmup)
    base = c["terminal value, cem_discount=1.0"][0]
    lines = ["# Discount over the horizon: the kernel's time and the cost per call (tools/bench_discount.py)", "",
             "Build %s, %s.  `get_action` at cfg2 sizes (m = 1, n = %d, p = %d, H = %d) through the class with a terminal value (one hidden "
             "layer of 64), the two models taking turns call by call; %d calls after %d warm-up calls.  The discounted model adds one launch "
             "per CEM iteration (`cadm_discount_returns` behind the rollout); both record trajectories."
             % (plain.lib.cadm_build_id().decode(), torch.cuda.get_device_name(plain.device), N, P, H, a.calls, a.warmup), "",
             "| get_action | median ms | min | p90 | x no discount |", "|---|---|---|---|---|"]
    for name, (med, lo, p90) in c.items():
        lines.append("| %s | %.3f | %.3f | %.3f | %.3f |" % (name, med, lo, p90, med / base))
    k = kernel_times(plain, disc, N, a.batch, a.rounds)
    ref = k["cadm_constrain_returns, terminate, no table"]
    lines += ["", "Kernels alone on traj [%d, 1, %d, %d, %d] (%d rows, %.1f MB): device events around %d back-to-back launches, per launch, "
              "median of %d rounds.  The yardstick is the TERMINATE constraint kernel with no table set (the launch of every earlier build), "
              "under bounds nothing violates and with the counts asked for, so that it walks all %d steps: the same loads and reward chain, "
              "plus its tests." % (H, N, P, D, N * P, H * N * P * D * 4 / 1e6, a.batch, a.rounds, H), "",
              "| kernel | us / launch | (min - max) | x yardstick |", "|---|---|---|---|"]
    for name, (med, lo, hi) in k.items():
        lines.append("| %s | %.2f | %.2f - %.2f | %.2f |" % (name, med, lo, hi, med / ref[0]))
    new = k["cadm_discount_returns"]
    spread = ref[2] - ref[1]
    if new[0] <= ref[0] + spread:
        lines += ["", "The new kernel costs no more than the yardstick plus the run's own spread (%.2f us)." % spread]
    else:
        lines += ["", "The new kernel costs %.2f us more than the yardstick (spread of the yardstick in this run: %.2f us)." % (new[0] - ref[0], spread)]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
