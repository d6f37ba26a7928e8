#!/usr/bin/env python3
"""Risk-aware candidate scores (csrc/score.hip) next to the plain particle mean: kernel time and get_action call time.

Kernel time: device events around BATCH back-to-back launches of one entry point on one stream, per launch, at m n = 200 and 2000
candidates of p = 20 particles; every mode and `cadm_particle_mean` take turns inside each of ROUNDS rounds, the median round is
reported with the fastest and slowest.  The host's own time to enqueue the batch is printed beside it: where the two agree the
figure is the enqueue rate of this host, not the kernel.
Call time: `get_action` (numpy in, numpy out, one env, cfg2 sizes: halfcheetah, 4 x 200 swish, ensemble 5, 20 particles, H = 30,
n = 200, 5 iterations, 50 elites) on the opt-in route (coloured noise, 15 kept elites), cem_score="mean" against every other score
in the same process, the models taking turns; host clock around calls that end in a stream synchronisation.
Writes a markdown table (--out, default stdout only).  Needs a GPU: there is no fallback."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cadm_amd import _lib, synth
from cadm_amd._lib import ptr
from cadm_amd.engine import HipEngine
from cadm_amd.synth import make_engine

MODES = [("particle_mean", None), ("mean_std kappa=1", ("mean_std", 1.0, None)), ("member_std kappa=1", ("member_std", 1.0, None)),
         ("cvar k=2", ("cvar", 0.0, 2)), ("cvar k=10", ("cvar", 0.0, 10))]


def kernel_times(eng, total, batch, rounds):
    """{name: (median, min, max, host enqueue median)} in microseconds per launch"""
    rows = torch.empty((1, total, eng.p), dtype=torch.float32, device=eng.device).uniform_(-30.0, 30.0)
    out = torch.empty((1, total), dtype=torch.float32, device=eng.device)
    lib, ctx = eng.lib, eng._ctx
    calls = {}
    for name, sc in MODES:
        if sc is None:
            calls[name] = lambda: lib.cadm_particle_mean(ctx, ptr(rows), 1, total, ptr(out), eng.stream)
        else:
            prm = HipEngine.score_params(*sc)
            calls[name] = lambda prm=prm: lib.cadm_particle_score(ctx, ptr(rows), 1, total, prm, ptr(out), eng.stream)
    dev, host = {k: [] for k in calls}, {k: [] for k in calls}
    for r in range(rounds + 1):                          # (round 0 warms every kernel up and is dropped)
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(batch):
                rc = fn()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            if rc != 0:
                raise RuntimeError("%s failed: %s" % (name, lib.cadm_last_error().decode()))
            if r > 0:
                dev[name].append(e0.elapsed_time(e1) * 1e3 / batch)
                host[name].append((t1 - t0) * 1e6 / batch)
    return {k: (float(np.median(v)), min(v), max(v), float(np.median(host[k]))) for k, v in dev.items()}


def call_times(calls, rounds):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import make_env_spec
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=30, seed=0, trained_like=True)
    st = prob["stats"]
    nz = {k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")}
    settings = [("mean", {}), ("mean_std kappa=1", dict(cem_score="mean_std", cem_risk=1.0)),
                ("member_std kappa=1", dict(cem_score="member_std", cem_risk=1.0)), ("cvar alpha=0.1 (k=2)", dict(cem_score="cvar", cem_risk=0.1)),
                ("cvar alpha=0.5 (k=10)", dict(cem_score="cvar", cem_risk=0.5))]
    models = []
    for name, kw in settings:
        model = MLPEnsembleCEMDynamicsModel("dyn", make_env_spec("halfcheetah"), hidden_sizes=(200,) * 4, hidden_nonlinearity="swish", n_forwards=30,
                                            n_candidates=200, ensemble_size=5, n_particles=20, use_cem=True, normalize_input=True, seed=7,
                                            cem_noise_beta=2.0, cem_keep_elites=15, **kw)
        model.engine.set_net("context_model", prob["cp"])
        model.engine.set_net("ff_model", prob["ff"])
        model.set_normalization(nz)
        models.append((name, model))
    A = prob["A"]
    var = np.full((1, 30, A), 0.25)
    state = {name: np.zeros((1, 30, A)) for name, _ in models}

    def step(name, model):
        plan = model.get_action(prob["obs"], prob["cp_obs"], prob["cp_act"], state[name], var)
        state[name] = np.concatenate([plan[:, 1:], np.zeros((1, 1, A))], axis=1)      # the samplers' warm start

    res = {name: [] for name, _ in models}
    for r in range(rounds + 1):                          # (round 0: warm-up, dropped)
        for name, model in models:
            t0 = time.perf_counter()
            for _ in range(calls):
                step(name, model)
            if r > 0:
                res[name].append((time.perf_counter() - t0) * 1e3 / calls)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=200, help="launches between the two events")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="get_action calls per model and round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_risk.py measures on a GPU; none is visible")
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=30, seed=0)
    eng = make_engine(prob, p=20)
    lines = ["# Risk-aware candidate scores next to the particle mean (tools/bench_risk.py)", "",
             "Build %s, %s.  Kernel time: device events around %d back-to-back launches, per launch, median of %d rounds (fastest - slowest); "
             "p = 20, E = 5.  `host` is this host's time to enqueue one launch in the same loop." % (
                 eng.lib.cadm_build_id().decode(), torch.cuda.get_device_name(eng.device), a.batch, a.rounds), "",
             "| entry | m n | us / launch | (min - max) | host us / launch | x particle_mean |", "|---|---|---|---|---|---|"]
    for total in (200, 2000):
        t = kernel_times(eng, total, a.batch, a.rounds)
        base = t["particle_mean"][0]
        for name, _ in MODES:
            med, lo, hi, h = t[name]
            lines.append("| %s | %d | %.2f | %.2f - %.2f | %.2f | %.2f |" % (name, total, med, lo, hi, h, med / base))
    c = call_times(a.calls, a.rounds)
    base = c["mean"][0]
    lines += ["", "`get_action` on the opt-in route (cfg2 sizes, m = 1, n = 200, cem_noise_beta=2, cem_keep_elites=15), %d calls per round, "
              "median of %d rounds, the models taking turns:" % (a.calls, a.rounds), "",
              "| cem_score | ms / get_action | (min - max) | x mean |", "|---|---|---|---|"]
    for name, (med, lo, hi) in c.items():
        lines.append("| %s | %.3f | %.3f - %.3f | %.3f |" % (name, med, lo, hi, med / base))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
