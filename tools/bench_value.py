#!/usr/bin/env python3
"""The terminal value of the opt-in planner (csrc/value.hip): what its launch costs and what it adds to a get_action call.

Kernel time: device events around BATCH back-to-back launches of `cadm_value_returns` on one stream, per launch, on the rows of one
planner iteration at the headline sizes (m = 1, p = 20, H = 30, halfcheetah: R = 4 000 rows at 200 candidates, 40 000 at 2 000) for a
(256, 256) relu net and, for orientation, a (512, 512) one and a linear V; median of ROUNDS rounds with the fastest and slowest, the
host's own time to enqueue one launch beside it, and the rate the net's 2 R sum(K N) floating-point operations make of the median.
Call time: `get_action` (numpy in, numpy out, one env, cfg2 sizes: halfcheetah, 4 x 200 swish, ensemble 5, 20 particles, H = 30,
5 iterations, 50 elites) at 200 and at 2 000 candidates, four models taking turns in one process: the default route; the opt-in loop
(cem_add_mean=True, which records nothing); the opt-in loop recording its trajectories (one inert penalty constraint: the cheapest
option that makes the rollout write them); and that loop with a (256, 256) relu value net.  Host clock around calls that end in a
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

NETS = [("linear", ()), ("256 x 2", (256, 256)), ("512 x 2", (512, 512))]


def he_net(D, hidden, seed):
    rng = np.random.default_rng(seed)
    dims = [D] + list(hidden) + [1]
    return [((rng.standard_normal((dims[l], dims[l + 1])) * np.sqrt(2.0 / dims[l])).astype(np.float32),
             (0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32)) for l in range(len(dims) - 1)]


def kernel_times(eng, n, batch, rounds):
    """{net: (median, min, max, host enqueue median, flops per launch)} in microseconds per launch, R = n p rows"""
    traj = torch.empty((eng.H, 1, n, eng.p, eng.D), dtype=torch.float32, device=eng.device).normal_()
    rows = torch.empty((1, n, eng.p), dtype=torch.float32, device=eng.device).uniform_(-30.0, 30.0)
    lib, ctx = eng.lib, eng._ctx
    out = {}
    for name, hidden in NETS:
        prm = HipEngine.value_params(hidden, "relu", 1.0)
        eng.set_value_net(prm, he_net(eng.D, hidden, 1))
        dev, host = [], []
        for r in range(rounds + 1):                          # (round 0 warms the kernel up and is dropped)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(batch):
                rc = lib.cadm_value_returns(ctx, prm, ptr(traj), None, 1, n, ptr(rows), ptr(rows), None, eng.stream)
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            if rc != 0:
                raise RuntimeError("cadm_value_returns failed: %s" % lib.cadm_last_error().decode())
            if r > 0:
                dev.append(e0.elapsed_time(e1) * 1e3 / batch)
                host.append((t1 - t0) * 1e6 / batch)
        dims = [eng.D] + list(hidden) + [1]
        flops = 2.0 * n * eng.p * sum(dims[l] * dims[l + 1] for l in range(len(dims) - 1))
        out[name] = (float(np.median(dev)), min(dev), max(dev), float(np.median(host)), flops)
    return out


def call_times(n, calls, rounds):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import make_env_spec
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=30, seed=0, trained_like=True)
    st = prob["stats"]
    nz = {k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")}
    record = dict(cem_constraints=[dict(dim=0, lo=-1e30)], cem_constraint_mode="penalty", cem_constraint_weight=0.0)
    settings = [("default route", {}), ("opt-in loop (cem_add_mean=True)", dict(cem_add_mean=True)),
                ("+ recording trajectories (one inert penalty constraint)", dict(cem_add_mean=True, **record)),
                ("+ cem_terminal_value (256, 256) relu", dict(cem_add_mean=True, cem_terminal_value=dict(hidden_sizes=(256, 256)), **record))]
    models = []
    for name, kw in settings:
        model = MLPEnsembleCEMDynamicsModel("dyn", make_env_spec("halfcheetah"), hidden_sizes=(200,) * 4, hidden_nonlinearity="swish", n_forwards=30,
                                            n_candidates=n, ensemble_size=5, n_particles=20, use_cem=True, normalize_input=True, seed=7, **kw)
        model.engine.set_net("context_model", prob["cp"])
        model.engine.set_net("ff_model", prob["ff"])
        model.set_normalization(nz)
        if "cem_terminal_value" in kw:
            model.set_terminal_value(he_net(model.obs_space_dims, (256, 256), 2))
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
        raise SystemExit("bench_value.py measures on a GPU; none is visible")
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=30, seed=0)
    eng = make_engine(prob, p=20)
    lines = ["# The terminal value's launch and what it adds to a call (tools/bench_value.py)", "",
             "Build %s, %s.  Kernel time: device events around %d back-to-back launches of `cadm_value_returns`, per launch, median of %d "
             "rounds (fastest - slowest); D = 18, p = 20, relu.  `host` is this host's time to enqueue one launch in the same loop; GFLOP/s "
             "is the net's 2 R sum(K N) operations over the median." % (eng.lib.cadm_build_id().decode(), torch.cuda.get_device_name(eng.device),
                                                                       a.batch, a.rounds), "",
             "| net | candidates | rows R | us / launch | (min - max) | host us / launch | GFLOP/s |", "|---|---|---|---|---|---|---|"]
    for n in (200, 2000):
        t = kernel_times(eng, n, a.batch, a.rounds)
        for name, _ in NETS:
            med, lo, hi, h, fl = t[name]
            lines.append("| %s | %d | %d | %.2f | %.2f - %.2f | %.2f | %.0f |" % (name, n, n * eng.p, med, lo, hi, h, fl / med * 1e-3))
    for n in (200, 2000):
        c = call_times(n, a.calls, a.rounds)
        keys = list(c)
        lines += ["", "`get_action` (cfg2 sizes, m = 1, n = %d, 5 iterations), %d calls per round, median of %d rounds, the models taking turns:"
                  % (n, a.calls, a.rounds), "", "| model | ms / get_action | (min - max) | against the row above |", "|---|---|---|---|"]
        for i, name in enumerate(keys):
            med, lo, hi = c[name]
            lines.append("| %s | %.3f | %.3f - %.3f | %s |" % (name, med, lo, hi, "" if i == 0 else "%+.3f ms" % (med - c[keys[i - 1]][0])))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
