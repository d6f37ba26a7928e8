#!/usr/bin/env python3
"""Plans on knots in the opt-in planner (csrc/knots.hip): what shaping the candidates costs a call.

`get_action` (numpy in, numpy out, one env, cfg2 sizes: halfcheetah, 4 x 200 swish, ensemble 5, 20 particles, H = 30, n = 200,
5 iterations, 50 elites) four ways in one process, the models taking turns call by call: cem_noise_beta=1.0 alone (cem_knots=1: no
shaping launch); cem_knots=3 hold; cem_knots=3 linear; cem_knots=3 hold anchored on the episode (the phase's torch update on top).
Host clock around calls that end in a stream synchronisation; the median over --calls calls after --warmup.  The knotted models plan
other actions than the plain one, so the difference is the added launches (one per CEM iteration, one per call) on the same rollouts.
Kernel time: device events around --batch back-to-back launches of `cadm_shape_actions` on [1, 200, 30, 6] floats (144 KB), per
launch, per interp; the median round with the fastest and slowest.
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

H, N, P, A, R = 30, 200, 20, 6, 3


def call_times(calls, warmup):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import make_env_spec
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=H, seed=0, trained_like=True)
    st = prob["stats"]
    nz = {k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")}
    settings = [("cem_noise_beta=1.0 (cem_knots=1)", {}),
                ("+ cem_knots=%d, hold" % R, dict(cem_knots=R)),
                ("+ cem_knots=%d, linear" % R, dict(cem_knots=R, cem_knot_interp="linear")),
                ("+ cem_knots=%d, hold, anchor episode" % R, dict(cem_knots=R, cem_knot_anchor="episode"))]
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
                raise RuntimeError("call %d of %r: a non-finite plan" % (i, name))
            state[name] = np.concatenate([plan[:, 1:], np.zeros((1, 1, A))], axis=1)      # the samplers' warm start
    return {k: (float(np.median(v)), min(v), float(np.percentile(v, 90))) for k, v in res.items()}, models[1][1].engine


def kernel_times(eng, batch, rounds):
    """{interp: (median, min, max)} in microseconds per launch of cadm_shape_actions at [1, N, H, A]"""
    acts = torch.empty((1, N, H, A), dtype=torch.float32, device=eng.device).uniform_(-1.0, 1.0)
    phase = torch.ones((1,), dtype=torch.int32, device=eng.device)
    lib, ctx = eng.lib, eng._ctx
    res = {}
    for interp in ("hold", "linear"):
        prm = HipEngine.knot_params(R, interp)
        times = []
        for r in range(rounds + 1):                      # (round 0 warms the kernel up and is dropped)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(batch):
                rc = lib.cadm_shape_actions(ctx, prm, ptr(phase), 1, N, ptr(acts), eng.stream)
            e1.record()
            torch.cuda.synchronize()
            if rc != 0:
                raise RuntimeError("cadm_shape_actions failed: %s" % lib.cadm_last_error().decode())
            if r > 0:
                times.append(e0.elapsed_time(e1) * 1e3 / batch)
        res[interp] = (float(np.median(times)), min(times), max(times))
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
        raise SystemExit("bench_knots.py measures on a GPU; none is visible")
    c, eng = call_times(a.calls, a.warmup)
    base = next(iter(c.values()))[0]
    lines = ["# Plans on knots: the cost of shaping the candidates (tools/bench_knots.py)", "",
             "Build %s, %s.  `get_action` at cfg2 sizes (m = 1, n = %d, p = %d, H = %d), the four models taking turns call by call; "
             "%d calls after %d warm-up calls.  The knotted models add one `cadm_shape_actions` launch per CEM iteration and two small "
             "launches per call; they plan other actions than the plain model, on rollouts of the same size."
             % (eng.lib.cadm_build_id().decode(), torch.cuda.get_device_name(eng.device), N, P, H, a.calls, a.warmup), "",
             "| get_action | median ms | min | p90 | x plain |", "|---|---|---|---|---|"]
    for name, (med, lo, p90) in c.items():
        lines.append("| %s | %.3f | %.3f | %.3f | %.3f |" % (name, med, lo, p90, med / base))
    k = kernel_times(eng, a.batch, a.rounds)
    lines += ["", "`cadm_shape_actions` alone at that geometry ([1, %d, %d, %d] floats, %.0f KB, spacing %d, phase 1): device events around %d "
              "back-to-back launches, per launch, median of %d rounds:" % (N, H, A, N * H * A * 4 / 1e3, R, a.batch, a.rounds), "",
              "| interp | us / launch | (min - max) |", "|---|---|---|"]
    for interp, (med, lo, hi) in k.items():
        lines.append("| %s | %.2f | %.2f - %.2f |" % (interp, med, lo, hi))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
