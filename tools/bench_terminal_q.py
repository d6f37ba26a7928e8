#!/usr/bin/env python3
"""The terminal value from Q critics of the opt-in planner (csrc/critic.hip): where the fused launch stands against the separate kernels
it replaces, and what the term adds to a get_action call.

Sizes: the headline row count m n p = 1 x 200 x 20 = 4000 terminal states of halfcheetah (D = 18, A = 6), a (256, 256) relu actor with
a tanh squash, C = 2 (256, 256) relu critics.
Fused: one `cadm_critic_eval` (actor, both critics, the reduction).  Separate: one `cadm_policy_eval` plus C `cadm_value_eval` of a
(256, 256) relu value net on the same rows -- the kernels a caller had before, C + 1 launches and C + 1 loads of the states.  Device
events around BATCH back-to-back repetitions on one stream, per repetition; the two take turns round by round in one process; round 0
warms up; median of ROUNDS rounds with the fastest and slowest.
Call time: `get_action` (numpy in, numpy out) with `cem_noise_beta=1.0` alone against the same plus `cem_terminal_q`: two models taking
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

HIDDEN, C, H, N, PARTICLES = (256, 256), 2, 30, 200, 20


def he_net(K, hidden, out, seed):
    rng = np.random.default_rng(seed)
    dims = [K] + list(hidden) + [out]
    return [((rng.standard_normal((dims[l], dims[l + 1])) * np.sqrt(2.0 / dims[l])).astype(np.float32),
             (0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32)) for l in range(len(dims) - 1)]


def interleaved(fns, batch, rounds):
    """{name: (median, min, max)} microseconds per repetition of every fn, the fns taking turns round by round (round 0 warms up)"""
    dev = {name: [] for name, _ in fns}
    for r in range(rounds + 1):
        for name, fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r > 0:
                dev[name].append(e0.elapsed_time(e1) * 1e3 / batch)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in dev.items()}


def kernel_times(batch, rounds):
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=H, seed=0, trained_like=True)
    eng = make_engine(prob, p=PARTICLES)
    lib, ctx = eng.lib, eng._ctx
    D, A, rows = eng.D, eng.A, N * PARTICLES
    eng.set_policy_net(HipEngine.policy_params(HIDDEN, "relu", "tanh", 1, 0.0), he_net(D, HIDDEN, A, 1))
    eng.set_critic_nets(HipEngine.critic_params(HIDDEN, "relu", C, "min", 1.0), [he_net(D + A, HIDDEN, 1, 2 + c) for c in range(C)])
    eng.set_value_net(HipEngine.value_params(HIDDEN, "relu", 1.0), he_net(D, HIDDEN, 1, 9))
    x = torch.empty((rows, D), dtype=torch.float32, device=eng.device).normal_()
    q = torch.empty((rows,), dtype=torch.float32, device=eng.device)
    v = torch.empty((C, rows), dtype=torch.float32, device=eng.device)
    a = torch.empty((rows, A), dtype=torch.float32, device=eng.device)

    def fused():
        lib.cadm_critic_eval(ctx, ptr(x), None, rows, ptr(q), None, None, eng.stream)

    def separate():
        lib.cadm_policy_eval(ctx, ptr(x), rows, ptr(a), eng.stream)
        for c in range(C):
            lib.cadm_value_eval(ctx, ptr(x), rows, ptr(v[c]), eng.stream)

    fused(), separate()
    torch.cuda.synchronize()
    assert torch.isfinite(q).all() and torch.isfinite(v).all() and torch.isfinite(a).all()
    res = interleaved([("fused: one `cadm_critic_eval` (actor, %d critics, reduce)" % C, fused),
                       ("separate: one `cadm_policy_eval` + %d `cadm_value_eval`" % C, separate)], batch, rounds)
    bid, dev = eng.lib.cadm_build_id().decode(), torch.cuda.get_device_name(eng.device)
    eng.close()
    return res, rows, bid, dev


def call_times(calls, warmup):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import make_env_spec
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=H, seed=0, trained_like=True)
    st = prob["stats"]
    nz = {k: (st[k + "_mean"], st[k + "_std"]) for k in ("obs", "delta", "act", "cp_obs", "cp_act", "back_delta")}
    tq = dict(hidden_sizes=HIDDEN, activation="relu", n_critics=C, reduce="min", weight=1.0,
              policy=dict(hidden_sizes=HIDDEN, activation="relu", squash="tanh"))
    settings = [("cem_noise_beta=1.0", dict(cem_noise_beta=1.0)),
                ("+ cem_terminal_q (256, 256) relu, %d critics, (256, 256) actor" % C, dict(cem_noise_beta=1.0, cem_terminal_q=tq))]
    models = []
    for name, kw in settings:
        model = MLPEnsembleCEMDynamicsModel("dyn", make_env_spec("halfcheetah"), hidden_sizes=(200,) * 4, hidden_nonlinearity="swish", n_forwards=H,
                                            n_candidates=N, ensemble_size=5, n_particles=PARTICLES, use_cem=True, normalize_input=True, seed=7, **kw)
        model.engine.set_net("context_model", prob["cp"])
        model.engine.set_net("ff_model", prob["ff"])
        model.set_normalization(nz)
        if "cem_terminal_q" in kw:
            D, A = model.obs_space_dims, prob["A"]
            model.set_policy(he_net(D, HIDDEN, A, 1))
            model.set_critics([he_net(D + A, HIDDEN, 1, 2 + c) for c in range(C)])
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
    ap.add_argument("--batch", type=int, default=200, help="repetitions between the two events")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200, help="timed get_action calls per model")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_terminal_q.py measures on a GPU; none is visible")
    res, rows, bid, dev = kernel_times(a.batch, a.rounds)
    lines = ["# The fused terminal Q against the kernels it replaces, and what the term adds to a call (tools/bench_terminal_q.py)", "",
             "Build %s, %s.  Device events around %d back-to-back repetitions on one stream, per repetition, the two taking turns round by "
             "round in one process, round 0 discarded, median of %d rounds (fastest - slowest); %d rows (m n p = 1 x %d x %d) of halfcheetah "
             "states, D = 18, A = 6, a (256, 256) relu actor, tanh squash, C = %d (256, 256) relu critics; the separate value net is "
             "(256, 256) relu on D inputs." % (bid, dev, a.batch, a.rounds, rows, N, PARTICLES, C), "", "| what | us | (min - max) |", "|---|---|---|"]
    for name, (med, lo, hi) in res.items():
        lines.append("| %s | %.1f | %.1f - %.1f |" % (name, med, lo, hi))
    meds = [v[0] for v in res.values()]
    lines += ["", "Fused / separate: %.2f." % (meds[0] / meds[1])]
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
