#!/usr/bin/env python3
"""Stochastic actor head (csrc/policy_gauss.hip): what a sampled action costs next to the mode action, and what sampling costs a whole
`imagine` call.

Sizes: tools/bench_imagine.py's -- the headline model (halfcheetah with context, 4 x 200 swish, ensemble 5) at p = 5 and p = 20
particles, m = 4096 start states, n = 1 branch, k = 5 steps, a (256, 256) relu actor with a tanh squash whose last layer has 2 A
outputs, log-std bounds (-5, 2) clamped; the mode route perturbs with noise_std = 0.1.
Measured: `cadm_policy_sample` against `cadm_policy_eval` at 4096 rows, and `cadm_imagine_sampled` against `cadm_imagine`, all in the
same run: device events around BATCH back-to-back calls on one stream, per call; median of ROUNDS rounds with the fastest and the
slowest.
With --parent DIR (a built checkout of the parent commit) `bench.py --gpus 1` runs on this tree and on that one, taking turns, each in
a fresh process: the default path launches nothing new, so the two must agree within the tool's run-to-run spread.
Writes a markdown file (--out, default profiles/gauss_policy.md).  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cadm_amd import _lib, synth
from cadm_amd import planner as hplanner
from cadm_amd._lib import ptr
from cadm_amd.engine import HipEngine
from cadm_amd.synth import make_engine

HIDDEN, NOISE, M, N, K = (256, 256), 0.1, 4096, 1, 5


def he_actor(D, hidden, A, seed):
    """D -> hidden -> 2 A: He-initialised, the log-std columns small so that sigma stays near exp(-1)"""
    rng = np.random.default_rng(seed)
    dims = [D] + list(hidden) + [2 * A]
    layers = [((rng.standard_normal((dims[l], dims[l + 1])) * np.sqrt(2.0 / dims[l])).astype(np.float32),
               (0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32)) for l in range(len(dims) - 1)]
    W, b = layers[-1]
    W[:, A:] *= 0.3
    b[A:] -= 1.0
    return layers


def timed(fn, batch, rounds):
    """(median, min, max) microseconds per call of `fn` over `rounds` rounds of `batch` back-to-back calls (round 0 warms up)"""
    dev = []
    for r in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(batch):
            rc = fn()
            assert rc == 0, rc
        e1.record()
        torch.cuda.synchronize()
        if r > 0:
            dev.append(e0.elapsed_time(e1) * 1e3 / batch)
    return float(np.median(dev)), min(dev), max(dev)


def measure(p, batch, rounds):
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=30, seed=0, trained_like=True)
    eng = make_engine(prob, p=p)
    lib, ctx = eng.lib, eng._ctx
    layers = he_actor(eng.D, HIDDEN, eng.A, 1)
    mean_layers, W_ls, b_ls = hplanner.split_gaussian_layers(layers, eng.A)
    eng.set_policy_net(HipEngine.policy_params(HIDDEN, "relu", "tanh", 1, 0.0), mean_layers)
    eng.set_policy_head(hplanner.policy_head_params(dict(kind="gaussian"), has_actor=True), W_ls, b_ls)
    obs = eng._t(prob["obs"])
    ctx_vec = eng.context_forward(prob["cp_obs"], prob["cp_act"])
    out = eng.imagine(obs, ctx_vec, K, N, None, 0.0, None, None, 1, 1, sample=True)      # (checks the route; the states of a step)
    assert bool(out["valid"].all()) and bool(torch.isfinite(out["logp"]).all())
    R, D, A = M * N, eng.D, eng.A
    state = out["states"][1].reshape(R, D).contiguous()
    a1 = torch.empty((R, A), dtype=torch.float32, device=eng.device)
    lp = torch.empty((R,), dtype=torch.float32, device=eng.device)
    res = [("`cadm_policy_eval`, %d rows" % R, timed(lambda: lib.cadm_policy_eval(ctx, ptr(state), R, ptr(a1), eng.stream), batch, rounds)),
           ("`cadm_policy_sample`, %d rows" % R,
            timed(lambda: lib.cadm_policy_sample(ctx, ptr(state), R, 0, 1, 1, 1, ptr(a1), ptr(lp), None, eng.stream), batch, rounds))]
    buf = torch.empty((lib.cadm_imagine_sampled_workspace_bytes(ctx, M, N, K, None),), dtype=torch.uint8, device=eng.device)
    res += [("`cadm_imagine`, k = %d, noise_std = %g" % (K, NOISE),
             timed(lambda: lib.cadm_imagine(ctx, ptr(obs), ptr(ctx_vec), None, M, N, K, NOISE, None, None, 1, 1, ptr(buf), eng.stream),
                   max(batch // 10, 1), rounds)),
            ("`cadm_imagine_sampled`, k = %d" % K,
             timed(lambda: lib.cadm_imagine_sampled(ctx, ptr(obs), ptr(ctx_vec), M, N, K, None, None, 1, 1, ptr(buf), eng.stream),
                   max(batch // 10, 1), rounds))]
    bid, dev = lib.cadm_build_id().decode(), torch.cuda.get_device_name(eng.device)
    eng.close()
    return res, bid, dev


def headline(tree, steps, warmup):
    """ms per get_action of `bench.py --gpus 1` in `tree`, in a fresh process"""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree, check=True,
                       stdout=subprocess.PIPE, universal_newlines=True)
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return float(out["ms_per_step"]), out["build_id"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100, help="calls between the two events (a tenth of it for a whole imagine call)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py's headline there and here, taking turns")
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauss_policy.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gauss_policy.py measures on a GPU; none is visible")
    lines = ["# Stochastic actor head: a sampled action next to the mode action, alone and inside imagine (tools/bench_gauss_policy.py)", ""]
    for p in (5, 20):
        res, bid, dev = measure(p, a.batch, a.rounds)
        if p == 5:
            lines += ["Build %s, %s.  ONE run on ONE box.  Halfcheetah with context, E = 5, m = %d, n = %d, k = %d, D = 18, A = 6, a (256, 256) relu "
                      "actor with 2 A outputs, log-std clamped to (-5, 2).  Device events around back-to-back calls on one stream, per call, median "
                      "of %d rounds (fastest - slowest)." % (bid, dev, M, N, K, a.rounds), ""]
        lines += ["## p = %d" % p, "", "| what | us | (min - max) |", "|---|---|---|"]
        for name, (med, lo, hi) in res:
            lines.append("| %s | %.1f | %.1f - %.1f |" % (name, med, lo, hi))
        ev, sm, im, ims = (r[1][0] for r in res)
        lines += ["", "A sampled action costs %.2f x the mode action (%+.1f us: the second output layer, the draw, the log-density); a sampled "
                  "imagine call %.3f x the mode call with noise (%+.1f us over %d steps)." % (sm / ev, sm - ev, ims / im, ims - im, K), ""]
    if a.parent:
        here, there = [], []
        for _ in range(a.turns):
            ms, bid_here = headline(ROOT, a.steps, a.warmup)
            here.append(ms)
            ms, bid_parent = headline(os.path.abspath(a.parent), a.steps, a.warmup)
            there.append(ms)
        lines += ["## bench.py's headline, this tree and the parent commit taking turns", "",
                  "`bench.py --gpus 1 --steps %d --warmup %d`, ms per get_action, %d turns each, a fresh process per run, in the order this, "
                  "parent, this, ..  The default path launches nothing new." % (a.steps, a.warmup, a.turns), "",
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
