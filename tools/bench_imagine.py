#!/usr/bin/env python3
"""Imagined rollouts for a learner (csrc/imagine.hip): what one `imagine` call costs, where the time goes, and what the same
transitions cost composed stepwise from the public calls that existed before it.

Sizes: the headline model (halfcheetah with context, 4 x 200 swish, ensemble 5) at p = 5 and p = 20 particles, m = 4096 start states,
n = 1 branch, k = 5 steps, a (256, 256) relu policy with a tanh squash, noise_std = 0.1.
One call: device events around BATCH back-to-back `cadm_imagine` calls into one buffer, per call; median of ROUNDS rounds with the
fastest and slowest; transitions per second = m n k / that.
The split: the same around each of the three kernels of a step alone, on the step's rows -- `cadm_policy_eval` (the policy step),
`cadm_rollout_returns` with per-row start states on a one-step engine with the same weights (the rollout), `cadm_imagine_select` (the
select stage).  The select stage's bytes (next, rows1 and states[t] read; states[t + 1], the broadcast and the scalars written) are set
against the rate of a device-to-device copy of 256 MiB measured in the same run.
Stepwise: per step `policy_eval`, `rollout_returns(obs_rows=...)` of the one-step engine with the trajectories, and torch indexing
for the draw, the gather, the member variance, the finite test and the re-seeding -- host clock around k steps that end in a stream
synchronisation, as a caller would have written it.
Writes a markdown table (--out, default stdout only).  Needs a GPU: there is no fallback."""
import argparse
import ctypes as ct
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

HIDDEN, NOISE, M, N, K = (256, 256), 0.1, 4096, 1, 5


def he_policy(D, hidden, A, seed):
    rng = np.random.default_rng(seed)
    dims = [D] + list(hidden) + [A]
    return [((rng.standard_normal((dims[l], dims[l + 1])) * np.sqrt(2.0 / dims[l])).astype(np.float32),
             (0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32)) for l in range(len(dims) - 1)]


def timed(fn, batch, rounds):
    """(median, min, max) microseconds per call of `fn` over `rounds` rounds of `batch` back-to-back calls (round 0 warms up)"""
    dev = []
    for r in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if r > 0:
            dev.append(e0.elapsed_time(e1) * 1e3 / batch)
    return float(np.median(dev)), min(dev), max(dev)


def copy_rate(rounds):
    """bytes per second (read + written) of a device-to-device copy of 256 MiB"""
    src = torch.empty((64 << 20,), dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    us, _, _ = timed(lambda: dst.copy_(src), 10, rounds)
    return 2.0 * src.numel() * 4 / (us * 1e-6)


def stepwise(eng, twin, obs, ctx_vec, seed):
    """the k steps composed from policy_eval, a one-step rollout_returns and torch indexing -> the same dict of tensors"""
    m, p, E, D = obs.shape[0], eng.p, eng.E, eng.D
    rows_i = torch.arange(m, device=obs.device)
    state, alive = obs, torch.ones((m,), dtype=torch.bool, device=obs.device)
    gen = torch.Generator(device=obs.device).manual_seed(seed)
    out = dict(states=[obs], act=[], rew=[], valid=[], member=[], disagreement=[])
    for t in range(K):
        a = eng.policy_eval(state)
        a = torch.clamp(a + NOISE * torch.randn(a.shape, device=a.device, generator=gen), -1.0, 1.0)
        start = state[:, None, :].expand(m, p, D).reshape(-1, D)
        rows, traj = twin.rollout_returns(obs, ctx_vec, a[:, None, None, :], obs_rows=start, seed=seed, call=0, it=_lib.IMAGINE_IT + 2 * t,
                                          want_traj=True)
        sel = torch.randint(0, p, (m,), device=obs.device, generator=gen)
        nxt = traj[0, :, 0]                                          # [m, p, D]
        s1 = nxt[rows_i, sel]
        u = nxt.view(m, E, p // E, D).mean(dim=2).var(dim=1, unbiased=False).sum(dim=-1)
        valid = alive & torch.isfinite(s1).all(dim=-1)
        state = torch.where(valid[:, None], s1, state)
        out["states"].append(state)
        out["act"].append(a)
        out["rew"].append(torch.where(valid, rows[rows_i, 0, sel], torch.zeros_like(u)))
        out["valid"].append(valid)
        out["member"].append(torch.where(alive, sel // (p // E), torch.full_like(sel, -1)))
        out["disagreement"].append(torch.where(torch.isfinite(u), u, torch.full_like(u, float("inf"))))
        alive = valid
    return {k: torch.stack(v) for k, v in out.items()}


def measure(p, batch, rounds):
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=30, seed=0, trained_like=True)
    eng, twin = make_engine(prob, p=p), make_engine(prob, p=p, H=1)
    lib, ctx = eng.lib, eng._ctx
    eng.set_policy_net(HipEngine.policy_params(HIDDEN, "relu", "tanh", 1, 0.0), he_policy(eng.D, HIDDEN, eng.A, 1))
    obs = eng._t(prob["obs"])
    ctx_vec, tv = eng.context_forward(prob["cp_obs"], prob["cp_act"]), twin.context_forward(prob["cp_obs"], prob["cp_act"])
    out = eng.imagine(obs, ctx_vec, K, N, None, NOISE, None, None, 1, 1)      # (checks the rollout; the tensors of a step for the split)
    assert bool(out["valid"].all()) and bool(torch.isfinite(out["states"]).all())
    R, D, A = M * N, eng.D, eng.A
    need = lib.cadm_imagine_workspace_bytes(ctx, M, N, K, None)
    buf = torch.empty((need,), dtype=torch.uint8, device=eng.device)
    res = [("`cadm_imagine`, k = %d (%d launches)" % (K, 3 * K + 1),
            timed(lambda: lib.cadm_imagine(ctx, ptr(obs), ptr(ctx_vec), None, M, N, K, NOISE, None, None, 1, 1, ptr(buf), eng.stream),
                  max(batch // 10, 1), rounds))]
    state = out["states"][1].reshape(R, D).contiguous()
    act = out["act"][1].reshape(M, N, 1, A).contiguous()
    a1 = torch.empty((R, A), dtype=torch.float32, device=eng.device)
    res.append(("policy step, %d rows (`cadm_policy_eval`)" % R, timed(lambda: lib.cadm_policy_eval(ctx, ptr(state), R, ptr(a1), eng.stream), batch, rounds)))
    start = state[:, None, :].expand(R, p, D).contiguous()
    rows1 = torch.empty((M, N, p), dtype=torch.float32, device=eng.device)
    nxt = torch.empty((1, M, N, p, D), dtype=torch.float32, device=eng.device)
    twin.rollout_returns(obs, tv, act, obs_rows=start.reshape(-1, D), seed=1, call=1, it=_lib.IMAGINE_IT + 2)
    res.append(("one-step rollout, %d x %d particle rows (`cadm_rollout_returns`)" % (R, p),
                timed(lambda: lib.cadm_rollout_returns(twin._ctx, ptr(obs), ptr(start), ptr(tv), ptr(act), None, 1, 1, 1, _lib.IMAGINE_IT + 2, 0, N, M, N,
                                                       ptr(rows1), ptr(nxt), twin.stream), batch, rounds)))
    alive = torch.ones((R,), dtype=torch.uint8, device=eng.device)
    o = eng.imagine_select(nxt[0].reshape(R, p, D), rows1.reshape(R, p), state, alive, t=1, seed=1, call=1)
    sel_us = timed(lambda: lib.cadm_imagine_select(ctx, ptr(nxt), ptr(rows1), ptr(state), None, R, 1, None, None, 1, 1, ptr(o["alive"]), ptr(o["state"]),
                                                   ptr(o["rew"]), ptr(o["done"]), ptr(o["valid"]), ptr(o["member"]), ptr(o["disagreement"]),
                                                   ptr(o["length"]), ptr(o["bcast"]), eng.stream), batch, rounds)
    res.append(("select stage, %d rows (`cadm_imagine_select`)" % R, sel_us))
    sel_bytes = 4 * R * (2 * p * D + p + 2 * D + 3) + 3 * R + 4 * R
    host = []
    stepwise(eng, twin, obs, tv, 1)
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stepwise(eng, twin, obs, tv, 1)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    fused = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.imagine(obs, ctx_vec, K, N, None, NOISE, None, None, 1, 1)
        torch.cuda.synchronize()
        fused.append((time.perf_counter() - t0) * 1e6)
    bid, dev = lib.cadm_build_id().decode(), torch.cuda.get_device_name(eng.device)
    eng.close()
    twin.close()
    return res, sel_bytes, (float(np.median(host)), min(host), max(host)), (float(np.median(fused)), min(fused), max(fused)), bid, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100, help="calls between the two events (a tenth of it for the whole chain)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_imagine.py measures on a GPU; none is visible")
    rate = copy_rate(a.rounds)
    lines = ["# Imagined rollouts: one call, its kernels, and the stepwise composition (tools/bench_imagine.py)", ""]
    for p in (5, 20):
        res, sel_bytes, host, fused, bid, dev = measure(p, a.batch, a.rounds)
        if p == 5:
            lines += ["Build %s, %s.  Halfcheetah with context, E = 5, m = %d, n = %d, k = %d, D = 18, A = 6, a (256, 256) relu policy, noise_std = %g.  "
                      "Device events around back-to-back calls on one stream, per call, median of %d rounds (fastest - slowest).  Device-to-device "
                      "copy of 256 MiB: %.2f TB/s read + written." % (bid, dev, M, N, K, NOISE, a.rounds, rate / 1e12), ""]
        lines += ["## p = %d" % p, "", "| what | us | (min - max) |", "|---|---|---|"]
        for name, (med, lo, hi) in res:
            lines.append("| %s | %.1f | %.1f - %.1f |" % (name, med, lo, hi))
        call_us, sel_us = res[0][1][0], res[3][1][0]
        lines += ["", "Transitions per second of one call: %.1f M (m n k = %d in %.1f us)." % (M * N * K / call_us, M * N * K, call_us),
                  "Select stage: %.1f us for %.2f MB, which the measured copy rate moves in %.1f us." % (sel_us, sel_bytes / 1e6, sel_bytes / rate * 1e6),
                  "Host clock, k steps ending in a synchronisation, median of %d (min - max): `HipEngine.imagine` %.0f us (%.0f - %.0f); composed "
                  "stepwise from `policy_eval`, `rollout_returns(obs_rows=...)` and torch indexing %.0f us (%.0f - %.0f): %.2f x."
                  % ((a.rounds,) + fused + host + (host[0] / fused[0],)), ""]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
