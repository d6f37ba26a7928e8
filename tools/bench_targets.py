#!/usr/bin/env python3
"""Value-expansion targets (csrc/imagine_targets.hip): what one `cadm_imagine_targets` call costs against the equivalent loop of small
torch ops a caller would have written, at (m, n, k) = (4096, 4, 5) on seeded synthetic transitions (a third of the rows ended early).

The call: device events around BATCH back-to-back calls into one buffer, per call, with and without the STEVE outputs; median of
ROUNDS rounds with the fastest and slowest.  Its bytes (rew, valid, done, disagreement, boot read; the views written) are set against
the rate of a device-to-device copy of 256 MiB measured in the same run.  The torch loop: the same lambda-returns, n-step targets and
STEVE combination over the k steps with masks, device events and host clock (a stream synchronisation at the end) per evaluation; its
results are compared with the kernel's at 1e-5 of the largest target (torch's reduction order is not the kernel's).
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
from cadm_amd.synth import make_engine

M, N, K = 4096, 4, 5
GAMMA, LAM, BETA, FLOOR = 0.99, 0.95, 0.5, 1e-2


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


def hosted(fn, batch, rounds):
    """the same on the host clock, a synchronisation behind every round's calls"""
    t = []
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batch):
            fn()
        torch.cuda.synchronize()
        if r > 0:
            t.append((time.perf_counter() - t0) * 1e6 / batch)
    return float(np.median(t)), min(t), max(t)


def copy_rate(rounds):
    """bytes per second (read + written) of a device-to-device copy of 256 MiB"""
    src = torch.empty((64 << 20,), dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    us, _, _ = timed(lambda: dst.copy_(src), 10, rounds)
    return 2.0 * src.numel() * 4 / (us * 1e-6)


def inputs(dev):
    rng = np.random.default_rng(0)
    end = np.where(rng.random((M, N)) < 1.0 / 3.0, rng.integers(0, K + 1, (M, N)), K)
    term = (rng.random((M, N)) < 0.5) & (end < K) & (end >= 1)
    t = np.arange(K)[:, None, None]
    valid = t < end[None]
    x = dict(rew=np.where(valid, 3.0 * rng.standard_normal((K, M, N)), 0.0).astype(np.float32), valid=valid.astype(np.uint8),
             done=((t == end[None] - 1) & term[None]).astype(np.uint8),
             disagreement=np.where(valid, np.abs(rng.standard_normal((K, M, N))), 0.0).astype(np.float32),
             boot=(30.0 * rng.standard_normal((K + 1, M, N))).astype(np.float32))
    return {k: torch.as_tensor(v).to(dev) for k, v in x.items()}


def torch_loop(x, steve):
    """the targets as a loop of small torch ops over the k steps"""
    rew, boot = x["rew"], x["boot"]
    valid, done = x["valid"].bool(), x["done"].bool()
    used = torch.cumprod(valid.to(torch.int32), dim=0).bool()
    L = used.sum(dim=0)
    term = (L >= 1) & torch.gather(done, 0, (L - 1).clamp(min=0)[None])[0]
    rt = rew - BETA * x["disagreement"]
    lam, G = torch.zeros_like(rew), torch.zeros_like(rew[0])
    for t in range(K - 1, -1, -1):
        last = torch.where(term, rt[t], rt[t] + GAMMA * boot[t + 1])
        G = torch.where(L - 1 == t, last, rt[t] + GAMMA * ((1.0 - LAM) * boot[t + 1] + LAM * G))
        lam[t] = torch.where(used[t], G, torch.zeros_like(G))
    nstep, ok = torch.zeros_like(rew), torch.zeros_like(used)
    acc, xh, disc = torch.zeros_like(rew[0]), torch.zeros_like(rew[0]), 1.0
    for h in range(1, K + 1):
        acc = torch.where(used[h - 1], acc + disc * rt[h - 1], acc)
        disc *= GAMMA
        xh = torch.where(used[h - 1], torch.where((L == h) & term, acc, acc + disc * boot[h]), xh)
        ok[h - 1] = (used[h - 1] | term) & torch.isfinite(xh)
        nstep[h - 1] = torch.where(ok[h - 1], xh, torch.zeros_like(xh))
    out = dict(lambda_return=lam, nstep=nstep)
    if steve:
        c = ok.sum(dim=2)
        cf = c.clamp(min=1).to(rew.dtype)
        mean = (nstep * ok).sum(dim=2) / cf
        var = (((nstep - mean[:, :, None]) ** 2) * ok).sum(dim=2) / cf
        w = torch.where(c >= 2, 1.0 / (var + FLOOR), torch.zeros_like(var))
        W = w.sum(dim=0)
        out["steve"] = torch.where(W > 0, (w * mean).sum(dim=0) / W.clamp(min=1e-30), boot[0, :, 0])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = make_engine(synth.make_problem(env="pendulum", context=False, E=5, m=2, H=3, seed=52), p=5)      # the kernel reads no weights
    x = inputs(eng.device)
    rate = copy_rate(a.rounds)
    lines = ["| (m, n, k) = (%d, %d, %d) | plain | with STEVE |" % (M, N, K), "|---|---|---|"]
    cols = {}
    for steve in (False, True):
        prm = _lib.TargetParams(GAMMA, LAM, BETA, float("inf"), FLOOR if steve else 0.0, int(steve))
        need = eng.lib.cadm_imagine_targets_workspace_bytes(eng._ctx, M, N, K, int(steve), None)
        buf = torch.empty((need,), dtype=torch.uint8, device=eng.device)
        call = lambda: _lib.check(eng.lib.cadm_imagine_targets(eng._ctx, ptr(x["rew"]), ptr(x["valid"]), ptr(x["done"]), ptr(x["disagreement"]),
                                                               ptr(x["boot"]), M, N, K, ct.byref(prm), ptr(buf), eng.stream), "cadm_imagine_targets", eng.lib)
        got = eng.imagine_targets(x["rew"], x["valid"], x["done"], x["disagreement"], x["boot"], GAMMA, LAM, BETA, None, FLOOR if steve else None)
        ref = torch_loop(x, steve)
        scale = float(got["nstep"].abs().max())
        for key in ref:
            err = float((got[key] - ref[key]).abs().max())
            assert err <= 1e-5 * scale, "%s: the torch loop is %.3e from the kernel (scale %.3e)" % (key, err, scale)
        rows = M * N
        nbytes = rows * K * (4 + 1 + 1 + 4) + rows * (K + 1) * 4 + rows * K * (4 + 4 + 1 + 1) + (M * (4 + 1) + 4 * K * M * 4 if steve else 0)
        cols[steve] = dict(kernel=timed(call, a.batch, a.rounds), engine=hosted(lambda: eng.imagine_targets(
            x["rew"], x["valid"], x["done"], x["disagreement"], x["boot"], GAMMA, LAM, BETA, None, FLOOR if steve else None), a.batch, a.rounds),
            loop_dev=timed(lambda: torch_loop(x, steve), 5, a.rounds), loop_host=hosted(lambda: torch_loop(x, steve), 5, a.rounds), bytes=nbytes)
    fmt = lambda t: "%.1f us (%.1f - %.1f)" % t
    for name, key in (("`cadm_imagine_targets`, device events", "kernel"), ("host clock, `HipEngine.imagine_targets` and a synchronisation", "engine"),
                      ("the torch loop, device events", "loop_dev"), ("the torch loop, host clock and a synchronisation", "loop_host")):
        lines.append("| %s | %s | %s |" % (name, fmt(cols[False][key]), fmt(cols[True][key])))
    lines.append("| the call's bytes, and their time at the copy rate (%.2f TB/s) | %s | %s |" % (
        rate / 1e12, *("%.2f MB, %.2f us" % (cols[s]["bytes"] / 1e6, cols[s]["bytes"] / rate * 1e6) for s in (False, True))))
    lines.append("| torch loop / call (device events) | %s | %s |" % tuple("%.1f x" % (cols[s]["loop_dev"][0] / cols[s]["kernel"][0]) for s in (False, True)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
