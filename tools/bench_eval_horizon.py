#!/usr/bin/env python
"""Time `evaluate_horizon` and its statistics kernel (csrc/horizon.hip) on one GPU.

Workload: halfcheetah CaDM (E = 5, 200 x 4, context 10), 20 particles, 20 000 held-out windows of F = 10 steps.
  * evaluate_horizon: host clock around the class call (upload of the windows, encoder + rollout + statistics per chunk, the few
    hundred bytes of results back), and device events around the engine call on the already-resident dataset;
  * the statistics kernel alone: device events around `cadm_horizon_error` (stage 1 + stage 2) on one chunk's trajectory tensor and
    on the whole set's; bytes it has to read (trajectory + truth + mask) over that time, next to the 8 TB/s HBM peak.
A trajectory tensor that the rollout of the same chunk has just written may still sit in the 256 MiB Infinity Cache; the whole-set
tensor (288 MB) does not fit, so that line is the HBM figure.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
INNER = 10


def event_ms(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=20000)
    ap.add_argument("--future", type=int, default=10)
    ap.add_argument("--particles", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import EnvSpec
    from cadm_amd._lib import ptr
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_horizon: no GPU visible; nothing is measured on the host")
    N, F, p, E, D, A, Hh = a.windows, a.future, a.particles, 5, 18, 6, 10
    model = MLPEnsembleCEMDynamicsModel("dyn", EnvSpec("halfcheetah"), n_forwards=max(F, 30), n_particles=p, ensemble_size=E,
                                        history_length=Hh, future_length=F, use_cem=True)
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((N, F * D)).astype(np.float32)
    w = dict(obs=obs, act=rng.uniform(-1, 1, (N, F * A)).astype(np.float32),
             obs_next=(obs + 0.1 * rng.standard_normal((N, F * D))).astype(np.float32),
             cp_obs=(0.1 * rng.standard_normal((N, D * Hh))).astype(np.float32),
             cp_act=rng.uniform(-1, 1, (N, A * Hh)).astype(np.float32), future_bool=np.ones((N, F), np.float32))
    d0 = w["obs_next"][:, :D] - w["obs"][:, :D]
    model.compute_normalization(w["obs"][:, :D], w["act"][:, :A], d0, w["cp_obs"], w["cp_act"], -d0)
    args = (w["obs"], w["act"], w["obs_next"], w["cp_obs"], w["cp_act"], w["future_bool"])
    for _ in range(a.warmup):
        res = model.evaluate_horizon(*args, chunk=a.chunk)
    host = []
    for _ in range(max(3, a.reps // 4)):
        t0 = time.perf_counter()
        res = model.evaluate_horizon(*args, chunk=a.chunk)
        host.append((time.perf_counter() - t0) * 1e3)
    eng = model.engine
    dev = {k: eng._t(v) for k, v in w.items()}
    dev_ms = event_ms(lambda: eng.eval_horizon(dev, N, F, chunk=a.chunk, seed=1, call=1), a.reps, a.warmup)
    out = dict(windows=N, future=F, particles=p, chunk=a.chunk, evaluate_horizon_host_ms=float(np.median(host)),
               eval_horizon_device_ms=dev_ms[0], eval_horizon_device_ms_min_max=dev_ms[1:], rmse=[float(v) for v in res["rmse"]],
               diverged=int(res["diverged"].sum()))
    truth, mask = dev["obs_next"].view(N, F, D), dev["future_bool"]
    for name, m in (("chunk", min(a.chunk, N)), ("all", N)):
        traj = torch.randn((F, m, 1, p, D), device=eng.device)
        nbytes = traj.numel() * 4 + m * F * D * 4 + m * F * 4
        # the bare library call on buffers allocated once, INNER calls back to back per event pair: the queue stays ahead of the host
        blocks = (m + 63) // 64
        partials = torch.empty((blocks * F * ((2 + E) * D + 2),), device=eng.device)
        o = eng._horizon_outputs(F, D)
        call = (ptr(traj), ptr(truth), F * D, ptr(mask), m, F, p, E, D, 0, ptr(partials), blocks, ptr(o["se"]), ptr(o["spread"]),
                ptr(o["se_member"]), ptr(o["count"]), ptr(o["diverged"]), 1, eng.stream)

        def run():
            for _ in range(INNER):
                rc = eng.lib.cadm_horizon_error(*call)
                assert rc == 0, rc
        ms = tuple(v / INNER for v in event_ms(run, a.reps, a.warmup))
        out["stats_%s" % name] = dict(windows=m, bytes_read=nbytes, ms=ms[0], ms_min_max=ms[1:], bytes_per_s=nbytes / (ms[0] * 1e-3),
                                      share_of_hbm_peak=nbytes / (ms[0] * 1e-3) / HBM_PEAK)
        del traj
    print(json.dumps(out))


if __name__ == "__main__":
    main()
