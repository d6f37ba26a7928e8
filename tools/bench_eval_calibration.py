#!/usr/bin/env python
"""Time `evaluate_calibration` and its statistics kernel (csrc/calibration.hip) on one GPU, next to `evaluate_horizon` on the same box.

Workload (tools/bench_eval_horizon.py's): halfcheetah CaDM (E = 5, 200 x 4, context 10), 20 particles, 20 000 held-out windows of
F = 10 steps, chunks of 4096.
  * evaluate_calibration and evaluate_horizon: host clock around the class call (upload of the windows, encoder + rollout + statistics
    per chunk, the results back), and device events around the engine call on the already-resident dataset; the cost of the new
    call is read as a ratio to the existing one;
  * the statistics kernel alone: device events around `cadm_calibration_stats` (stage 1 + stage 2, the clears included) and around
    `cadm_horizon_error` on the same trajectory tensor, one chunk's and the whole set's; bytes read over that time, next to the
    8 TB/s HBM peak.
Prints one JSON line and writes a report (default profiles/eval_calibration.md).  `--bench-this` / `--bench-parent`: results of
`bench.py --gpus 1` on this build and on its parent, run taking turns (row-steps/s, one number per run), recorded in the same file."""
import argparse
import ctypes as ct
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def host_ms(fn, n):
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def report(out, a):
    lines = ["# evaluate_calibration: what it costs", "",
             "One run on one MI355X (`tools/bench_eval_calibration.py`, library build `%s`); medians of %d repetitions, nothing here is a"
             % (out["build_id"], a.reps), "bar.  halfcheetah CaDM, E = 5, 200 x 4, context 10; %d windows, F = %d, p = %d, chunk %d."
             % (out["windows"], out["future"], out["particles"], out["chunk"]), "",
             "| call | evaluate_calibration | evaluate_horizon | ratio |", "|---|---|---|---|"]
    for label, k in (("class call, host clock (ms)", "host_ms"), ("engine call on the resident dataset, device events (ms)", "device_ms")):
        c, h = out["evaluate_calibration_" + k], out["evaluate_horizon_" + k]
        lines.append("| %s | %.2f | %.2f | %.2f |" % (label, c, h, c / h))
    lines += ["", "The statistics kernels alone on the same trajectory tensor (stage 1 + stage 2; the calibration call also clears its integer "
              "outputs), %d calls back to back per event pair:" % INNER, "",
              "| windows | bytes read | cadm_calibration_stats (ms) | GB/s | share of 8 TB/s | cadm_horizon_error (ms) | ratio |", "|---|---|---|---|---|---|---|"]
    for name in ("chunk", "all"):
        s = out["stats_" + name]
        lines.append("| %d | %d | %.4f | %.0f | %.3f | %.4f | %.2f |" % (s["windows"], s["bytes_read"], s["calibration_ms"], s["calibration_bytes_per_s"] / 1e9,
                                                                     s["calibration_share_of_hbm_peak"], s["horizon_ms"], s["calibration_ms"] / s["horizon_ms"]))
    lines += ["", "z2 per step (mean over dims) %s against z2_ideal %.3f; calibration_error per step %s; diverged %d." % (
        [round(v, 2) for v in out["z2"]], out["z2_ideal"], [round(v, 3) for v in out["calibration_error"]], out["diverged"]),
        "(The model is untrained: the figures show that the call ran, not that anything is calibrated.)", ""]
    if a.bench_this and a.bench_parent:
        lines += ["## bench.py on this build and on its parent", "",
                  "`bench.py --gpus 1`, the two builds taking turns on the same box (row-steps/s per run; the default planner path does not run any "
                  "code of this feature):", "", "| build | runs | median |", "|---|---|---|"]
        for label, v in (("this build", a.bench_this), ("parent", a.bench_parent)):
            lines.append("| %s | %s | %.4g |" % (label, ", ".join("%.4g" % x for x in v), float(np.median(v))))
        lines += ["", "ratio of the medians (this / parent): %.4f" % (float(np.median(a.bench_this)) / float(np.median(a.bench_parent))), ""]
    else:
        lines += ["bench.py on this build and its parent: not run with this report.", ""]
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=20000)
    ap.add_argument("--future", type=int, default=10)
    ap.add_argument("--particles", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_calibration.md"))
    ap.add_argument("--bench-this", type=float, nargs="*", default=None)
    ap.add_argument("--bench-parent", type=float, nargs="*", default=None)
    a = ap.parse_args()
    import torch
    from cadm_amd import _lib
    from cadm_amd._lib import ptr
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.envs import EnvSpec
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_calibration: no GPU visible; nothing is measured on the host")
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
        res = model.evaluate_calibration(*args, chunk=a.chunk)
        model.evaluate_horizon(*args, chunk=a.chunk)
    n_host = max(3, a.reps // 4)
    eng = model.engine
    dev = {k: eng._t(v) for k, v in w.items()}
    cal_ms = event_ms(lambda: eng.eval_calibration(dev, N, F, chunk=a.chunk, seed=1, call=1), a.reps, a.warmup)
    hor_ms = event_ms(lambda: eng.eval_horizon(dev, N, F, chunk=a.chunk, seed=1, call=1), a.reps, a.warmup)
    out = dict(windows=N, future=F, particles=p, chunk=a.chunk, build_id=eng.lib.cadm_build_id().decode(),
               evaluate_calibration_host_ms=host_ms(lambda: model.evaluate_calibration(*args, chunk=a.chunk), n_host),
               evaluate_horizon_host_ms=host_ms(lambda: model.evaluate_horizon(*args, chunk=a.chunk), n_host),
               evaluate_calibration_device_ms=cal_ms[0], evaluate_calibration_device_ms_min_max=cal_ms[1:],
               evaluate_horizon_device_ms=hor_ms[0], evaluate_horizon_device_ms_min_max=hor_ms[1:],
               z2=[float(v) for v in np.nanmean(res["z2"], axis=1)], z2_ideal=float(res["z2_ideal"]),
               calibration_error=[float(v) for v in res["calibration_error"]], diverged=int(res["diverged"].sum()))
    truth, mask = dev["obs_next"].view(N, F, D), dev["future_bool"]
    for name, m in (("chunk", min(a.chunk, N)), ("all", N)):
        traj = torch.randn((F, m, 1, p, D), device=eng.device)
        nbytes = traj.numel() * 4 + m * F * D * 4 + m * F * 4
        # the bare library calls on buffers allocated once, INNER calls back to back per event pair: the queue stays ahead of the host
        blocks = (m + 63) // 64
        partials = torch.empty((blocks * F * ((2 + E) * D + 2),), device=eng.device)      # the larger of the two kernels' partials
        o, c = eng._calibration_outputs(F, D, p, E)
        cal_call = (ptr(traj), ptr(truth), F * D, ptr(mask), m, F, p, E, D, 0, ptr(partials), blocks, ct.byref(c), 1, eng.stream)
        ho = eng._horizon_outputs(F, D)
        hor_call = (ptr(traj), ptr(truth), F * D, ptr(mask), m, F, p, E, D, 0, ptr(partials), blocks, ptr(ho["se"]), ptr(ho["spread"]),
                    ptr(ho["se_member"]), ptr(ho["count"]), ptr(ho["diverged"]), 1, eng.stream)

        def run(fn, call):
            def body():
                for _ in range(INNER):
                    rc = fn(*call)
                    assert rc == 0, rc
            return tuple(v / INNER for v in event_ms(body, a.reps, a.warmup))
        cm, hm = run(eng.lib.cadm_calibration_stats, cal_call), run(eng.lib.cadm_horizon_error, hor_call)
        out["stats_%s" % name] = dict(windows=m, bytes_read=nbytes, calibration_ms=cm[0], calibration_ms_min_max=cm[1:], horizon_ms=hm[0],
                                      horizon_ms_min_max=hm[1:], calibration_bytes_per_s=nbytes / (cm[0] * 1e-3),
                                      calibration_share_of_hbm_peak=nbytes / (cm[0] * 1e-3) / HBM_PEAK)
        del traj
    print(json.dumps(out))
    report(out, a)


if __name__ == "__main__":
    main()
