"""Cost of the opt-in plan forecast at the headline geometry (cfg2: halfcheetah with context, m = 1, n = 200 candidates, p = 20, H = 30).

  python tools/bench_forecast.py [--blocks 10] [--calls 30]

Through the drop-in class, numpy in -> numpy out, as bench.py's headline calls it: blocks of `calls` plain get_action calls, of
get_action(..., return_forecast=True) calls and of forecast() calls alone take turns (clock drift hits all three alike), after
bench.py's clock ramp and 30 untimed calls of each kind.  Prints one JSON line: the medians in milliseconds, their difference, and
the quartiles."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--calls", type=int, default=30)
    a = ap.parse_args()
    import bench
    from cadm_amd import synth
    pl = bench.Planner(synth.CONFIGS["cfg2"], 1, synth.CONFIGS["cfg2"]["n"], 1, 0, 0, None)
    prob, model = pl.prob, pl.model
    pl.ramp()
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"].copy(), prob["init_var"])
    for _ in range(30):
        plan = model.get_action(*args)
        model.get_action(*args, return_forecast=True)
        model.forecast(prob["obs"], plan, prob["cp_obs"], prob["cp_act"])
    times = dict(plain=[], with_forecast=[], forecast_alone=[])
    calls = dict(plain=lambda: model.get_action(*args), with_forecast=lambda: model.get_action(*args, return_forecast=True),
                 forecast_alone=lambda: model.forecast(prob["obs"], plan, prob["cp_obs"], prob["cp_act"]))
    for _ in range(a.blocks):
        for k, fn in calls.items():
            for _ in range(a.calls):
                t0 = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t0)
    ms = lambda v, q: round(float(np.quantile(v, q)) * 1e3, 4)
    res = dict(geometry="cfg2: halfcheetah, context, m=1, n=200, p=20, H=30, E=5", calls_each=a.blocks * a.calls)
    for k, v in times.items():
        res[k + "_ms"] = dict(median=ms(v, 0.5), q25=ms(v, 0.25), q75=ms(v, 0.75))
    res["cost_ms"] = round(res["with_forecast_ms"]["median"] - res["plain_ms"]["median"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
