"""Rollout launch time of a spec-restated env (cadm_amd/env_spec.py restate: a module built by cadm_amd/jit.py) against the same
kind's compiled-in kernel: the BASELINE cfg2 / cfg3 launches (halfcheetah CaDM, E 5, p 20, H 30; n = 200 / 2000), device Philox,
interleaved in one process (A, B, A, B, ...) and timed with the library's hipEvent bracketing (cadm_profile_*).
    python tools/spec_rollout_time.py [--kind halfcheetah] [--reps 200]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cadm_amd import synth  # noqa: E402
from cadm_amd.env_spec import restate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="halfcheetah")
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    out = {}
    for cfg, n in (("cfg2", 200), ("cfg3", 2000)):
        engs = {}
        for name, env in (("builtin", args.kind), ("spec", restate(args.kind))):
            prob = synth.make_problem(env=env, context=True, E=5, m=1, H=30, trained_like=True, seed=1)
            engs[name] = (synth.make_engine(prob, p=20), prob)
        acts = np.random.default_rng(0).uniform(-1, 1, (1, n, 30, engs["builtin"][1]["A"])).astype(np.float32)
        state = {}
        for name, (eng, prob) in engs.items():
            state[name] = (eng._t(acts), eng.context_forward(prob["cp_obs"], prob["cp_act"]), eng._t(prob["obs"]))
            for _ in range(10):
                eng.rollout_returns(state[name][2], state[name][1], state[name][0], seed=1, call=1)
            torch.cuda.synchronize()
            eng.profile_enable(True)
            eng.profile_read()
        ms = {k: [] for k in engs}
        for r in range(args.reps):
            for name in (("builtin", "spec") if r % 2 == 0 else ("spec", "builtin")):
                eng = engs[name][0]
                a, c, o = state[name]
                eng.rollout_returns(o, c, a, seed=1, call=r)
                t, cnt = eng.profile_read()
                ms[name].append(t / max(cnt, 1))
        res = {k: dict(median_us=1e3 * float(np.median(v)), min_us=1e3 * float(np.min(v))) for k, v in ms.items()}
        res["spec_over_builtin_median"] = res["spec"]["median_us"] / res["builtin"]["median_us"]
        out[cfg] = res
        for eng, _ in engs.values():
            eng.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
