#!/usr/bin/env python3
"""Bitwise comparison of two builds of the library on the same inputs (developer tool; needs a GPU):
   python tools/compare_libs.py libA.so libB.so      -- rollouts (returns + trajectories) and every planner route (CEM plan from device
and from host arrays, random shooting, two iCEM calls that share a carry) over a set of problem shapes, the open-loop horizon error, then the training step: the losses of three steps, every weight tensor afterwards, the prediction heads and one
evaluation step.  A schedule-only change of a kernel, or a host-only change, must print 'identical' everywhere."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cadm_amd import _lib, synth
from cadm_amd.env_spec import EnvDecl

CASES = [  # env, context, hid, E, p, m, n, H, det
    ("halfcheetah", True, 200, 5, 20, 1, 200, 30, False),
    ("halfcheetah", True, 200, 5, 20, 1, 2000, 8, False),
    ("halfcheetah", True, 200, 5, 20, 3, 37, 7, False),
    ("halfcheetah", False, 200, 1, 1, 1, 200, 30, True),
    ("slim_humanoid", True, 200, 5, 20, 1, 1000, 6, False),
    ("slim_humanoid", True, 200, 5, 10, 2, 9, 5, False),
    ("ant", True, 128, 5, 5, 2, 60, 6, False),
    ("pendulum", True, 256, 5, 5, 2, 500, 6, False),
    ("cartpole", True, 256, 2, 4, 1, 33, 9, False),
    ("halfcheetah", True, 512, 5, 5, 1, 40, 4, False),
]

WD = (0.000025, 0.00005, 0.000075, 0.000075, 0.0001)
CWD = (0.000025, 0.00005, 0.000075)
SPEC = dict(obs_dim=11, act_dim=3, preproc=["drop", "sincos", "id", "id", "sincos"] + ["id"] * 6, postproc=["add"] * 5 + ["replace"] + ["add"] * 5,
            reward=[dict(kind="linear", dim=5), dict(kind="square", dim=3, w=-0.5, when="next_obs")], ctrl_cost=0.001)     # a user-declared env
TRAIN_CASES = [  # env, context + backward model, hidden sizes, E, B, det
    ("halfcheetah", True, (200,) * 4, 5, 256, False),
    ("halfcheetah", True, (200,) * 4, 5, 1856, False),            # the first batch size on the large-batch path at five members
    ("halfcheetah", True, (200,) * 4, 5, 96, True),
    ("ant", False, (200,) * 4, 5, 256, False),                    # vanilla: no context encoder, no backward model
    ("spec", True, (200,) * 4, 5, 37, False),
    ("slim_humanoid", True, (128, 200, 96, 200), 3, 100, False),  # unequal hidden widths, ragged row tile
]
EVAL_CASES = [  # env, context, windows N (no multiple of the chunk), steps F, chunk, det
    ("halfcheetah", True, 70, 3, 64, False),
    ("ant", False, 150, 4, 64, True),
]


def eval_case(lib, env, context, N, F, chunk, det):
    """open-loop horizon error of a small synthetic windowed set: device-drawn noise, then injected noise"""
    prob = synth.make_problem(env=env, context=context, E=5, m=N, H=6, trained_like=True, seed=7)
    rng = np.random.default_rng(3)
    D, A = prob["D"], prob["A"]
    obs = rng.standard_normal((N, F, D))
    obs[:, 0] = prob["obs"]
    mask = (rng.uniform(size=(N, F)) > 0.1).astype(np.float32)
    ds = dict(obs=obs.reshape(N, -1), act=rng.uniform(-1, 1, (N, F * A)), obs_next=obs.reshape(N, -1) + 0.1 * rng.standard_normal((N, F * D)),
              cp_obs=prob["cp_obs"], cp_act=prob["cp_act"], future_bool=mask)
    eng = synth.make_engine(prob, p=5, deterministic=det, lib=lib)
    dev = {k: eng._t(v) for k, v in ds.items() if v is not None}
    res = []
    for kw in (dict(seed=7, call=3), dict(eps=rng.standard_normal((F, N, 1, 5, D)).astype(np.float32))):
        res += [v.cpu().numpy() for _, v in sorted(eng.eval_horizon(dev, N, F, chunk=chunk, **kw).items())]
    torch.cuda.synchronize()
    eng.close()
    return res


def train_case(lib, env, full, hids, E, B, det):
    """losses of three training steps, every weight tensor afterwards, the prediction heads, one evaluation step"""
    prob = synth.make_problem(env=EnvDecl(**SPEC) if env == "spec" else env, context=full, E=E, hidden_sizes=hids, trained_like=True,
                              with_back=full, seed=9)
    batch = synth.make_train_batch(prob, B=B, seed=2)
    keys = ["obs", "act", "delta"] + (["obs_next", "back_delta", "cp_obs", "cp_act"] if full else [])
    eng = synth.make_engine(prob, p=E, deterministic=det, lib=lib)
    eng.train_configure(1e-3, WD, CWD, 1.0, 0.5 if full else 0.0, max_batch=B)
    dev = {k: eng._t(batch[k]) for k in keys}
    res = [eng.train_step(dev, train=True).cpu().numpy() for _ in range(3)]
    res += [v.cpu().numpy() for n in eng.net_names() for _, v in sorted(eng.nets[n].items())]
    res += [x.cpu().numpy() for x in eng.predict_heads(batch["obs"], batch["act"], batch["cp_obs"] if full else None,
                                                        batch["cp_act"] if full else None) if x is not None]
    res.append(eng.train_step(dev, train=False).cpu().numpy())
    torch.cuda.synchronize()
    eng.close()
    return res


def main():
    libs = [_lib.load_dev(os.path.abspath(p)) for p in sys.argv[1:3]]
    bad = 0
    for env, context, hid, E, p, m, n, H, det in CASES:
        prob = synth.make_problem(env=env, context=context, E=E, m=m, H=H, hidden_sizes=(hid,) * 4, trained_like=True, seed=5)
        rng = np.random.default_rng(1)
        if prob["discrete"]:
            acts = np.eye(prob["A"], dtype=np.float32)[rng.integers(0, prob["A"], (m, n, H))]
        else:
            acts = rng.uniform(-1, 1, (m, n, H, prob["A"])).astype(np.float32)
        eps = rng.standard_normal((H, m, n, p, prob["D"])).astype(np.float32)
        outs = []
        for lib in libs:
            eng = synth.make_engine(prob, p=p, deterministic=det, lib=lib)
            ctx = eng.context_forward(prob["cp_obs"], prob["cp_act"]) if context else None
            res = []
            for kw in (dict(eps=None if det else eps), dict(seed=3, call=7, it=1)):
                rows, traj = eng.rollout_returns(prob["obs"], ctx, acts, want_traj=True, norm_actions=not prob["discrete"], **kw)
                res += [rows.cpu().numpy(), traj.cpu().numpy()]
            if not prob["discrete"] and n >= 50:
                cp = (prob["cp_obs"], prob["cp_act"]) if context else (None, None)
                res.append(eng.cem_plan(prob["obs"], *cp, prob["init_mean"], prob["init_var"], n, seed=1, call=2).cpu().numpy())
                res.append(eng.cem_plan_host((prob["obs"], *cp, prob["init_mean"], prob["init_var"]), n, seed=1, call=3))
                res.append(eng.rs_plan(prob["obs"], *cp, n, seed=1, call=4).cpu().numpy())
                prm = eng.icem_params(noise_beta=1.0, keep_elites=3, decay=1.25, add_mean_last=True)
                carry = torch.zeros((m, 3, H, prob["A"]), dtype=torch.float32, device=eng.device)
                valid = torch.zeros((m,), dtype=torch.int32, device=eng.device)
                for call in (5, 6):      # the second call starts from the elites the first one left in the carry
                    res += [x.cpu().numpy() for x in eng.icem_plan(prm, prob["obs"], *cp, prob["init_mean"], prob["init_var"], n, carry=carry,
                                                                   carry_valid=valid, seed=1, call=call, want_best_return=True)]
                res += [carry.cpu().numpy(), valid.cpu().numpy()]
            torch.cuda.synchronize()
            outs.append(res)
            eng.close()
        same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(*outs))
        finite = all(np.isfinite(x).all() for x in outs[1])
        bad += 0 if (same and finite) else 1
        print("%-14s ctx=%d hid=%d E=%d p=%d m=%d n=%d H=%d det=%d: %s%s" % (env, context, hid, E, p, m, n, H, det,
              "identical" if same else "DIFFERENT", "" if finite else " (non-finite!)"))
    for case in EVAL_CASES:
        outs = [eval_case(lib, *case) for lib in libs]
        same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(*outs))
        finite = all(np.isfinite(x).all() for x in outs[1])
        bad += 0 if (same and finite) else 1
        print("eval_horizon %-14s ctx=%d N=%d F=%d chunk=%d det=%d: %s%s" % (case + ("identical" if same else "DIFFERENT", "" if finite else " (non-finite!)")))
    for case in TRAIN_CASES:
        outs = [train_case(lib, *case) for lib in libs]
        same = len(outs[0]) == len(outs[1]) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(*outs))
        finite = all(np.isfinite(x).all() for x in outs[1])
        bad += 0 if (same and finite) else 1
        print("train %-14s ctx+back=%d hid=%s E=%d B=%d det=%d: %s%s" % (case + ("identical" if same else "DIFFERENT", "" if finite else " (non-finite!)")))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
