"""GPU: imagined rollouts (`cadm_imagine_select`, `cadm_imagine`; csrc/imagine.hip) OFF the sizes tests/test_gpu_imagine.py runs at, where
the select stage owns 16 rows per workgroup and the chain is rolled on halfcheetah alone: at p = 30 .. 125 particles the 48 KiB LDS
budget cuts the group to 13, 8, 7 and 2 rows, at p = 255 (D = 48) it fits none, and the chain runs on pendulum (A = 1), ant and
slim_humanoid and, on halfcheetah at p = 50, through a cut group.

Engines, built when first asked for.  Kernel level, never rolled out (`imagine_ref.STAGE_ENGINES`; tests/test_imagine_ref.py holds the
restated `img_group` / `img_lds_bytes` to this table on the CPU; one group takes pad4(G p D) + pad4(G D) + pad4(D) + G of 12288 floats):
    slim35   slim_humanoid  D = 45  p = 35   p D = 1575 (odd)  G = 7   the 37 rows: 5 x 7 + 2; group starts of every alignment in one launch
    hc50     halfcheetah    D = 18  p = 50   p D = 900         G = 13  13, 13, 11
    wide30   corner_spec("widest")  D = 48  p = 30   p D = 1440  G = 8   4 x 8 + 5
    wide125  corner_spec("widest")  D = 48  p = 125  p D = 6000  G = 2   18 x 2 + 1; PE = 25
    wide255  corner_spec("widest")  D = 48  p = 255  one row's tile needs 12337 floats: refused
Rolled out, every one a geometry the library carries (nothing is built on demand), each with an H = 1 twin of the same weights:
    pend, ant, slim   `behind_rollout.POLICY_ENGINES` (context; A = 1, 8, 17; p = 5, 10, 15), m = 2, n = 4
    v-p50             tests/test_gpu_imagine.py's vanilla halfcheetah family at p = 50, m = 3, n = 6: 18 rows in groups of 13 and 5
    v-p685            that family at p = 685, the first multiple of E at which D = 18 fits no row: the refusal through the Python routes

No bar of its own: everything is bit equality -- against `imagine_ref.select_step`, against the twin's one-step rollout and
`uncertainty_cost`, against a sentinel.  The checks are tests/test_gpu_imagine.py's `check_stage` (the body of its
`test_stage_against_restatement`) and `check_chain`, imported.

Code no other test reaches -> the test here that does:
    imagine.hip  a tile stride of p D under G = 7, 13, 8, 2; `sv` and `ssel` behind a tile of another size       test_stage[*]
                 the tail group ng < G with G < 16 (2, 11, 5 and 1 rows)                                         test_stage[*]
                 the broadcast walk with p > S = 256 / D: dc = 0, dj = S, the `j >= p` carry over many passes     test_stage[*] (S = 5, 14, 5, 5)
                 groups that start 16-byte aligned and groups that do not in ONE launch (odd p D, G = 7), the
                 scalar-load path and the 16-byte one side by side                                               test_stage[slim35]
                 PE = 25 members' particles in the variance chain; sel up to 124                                 test_stage[wide125]
                 `img_group == 0`: `imagine_fill` refuses before any launch, from every entry                    test_refusal
                 the chain at A = 1, 8, 17 and D = 3, 28, 45 (`imagine_actions_kernel`, the policy step, the
                 one-step rollout from `cur`, the broadcast feeding it) on pendulum, ant, slim_humanoid          test_chain[pend], [ant], [slim]
                 a cut group and its partial tail inside the real chain                                          test_chain[v-p50]

Two things are not as the issue wrote them down; neither exposed a fault, and no kernel was changed.
(1) "Rows 100 .. 136 of 150: the position inside a group shifts, because 100 is not a multiple of 7, 13, 8 or 2."  100 is a multiple
of 2.  On wide125 the 37 rows are embedded at row 101 (`imagine_ref.STAGE_AT`), so that they do change their place inside the groups
of 2; on the others at 100, as the feature file does.
(2) It asked for the refusal of `imagine_select`, `imagine` and the class route on the widest geometry at p = 255.  `HipEngine.imagine`
and `model.imagine` make sure of a rollout kernel (`ensure_rollout`) before they reach the library's refusal, and on the widest
geometry that builds a module on demand -- which this file must not do.  So the C entries `cadm_imagine_select` and `cadm_imagine` and
`HipEngine.imagine_select` are refused on the widest geometry at p = 255, with every output buffer filled with a sentinel and intact
afterwards; `HipEngine.imagine` and `model.imagine` are refused with the same message on halfcheetah at p = 685 (685 x 18 = 12330
floats), a geometry the library carries.

Measured on an MI355X: every comparison is bit equality and every case passes.  The whole file runs in 3 s, the slowest case (the
refusal, which builds three models) in 0.3 s."""
import ctypes as ct

import numpy as np
import pytest
import torch

import behind_rollout as br
import imagine_ref as iref
from cadm_amd import _lib
from cadm_amd import synth
from helpers import _np, corner_spec, make_engine, plan_model
from test_gpu_imagine import BIG, _same, _set_policy, check_chain, check_stage

pytestmark = pytest.mark.gpu

F = np.float32
REFUSAL = "does not fit the select kernel's LDS"


@pytest.fixture(scope="module")
def engines(gpu):
    """name -> (problem, engine), built when first asked for: `imagine_ref.STAGE_ENGINES` (kernel level: tests/test_gpu_imagine.py's
    problem of the kind, m = 2, H = 3, seed 52); "pend", "ant", "slim" of `behind_rollout.POLICY_ENGINES` and "v-p<p>" of
    tests/test_gpu_imagine.py's vanilla halfcheetah family, each with "-h1" for the twin of the same weights and horizon 1"""
    built, probs = {}, {}

    def get(name):
        if name in built:
            return built[name]
        base, _, twin = name.partition("-h")
        if name in iref.STAGE_ENGINES:
            kind, D, p, _, _ = iref.STAGE_ENGINES[name]
            prob = synth.make_problem(env=corner_spec(kind) if kind == "widest" else kind, context=True, E=5, m=2, H=3, seed=52)
            eng = make_engine(prob, p=p)
        elif base.startswith("v-p"):
            if "v" not in probs:
                probs["v"] = synth.make_problem(env="halfcheetah", context=False, E=5, m=3, H=4, seed=11, trained_like=True)
            prob, p, D = probs["v"], int(base[3:]), 18
            eng = make_engine(prob, p=p, H=1 if twin else 4)
        else:
            kind, D, A, E, p, H, context, bounds = br.POLICY_ENGINES[base]
            assert bounds is None
            if base not in probs:
                probs[base] = br.policy_problem(base)
            prob = probs[base]
            eng = make_engine(prob, p=p, H=1 if twin else H)
        assert (eng.D, eng.p, eng.E) == (D, p, 5)
        assert name in iref.STAGE_ENGINES or eng.lib.cadm_rollout_builtin(eng._ctx), "%s: nothing may be built on demand" % name
        built[name] = (prob, eng)
        return built[name]
    yield get
    for n_, (_, eng) in built.items():
        assert n_ not in iref.STAGE_ENGINES or not eng._rollout_ready, "a kernel-level engine was rolled out"
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------- 1: the stage under a cut group
@pytest.mark.parametrize("name", ["slim35", "hc50", "wide30", "wide125"])
def test_stage(engines, name):
    """tests/test_gpu_imagine.py's `test_stage_against_restatement`, its whole body, where the budget cuts the group: every output of
    `imagine_select` on 37 rows against `imagine_ref.select_step` bit for bit -- with and without constraints and per-dim weights, from
    an aligned buffer and from one that starts one float behind, without a broadcast, at rows 100 .. 136 (wide125: 101 .. 137) of 150
    under the same sel, under a clamped sel.  The group is asserted against the restated `img_group` first."""
    _, eng = engines(name)
    _, D, p, G, groups = iref.STAGE_ENGINES[name]
    assert iref.group(eng.p, eng.D) == G < iref.GROUP and iref.lds_bytes(G, p, D) <= iref.LDS_BUDGET < iref.lds_bytes(G + 1, p, D)
    at = iref.STAGE_AT.get(name, 100)
    assert [min(G, 37 - r) for r in range(0, 37, G)] == groups and groups[-1] < G and at % G != 0 and p > 256 // D
    if name == "slim35":
        assert sorted({(r * p * D) % 4 for r in range(0, 37, G)}) == [0, 1, 2, 3]
    check_stage(eng, name, at)


# ---------------------------------------------------------------------------------------------------------------------- 2: the refusal
def _sentinels(eng, sizes):
    return [torch.full((max(int(s), 1),), 0xA5, dtype=torch.uint8, device=eng.device) for s in sizes]


def _intact(bufs, what):
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert bool((b == 0xA5).all()), "%s: output buffer %d was written by a refused call" % (what, i)


def test_refusal(engines):
    """`img_group == 0`.  The widest geometry at p = 255: `cadm_imagine_select` and `cadm_imagine` return CADM_EINVAL with "does not fit
    the select kernel's LDS", one row's 48 948 bytes and the bound in the message, and no output buffer -- each filled with a sentinel
    -- changes; `HipEngine.imagine_select` raises it.  Halfcheetah at p = 685 (a geometry the library carries): `HipEngine.imagine` and
    the class route raise it."""
    _, eng = engines("wide255")
    lib, ctx, D, p, A = eng.lib, eng._ctx, eng.D, eng.p, eng.A
    assert iref.group(p, D) == 0 and iref.lds_bytes(1, p, D) == 4 * 12337
    R, m, n, k = 5, 2, 2, 2
    src = torch.zeros((R * p * D,), dtype=torch.float32, device=eng.device)
    P = lambda t: ct.c_void_p(t.data_ptr())
    # alive, state_out, rew, done, valid, member, disagreement, length, bcast
    outs = _sentinels(eng, [R, 4 * R * D, 4 * R, R, R, 4 * R, 4 * R, 4 * R, 4 * R * p * D])
    rc = lib.cadm_imagine_select(ctx, P(src), P(src), P(src), None, R, 0, None, None, 0, 0, *[P(o) for o in outs], None)
    msg = lib.cadm_last_error().decode()
    assert rc == -1 and msg.startswith("cadm_imagine_select:") and REFUSAL in msg and "%d bytes" % (4 * 12337) in msg and "p (255) x D (48)" in msg, msg
    _intact(outs, "cadm_imagine_select")
    need = lib.cadm_imagine_workspace_bytes(ctx, m, n, k, None)
    assert need > 0
    ws = _sentinels(eng, [need + 4096])
    rc = lib.cadm_imagine(ctx, P(src), P(src), P(src), m, n, k, 0.0, None, None, 0, 0, P(ws[0]), None)
    msg = lib.cadm_last_error().decode()
    assert rc == -1 and msg.startswith("cadm_imagine:") and REFUSAL in msg, msg
    _intact(ws, "cadm_imagine")
    assert not _np(src).any()
    with pytest.raises(_lib.CadmError, match=REFUSAL):
        eng.imagine_select(np.zeros((R, p, D), F), np.zeros((R, p), F), np.zeros((R, D), F), np.ones((R,), np.uint8))
    # the Python routes behind `ensure_rollout`, on a geometry the library carries
    prob, big = engines("v-p685")
    assert iref.group(big.p, big.D) == 0 and iref.group(680, big.D) == 1
    acts = np.zeros((3, n, k, big.A), F)
    with pytest.raises(_lib.CadmError, match=REFUSAL):
        big.imagine(np.asarray(prob["obs"], F), None, k, n, acts)
    model, mprob = plan_model(False, 4, n_particles=685, **BIG)
    with pytest.raises(_lib.CadmError, match=REFUSAL):
        model.imagine(mprob["obs"], horizon=k, branches=n, actions=np.zeros((2, n, k, 6), F))
    ok, _ = plan_model(False, 4, n_particles=50, **BIG)      # ... and p = 50 is taken
    out = ok.imagine(mprob["obs"], horizon=k, branches=n, actions=np.zeros((2, n, k, 6), F), numpy=True)
    assert out["valid"].all() and np.isfinite(out["states"]).all()


# ---------------------------------------------------------------------------------------------------------------------- 3: the chain
CHAINS = [("pend", 2, 4), ("ant", 2, 4), ("slim", 2, 4), ("v-p50", 3, 6)]


@pytest.mark.parametrize("name,m,n", CHAINS, ids=[c[0] for c in CHAINS])
def test_chain(engines, name, m, n):
    """tests/test_gpu_imagine.py's `check_chain` for k = 3 -- every step bit for bit against the H = 1 twin's one-step rollout from the
    broadcast of states[t], `uncertainty_cost`'s step of its trajectory and the restatement -- under given actions drawn beyond the
    bounds (the clip binds), under the registered policy without noise (act[t] is `policy_eval(states[t])`) and with noise 0.3 (every
    row moves, the actions stay inside the bounds)."""
    prob, eng = engines(name)
    _, twin = engines(name + "-h1")
    assert twin.H == 1 and (twin.D, twin.A, twin.p) == (eng.D, eng.A, eng.p)
    if name == "v-p50":
        G = iref.group(eng.p, eng.D)
        assert G == 13 and [min(G, m * n - r) for r in range(0, m * n, G)] == [13, 5]
    k, seed, call = 3, 21, 6
    lb, ub = F(eng.cfg.lower_bound), F(eng.cfg.upper_bound)
    actions = np.random.default_rng(m * 10 + n).uniform(1.3 * lb, 1.3 * ub, (m, n, k, eng.A)).astype(F)
    out, sels = check_chain(eng, twin, prob, m, n, k, seed, call, actions=actions)
    assert ((out["act"] == lb) | (out["act"] == ub)).any() and (out["act"] >= lb).all() and (out["act"] <= ub).all()
    assert out["valid"][0].all() and (out["member"][0] == sels[0] // (eng.p // eng.E)).all()
    assert not np.array_equal(out["states"][1][:, 0], out["states"][1][:, 1]), "the branches of one start state differ"
    _set_policy(eng)
    try:
        clean, _ = check_chain(eng, twin, prob, m, n, k, seed, call)
        for t in range(k):
            _same(clean["act"][t], _np(eng.policy_eval(clean["states"][t])), "act[%d] is policy_eval(states[%d])" % (t, t))
        loud, _ = check_chain(eng, twin, prob, m, n, k, seed, call, noise=0.3)
        assert (loud["act"] >= lb).all() and (loud["act"] <= ub).all()
        moved = (loud["act"][0] != clean["act"][0]).any(axis=-1)
        assert moved.all(), "a row without noise"
        _same(loud["states"][0], clean["states"][0], "the start states")
    finally:
        eng.set_policy_net(None)
