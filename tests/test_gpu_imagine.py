"""GPU: imagined rollouts for a learner -- the stage between two one-step rollouts (`cadm_imagine_select`, csrc/imagine.hip) against
the numpy restatement (tests/imagine_ref.py) bit for bit, the chain (`cadm_imagine`) one step at a time against the public one-step
rollout of a second engine, the policy's actions and their noise, k against the engine's horizon, termination, the counters, the
learned reward, the class route and the refusals.

Geometries: the stage alone on pendulum (D = 3), hopper_like (D = 11) and the widest declarable env (D = 48) at p = 5 and on
halfcheetah at p = 20 -- kernel-level engines that are never rolled out; everything that rolls out on the compiled-in halfcheetah
200 x 4 kernel, vanilla and with context, through tests/test_gpu_policy.py's engine families whose H = 1 twins share their weights.

The stage owns 16 consecutive rows per workgroup at these sizes, so a group's span of `next` starts 16-byte aligned whenever the
buffer does; the scalar-load path is reached by handing the stage a buffer that starts one float behind an aligned address.
tests/test_gpu_imagine_envelope.py runs `check_stage` and `check_chain` where the LDS budget cuts the group below 16 and on the other
built-in kinds."""
import ctypes as ct
import math

import numpy as np
import pytest
import torch

import imagine_ref as iref
import policy_ref as pref
import reward_ref as rref
import uncertainty_ref as uref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import _np, assert_close, corner_spec, make_engine, plan_act, plan_model

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")
BIG = dict(hidden=(200,) * 4)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %r %s against %r %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype == np.float32:
        got, want = _bits(got), _bits(want)
    np.testing.assert_array_equal(got, want, err_msg=what)


@pytest.fixture(scope="module")
def engines(gpu):
    """name -> (problem, engine), built when first asked for.  Kernel level, never rolled out: "pend", "hopper", "wide" (p = 5) and "hc20"
    (halfcheetah, p = 20).  Halfcheetah 200 x 4 (the compiled-in rollout), m = 3 in the problem: "v-p5-hH" vanilla, "c-p20-hH" with
    context, "cd-p5-hH" with context and deterministic -- engines of one family share their weights, so "...-h1" is the one-step twin."""
    built, probs = {}, {}
    level = ("pend", "hopper", "wide", "hc20")

    def get(name):
        if name not in built:
            if name in level:
                from test_gpu_constraints import hopper_like
                env = {"pend": "pendulum", "hopper": hopper_like(), "wide": corner_spec("widest"), "hc20": "halfcheetah"}[name]
                prob = synth.make_problem(env=env, context=name != "pend", E=5, m=2, H=3, seed=52)
                built[name] = (prob, make_engine(prob, p=20 if name == "hc20" else 5))
            else:
                fam, p, H = name.split("-")
                if fam not in probs:
                    probs[fam] = synth.make_problem(env="halfcheetah", context=fam != "v", E=5, m=3, H=4, seed=11, trained_like=True)
                built[name] = (probs[fam], make_engine(probs[fam], p=int(p[1:]), H=int(H[1:]), deterministic=fam == "cd"))
        return built[name]
    yield get
    for n_, (_, eng) in built.items():
        assert n_ not in level or not eng._rollout_ready, "a kernel-level engine was rolled out"
        eng.close()


def _set_policy(eng, hidden=(50, 30), act="tanh", seed=40):
    layers = pref.he_policy(eng.D, hidden, eng.A, seed, 0.5)
    eng.set_policy_net(HipEngine.policy_params(hidden, act, "tanh", 1, 0.0), layers)
    return layers


def _select_np(o):
    return {k: None if v is None else _np(v) for k, v in o.items()}


# ---------------------------------------------------------------------------------------------------------------------- 1: the stage alone
CONS = [dict(dim=0, lo=-1.5, hi=1.5), dict(dim=2, hi=2.5)]


def _synthetic(eng, R, seed, call, t):
    """next / rows1 / state / alive / length for R rows and the restated draw, with every special case planted by row"""
    rng = np.random.default_rng(90 + eng.D)
    p, D = eng.p, eng.D
    nxt = rng.standard_normal((R, p, D)).astype(F)
    rows1 = rng.standard_normal((R, p)).astype(F)
    state = rng.standard_normal((R, D)).astype(F)
    alive = np.ones((R,), np.uint8)
    length = rng.integers(0, 5, R).astype(np.int32)
    sel = iref.select(iref.words(seed, call, np.arange(R), t), p)
    other = (sel + 1 + np.arange(R) % (p - 1)) % p              # a particle that is not the selected one
    assert (other != sel).all()
    nxt[3, sel[3], D - 1] = NAN                                  # non-finite values in the selected particle
    nxt[4, sel[4], 1] = math.inf
    nxt[33, sel[33], 0] = -math.inf                              # (in the partial last group)
    nxt[5, other[5], 1] = NAN                                    # ... and in a particle that is not selected
    nxt[6, other[6], D - 1] = -math.inf
    nxt[36, other[36], 0] = NAN
    nxt[7, sel[7], 0] = 1.5                                      # on a bound exactly: violates
    nxt[8, sel[8], 0] = -1.5
    nxt[9, sel[9], 2] = 2.5
    nxt[10, sel[10], 0], nxt[10, sel[10], 2] = np.nextafter(F(1.5), F(0)), np.nextafter(F(2.5), F(0))      # just inside: healthy
    nxt[11, other[11], 0] = 9.0                                  # a violation in a particle that is not selected does not count
    nxt[11, sel[11], 0], nxt[11, sel[11], 2] = 0.0, 0.0
    alive[[12, 13, 20, 35]] = 0                                  # rows that were dead before the step
    nxt[13, sel[13], 0] = NAN
    nxt[20, :, :] = math.inf
    return nxt, rows1, state, alive, length, sel


def check_stage(eng, name, at=100):
    """The body of `test_stage_against_restatement` on any engine; at: the row of a batch of 150 at which the 37 rows are run again."""
    R, seed, call, t = 37, 11, 5, 2
    nxt, rows1, state, alive, length, sel = _synthetic(eng, R, seed, call, t)
    assert len(np.unique(sel)) >= 5
    cons = HipEngine.constraint_params(CONS, "terminate", 1.0)
    w = uref.make_w("per-dim", eng.D, 3)
    shifted = torch.zeros((nxt.size + 5,), dtype=torch.float32, device=eng.device)
    shifted[1:1 + nxt.size] = torch.as_tensor(nxt.reshape(-1)).to(eng.device)
    shifted = shifted[1:1 + nxt.size].view(nxt.shape)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for c_ref, c_dev, w_ in ((CONS, cons, w), (None, None, None), (CONS, cons, None)):
        want = iref.select_step(nxt, rows1, state, alive, sel, eng.E, c_ref, w_, length)
        got = _select_np(eng.imagine_select(nxt, rows1, state, alive, t=t, constraints=c_dev, w=w_, seed=seed, call=call, length=length))
        for key in want:
            _same(got[key], want[key], "%s %s" % (name, key))
        again = _select_np(eng.imagine_select(shifted, rows1, state, alive, t=t, constraints=c_dev, w=w_, seed=seed, call=call, length=length))
        for key in want:
            _same(again[key], want[key], "%s %s from a buffer one float behind alignment" % (name, key))
        last = _select_np(eng.imagine_select(nxt, rows1, state, alive, t=t, constraints=c_dev, w=w_, seed=seed, call=call, want_bcast=False))
        assert last["bcast"] is None
        _same(last["state"], want["state"], "%s state without a broadcast" % name)
    # what the planted rows must show, so that the comparison above is about something
    assert want["valid"][[3, 4, 33, 12, 13, 20, 35]].sum() == 0 and want["done"][[7, 8, 9]].all() and not want["done"][[10, 11]].any()
    assert want["valid"][[5, 6, 36, 7, 8, 9, 10, 11]].all() and (want["disagreement"][[6, 36]] == np.inf).all()
    assert (want["member"][[12, 13, 20, 35]] == -1).all() and np.isfinite(want["state"]).all() and np.isfinite(want["bcast"]).all()
    # another key or step: other draws
    moved = _select_np(eng.imagine_select(nxt, rows1, state, alive, t=t + 1, seed=seed, call=call))
    assert (moved["member"] != got["member"]).any()
    np.testing.assert_array_equal(moved["member"][alive > 0], iref.select(iref.words(seed, call, np.arange(R), t + 1), eng.p)[alive > 0] // (eng.p // eng.E))
    # the same rows at rows 100 .. 136 of 150: the draw is keyed by the row index, so the test feeds the sel the rows had at 0 .. 36
    rng = np.random.default_rng(4)
    big = lambda x, fill: np.concatenate([fill(at), x, fill(150 - R - at)], axis=0)
    nb = big(nxt, lambda k: rng.standard_normal((k,) + nxt.shape[1:]).astype(F))
    rb = big(rows1, lambda k: rng.standard_normal((k, eng.p)).astype(F))
    sb = big(state, lambda k: rng.standard_normal((k, eng.D)).astype(F))
    ab = big(alive, lambda k: np.ones((k,), np.uint8))
    lb = big(length, lambda k: np.zeros((k,), np.int32))
    selb = big(sel, lambda k: rng.integers(0, eng.p, k).astype(np.int32))
    want = iref.select_step(nxt, rows1, state, alive, sel, eng.E, CONS, w, length)
    moved = _select_np(eng.imagine_select(nb, rb, sb, ab, t=t, sel=selb, constraints=cons, w=w, seed=seed + 1, call=call, length=lb))
    for key in want:
        _same(moved[key][at:at + R], want[key], "%s %s at rows %d .. %d" % (name, key, at, at + R - 1))
    # a sel outside 0 .. p - 1 is clamped, never an index
    wild = _select_np(eng.imagine_select(nxt, rows1, state, alive, t=t, sel=np.where(np.arange(R) % 2 == 0, -7, 1000).astype(np.int32)))
    np.testing.assert_array_equal(wild["member"][alive > 0], np.where(np.arange(R) % 2 == 0, 0, eng.E - 1)[alive > 0])


@pytest.mark.parametrize("name", ["pend", "hopper", "wide", "hc20"])
def test_stage_against_restatement(engines, name):
    """`imagine_select` on 37 rows (two full groups of 16 and a tail of 5) of synthetic particles: every output -- states[t + 1], rew,
    done, valid, member, disagreement, alive, length and the p-fold broadcast -- equals the restatement bit for bit, with and without
    constraints and per-dim weights, from an aligned buffer (16-byte loads) and from one that starts one float behind (scalar loads; p D
    is odd at D = 3 and 11), run to run; and the same rows at another position of a larger batch, fed the same sel, give the same bits."""
    _, eng = engines(name)
    check_stage(eng, name)


# ---------------------------------------------------------------------------------------------------------------------- 2: the chain, one step at a time
def check_chain(eng, twin, prob, m, n, k, seed, call, actions=None, noise=0.0, constraints=None, w=None):
    """`imagine` on the first m envs of `prob`, every step checked on its own against the H = 1 twin so that nothing compounds -> (out as
    numpy, the sel of every step)."""
    context = eng.C > 0
    obs = np.asarray(prob["obs"], F)[:m]
    hist = (prob["cp_obs"][:m], prob["cp_act"][:m]) if context else None
    ctx_vec = eng.context_forward(*hist) if context else None
    cons = None if constraints is None else HipEngine.constraint_params(constraints, "penalty", 0.0)
    out = _select_np(eng.imagine(obs, ctx_vec, k, n, actions, noise, cons, w, seed, call))
    again = _select_np(eng.imagine(obs, ctx_vec, k, n, actions, noise, cons, w, seed, call))
    for key in out:
        _same(again[key], out[key], "run to run: %s" % key)
    p, D, A, R = eng.p, eng.D, eng.A, m * n
    assert out["states"].shape == (k + 1, m, n, D) and out["act"].shape == (k, m, n, A) and out["length"].shape == (m, n)
    _same(out["states"][0], np.ascontiguousarray(np.broadcast_to(obs[:, None, :], (m, n, D))), "states[0] is the start state of every branch")
    sels = iref.draws(seed, call, m, n, k, p)
    alive, length = np.ones((R,), np.uint8), np.zeros((R,), np.int32)
    unc = HipEngine.uncertainty_params("epistemic", 1.0, w, "var", None, obs_dim=D)
    tv = twin.context_forward(*hist) if context else None
    for t in range(k):
        a = out["act"][t]
        if actions is not None:
            _same(a, np.clip(np.asarray(actions, F)[:, :, t], F(eng.cfg.lower_bound), F(eng.cfg.upper_bound)), "act[%d] is the clipped given action" % t)
        bro = np.ascontiguousarray(np.broadcast_to(out["states"][t][:, :, None, :], (m, n, p, D)))
        rows, traj = twin.rollout_returns(obs, tv, np.ascontiguousarray(a[:, :, None, :]), obs_rows=bro.reshape(-1, D), seed=seed, call=call,
                                          it=hplanner.IMAGINE_IT + 2 * t, want_traj=True)
        step = _np(twin.uncertainty_cost(traj, unc, want_steps=True)[0])
        rows, traj = _np(rows), _np(traj)
        assert traj.shape == (1, m, n, p, D) and step.shape == (m, n, 1)
        want = iref.select_step(traj[0].reshape(R, p, D), rows.reshape(R, p), out["states"][t].reshape(R, D), alive, sels[t].reshape(R), eng.E,
                                constraints, w, length)
        live = alive.reshape(m, n) > 0
        picked = np.take_along_axis(traj[0], sels[t][:, :, None, None].astype(np.int64), axis=2)[:, :, 0]
        ok = out["valid"][t] > 0
        _same(out["states"][t + 1][ok], picked[ok], "step %d: the selected particles of the one-step rollout" % t)
        _same(out["rew"][t][ok], np.take_along_axis(rows, sels[t][:, :, None].astype(np.int64), axis=2)[:, :, 0][ok], "step %d: rew is rows at sel" % t)
        _same(out["disagreement"][t][live], np.where(np.isfinite(step[:, :, 0]), step[:, :, 0], F(np.inf))[live],
              "step %d: disagreement is uncertainty_cost's step" % t)
        for key, name in (("state", "states"), ("rew", "rew"), ("done", "done"), ("valid", "valid"), ("member", "member"),
                          ("disagreement", "disagreement")):
            got = out[name][t + 1] if key == "state" else out[name][t]
            _same(got.reshape(want[key].shape), want[key], "step %d: %s against the restatement" % (t, name))
        alive, length = want["alive"], want["length"]
        if not eng.deterministic and p > eng.E:      # two particles of one member differ by their head noise
            assert not np.array_equal(traj[0][:, :, 0], traj[0][:, :, 1])
    _same(out["length"].reshape(R), length, "length")
    _same(out["alive"].reshape(R), alive, "alive")
    _same(out["length"], out["valid"].sum(axis=0).astype(np.int32), "length is the count of valid transitions")
    return out, sels


CHAINS = [("v-p5", 3, 4), ("v-p5", 3, 1), ("c-p20", 3, 4), ("c-p20", 3, 1), ("cd-p5", 2, 3)]


@pytest.mark.parametrize("fam,m,n", CHAINS, ids=["%s-m%d-n%d" % c for c in CHAINS])
def test_chain_with_given_actions(engines, fam, m, n):
    """k = 3 steps under the caller's actions (drawn beyond the bounds, so the clip binds): per step the particles `imagine` selected from
    are, bit for bit, `rollout_returns(obs_rows = the broadcast of states[t], it = CADM_IMAGINE_IT + 2 t)` of the H = 1 twin, rew is that
    rollout's rows at sel, disagreement is `uncertainty_cost`'s step of its traj, and states, member, valid, done follow the
    restatement.  The branches of one start state differ (their own draws and head noise); a deterministic ctx still draws sel."""
    prob, eng = engines("%s-h4" % fam)
    _, twin = engines("%s-h1" % fam)
    k, seed, call = 3, 21, 6
    actions = np.random.default_rng(m * 10 + n).uniform(-1.3, 1.3, (m, n, k, eng.A)).astype(F)
    out, sels = check_chain(eng, twin, prob, m, n, k, seed, call, actions=actions)
    assert out["valid"].all() and not out["done"].any() and (out["length"] == k).all() and np.isfinite(out["rew"]).all()
    assert (out["member"] == sels // (eng.p // eng.E)).all() and (np.abs(out["act"]) == 1).any()
    assert (out["disagreement"] > 0).all() and np.isfinite(out["disagreement"]).all()
    if n > 1:
        assert not np.array_equal(out["states"][1][:, 0], out["states"][1][:, 1])
    # per-dim weights change the disagreement and nothing else
    w = uref.make_w("per-dim", eng.D, 1)
    other, _ = check_chain(eng, twin, prob, m, n, k, seed, call, actions=actions, w=w)
    for key in out:
        assert (key == "disagreement") != np.array_equal(other[key], out[key]), key


# ---------------------------------------------------------------------------------------------------------------------- 3: the chain with the policy
@pytest.mark.parametrize("fam", ["v-p5", "c-p20"])
def test_chain_with_the_policy(engines, fam):
    """noise_std = 0: act[t] is `policy_eval(states[t])`, bit for bit, and the chain checks out step by step as with given actions.
    noise_std > 0: EVERY row, row 0 of every start state included, differs from the clean action of its state by noise_std * xi of Philox
    counter (row, t, g, 7) keyed (seed, call), at `assert_close`'s 1e-5 wherever the clip does not bind; the actions stay inside the bounds."""
    prob, eng = engines("%s-h4" % fam)
    _, twin = engines("%s-h1" % fam)
    _set_policy(eng)
    m, n, k, seed, call, noise = 3, 4, 3, 8, 2, 0.3
    try:
        out, _ = check_chain(eng, twin, prob, m, n, k, seed, call)
        for t in range(k):
            _same(out["act"][t], _np(eng.policy_eval(out["states"][t])), "act[%d] is policy_eval(states[%d])" % (t, t))
        loud, _ = check_chain(eng, twin, prob, m, n, k, seed, call, noise=noise)
        assert np.abs(loud["act"]).max() <= 1.0
        for t in range(k):
            clean = _np(eng.policy_eval(loud["states"][t])).astype(np.float64)
            z = iref.xi(seed, call, m * n, t, eng.A).reshape(m, n, eng.A)
            a = loud["act"][t]
            free = (a > F(-1)) & (a < F(1))
            assert free.mean() > 0.5
            diff = a.astype(np.float64) - clean
            assert (np.abs(diff) > 0).any(axis=-1).all(), "a row without noise"
            assert_close(diff[free], (F(noise) * z)[free], what="step %d: the noise" % t)
            print("\n[%s t=%d] worst |noise err| %.3e" % (fam, t, np.abs(diff[free] - (F(noise) * z)[free].astype(np.float64)).max()))
        _same(loud["states"][0], out["states"][0], "the start states")
        assert not np.array_equal(loud["act"][0], out["act"][0])
    finally:
        eng.set_policy_net(None)
    with pytest.raises(_lib.CadmError, match="neither actions nor a registered policy"):
        eng.imagine(np.asarray(prob["obs"], F), eng.context_forward(prob["cp_obs"], prob["cp_act"]) if eng.C else None, 2, 2)


# ---------------------------------------------------------------------------------------------------------------------- 4: k and the engine's horizon
@pytest.mark.parametrize("k", [6, 1])
def test_k_is_independent_of_the_horizon(engines, k):
    prob, eng = engines("v-p5-h4")
    _, twin = engines("v-p5-h1")
    actions = np.random.default_rng(k).uniform(-1, 1, (2, 3, k, eng.A)).astype(F)
    out, _ = check_chain(eng, twin, prob, 2, 3, k, 4, 1, actions=actions)
    assert out["states"].shape[0] == k + 1 and out["valid"].all()
    # the H = 1 twin itself gives the same bits: nothing depends on the engine's horizon
    mine = _select_np(twin.imagine(np.asarray(prob["obs"], F)[:2], None, k, 3, actions, 0.0, None, None, 4, 1))
    for key in out:
        _same(mine[key], out[key], "H = 1 engine: %s" % key)


# ---------------------------------------------------------------------------------------------------------------------- 5: termination
def test_termination(engines):
    """A constraint that binds -- its bound is a value a row's state takes at step 2, so that row lands ON it: done is set once per row
    at most, every later step of the row is valid = 0, frozen and empty, length is the count; the rows that never leave are bit for bit
    what they are without constraints.  A constraint that never binds leaves every output as it is without one."""
    prob, eng = engines("v-p5-h4")
    _, twin = engines("v-p5-h1")
    m, n, k, seed, call = 3, 8, 4, 13, 3
    actions = np.random.default_rng(7).uniform(-1, 1, (m, n, k, eng.A)).astype(F)
    free, _ = check_chain(eng, twin, prob, m, n, k, seed, call, actions=actions)
    x0 = free["states"][1:, :, :, 0]                              # [k, m, n]
    peak = x0.max(axis=0)
    row = np.unravel_index(np.argsort(peak.reshape(-1))[peak.size // 2], peak.shape)      # the row with the median peak
    hi = float(peak[row])
    cons = [dict(dim=0, hi=hi)]
    out, _ = check_chain(eng, twin, prob, m, n, k, seed, call, actions=actions, constraints=cons)
    done, valid = out["done"].astype(bool), out["valid"].astype(bool)
    assert (done.sum(axis=0) <= 1).all() and 0 < done.sum() < m * n and done[:, row[0], row[1]].any(), "a value on the bound violates"
    first = np.where(done.any(axis=0), done.argmax(axis=0), k)
    want_first = np.where((x0 >= F(hi)).any(axis=0), (x0 >= F(hi)).argmax(axis=0), k)
    np.testing.assert_array_equal(first, want_first)
    steps = np.arange(k)[:, None, None]
    np.testing.assert_array_equal(valid, steps <= first[None])
    assert not (done & ~valid).any()
    np.testing.assert_array_equal(out["length"], np.minimum(first + 1, k))
    for t in range(k):
        dead = t > first
        _same(out["states"][t + 1][dead], out["states"][t][dead], "step %d: a dead row is frozen" % t)
        assert (out["rew"][t][dead] == 0).all() and (out["member"][t][dead] == -1).all() and (out["disagreement"][t][dead] == 0).all()
        for key in ("rew", "member", "disagreement", "act"):
            _same(out[key][t][~dead], free[key][t][~dead], "step %d: %s of the rows still alive" % (t, key))
        _same(out["states"][t + 1][~dead], free["states"][t + 1][~dead], "step %d: states of the rows still alive" % t)
    never, _ = check_chain(eng, twin, prob, m, n, k, seed, call, actions=actions, constraints=[dict(dim=0, lo=-1e30, hi=1e30), dict(dim=5, hi=1e30)])
    for key in free:
        _same(never[key], free[key], "a constraint that never binds: %s" % key)


# ---------------------------------------------------------------------------------------------------------------------- 6: counters, determinism
def _layers(seed=17):
    return pref.he_policy(18, (16,), 6, seed, 0.5)


@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "context"])
def test_counters_and_determinism(gpu, context):
    """Two models with one seed give identical outputs; a second call differs, because `_imagine_call` moved; `get_action`'s `_call`
    never moves, and its plans are bit-identical with and without an `imagine` between them -- on the reference planner with an
    `imagine_policy`-only model (whose `_opt` stays None) and on the opt-in planner with a policy prior."""
    ip = dict(hidden_sizes=(16,), activation="tanh")
    H = 4
    a, prob = plan_model(context, H, imagine_policy=ip, **BIG)
    b, _ = plan_model(context, H, imagine_policy=ip, **BIG)
    assert a._opt is None and b._opt is None, "imagine_policy must not switch the planner"
    hist = (prob["cp_obs"], prob["cp_act"]) if context else ()
    for model in (a, b):
        model.set_policy(_layers())
    o1 = a.imagine(prob["obs"], *hist, horizon=3, branches=2, noise_std=0.2, numpy=True)
    o2 = b.imagine(prob["obs"], *hist, horizon=3, branches=2, noise_std=0.2, numpy=True)
    assert a._imagine_call == 1 and a._call == 0 and a._eval_call == 0
    for key in o1:
        _same(np.asarray(o2[key]), np.asarray(o1[key]), "two models, one seed: %s" % key)
    o3 = a.imagine(prob["obs"], *hist, horizon=3, branches=2, noise_std=0.2, numpy=True)
    assert a._imagine_call == 2 and not np.array_equal(o3["states"][1], o1["states"][1]) and not np.array_equal(o3["member"], o1["member"])
    _same(o3["states"][0], o1["states"][0], "the start states")
    other = a.imagine(prob["obs"], *hist, horizon=3, branches=2, noise_std=0.2, seed=a.seed + 1, numpy=True)
    assert not np.array_equal(other["states"][1], o3["states"][1])
    # the engine route under the key the class used
    eng = a.engine
    ctx_vec = eng.context_forward(*hist) if context else None
    direct = eng.imagine(np.asarray(prob["obs"], F), ctx_vec, 3, 2, None, 0.2, None, None, a.seed, 0)
    for key in ("states", "act", "rew", "member", "disagreement"):
        _same(_np(direct[key]), o1[key], "the class route is the engine's under (seed, 0): %s" % key)
    mean, var = prob["init_mean"], prob["init_var"]
    # plans with and without an imagine between them: the reference planner ...
    p1, p2 = plan_act(a, prob, context, mean, var), plan_act(a, prob, context, mean, var)
    q1 = plan_act(b, prob, context, mean, var)
    b.imagine(prob["obs"], *hist, horizon=2, branches=3)
    q2 = plan_act(b, prob, context, mean, var)
    assert a._call == b._call == 2 and b._imagine_call == 2
    _same(q1, p1, "the first plan")
    _same(q2, p2, "the plan behind an imagine")
    ref, _ = plan_model(context, H, **BIG)                        # ... which is the plan of a model that never heard of imagine_policy
    _same(plan_act(ref, prob, context, mean, var), p1, "imagine_policy leaves get_action on the reference path")
    # ... and the opt-in planner with a policy prior
    pp = dict(hidden_sizes=(16,), activation="tanh", n_samples=4, noise_std=0.1)
    c, _ = plan_model(context, H, cem_policy_prior=pp, **BIG)
    d, _ = plan_model(context, H, cem_policy_prior=pp, **BIG)
    for model in (c, d):
        model.set_policy(_layers())
    r1, r2 = plan_act(c, prob, context, mean, var), plan_act(c, prob, context, mean, var)
    s1 = plan_act(d, prob, context, mean, var)
    od = d.imagine(prob["obs"], *hist, horizon=2, branches=2, numpy=True)
    s2 = plan_act(d, prob, context, mean, var)
    _same(s1, r1, "opt-in: the first plan")
    _same(s2, r2, "opt-in: the plan behind an imagine")
    assert not np.array_equal(r1, r2) and od["valid"].all() and d._call == 2 and d._imagine_call == 1


# ---------------------------------------------------------------------------------------------------------------------- 7: the learned reward
def test_learned_reward(gpu):
    """With `cem_reward_net` and a registered net: rew_net is `model.reward_net(obs, act, next_obs)` on the same transitions, bit for bit,
    and rew = rew_env + weight * rew_net as one float32 multiply and one float32 add; rew_env is what the model without the net gives."""
    weight = 0.37
    rn = dict(inputs="obs_act_next_obs", hidden_sizes=(24, 8), activation="tanh", weight=weight)
    model, prob = plan_model(False, 4, cem_reward_net=rn, **BIG)
    plain, _ = plan_model(False, 4, **BIG)
    K = rref.input_dims("obs_act_next_obs", 18, 6)
    model.set_reward_net(rref.he_net(K, (24, 8), seed=3))
    actions = np.random.default_rng(1).uniform(-1, 1, (2, 3, 3, 6)).astype(F)
    out = model.imagine(prob["obs"], horizon=3, branches=3, actions=actions, numpy=True)
    base = plain.imagine(prob["obs"], horizon=3, branches=3, actions=actions, numpy=True)
    assert "rew_net" not in base and out["valid"].all()
    _same(out["rew_env"], base["rew"], "rew_env is the rollout's own reward")
    _same(out["rew_net"], model.reward_net(out["obs"], out["act"], out["next_obs"]).astype(F), "rew_net is reward_net of the transitions")
    prod = F(weight) * out["rew_net"]
    assert prod.dtype == F
    _same(out["rew"], out["rew_env"] + prod, "rew = rew_env + weight * rew_net, one multiply and one add")
    assert np.abs(out["rew_net"]).min() > 0
    # under constraints (a bound half of the rows cross within two steps): the net's term is 0 where the transition is not valid
    hi = float(np.median(out["states"][1:3, :, :, 0].max(axis=0)))
    cons_model, _ = plan_model(False, 4, cem_reward_net=rn, cem_constraints=[dict(dim=0, hi=hi)], cem_constraint_weight=1.0, **BIG)
    cons_model.set_reward_net(rref.he_net(K, (24, 8), seed=3))
    cut = cons_model.imagine(prob["obs"], horizon=3, branches=3, actions=actions, numpy=True)
    dead = cut["valid"] == 0
    assert dead.any() and cut["done"].any() and (cut["rew_net"][dead] == 0).all() and (cut["rew"][dead] == 0).all()
    _same(cut["rew_net"][~dead], out["rew_net"][~dead], "the valid transitions keep their term")
    # a declared net that is not registered adds nothing
    model.clear_reward_net()
    bare = model.imagine(prob["obs"], horizon=3, branches=3, actions=actions, seed=model.seed, numpy=True)
    assert "rew_net" not in bare


# ---------------------------------------------------------------------------------------------------------------------- 8: the class route
def test_class_route_shapes_and_refusals(gpu, monkeypatch):
    from cadm_amd.dynamics.mlp_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as VanillaModel
    from cadm_amd.envs import make_env_spec
    ip = dict(hidden_sizes=(16,), activation="tanh")
    model, prob = plan_model(True, 4, imagine_policy=ip, **BIG)
    D, A, m, k, n = 18, 6, 2, 3, 2
    hist = (prob["cp_obs"], prob["cp_act"])
    with pytest.raises(RuntimeError, match="no policy net"):
        model.policy_action(np.zeros((3, D), F))
    with pytest.raises(ValueError, match="neither a registered policy"):
        model.imagine(prob["obs"], *hist)
    model.set_policy(_layers())
    assert_close(model.policy_action(np.asarray(prob["obs"], F)), pref.action64(np.asarray(prob["obs"], F), _layers(), "tanh"), what="policy_action")
    out = model.imagine(prob["obs"], *hist, horizon=k, branches=n, noise_std=0.1, disagreement_w="delta_std")
    shapes = dict(states=((k + 1, m, n, D), torch.float32), obs=((k, m, n, D), torch.float32), next_obs=((k, m, n, D), torch.float32),
                  act=((k, m, n, A), torch.float32), rew=((k, m, n), torch.float32), done=((k, m, n), torch.uint8), valid=((k, m, n), torch.uint8),
                  member=((k, m, n), torch.int32), disagreement=((k, m, n), torch.float32), length=((m, n), torch.int32), n_valid=((), torch.int64))
    assert set(out) == set(shapes)
    for key, (shape, dtype) in shapes.items():
        assert isinstance(out[key], torch.Tensor) and out[key].device.type == "cuda" and tuple(out[key].shape) == shape and out[key].dtype == dtype, key
    assert out["obs"].data_ptr() == out["states"].data_ptr() and out["next_obs"].data_ptr() == out["states"][1:].data_ptr()
    assert int(out["n_valid"]) == k * m * n
    flat = out["obs"][out["valid"].bool()]
    assert tuple(flat.shape) == (k * m * n, D)
    # delta_std weights: 1 / (sigma_delta + 1e-10)^2 of the model's statistics, the same chain
    sd = np.asarray(model._stats12()[5], np.float64).reshape(-1) + 1e-10
    model._imagine_call = 0
    same = model.imagine(prob["obs"], *hist, horizon=k, branches=n, noise_std=0.1, disagreement_w=(1.0 / (sd * sd)).astype(F), numpy=True)
    _same(same["disagreement"], _np(out["disagreement"]), "delta_std")
    model._imagine_call = 0
    unit = model.imagine(prob["obs"], *hist, horizon=k, branches=n, noise_std=0.1, numpy=True)
    assert not np.array_equal(unit["disagreement"], same["disagreement"])
    _same(unit["states"], same["states"], "the weights change the disagreement only")
    assert isinstance(unit["n_valid"], int) and all(isinstance(v, np.ndarray) for key, v in unit.items() if key != "n_valid")
    assert unit["done"].dtype == np.uint8 and unit["member"].dtype == np.int32 and unit["length"].dtype == np.int32
    # tensors in, and the clear
    acts = torch.zeros((m, n, k, A), device="cuda")
    with pytest.raises(ValueError, match="one source of actions"):
        model.imagine(prob["obs"], *hist, horizon=k, branches=n, actions=acts)
    model.clear_policy()
    given = model.imagine(torch.as_tensor(np.asarray(prob["obs"], F)).cuda(), *hist, horizon=k, branches=n, actions=acts, numpy=True)
    assert (given["act"] == 0).all() and given["valid"].all()
    calls = model._imagine_call
    # the refusals, before any launch: no counter moves
    for kw_, match in ((dict(horizon=0), "horizon must be"), (dict(branches=0), "branches must be"), (dict(horizon=k, branches=n), "neither a registered"),
                       (dict(horizon=k, branches=n, actions=acts[:, :1]), "actions"), (dict(horizon=k, branches=n, actions=acts, noise_std=0.1), "noise_std"),
                       (dict(horizon=hplanner.IMAGINE_MAX_STEPS + 1, actions=acts), "iteration words"),
                       (dict(branches=1 << 24, actions=acts), "more than one rollout launch")):
        with pytest.raises(ValueError, match=match):
            model.imagine(prob["obs"], *hist, **kw_)
    with pytest.raises(ValueError, match=r"obs \(2, 17\)"):
        model.imagine(np.zeros((2, 17), F), *hist, horizon=k, branches=n, actions=acts)
    poison = np.asarray(prob["obs"], F).copy()
    poison[1, 3] = NAN
    with pytest.raises(ValueError, match="non-finite"):
        model.imagine(poison, *hist, horizon=k, branches=n, actions=acts)
    with pytest.raises(ValueError, match="cp_obs and cp_act are required"):
        model.imagine(prob["obs"], horizon=k, branches=n, actions=acts)
    with pytest.raises(ValueError, match="cp_obs"):
        model.imagine(prob["obs"], prob["cp_obs"][:, :-1], prob["cp_act"], horizon=k, branches=n, actions=acts)
    import torch.distributed as dist
    with monkeypatch.context() as mp:
        mp.setattr(dist, "get_world_size", lambda group=None: 2)
        mp.setattr(model, "_group", object())
        with pytest.raises(NotImplementedError, match="more than one rank"):
            model.imagine(prob["obs"], *hist, horizon=k, branches=n, actions=acts)
    assert model._imagine_call == calls and model._call == 0
    # a discrete action space; imagine_policy next to a planner-declared actor; a model without any declaration
    disc = VanillaModel("dyn", make_env_spec("cartpole"), hidden_sizes=(200,) * 4, n_forwards=4, n_candidates=64, n_particles=5)
    with pytest.raises(NotImplementedError, match="discrete"):
        disc.imagine(np.zeros((2, disc.obs_space_dims), F), horizon=2, actions=np.zeros((2, 1, 2, 1), F))
    with pytest.raises(NotImplementedError, match="discrete"):
        VanillaModel("dyn", make_env_spec("cartpole"), hidden_sizes=(200,) * 4, n_forwards=4, n_candidates=64, n_particles=5, imagine_policy=ip)
    with pytest.raises(ValueError, match="planner-declared actor"):
        plan_model(False, 4, imagine_policy=ip, cem_policy_prior=dict(hidden_sizes=(16,), n_samples=4), **BIG)
    with pytest.raises(ValueError, match="imagine_policy must be"):
        plan_model(False, 4, imagine_policy=(16,), **BIG)
    none, _ = plan_model(False, 4, **BIG)
    with pytest.raises(ValueError, match="no imagine_policy"):
        none.set_policy(_layers())
    # the vanilla class inherits the call: no history
    v, vp = plan_model(False, 4, imagine_policy=ip, **BIG)
    v.set_policy(vref_sequential(_layers(), "tanh"))
    vo = v.imagine(vp["obs"], horizon=2, branches=2, numpy=True)
    assert vo["states"].shape == (3, 2, 2, D) and vo["valid"].all()
    with pytest.raises(ValueError, match="no context encoder"):
        v.imagine(vp["obs"], *hist, horizon=2)


def vref_sequential(layers, act):
    import value_ref as vref
    return vref.sequential(layers, act)


def test_c_entries_refuse_bad_arguments(engines):
    """`cadm_imagine` and `cadm_imagine_select` refuse with CADM_EINVAL (no actor: CADM_ESTATE) and a message that names them, before any
    HIP call: the dummy buffer next to the bad argument is never touched."""
    prob, eng = engines("c-p20-h4")
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=eng.device)
    P = ct.c_void_p(buf.data_ptr())

    def run(c=ctx, obs=P, cv=P, acts=P, m=2, n=2, k=2, noise=0.0, cons=None, dis=None, ws=P):
        return lib.cadm_imagine(c, obs, cv, acts, m, n, k, noise, cons, dis, 0, 0, ws, None)

    def refused(rc, name, frag, code=-1):
        msg = lib.cadm_last_error().decode()
        assert rc == code, "%s: expected %d, got %d (%s)" % (name, code, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg
    who = "cadm_imagine"
    refused(run(obs=None), who, "null")
    refused(run(ws=None), who, "null")
    for kw in (dict(m=0), dict(n=0), dict(k=0), dict(k=-3)):
        refused(run(**kw), who, "must be >= 1")
    refused(run(k=(_lib.POLICY_IT - _lib.IMAGINE_IT) // 2 + 1), who, "iteration words")
    refused(run(n=1 << 24), who, "more than one rollout launch")
    refused(run(cv=None), who, "ctx_vec")
    for v in (NAN, math.inf, -0.5):
        refused(run(noise=v), who, "noise_std")
    refused(run(acts=None), who, "neither actions nor a registered policy", code=-4)
    cons = HipEngine.constraint_params([dict(dim=0, hi=1.0)], "penalty", 0.0)
    cons.dim[0] = eng.D
    refused(run(cons=ct.byref(cons)), who, "constraint 0 reads dim")
    dis = HipEngine.uncertainty_params("epistemic", 1.0, None)
    dis.w[0] = -1.0
    refused(run(dis=ct.byref(dis)), who, "uncertainty weight")
    assert lib.cadm_imagine_workspace_bytes(ctx, 0, 2, 2, None) == 0 and lib.cadm_imagine_workspace_bytes(None, 2, 2, 2, None) == 0
    a256 = lambda x: (x + 255) // 256 * 256
    m, n, k, R = 2, 3, 4, 6
    off = (ct.c_uint64 * _lib.IMAGINE_VIEWS)()
    total = lib.cadm_imagine_workspace_bytes(ctx, m, n, k, off)
    sizes = [4 * (k + 1) * R * eng.D, 4 * k * R * eng.A, 4 * k * R, k * R, k * R, 4 * k * R, 4 * k * R, 4 * R, R, 4 * R * eng.p] + [4 * R * eng.p * eng.D] * 2
    assert list(off) == [int(v) for v in np.cumsum([0] + [a256(s) for s in sizes[:8]])] and total == sum(a256(s) for s in sizes)
    sel = lambda c=ctx, nxt=P, rows=4, t=0, bc=None: lib.cadm_imagine_select(c, nxt, P, P, None, rows, t, None, None, 0, 0, P, P, P, P, P, P, P, None, bc, None)
    refused(sel(nxt=None), "cadm_imagine_select", "null")
    refused(sel(rows=0), "cadm_imagine_select", "rows must be")
    refused(sel(t=-1), "cadm_imagine_select", "rows must be")
    refused(sel(bc=P), "cadm_imagine_select", "aliases")
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=2, H=4, seed=1)
    deng = make_engine(dprob, p=5)
    refused(run(c=deng._ctx), who, "continuous-action")
    refused(sel(c=deng._ctx), "cadm_imagine_select", "continuous-action")
    deng.close()
    seng = make_engine(prob, p=5)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(seng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    refused(run(c=seng._ctx), who, "sharded")
    assert lib.cadm_dist_destroy(seng._ctx) == 0
    seng.close()
    ieng = make_engine(prob, p=5, num_cem_iters=_lib.IMAGINE_IT + 1)
    refused(run(c=ieng._ctx), who, "iteration words")
    ieng.close()
    assert (_np(buf) == 0).all()
    with pytest.raises(ValueError, match="imagine: obs"):
        eng.imagine(np.zeros((2, eng.D + 1), F), None, 2, 2)
    with pytest.raises(ValueError, match="imagine: actions"):
        eng.imagine(np.zeros((2, eng.D), F), None, 2, 2, np.zeros((2, 2, 3, eng.A), F))
    with pytest.raises(ValueError, match="imagine_select: next"):
        eng.imagine_select(np.zeros((4, eng.p, eng.D + 1), F), np.zeros((4, eng.p), F), np.zeros((4, eng.D), F), np.ones(4, np.uint8))
