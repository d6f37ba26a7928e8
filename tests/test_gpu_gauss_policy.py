"""GPU: the stochastic actor head -- `cadm_policy_sample` (csrc/policy_gauss.hip) against the float64 restatement
(tests/gauss_policy_ref.py) under bars derived from the reference's own values, its mode against `cadm_policy_eval` bit for bit, its
determinism and its Philox keys, a poisoned row, `cadm_imagine_sampled` against the pieces it is made of, the planner left untouched,
and the head's lifecycle and refusals.

Geometries, the smallest at which the kernel can go wrong: A = 1 (pendulum: half of a Box-Muller pair is used), A = 6 (halfcheetah:
two Philox groups, the second half empty), A = 24 (the widest declarable env, the widest tests/test_gpu_policy_envelope.py declares);
the linear policy (L = 0: both output layers read the input tile) and L = 2 with widths (33, 70), no multiples of 4 or 64; every hidden
activation, both squashes, both log-std bounds; 37 rows (two full 16-row tiles and a tail of 5) at Philox rows that end at 2^32 - 1.
The log-std layer is scaled on the reference so that the raw log-std leaves (lo, hi) on either side and mostly lies inside."""
import ctypes as ct

import numpy as np
import pytest
import torch

import gauss_policy_ref as gref
import imagine_ref as iref
import policy_ref as pref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import _np, corner_spec, make_engine, plan_act, plan_model

pytestmark = pytest.mark.gpu

F = np.float32
LO, HI = -3.0, 0.5
NETS = [(), (33, 70)]
BIG = dict(hidden=(200,) * 4)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %r %s against %r %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype == np.float32:
        got, want = _bits(got), _bits(want)
    np.testing.assert_array_equal(got, want, err_msg=what)


def _out(o):
    return {k: _np(v) for k, v in o.items()}


@pytest.fixture(scope="module")
def engines(gpu):
    """name -> engine, built when first asked for; kernel level, never rolled out: "pend" (D = 3, A = 1), "hc" (D = 18, A = 6), "wide"
    (D = 48, A = 24), "hc-bounds" (halfcheetah with the action bounds [-0.5, 2])"""
    built = {}

    def get(name):
        if name not in built:
            env = {"pend": "pendulum", "hc": "halfcheetah", "hc-bounds": "halfcheetah", "wide": corner_spec("widest")}[name]
            prob = synth.make_problem(env=env, context=name == "wide", E=5, m=2, H=3, seed=52)
            kw = dict(lower_bound=-0.5, upper_bound=2.0) if name == "hc-bounds" else {}
            built[name] = make_engine(prob, p=5, **kw)
        return built[name]
    yield get
    for eng in built.values():
        assert not eng._rollout_ready, "a kernel-level engine was rolled out"
        eng.close()


def _head(bound="clamp", lo=LO, hi=HI):
    return hplanner.policy_head_params(dict(kind="gaussian", log_std_bounds=(lo, hi), log_std_bound=bound), has_actor=True)


def _states(D, rows, seed):
    return np.random.default_rng(2000 + seed).standard_normal((rows, D)).astype(F)


def _set(eng, hidden, act, squash, bound, x, seed=0, mean=None, std=None, lo=LO, hi=HI):
    """register a SAC actor D -> hidden -> 2 A on the engine, as `set_policy` does: the mean columns, then the head; returns its layers"""
    layers = gref.actor(eng.D, hidden, eng.A, act, x, lo, hi, seed=seed, mean=mean, std=std)
    mean_layers, W_ls, b_ls = gref.split(layers, eng.A)
    eng.set_policy_net(HipEngine.policy_params(hidden, act, squash, 1, 0.0), mean_layers, obs_mean=mean, obs_std=std)
    eng.set_policy_head(_head(bound, lo, hi), W_ls, b_ls)
    return layers


# ---------------------------------------------------------------------------------------------------------------------- 1: the mode
@pytest.mark.parametrize("hidden,act", [((33, 70), "swish"), ((), "relu")], ids=["33x70-swish", "linear"])
def test_mode_is_policy_eval(engines, hidden, act):
    """`mode` has `policy_eval`'s bits at R = 1, 17 and 165 and inside a launch large enough for two row tiles per workgroup -- and
    there act and logp have the bits of the small launch too: nothing depends on the row tiles or on where a row sits."""
    eng = engines("hc")
    x = _states(eng.D, 165, 7)
    _set(eng, hidden, act, "tanh", "clamp", x, seed=21)
    full = _np(eng.policy_eval(x))
    small = _out(eng.policy_sample(x, seed=3, call=4, t=1))
    _same(small["mode"], full, "R = 165")
    for R in (1, 17):
        _same(_np(eng.policy_sample(x[:R], seed=3, call=4, t=1)["mode"]), full[:R], "R = %d" % R)
    reps = 2 * 16 * 256 // 165 + 8
    big_x = np.concatenate([x] * reps, axis=0)
    assert big_x.shape[0] > 2 * 16 * 256
    big = _out(eng.policy_sample(big_x, seed=3, call=4, t=1))
    _same(big["mode"], _np(eng.policy_eval(big_x)), "the two-row-tile launch against policy_eval's")
    _same(big["mode"][-165:], full, "the two-row-tile launch, tail")
    for key in ("act", "logp", "mode"):
        _same(big[key][:165], small[key], "two row tiles against one: %s" % key)
    last = (reps - 1) * 165
    again = _out(eng.policy_sample(x, row0=last, seed=3, call=4, t=1))
    for key in ("act", "logp"):
        _same(big[key][last:], again[key], "the same Philox rows at another position: %s" % key)


# ---------------------------------------------------------------------------------------------------------------------- 2: the values
@pytest.mark.parametrize("bound", gref.BOUNDS)
@pytest.mark.parametrize("squash", pref.SQUASH)
def test_values_against_restatement(engines, squash, bound):
    """act and logp against the float64 restatement under `gref.bars` (their derivation stands there), on the draws of oracle/philox.py
    at Philox rows 2^32 - 37 .. 2^32 - 1 of step 2; the raw log-std of every case leaves (lo, hi) on both sides and mostly lies inside."""
    R, row0, t, seed, call = 37, 2 ** 32 - 37, 2, 11, 5
    worst_a = worst_l = 0.0
    for name in ("pend", "hc", "wide", "hc-bounds"):
        eng = engines(name)
        lb, ub = (-0.5, 2.0) if name == "hc-bounds" else (-1.0, 1.0)
        x = _states(eng.D, R, eng.A)
        e = gref.xi(seed, call, row0 + np.arange(R), t, eng.A)
        r = gref.xi_radius(seed, call, row0 + np.arange(R), t, eng.A)
        for hidden in NETS:
            for act in pref.ACTS if name != "hc-bounds" else ("tanh",):
                what = "%s A=%d %r %s %s %s" % (name, eng.A, hidden, act, squash, bound)
                layers = _set(eng, hidden, act, squash, bound, x, seed=len(hidden))
                zr = gref.z64(x, layers, act)
                below, above, inside = gref.shares(zr[:, eng.A:], LO, HI)
                assert below >= 0.1 and above >= 0.1 and inside >= 0.5, "%s: shares %r" % (what, (below, above, inside))
                ref = gref.sample64(zr, e, squash, bound, LO, HI, lb, ub)
                act_bar, logp_bar = gref.bars(zr, ref, e, r, squash, bound, LO, HI, lb, ub)
                got = _out(eng.policy_sample(x, row0=row0, t=t, seed=seed, call=call))
                assert got["act"].shape == (R, eng.A) and got["logp"].shape == (R,) and np.isfinite(got["logp"]).all(), what
                assert got["act"].min() >= F(lb) and got["act"].max() <= F(ub), what
                ra = float((np.abs(got["act"].astype(np.float64) - ref["act"]) / act_bar).max())
                rl = float((np.abs(got["logp"].astype(np.float64) - ref["logp"]) / logp_bar).max())
                worst_a, worst_l = max(worst_a, ra), max(worst_l, rl)
                print("\n[%s] |act err| / bar %.3f, |logp err| / bar %.3f" % (what, ra, rl))
                assert ra <= 1.0, what
                assert rl <= 1.0, what
                assert np.abs(got["mode"].astype(np.float64) - ref["mode"]).max() <= 1e-5 * (ub - lb), what
    print("\n[%s %s] worst |act err| / bar %.3f, worst |logp err| / bar %.3f" % (squash, bound, worst_a, worst_l))


def test_values_with_statistics(engines):
    """obs_mean / obs_std that are not 0 / 1 reach both output layers"""
    eng = engines("hc")
    R, seed, call = 37, 2, 3
    rng = np.random.default_rng(8)
    x = _states(eng.D, R, 3)
    mean, std = rng.standard_normal(eng.D).astype(F), rng.uniform(0.3, 4.0, eng.D).astype(F)
    layers = _set(eng, (33, 70), "swish", "tanh", "tanh", x, seed=5, mean=mean, std=std)
    zr = gref.z64(x, layers, "swish", mean, std)
    assert np.abs(zr - gref.z64(x, layers, "swish")).max() > 1e-3, "the statistics must matter"
    e, r = gref.xi(seed, call, np.arange(R), 0, eng.A), gref.xi_radius(seed, call, np.arange(R), 0, eng.A)
    ref = gref.sample64(zr, e, "tanh", "tanh", LO, HI)
    act_bar, logp_bar = gref.bars(zr, ref, e, r, "tanh", "tanh", LO, HI)
    got = _out(eng.policy_sample(x, seed=seed, call=call))
    assert (np.abs(got["act"].astype(np.float64) - ref["act"]) <= act_bar).all()
    assert (np.abs(got["logp"].astype(np.float64) - ref["logp"]) <= logp_bar).all()


# ---------------------------------------------------------------------------------------------------------------------- 3: determinism, keys
def test_determinism_and_keys(engines):
    eng = engines("hc")
    R = 37
    x = _states(eng.D, R, 9)
    layers = _set(eng, (33, 70), "relu", "none", "clamp", x, seed=2)
    base = _out(eng.policy_sample(x, seed=6, call=7, t=1))
    again = _out(eng.policy_sample(x, seed=6, call=7, t=1))
    for key in base:
        _same(again[key], base[key], "run to run: %s" % key)
    tail = _out(eng.policy_sample(x[5:], row0=5, seed=6, call=7, t=1))
    for key in base:
        _same(tail[key], base[key][5:], "policy_sample(x[5:], row0=5): %s" % key)
    lead = eng.policy_sample(x[:36].reshape(4, 9, eng.D), seed=6, call=7, t=1)
    assert tuple(lead["act"].shape) == (4, 9, eng.A) and tuple(lead["logp"].shape) == (4, 9)
    _same(_np(lead["logp"]).reshape(-1), base["logp"][:36], "leading dims are flattened")
    for kw in (dict(seed=7, call=7, t=1), dict(seed=6, call=8, t=1), dict(seed=6, call=7, t=2)):
        other = _out(eng.policy_sample(x, **kw))
        assert not np.array_equal(other["act"], base["act"]) and not np.array_equal(other["logp"], base["logp"]), kw
        _same(other["mode"], base["mode"], "the mode draws nothing")
    # without a squash u = act wherever the clip does not bind: the draw itself, recovered from the reference's mu and sigma
    zr = gref.z64(x, layers, "relu")
    sig = np.exp(np.clip(zr[:, eng.A:], LO, HI))
    free = (np.abs(base["act"]) < 1.0) & (sig > 0.2)
    assert free.mean() > 0.2
    rec = (base["act"].astype(np.float64) - zr[:, :eng.A]) / sig
    assert np.abs(rec - gref.xi(6, 7, np.arange(R), 1, eng.A))[free].max() < 1e-3, "the draws are word 8's"
    assert np.abs(rec - iref.xi(6, 7, R, 1, eng.A))[free].mean() > 0.3, "the draws must not be imagine's action noise (word 7) under the same key"


# ---------------------------------------------------------------------------------------------------------------------- 4: poison
@pytest.mark.parametrize("name", ["pend", "hc"])
def test_a_poisoned_row(engines, name):
    eng = engines(name)
    R = 37
    x = _states(eng.D, R, 4)
    _set(eng, (33, 70), "tanh", "tanh", "tanh", x, seed=3)
    clean = _out(eng.policy_sample(x, seed=1, call=2))
    bad = x.copy()
    bad[3, 0], bad[20, eng.D - 1], bad[36, 0] = np.nan, np.inf, -np.inf
    got = _out(eng.policy_sample(bad, seed=1, call=2))
    hit = np.zeros(R, bool)
    hit[[3, 20, 36]] = True
    assert np.isnan(got["logp"][hit]).all() and np.isfinite(got["logp"][~hit]).all()
    assert (got["act"][hit] == pref.fallback(-1.0, 1.0)).all() and (got["mode"][hit] == pref.fallback(-1.0, 1.0)).all()
    for key in clean:
        _same(got[key][~hit], clean[key][~hit], "the neighbours of a poisoned row: %s" % key)
    _same(got["mode"], _np(eng.policy_eval(bad)), "mode is policy_eval's, fallback included")


# ---------------------------------------------------------------------------------------------------------------------- 5: imagine
IP = dict(hidden_sizes=(16,), activation="tanh")
HEAD = dict(kind="gaussian", log_std_bounds=(LO, HI), log_std_bound="tanh")


def _sac(seed=17):
    x = _states(18, 64, 1)
    return gref.actor(18, (16,), 6, "tanh", x, LO, HI, seed=seed)


def test_imagine_sampled(gpu):
    """m = 5, branches = 3, horizon = 3: `imagine(sample=False)` of a model with a head is the imagine of a model without one that was
    given the sliced net; on the sampled route act[t] and logp[t] are `policy_sample(states[t], t=t)` under the call's key and every
    other output is `imagine` under those actions, with and without a constraint that ends rows; the class route is the engine's."""
    m, n, k = 5, 3, 3
    model, prob = plan_model(False, 4, m=m, imagine_policy=IP, policy_head=HEAD, **BIG)
    plain, _ = plan_model(False, 4, m=m, imagine_policy=IP, **BIG)
    assert model._opt is None, "policy_head must not switch the planner"
    layers = _sac()
    with pytest.raises(ValueError, match="2 A = 12"):
        model.set_policy(gref.split(layers, 6)[0])
    with pytest.raises(RuntimeError, match="set_policy"):
        model.policy_sample(prob["obs"])
    model.set_policy(layers)
    plain.set_policy(gref.split(layers, 6)[0])
    obs = np.asarray(prob["obs"], F)
    assert obs.shape == (m, 18)
    # sample=False: today's route
    a = model.imagine(obs, horizon=k, branches=n, noise_std=0.3, sample=False, numpy=True)
    b = plain.imagine(obs, horizon=k, branches=n, noise_std=0.3, numpy=True)
    assert "logp" not in a and sorted(a) == sorted(b)
    for key in b:
        _same(np.asarray(a[key]), np.asarray(b[key]), "sample=False against a model without a head: %s" % key)
    with pytest.raises(ValueError, match="needs a registered Gaussian head"):
        plain.imagine(obs, sample=True)
    # the class route: sampled by default, keyed (seed, the counter)
    eng, seed, call = model.engine, model.seed, model._imagine_call
    o = model.imagine(obs, horizon=k, branches=n, numpy=True)
    assert model._imagine_call == call + 1 and model._call == 0
    assert o["logp"].shape == (k, m, n) and o["logp"].dtype == F and np.isfinite(o["logp"]).all()
    free = _out(eng.imagine(obs, None, k, n, None, 0.0, None, None, seed, call, sample=True))
    for key in ("states", "act", "rew", "done", "valid", "member", "disagreement", "length", "logp"):
        _same(np.asarray(o[key]), free[key], "the class route is the engine's under (seed, call): %s" % key)
    # a constraint that ends some rows: its bound is the median over the rows of the peak of dim 0
    peak = free["states"][1:, :, :, 0].max(axis=0)
    hi = float(np.sort(peak.reshape(-1))[peak.size // 2])
    cons = HipEngine.constraint_params([dict(dim=0, hi=hi)], "terminate", 1.0)
    ended = _out(eng.imagine(obs, None, k, n, None, 0.0, cons, None, seed, call, sample=True))
    assert 0 < ended["done"].sum() < m * n and (ended["valid"] == 0).any(), "at least one row must terminate"
    for out, c in ((free, None), (ended, cons)):
        for t in range(k):
            s = _out(eng.policy_sample(out["states"][t].reshape(-1, 18), t=t, seed=seed, call=call))
            _same(out["act"][t].reshape(-1, 6), s["act"], "act[%d] is policy_sample(states[%d])" % (t, t))
            _same(out["logp"][t].reshape(-1), s["logp"], "logp[%d] is policy_sample(states[%d])" % (t, t))
        given = _out(eng.imagine(obs, None, k, n, np.ascontiguousarray(np.transpose(out["act"], (1, 2, 0, 3))), 0.0, c, None, seed, call))
        assert set(out) == set(given) | {"logp"}
        for key in given:
            _same(out[key], given[key], "sampled imagine against imagine under its actions: %s" % key)
    # policy_sample on the class: its own counter, the engine's call
    ps = model.policy_sample(obs, seed=3)
    assert model._sample_call == 1 and model._imagine_call == call + 1 and model._call == 0
    want = _out(eng.policy_sample(obs, seed=3, call=0))
    for key in want:
        _same(ps[key], want[key], "model.policy_sample: %s" % key)
    _same(ps["mode"], model.policy_action(obs), "mode is policy_action")
    assert not np.array_equal(model.policy_sample(obs, seed=3)["act"], ps["act"]), "the counter moved"
    # lifecycle on the class: a new net works, clear_policy drops both
    model.set_policy(_sac(seed=18))
    assert not np.array_equal(model.policy_sample(obs, seed=3, numpy=True)["mode"], ps["mode"])
    model.clear_policy()
    with pytest.raises(RuntimeError, match="set_policy"):
        model.policy_sample(obs)
    with pytest.raises(_lib.CadmError, match="cadm_set_policy_net"):
        eng.policy_sample(obs)


# ---------------------------------------------------------------------------------------------------------------------- 6: the planner
def test_planner_is_untouched(gpu):
    """get_action of a model with `cem_policy_prior` over three calls: a declared and registered head changes no bit against the same
    model without `policy_head` and with the hand-sliced net."""
    pp = dict(hidden_sizes=(16,), activation="tanh", n_samples=4, noise_std=0.1)
    a, prob = plan_model(False, 4, cem_policy_prior=pp, policy_head=HEAD, **BIG)
    b, _ = plan_model(False, 4, cem_policy_prior=pp, **BIG)
    layers = _sac()
    a.set_policy(layers)
    b.set_policy(gref.split(layers, 6)[0])
    mean, var = prob["init_mean"], prob["init_var"]
    plans = []
    for i in range(3):
        pa, pb = plan_act(a, prob, False, mean, var), plan_act(b, prob, False, mean, var)
        _same(pa, pb, "get_action %d with a head against the sliced net" % i)
        plans.append(pa)
    assert not np.array_equal(plans[0], plans[1]) and a._call == b._call == 3
    _same(a.policy_action(prob["obs"]), b.policy_action(prob["obs"]), "policy_action is the mode")
    _same(a.policy_proposals(prob["obs"]), b.policy_proposals(prob["obs"]), "the proposals keep noise_std around the mode")


# ---------------------------------------------------------------------------------------------------------------------- 7: lifecycle, refusals
def test_lifecycle_and_refusals(engines):
    eng = engines("hc")
    lib, ctx = eng.lib, eng._ctx
    x = _states(eng.D, 8, 0)
    eng.set_policy_net(None)
    with pytest.raises(_lib.CadmError, match="cadm_set_policy_net"):
        eng.policy_sample(x)
    W, b = np.zeros((33, eng.A), F), np.zeros((eng.A,), F)
    with pytest.raises(_lib.CadmError, match="cadm_set_policy_net"):
        eng.set_policy_head(_head(), W, b)                    # a head hangs on a registered net
    layers = _set(eng, (50, 33), "relu", "tanh", "clamp", x, seed=1)
    first = _out(eng.policy_sample(x))
    mean_layers, W_ls, b_ls = gref.split(layers, eng.A)
    eng.set_policy_net(HipEngine.policy_params((50, 33), "relu", "tanh", 1, 0.0), mean_layers)      # a bare set_policy_net drops the head
    with pytest.raises(_lib.CadmError, match="cadm_set_policy_head"):
        eng.policy_sample(x)
    obs = torch.zeros((2, eng.D), dtype=torch.float32, device=eng.device)
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=eng.device)
    P = ct.c_void_p(buf.data_ptr())
    rc = lib.cadm_imagine_sampled(ctx, ct.c_void_p(obs.data_ptr()), None, 2, 2, 2, None, None, 0, 0, P, None)
    assert rc == -4 and "cadm_set_policy_head" in lib.cadm_last_error().decode()
    eng.set_policy_head(_head(), W_ls, b_ls)
    for key, v in _out(eng.policy_sample(x)).items():
        _same(v, first[key], "the head set again: %s" % key)
    eng.set_policy_head(None)                                  # the head alone is cleared; the net stays
    with pytest.raises(_lib.CadmError, match="cadm_set_policy_head"):
        eng.policy_sample(x)
    _same(_np(eng.policy_eval(x)), first["mode"], "the net without its head")
    # a new net with another last hidden width, and its head
    _set(eng, (70,), "swish", "none", "tanh", x, seed=2)
    assert np.isfinite(_np(eng.policy_sample(x)["logp"])).all()
    # wrong shapes
    with pytest.raises(ValueError, match="expected"):
        eng.set_policy_head(_head(), np.zeros((70, eng.A + 1), F), b)
    with pytest.raises(ValueError, match="expected"):
        eng.set_policy_head(_head(), np.zeros((70, eng.A), F), np.zeros((eng.A + 1,), F))
    with pytest.raises(ValueError, match="last layer reads 70"):
        eng.set_policy_head(_head(), np.zeros((33, eng.A), F), b)
    with pytest.raises(ValueError, match="not finite"):
        eng.set_policy_head(_head(), np.full((70, eng.A), np.nan, F), b)
    assert np.isfinite(_np(eng.policy_sample(x)["logp"])).all(), "a refused head leaves the registered one"
    # the C entries, before any HIP call
    def refused(rc, name, frag, code=-1):
        msg = lib.cadm_last_error().decode()
        assert rc == code, "%s: expected %d, got %d (%s)" % (name, code, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg
    prm = _head()
    who = "cadm_set_policy_head"
    refused(lib.cadm_set_policy_head(None, ct.byref(prm), P, P, None), who, "null")
    refused(lib.cadm_set_policy_head(ctx, ct.byref(prm), None, P, None), who, "null")
    refused(lib.cadm_set_policy_head(ctx, ct.byref(prm), P, None, None), who, "null")
    for field, v, frag in (("kind", 0, "unknown head kind"), ("kind", 2, "unknown head kind"), ("bound", 2, "unknown log-std bound"),
                           ("bound", -1, "unknown log-std bound"), ("log_std_max", float("inf"), "log-std bounds"),
                           ("log_std_min", float("nan"), "log-std bounds"), ("log_std_min", 2.0, "log-std bounds"),
                           ("log_std_max", 10.5, "log-std bounds")):
        bad = _head()
        setattr(bad, field, v)
        refused(lib.cadm_set_policy_head(ctx, ct.byref(bad), P, P, None), who, frag)
    who = "cadm_policy_sample"
    run = lambda c=ctx, s=P, R=4, row0=0, t=0, a=P, lp=P: lib.cadm_policy_sample(c, s, R, row0, t, 0, 0, a, lp, None, None)
    for kw in (dict(c=None), dict(s=None), dict(a=None), dict(lp=None)):
        refused(run(**kw), who, "null")
    refused(run(R=0), who, "R must be >= 1")
    refused(run(R=-2), who, "R must be >= 1")
    refused(run(t=-1), who, "t must be >= 0")
    refused(run(R=4, row0=2 ** 32 - 3), who, "beyond the 2^32 rows")
    assert run(R=4, row0=2 ** 32 - 4) == 0
    assert lib.cadm_imagine_sampled_workspace_bytes(ctx, 0, 2, 2, None) == 0 and lib.cadm_imagine_sampled_workspace_bytes(None, 2, 2, 2, None) == 0
    m, n, k = 2, 3, 4
    off, soff = (ct.c_uint64 * _lib.IMAGINE_VIEWS)(), (ct.c_uint64 * _lib.IMAGINE_SAMPLED_VIEWS)()
    plain, sampled = lib.cadm_imagine_workspace_bytes(ctx, m, n, k, off), lib.cadm_imagine_sampled_workspace_bytes(ctx, m, n, k, soff)
    a256 = lambda v: (v + 255) // 256 * 256
    assert list(soff)[:9] == list(off) and soff[9] == off[8] + a256(m * n) and sampled == plain + a256(4 * k * m * n)
    who = "cadm_imagine_sampled"
    O = ct.c_void_p(obs.data_ptr())
    refused(lib.cadm_imagine_sampled(ctx, None, None, 2, 2, 2, None, None, 0, 0, P, None), who, "null")
    refused(lib.cadm_imagine_sampled(ctx, O, None, 2, 2, 2, None, None, 0, 0, None, None), who, "null")
    refused(lib.cadm_imagine_sampled(ctx, O, None, 2, 0, 2, None, None, 0, 0, P, None), who, "must be >= 1")
    eng.set_policy_net(None)
    refused(lib.cadm_imagine_sampled(ctx, O, None, 2, 2, 2, None, None, 0, 0, P, None), who, "cadm_set_policy_net", code=-4)
