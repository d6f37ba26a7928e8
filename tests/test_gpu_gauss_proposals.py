"""GPU: proposals of the policy prior drawn from the actor's Gaussian head (`cadm_set_policy_proposals`, csrc/policy_gauss.hip's roll
flavour) -- the bitwise anchor against the noise route, std_scale = 0, every step's actions against the float64 restatement
(tests/gauss_proposals_ref.py) under the bar derived there, sequence 0 against `cadm_policy_eval`, the next states against a one-step
rollout, determinism and Philox keys, a poisoned particle, the fused loops against the stepwise one, the class route, and the
setting's lifecycle and refusals.

Geometries: pendulum (A = 1: one dim of a Philox group) and halfcheetah (A = 6: the second group is used), both with context, m = 2,
P = 3, H = 4, p = 5; and tests/test_gpu_policy_envelope.py's engine "big" at m = 65, P = 127 -- 8255 rows, more than two 16-row tiles
per CU -- where the roll's steps run the two-row-tile instantiation.  The whole file runs in a few seconds per case."""
import ctypes as ct

import numpy as np
import pytest
import torch

import behind_rollout as br
import critic_ref as cref
import gauss_policy_ref as gref
import gauss_proposals_ref as gp
import policy_ref as pref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import _np, make_engine, plan_act, plan_model, zero_carry

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")
M, N, KE, ITERS = 2, 24, 8, 3
BIG_M, BIG_P = br.POLICY_ROLLS["big"][1][0]
KINDS = {"pend": "pendulum", "hc": "halfcheetah"}
EINVAL, ESTATE = -1, -4


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %r against %r" % (what, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


@pytest.fixture(scope="module")
def engines(gpu):
    """name -> (problem, engine), built when first asked for.  "pend" / "hc": with context, m = 2, H = 4, p = 5; "<name>-h1": the twin
    with n_forwards = 1 and the same weights; "hc-det": halfcheetah's deterministic twin (H = 4); "big": behind_rollout's (vanilla
    halfcheetah, H = 2, p = 5); "loop" / "loop-vanilla": tests/test_gpu_policy.py's planner geometry (m = 2, p = 5, H = 5); 8 elites,
    3 CEM iterations everywhere"""
    built, probs = {}, {}

    def get(name):
        if name not in built:
            base = name.split("-")[0]
            kw = dict(num_elites=KE, num_cem_iters=ITERS)
            if base == "big":
                prob = br.policy_problem("big")
                built[name] = (prob, make_engine(prob, p=5, H=2, **kw))
            elif base == "loop":
                prob = synth.make_problem(env="halfcheetah", context=name == "loop", E=5, m=M, H=5, seed=3, trained_like=True)
                built[name] = (prob, make_engine(prob, p=gp.NP, **kw))
            else:
                if base not in probs:
                    probs[base] = synth.make_problem(env=KINDS[base], context=True, E=5, m=gp.M, H=gp.H, seed=3, trained_like=True)
                built[name] = (probs[base], make_engine(probs[base], p=gp.NP, H=1 if name.endswith("-h1") else gp.H,
                                                        deterministic=name.endswith("-det"), **kw))
        return built[name]
    yield get
    for _, eng in built.values():
        eng.close()


def _head(bound="clamp", lo=gp.LO, hi=gp.HI):
    return hplanner.policy_head_params(dict(kind="gaussian", log_std_bounds=(lo, hi), log_std_bound=bound), has_actor=True)


def _register(eng, layers, hidden, act, squash, bound="clamp", head=True):
    """the SAC actor `layers` (2 A outputs) on the engine as `set_policy` registers it: the mean columns, then the head"""
    mean_layers, W_ls, b_ls = gref.split(layers, eng.A)
    eng.set_policy_net(HipEngine.policy_params(hidden, act, squash, 1, 0.0), mean_layers)
    if head:
        eng.set_policy_head(_head(bound), W_ls, b_ls)
    return mean_layers


def _ctx(eng, prob, m):
    return eng.context_forward(prob["cp_obs"][:m], prob["cp_act"][:m]) if eng.C > 0 else None


def _propose(eng, prob, hidden, act, squash, P, source, scale=1.0, noise=0.0, m=None, seed=gp.SEED, call=gp.CALL, obs=None):
    """one `policy_propose` with states under a source of proposals; the engine is left on the noise route"""
    m = prob["obs"].shape[0] if m is None else m
    obs = np.asarray(prob["obs"], F)[:m] if obs is None else obs
    prm = HipEngine.policy_params(hidden, act, squash, P, noise)
    eng.set_policy_proposals(source, scale)
    try:
        seqs, states = eng.policy_propose(prm, obs, _ctx(eng, prob, m), seed=seed, call=call, want_states=True)
    finally:
        eng.set_policy_proposals("noise", 1.0)
    return _np(seqs), _np(states)


# ---------------------------------------------------------------------------------------------------------------------- 1: the anchor
@pytest.mark.parametrize("name,s", [("pend", 0.3), ("hc", 0.3), ("hc", 0.7), ("big", 0.3)])
def test_zero_log_std_layer_is_the_noise_route(engines, name, s):
    """Squash "none", W_ls = 0, b_ls = 0, lo < 0 < hi: l = 0 exactly, ls = 0, sig = expf(0) = 1, std_scale * sig = std_scale, so the
    head route at std_scale = s is the noise route at noise_std = s -- `seqs` and `states_out` bit for bit, no tolerance.  "big": 8255
    rows, the two-row-tile instantiation of both kernels."""
    prob, eng = engines(name)
    m, P = (BIG_M, BIG_P) if name == "big" else (gp.M, gp.P)
    if name == "big":
        cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
        assert (m * P + 15) // 16 > 2 * cus, "%d rows on %d CUs: one row tile per workgroup" % (m * P, cus)
        prob = br.with_rows(prob, m)
    layers = gp.anchor_layers(eng.D, gp.HIDDEN, eng.A, seed=3)
    _register(eng, layers, gp.HIDDEN, gp.ACT, "none")
    head, hs = _propose(eng, prob, gp.HIDDEN, gp.ACT, "none", P, "head", s)
    noise, ns = _propose(eng, prob, gp.HIDDEN, gp.ACT, "none", P, "noise", noise=s)
    assert head.shape == (m, P, eng.H, eng.A) and np.isfinite(head).all() and np.isfinite(hs).all()
    assert not np.array_equal(head[:, 1], head[:, 0]) and ((head > -1) & (head < 1)).mean() > 0.25, "a clipped action checks nothing"
    _same(head, noise, "seqs")
    _same(hs, ns, "states_out")


# ---------------------------------------------------------------------------------------------------------------------- 2: std_scale = 0
@pytest.mark.parametrize("name", ["pend", "hc", "hc-det"])
def test_std_scale_zero_draws_nothing(engines, name):
    """Squash "tanh", a real head, std_scale = 0: the roll is the noise route's at noise_std = 0, bit for bit, and every sequence has
    sequence 0's action wherever it read sequence 0's state -- at step 0 on every engine, at every step on the deterministic one (on a
    stochastic ctx the rows' particles part after the first one-step rollout: each row draws its own head noise)."""
    prob, eng = engines(name)
    x = np.asarray(prob["obs"], F)
    layers = gref.actor(eng.D, gp.HIDDEN, eng.A, gp.ACT, x, gp.LO, gp.HI, seed=eng.A)
    _register(eng, layers, gp.HIDDEN, gp.ACT, "tanh")
    head, hs = _propose(eng, prob, gp.HIDDEN, gp.ACT, "tanh", gp.P, "head", 0.0)
    noise, ns = _propose(eng, prob, gp.HIDDEN, gp.ACT, "tanh", gp.P, "noise", noise=0.0)
    _same(head, noise, "seqs")
    _same(hs, ns, "states_out")
    steps = slice(None) if name.endswith("-det") else slice(0, 1)
    _same(head[:, :, steps], np.repeat(head[:, :1, steps], gp.P, axis=1), "every sequence is sequence 0")
    loud, _ = _propose(eng, prob, gp.HIDDEN, gp.ACT, "tanh", gp.P, "head", 1.0)
    _same(loud[:, 0, 0], head[:, 0, 0], "sequence 0 draws nothing")
    assert (loud[:, 1:, 0] != head[:, 1:, 0]).all()


# ---------------------------------------------------------------------------------------------------------------------- 3: the values
def _calibrated(eng, prob, squash, seed):
    """a SAC actor whose log-std columns are calibrated (gref.actor) on the state estimates a pilot roll of its own mean columns reads --
    the mean columns do not depend on the calibration -- so that the raw log-std of the states the head route reads leaves (lo, hi) on
    either side and mostly lies inside"""
    raw = pref.he_policy(eng.D, gp.HIDDEN, 2 * eng.A, seed, 0.5)
    _register(eng, raw, gp.HIDDEN, gp.ACT, squash, head=False)
    _, st = _propose(eng, prob, gp.HIDDEN, gp.ACT, squash, gp.P, "noise", noise=0.3)
    est = pref.particle_mean32(st).reshape(-1, eng.D)
    layers = gref.actor(eng.D, gp.HIDDEN, eng.A, gp.ACT, est, gp.LO, gp.HI, seed=seed)
    for (W, b), (W0, b0) in zip(gref.split(layers, eng.A)[0], gref.split(raw, eng.A)[0]):
        assert np.array_equal(W, W0) and np.array_equal(b, b0)
    return layers


@pytest.mark.parametrize("std_scale", [1.0, 0.5])
@pytest.mark.parametrize("bound", gref.BOUNDS)
@pytest.mark.parametrize("squash", pref.SQUASH)
def test_values_against_restatement(engines, squash, bound, std_scale):
    """Every step on its own, so that nothing compounds (tests/test_gpu_policy.py's `check_roll` scheme): the actions against the float64
    restatement on the particle mean of the states that step read, under `gp.bar`; sequence 0 is `policy_eval` of the particle mean,
    bit for bit; the states the next step read are the twin's one-step `rollout_returns` of this step's actions, bit for bit."""
    worst, seed, call = 0.0, gp.SEED, gp.CALL
    for name in ("pend", "hc"):
        prob, eng = engines(name)
        _, twin = engines(name + "-h1")
        m, P, H, A = gp.M, gp.P, eng.H, eng.A
        layers = _calibrated(eng, prob, squash, seed=A)
        _register(eng, layers, gp.HIDDEN, gp.ACT, squash, bound)
        seqs, states = _propose(eng, prob, gp.HIDDEN, gp.ACT, squash, P, "head", std_scale)
        assert seqs.shape == (m, P, H, A) and states.shape == (H, m, P, eng.p, eng.D) and np.isfinite(seqs).all() and np.isfinite(states).all()
        obs = np.asarray(prob["obs"], F)[:m]
        _same(states[0], np.broadcast_to(obs[:, None, None, :], states[0].shape), "step 0 reads obs[mi]")
        raw = []
        for t in range(H):
            what = "%s %s %s x%g step %d" % (name, squash, bound, std_scale, t)
            # (step 0 reads obs[mi] itself: the mean of p copies is not the value bit for bit)
            est = pref.particle_mean32(states[t]) if t else np.ascontiguousarray(np.broadcast_to(obs[:, None, :], (m, P, eng.D)))
            xi, r = gp.draws(seed, call, m, P, t, A, std_scale)
            ref = gp.step64(est, layers, gp.ACT, squash, bound, gp.LO, gp.HI, xi, std_scale)
            raw.append(ref["l"])
            a = seqs[:, :, t]
            ratio = np.abs(a.astype(np.float64) - ref["act"]) / gp.bar(ref, xi, r, squash, bound, gp.LO, gp.HI)
            print("[%s] worst |act - ref| / bar %.3f" % (what, ratio.max()))
            worst = max(worst, float(ratio.max()))
            assert (ratio <= 1.0).all(), "%s: %.3f of the bar" % (what, ratio.max())
            assert a.min() >= -1.0 and a.max() <= 1.0
            _same(a[:, 0], _np(eng.policy_eval(est[:, 0])), what + ": sequence 0 against policy_eval")
            assert (a[:, 1:] != a[:, :1]).any(), what + ": sequences 1 .. P - 1 are draws"
            if t + 1 < H:
                _, nxt = twin.rollout_returns(obs, _ctx(twin, prob, m), np.ascontiguousarray(a[:, :, None, :]), obs_rows=states[t].reshape(-1, eng.D),
                                              seed=seed, call=call, it=hplanner.POLICY_IT + 2 * t, want_traj=True)
                _same(states[t + 1], _np(nxt)[0], what + ": the states the next step read against the one-step rollout")
        below, above, inside = gref.shares(np.stack(raw), gp.LO, gp.HI)
        print("[%s %s %s] log-std shares below / above / inside: %.2f %.2f %.2f" % (name, squash, bound, below, above, inside))
        if name == "hc":      # (24 values on pendulum, 144 here)
            assert below > 0 and above > 0 and inside > 0
    print("[%s %s x%g] worst |act - ref| / bar over both shapes: %.3f" % (squash, bound, std_scale, worst))


# ---------------------------------------------------------------------------------------------------------------------- 4: determinism, keys
@pytest.mark.parametrize("name", ["pend", "hc"])
def test_determinism_and_keys(engines, name):
    """Two runs give the same bits; another call gives other draws (sequence 0's first action, which draws nothing, stays); env 0
    proposed alone has the bits of env 0 of m = 2."""
    prob, eng = engines(name)
    layers = gref.actor(eng.D, gp.HIDDEN, eng.A, gp.ACT, np.asarray(prob["obs"], F), gp.LO, gp.HI, seed=eng.A)
    _register(eng, layers, gp.HIDDEN, gp.ACT, "tanh", "tanh")
    args = (eng, prob, gp.HIDDEN, gp.ACT, "tanh", gp.P, "head", 1.0)
    a, sa = _propose(*args)
    b, sb = _propose(*args)
    _same(a, b, "run to run")
    _same(sa, sb, "run to run, states")
    c, _ = _propose(*args, call=gp.CALL + 1)
    _same(c[:, 0, 0], a[:, 0, 0], "sequence 0, step 0")
    assert (c[:, 1:, 0] != a[:, 1:, 0]).all(), "another call draws anew"
    d, _ = _propose(*args, seed=gp.SEED + 1)
    assert (d[:, 1:, 0] != a[:, 1:, 0]).all(), "another seed draws anew"
    alone, sl = _propose(*args, m=1)
    _same(alone[0], a[0], "env 0 alone")
    _same(sl[:, 0], sa[:, 0], "env 0 alone, states")


# ---------------------------------------------------------------------------------------------------------------------- 5: a poisoned particle
def test_a_poisoned_env_takes_the_fallback(engines):
    """One env's obs holds a NaN: its sequences are clip(0, lb, ub) at every step, finite; the other env's sequences and states -- rows
    of the same 16-row tile -- are bit for bit what they are without it."""
    prob, eng = engines("hc")
    obs = np.asarray(prob["obs"], F)
    layers = gref.actor(eng.D, gp.HIDDEN, eng.A, gp.ACT, obs, gp.LO, gp.HI, seed=eng.A)
    _register(eng, layers, gp.HIDDEN, gp.ACT, "tanh")
    args = (eng, prob, gp.HIDDEN, gp.ACT, "tanh", gp.P, "head", 1.0)
    clean, cs = _propose(*args)
    bad = obs.copy()
    bad[1, 7] = NAN
    seqs, st = _propose(*args, obs=bad)
    assert np.isfinite(seqs).all() and (seqs[1] == pref.fallback(-1.0, 1.0)).all() and (clean[1] != 0).any()
    assert not np.isfinite(st[1:, 1]).all()
    _same(seqs[0], clean[0], "env 0 met its neighbour's poison")
    _same(st[:, 0], cs[:, 0], "env 0's states")


# ---------------------------------------------------------------------------------------------------------------------- 6: fused against stepwise
@pytest.mark.parametrize("combo", ["guided-cem", "guided-mppi", "critic-cem", "critic-mppi"])
def test_fused_equals_stepwise(engines, combo):
    """`cadm_guided_plan` and `cadm_critic_plan` with proposals drawn from the head == the same loop one launch at a time
    (`planner.icem_plan(..., policy=...)`: one `policy_propose`, then every iteration `icem_inject`), bit for bit over two consecutive
    calls: the plan, the best return, the carry; the stepwise loop's proposals are `policy_propose`'s under the head; on the noise route
    the plan is another."""
    mppi, critic = combo.endswith("mppi"), combo.startswith("critic")
    prob, eng = engines("loop" if mppi else "loop-vanilla")
    H, A, P, K, hidden = eng.H, eng.A, 6, 2, (50, 30)
    layers = gref.actor(eng.D, hidden, A, "tanh", np.asarray(prob["obs"], F), gp.LO, gp.HI, seed=40)
    _register(eng, layers, hidden, "tanh", "tanh")
    pol = HipEngine.policy_params(hidden, "tanh", "tanh", P, 0.0)
    crt = None
    if critic:
        crt = HipEngine.critic_params((64, 48), "tanh", 2, "min", 3.0)
        eng.set_critic_nets(crt, cref.he_critics(eng.D, A, (64, 48), 2, 32))
    icem = dict(noise_beta=1.0 if mppi else 0.0, keep_elites=K, decay=1.25, return_best=False, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if mppi else HipEngine.icem_params(**icem)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    tail = (None, None, None, None, None, None, True, None, None, None, None, None, None, None, prm)

    def fused(call, mean, carry, valid, **kw):
        if critic:
            return eng.critic_plan(crt, pol, *tail, *args, mean, prob["init_var"], N, carry=carry, carry_valid=valid, seed=4, call=call, **kw)
        return eng.guided_plan(pol, *tail, *args, mean, prob["init_var"], N, carry=carry, carry_valid=valid, seed=4, call=call, **kw)

    (ca, va), (cb, vb) = zero_carry(eng, M, K, H), zero_carry(eng, M, K, H)
    mean, plans = prob["init_mean"], {}
    eng.set_policy_proposals("head", 0.8)
    try:
        for call in (1, 2):
            a, ra = fused(call, mean, ca, va, want_best_return=True)
            b, info, extra = hplanner.icem_plan(eng, *args, mean, prob["init_var"], N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                                update="mppi" if mppi else "cem", temperature=0.5, relative=True, policy=pol, critic=crt, **icem)
            a = _np(a)
            assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
            _same(a, _np(b), "plan of call %d" % call)
            _same(_np(ra), _np(extra["best_ret"]), "best return of call %d" % call)
            _same(_np(ca), _np(cb), "carry of call %d" % call)
            props = _np(extra["proposals"])
            _same(props, _np(eng.policy_propose(pol, prob["obs"], _ctx(eng, prob, M), seed=4, call=call)), "the stepwise loop's proposals")
            assert not np.array_equal(props[:, 1], props[:, 0])
            if not mppi:
                for it, x in enumerate(info):
                    s = hplanner.policy_slot(K, it + 1 == ITERS, True)
                    _same(_np(x["actions"])[:, s:s + P], props, "iteration %d holds the proposals" % it)
            plans[call] = a
            mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)
    finally:
        eng.set_policy_proposals("noise", 1.0)
    other = _np(fused(1, prob["init_mean"], *zero_carry(eng, M, K, H)))
    assert np.isfinite(other).all() and not np.array_equal(_bits(other), _bits(plans[1])), "the noise route plans something else"


# ---------------------------------------------------------------------------------------------------------------------- 7: the class route
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_class_route(gpu, context):
    """`get_action` with proposals="head" runs and is the engine call under the setting the model made at construction;
    `policy_proposals` returns what was injected: the engine's `policy_propose` of the last call, sequence 0 the mode, the others draws;
    a model with proposals="noise" spelled out is bit for bit a model built without the new keys."""
    H, A, D = 5, 6, 18
    hidden, act = (64, 32), "swish"
    pp = dict(hidden_sizes=hidden, activation=act, n_samples=5)
    head = dict(kind="gaussian", log_std_bounds=(gp.LO, gp.HI))
    kw = dict(hidden=(200,) * 4, cem_keep_elites=2, policy_head=head)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    rng = np.random.default_rng(5)
    stats = (rng.standard_normal(D).astype(F), rng.uniform(0.5, 2.0, D).astype(F))
    model, prob = plan_model(context, H, cem_policy_prior=dict(pp, proposals="head", std_scale=0.7), **kw)
    assert model._proposals == ("head", float(F(0.7)))
    layers = gref.actor(D, hidden, A, act, np.asarray(prob["obs"], F), gp.LO, gp.HI, seed=17, mean=stats[0], std=stats[1])
    model.set_policy(layers, *stats)
    plan = plan_act(model, prob, context, mean, var)
    assert plan.shape == (M, H, A) and np.isfinite(plan).all() and np.abs(plan).max() <= 1.0 and model._call == 1
    eng, opt = model.engine, model._opt
    hist = (prob["cp_obs"], prob["cp_act"]) if context else (None, None)
    carry, valid = zero_carry(eng, M, 2, H)
    direct = eng.guided_plan(opt.policy_params, None, None, None, None, None, None, True, None, None, None, None, None, None, None, opt.params,
                             prob["obs"], *hist, mean, var, model.n_candidates, carry=carry, carry_valid=valid, seed=model.seed, call=1)
    _same(plan, _np(direct), "get_action against the engine call")
    hp = hist if context else ()
    props, st = model.policy_proposals(prob["obs"], *hp, return_states=True)
    assert props.shape == (M, 5, H, A) and st.shape == (H, M, 5, model.n_particles, D) and np.isfinite(props).all() and model._call == 1
    ctx_vec = eng.context_forward(*hist) if context else None
    _same(props, _np(eng.policy_propose(opt.policy_params, prob["obs"], ctx_vec, seed=model.seed, call=1)), "policy_proposals")
    _same(props[:, 0, 0], model.policy_action(np.asarray(prob["obs"], F)), "sequence 0 is the mode")
    assert (props[:, 1:, 0] != props[:, :1, 0]).all(), "sequences 1 .. P - 1 are draws"
    # the noise route spelled out against a model without the new keys
    plans, proposals = [], []
    for prior in (dict(pp, noise_std=0.2, proposals="noise", std_scale=1.0), dict(pp, noise_std=0.2)):
        other, _ = plan_model(context, H, cem_policy_prior=prior, **kw)
        assert other._proposals == ("noise", 1.0)
        other.set_policy(layers, *stats)
        plans.append(plan_act(other, prob, context, mean, var))
        proposals.append(other.policy_proposals(prob["obs"], *hp))
    _same(plans[0], plans[1], "proposals=\"noise\" against no key: the plan")
    _same(proposals[0], proposals[1], "proposals=\"noise\" against no key: the proposals")
    _same(proposals[0][:, 0, 0], props[:, 0, 0], "sequence 0, step 0: the mode on either route")
    assert not np.array_equal(_bits(proposals[0][:, 1:]), _bits(props[:, 1:]))
    with pytest.raises(ValueError, match="declare policy_head"):
        plan_model(context, H, cem_policy_prior=dict(pp, proposals="head"), hidden=(200,) * 4)


# ---------------------------------------------------------------------------------------------------------------------- 8: lifecycle, refusals
def test_lifecycle_and_refusals(engines):
    """Under HEAD: no head on the registered net is CADM_ESTATE, and so it is again after `set_policy_net` dropped the head, until the
    head is set again; the setting survives a second `set_policy_net` / `set_policy_head`; a noise_std > 0 in the call's params, lb >=
    ub, an unknown source and a std_scale negative or not finite are CADM_EINVAL -- before any HIP call: the dummy buffer next to the
    bad argument is never touched; NOISE with any scale plans as ever."""
    prob, eng = engines("loop")
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(8192, dtype=torch.float32, device=eng.device)
    Pb = ct.c_void_p(buf.data_ptr())
    hidden = (32, 16)
    layers = gref.actor(eng.D, hidden, eng.A, "relu", np.asarray(prob["obs"], F), gp.LO, gp.HI, seed=1)
    mp = HipEngine.mppi_params()

    def V(noise_std=0.0, n_samples=4):
        return ct.byref(HipEngine.policy_params(hidden, "relu", "tanh", n_samples, noise_std))

    def propose(v, c=ctx):
        return lib.cadm_policy_propose(c, v, Pb, Pb, M, 0, 1, Pb, None, Pb, None)

    def guided(v, c=ctx):
        return lib.cadm_guided_plan(c, v, None, None, None, None, None, None, 1, None, None, 0, None, None, None, None, None, 0, ct.byref(mp), Pb, Pb,
                                    Pb, Pb, Pb, None, None, M, N, 0, 1, Pb, Pb, None, None)

    def critic(v, c=ctx):
        return lib.cadm_critic_plan(c, None, v, None, None, None, None, None, None, 1, None, None, 0, None, None, None, None, None, 0, ct.byref(mp), Pb,
                                    Pb, Pb, Pb, Pb, None, None, M, N, 0, 1, Pb, Pb, None, None)

    def refused(rc, name, frag, code=EINVAL):
        msg = lib.cadm_last_error().decode()
        assert rc == code, "%s: expected %d, got %d (%s)" % (name, code, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    entries = (("cadm_policy_propose", propose), ("cadm_guided_plan", guided), ("cadm_critic_plan", critic))
    # the setting itself
    for bad in (2, -1):
        refused(lib.cadm_set_policy_proposals(ctx, bad, 1.0), "cadm_set_policy_proposals", "unknown source")
    for bad in (-0.5, NAN, float("inf")):
        refused(lib.cadm_set_policy_proposals(ctx, 1, bad), "cadm_set_policy_proposals", "std_scale")
    refused(lib.cadm_set_policy_proposals(None, 1, 1.0), "cadm_set_policy_proposals", "null")
    with pytest.raises(ValueError, match="proposals must be"):
        eng.set_policy_proposals("mode")
    with pytest.raises(ValueError, match="std_scale"):
        eng.set_policy_proposals("head", -1.0)
    # HEAD with a net and no head; with no net
    _register(eng, layers, hidden, "relu", "tanh", head=False)
    eng.set_policy_proposals("head", 1.0)
    try:
        for name, fn in entries:
            refused(fn(V()), name, "no Gaussian head", code=ESTATE)
        # with the head: accepted by the checks; a noise_std in the params is a second source
        mean_layers, W_ls, b_ls = gref.split(layers, eng.A)
        eng.set_policy_head(_head(), W_ls, b_ls)
        for name, fn in entries:
            refused(fn(V(noise_std=0.3)), name, "one source")
        seqs = _np(eng.policy_propose(HipEngine.policy_params(hidden, "relu", "tanh", 4, 0.0), prob["obs"], _ctx(eng, prob, M), seed=1, call=1))
        assert np.isfinite(seqs).all() and (seqs[:, 1:, 0] != seqs[:, :1, 0]).all()
        # a second set_policy_net drops the head and leaves the setting: CADM_ESTATE until the head is back, then the same bits
        eng.set_policy_net(HipEngine.policy_params(hidden, "relu", "tanh", 1, 0.0), mean_layers)
        for name, fn in entries:
            refused(fn(V()), name, "no Gaussian head", code=ESTATE)
        eng.set_policy_head(_head(), W_ls, b_ls)
        again = _np(eng.policy_propose(HipEngine.policy_params(hidden, "relu", "tanh", 4, 0.0), prob["obs"], _ctx(eng, prob, M), seed=1, call=1))
        _same(again, seqs, "the setting survived set_policy_net and set_policy_head")
        assert lib.cadm_set_policy_net(ctx, None, None, None, None, None, None) == 0
        for name, fn in entries[:2]:
            refused(fn(V()), name, "no policy net", code=ESTATE)
    finally:
        eng.set_policy_proposals("noise", 1.0)
    # lb >= ub: no head can be set on such a ctx, and HEAD is refused for the bounds, not for the head
    flat = make_engine(prob, p=gp.NP, num_elites=KE, num_cem_iters=ITERS, lower_bound=0.5, upper_bound=0.5)
    flat.set_policy_net(HipEngine.policy_params(hidden, "relu", "tanh", 1, 0.0), gref.split(layers, eng.A)[0])
    flat.set_policy_proposals("head", 1.0)
    for name, fn in entries:
        refused(fn(V(), c=flat._ctx), name, "leave no range")
    flat.close()
    assert (_np(buf) == 0).all()
    # NOISE: the engine plans as ever
    _register(eng, layers, hidden, "relu", "tanh")
    quiet = _np(eng.policy_propose(HipEngine.policy_params(hidden, "relu", "tanh", 4, 0.3), prob["obs"], _ctx(eng, prob, M), seed=1, call=1))
    _same(quiet[:, 0, 0], seqs[:, 0, 0], "sequence 0, step 0: the mode on either route")
    assert np.isfinite(quiet).all() and not np.array_equal(_bits(quiet[:, 1:]), _bits(seqs[:, 1:]))
