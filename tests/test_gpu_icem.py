"""GPU: the opt-in iCEM planner (csrc/icem.hip, `cadm_icem_plan`): coloured-noise sampling, elite carry-over, best plan, candidate decay.

Geometry of every test unless it says otherwise: halfcheetah, vanilla and CaDM, hidden (32,) * 4 (zero-padded on the compiled-in 128-wide
kernel: no on-demand build), ensemble 5, particles 5, m = 2, n = 64, num_elites = 8, K = 3, 3 CEM iterations, H = 5 and H = 6 (odd / even
H: without / with the Nyquist term).  Numpy restatements: tests/icem_ref.py."""
import ctypes as ct

import numpy as np
import pytest
import torch

import icem_ref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import _np, assert_close, make_engine, zero_carry
from helpers import plan_act as _act
from helpers import plan_model as _model

pytestmark = pytest.mark.gpu

HID = (32,) * 4
M, N, KE, K, ITERS, A = 2, 64, 8, 3, 3, 6


def _engine(H, context=True, seed=3, **kw):
    prob = synth.make_problem(env="halfcheetah", context=context, E=5, m=M, H=H, seed=seed, hidden_sizes=HID, trained_like=True)
    kw.setdefault("num_elites", KE)
    kw.setdefault("num_cem_iters", ITERS)
    return prob, make_engine(prob, p=5, **kw)


def _mean_var(rng, H, m=M):
    """A mean near both bounds (clipping and the constrained sd are hit), a var above and below the bound term ((ub - mean) / 2)^2."""
    mean = rng.uniform(-0.7, 0.7, (m, H, A)).astype(np.float32)
    var = rng.uniform(0.02, 0.1, (m, H, A)).astype(np.float32)
    mean[0, 0, 0], mean[0, H - 1, 1], mean[m - 1, 0, 2], mean[m - 1, H - 1, 5] = 0.98, -0.97, 0.9, -1.0
    var[0, 0, 0], var[m - 1, 0, 2] = 0.5, 0.5            # above the bound term: the bound term is the variance
    var[0, 0, 3], var[m - 1, H - 1, 4] = 1e-4, 3.0       # far below / above
    return mean, var


# ---------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("H", [5, 6])
@pytest.mark.parametrize("beta", [0.0, 0.5, 2.5])
def test_colored_sampler_injected(gpu, H, beta):
    """`cadm_sample_actions_colored` on injected unit-variance spectral draws against the float64 restatement: every element <= 1e-5."""
    prob, eng = _engine(H)
    rng = np.random.default_rng(10 * H + int(4 * beta))
    mean, var = _mean_var(rng, H)
    xi = rng.standard_normal((M, N, A, H)).astype(np.float32)
    got = _np(eng.sample_actions_colored(mean, var, N, beta, xi=xi))
    ref = icem_ref.colored_actions(mean, var, xi, beta)
    err = np.abs(got - ref).max()
    print("\n[H=%d beta=%g] coloured sampler vs float64: max abs %.2e" % (H, beta, err))
    assert got.shape == (M, N, H, A) and got.min() >= -1.0 and got.max() <= 1.0
    assert (got == 1.0).any() and (got[M - 1, :, H - 1, 5] == -1.0).all()      # the clip is hit; a mean on the bound stays there
    assert err <= 1e-5
    # the constrained sd bites: with the raw var the candidates of (0, 0, 0) would spread 0.7 wide instead of 0.01
    assert got[0, :, 0, 0].std() < 0.02


def test_colored_sampler_h1_is_the_plain_draw(gpu):
    """beta = 0, H = 1: z = x_0, so the action is mean + sd x_0 (float32; 1e-6 covers the rounding of the square root)."""
    prob, eng = _engine(1)
    rng = np.random.default_rng(5)
    mean, var = _mean_var(rng, 1)
    xi = rng.standard_normal((M, N, A, 1)).astype(np.float32)
    got = _np(eng.sample_actions_colored(mean, var, N, 0.0, xi=xi))
    a1, a2 = (mean + np.float32(1.0)) / np.float32(2.0), (np.float32(1.0) - mean) / np.float32(2.0)
    sd = np.sqrt(np.minimum(np.minimum(a1 * a1, a2 * a2), var))
    want = np.clip(mean[:, None] + sd[:, None] * np.transpose(xi, (0, 1, 3, 2)), np.float32(-1.0), np.float32(1.0))
    print("\n[H=1] max abs %.2e" % np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("H", [5, 6])
def test_colored_sampler_device_rng(gpu, H):
    """The device's spectral draws are Philox4x32-10 with the documented counters (restated from oracle/philox.py): actions within
    1e-5 of the float64 synthesis of the restated draws; same (seed, call, it): the same bits; another `it`: other draws."""
    prob, eng = _engine(H)
    rng = np.random.default_rng(H)
    mean, var = _mean_var(rng, H)
    seed, call, it, beta = 11, 5, 2, 1.5
    got = _np(eng.sample_actions_colored(mean, var, N, beta, seed=seed, call=call, it=it))
    xi = icem_ref.spectral_draws(seed, call, it, M, N, A, H)
    ref = icem_ref.colored_actions(mean, var, xi, beta)
    err = np.abs(got - ref).max()
    print("\n[H=%d] device RNG vs restated draws: max abs %.2e" % (H, err))
    assert err <= 1e-5
    np.testing.assert_array_equal(got, _np(eng.sample_actions_colored(mean, var, N, beta, seed=seed, call=call, it=it)))
    other = _np(eng.sample_actions_colored(mean, var, N, beta, seed=seed, call=call, it=it + 1))
    assert np.abs(other - got).max() > 0.1
    assert np.abs(_np(eng.sample_actions_colored(mean, var, N, beta, seed=seed, call=call + 1, it=it)) - got).max() > 0.1


def test_colored_noise_statistics(gpu):
    """2 x 4096 x 6 sequences at beta = 2, H = 30, bounds and var chosen so that nothing clips: per step the sample variance is within
    4 / sqrt(N) of 1 and the lag-1 sample correlation within 4 / sqrt(N) of the closed form rho_1 (N = sequences per step: sampling
    error, not a tuned number).  The seed was picked on the CPU from the restated draws (seeds 1..5 give 0.010 .. 0.016 against the
    bound 0.018 for the variance; the steps of a sequence are strongly correlated, so their deviations move together)."""
    H, n, beta = 30, 4096, 2.0
    prob, eng = _engine(H, context=False, lower_bound=-100.0, upper_bound=100.0)
    mean = np.random.default_rng(0).uniform(-1.0, 1.0, (M, H, A)).astype(np.float32)
    var = np.full((M, H, A), 0.01, np.float32)
    got = _np(eng.sample_actions_colored(mean, var, n, beta, seed=3, call=1, it=0)).astype(np.float64)
    z = ((got - mean[:, None]) / np.sqrt(np.float64(np.float32(0.01)))).transpose(0, 1, 3, 2).reshape(-1, H)      # [sequences, H]
    Nseq = z.shape[0]
    assert Nseq == 2 * 4096 * 6
    bound = 4.0 / np.sqrt(Nseq)
    v = z.var(axis=0)
    r1 = icem_ref.rho1(H, beta)
    c = np.array([np.corrcoef(z[:, t], z[:, t + 1])[0, 1] for t in range(H - 1)])
    print("\nvariance dev %.4f, lag-1 correlation dev %.4f (rho1 %.4f), bound %.4f" % (np.abs(v - 1).max(), np.abs(c - r1).max(), r1, bound))
    assert np.abs(v - 1.0).max() <= bound
    assert np.abs(c - r1).max() <= bound
    assert r1 > 0.8


# ---------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("H", [5, 6])
def test_keep_inject_track_best_exact(gpu, H):
    prob, eng = _engine(H, context=False)
    rng = np.random.default_rng(20 + H)
    n = 37                                                   # (odd: no multiple of anything)
    acts = rng.uniform(-1, 1, (M, n, H, A)).astype(np.float32)
    el = np.stack([rng.permutation(n)[:KE] for _ in range(M)]).astype(np.int32)
    ta, te = eng._t(acts), eng._t(el, dtype=torch.int32)
    kept = _np(eng.icem_keep(ta, te, K))
    np.testing.assert_array_equal(kept, acts[np.arange(M)[:, None], el[:, :K]])
    full = _np(eng.icem_keep(ta, te, KE))
    np.testing.assert_array_equal(full, acts[np.arange(M)[:, None], el])
    # inject, shift = 0: slots [0, K) replaced, the rest untouched
    src = rng.uniform(-1, 1, (M, K, H, A)).astype(np.float32)
    got = _np(eng.icem_inject(eng._t(acts).clone(), eng._t(src)))
    want = acts.copy()
    want[:, :K] = src
    np.testing.assert_array_equal(got, want)
    # shift = 1 with valid = [0, 1]: env 0 untouched entirely; env 1: steps [0, H - 1) of slots [0, K) take steps [1, H), step H - 1 stays
    valid = eng._t(np.array([0, 1], np.int32), dtype=torch.int32)
    got = _np(eng.icem_inject(eng._t(acts).clone(), eng._t(src), valid=valid, shift=1))
    want = acts.copy()
    want[1, :K, :H - 1] = src[1, :, 1:]
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[0], acts[0])
    np.testing.assert_array_equal(got[1, :K, H - 1], acts[1, :K, H - 1])
    np.testing.assert_array_equal(got[:, K:], acts[:, K:])
    # one slot at an offset (how the mean candidate reaches slot K)
    one = rng.uniform(-1, 1, (M, 1, H, A)).astype(np.float32)
    got = _np(eng.icem_inject(eng._t(acts).clone(), eng._t(one), slot0=K))
    want = acts.copy()
    want[:, K] = one[:, 0]
    np.testing.assert_array_equal(got, want)
    # track-best: strictly greater replaces; a tie keeps the earlier sequence, -0.0 against +0.0 included; NaN never replaces
    # (non-finite returns at length: tests/test_gpu_icem_envelope.py)
    cand = rng.standard_normal((M, n)).astype(np.float32)
    best_ret = eng._t(np.array([-np.inf, -np.inf], np.float32))
    best_seq = eng._t(np.full((M, H, A), np.nan, np.float32))
    tc = eng._t(cand)
    eng.icem_track_best(tc, te, ta, best_ret, best_seq)
    np.testing.assert_array_equal(_np(best_ret), cand[np.arange(M), el[:, 0]])
    np.testing.assert_array_equal(_np(best_seq), acts[np.arange(M), el[:, 0]])
    first_seq = _np(best_seq).copy()
    el2 = el.copy()
    el2[:, 0] = el[:, 1]
    cand2 = cand.copy()
    cand2[0, el2[0, 0]] = cand[0, el[0, 0]]                          # env 0: a tie -> stays
    cand2[1, el2[1, 0]] = cand[1, el[1, 0]] + np.float32(0.5)        # env 1: strictly greater -> replaced
    eng.icem_track_best(eng._t(cand2), eng._t(el2, dtype=torch.int32), ta, best_ret, best_seq)
    np.testing.assert_array_equal(_np(best_seq)[0], first_seq[0])
    np.testing.assert_array_equal(_np(best_seq)[1], acts[1, el2[1, 0]])
    np.testing.assert_array_equal(_np(best_ret), [cand[0, el[0, 0]], cand2[1, el2[1, 0]]])
    zr = eng._t(np.array([-0.0, 0.0], np.float32))
    zs = eng._t(first_seq)
    cand3 = cand.copy()
    cand3[0, el2[0, 0]], cand3[1, el2[1, 0]] = 0.0, -0.0
    eng.icem_track_best(eng._t(cand3), eng._t(el2, dtype=torch.int32), ta, zr, zs)
    np.testing.assert_array_equal(_np(zs), first_seq)
    assert np.signbit(_np(zr)[0]) and not np.signbit(_np(zr)[1])
    # a NaN return never replaces: where every return is NaN nothing changes ...
    eng.icem_track_best(eng._t(np.full_like(cand3, np.nan)), eng._t(el2, dtype=torch.int32), ta, zr, zs)
    np.testing.assert_array_equal(_np(zs), first_seq)
    assert np.signbit(_np(zr)[0]) and not np.signbit(_np(zr)[1])
    # ... and where the first elites' returns are NaN, the first elite whose return is not NaN stands for the iteration (the NaN
    # returns rank first among the refit's elites; before, elite 0 alone was read and the iteration counted for nothing)
    cand3[:, el2[:, 0]] = np.nan
    eng.icem_track_best(eng._t(cand3), eng._t(el2, dtype=torch.int32), ta, zr, zs)
    want_seq, want_ret = first_seq.copy(), np.array([-0.0, 0.0], np.float32)
    for mi in range(M):
        c = next(int(c) for c in el2[mi] if not np.isnan(cand3[mi, c]))
        assert c == el2[mi, 2]                                       # (elites 0 and 1 are the same, NaN, candidate)
        if cand3[mi, c] > want_ret[mi]:
            want_seq[mi], want_ret[mi] = acts[mi, c], cand3[mi, c]
    np.testing.assert_array_equal(_np(zs), want_seq)
    np.testing.assert_array_equal(_np(zr), want_ret)
    assert not np.array_equal(want_seq, first_seq)                   # (at these seeds env 1's next elite beats the stored 0.0)


# ---------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("case", icem_ref.LOOP_CASES, ids=[icem_ref.case_id(c) for c in icem_ref.LOOP_CASES])
def test_whole_loop_stepwise_against_numpy(gpu, case):
    """The loop through the stepwise exports (cadm_amd.planner.icem_plan) against the numpy loop of tests/icem_ref.py in float64, on the
    deterministic model with injected draws (truncated-normal z for beta = 0, spectral xi for beta = 1), K = 3 with env 1 starting from
    carried elites, the mean candidate in the last iteration.  Per iteration: candidate returns within 1e-5 (helpers.assert_close:
    of max(|ref|, rms(ref))), elites identical and in order, kept sequences bit-equal to the candidates they came from; the final plan
    within 1e-5 absolute for cem_return 'mean' and 'best'.  Condition, checked on the CPU (tests/test_icem_ref.py): at these seeds the
    float32 and float64 oracles rank the elites the same way, with no two of the 9 best returns closer than 2e-4 of their scale."""
    H, context, beta, decay = case[:4]
    lower, upper = icem_ref.case_env_bounds(case)[1]      # (the two last cases: ant; bounds (-0.5, 2))
    c = icem_ref.LOOP
    prob, z, xi, carry, valid = icem_ref.loop_case(case)
    eng = make_engine(prob, p=c["p"], deterministic=True, num_elites=c["num_elites"], num_cem_iters=c["iters"], lower_bound=lower, upper_bound=upper)
    tcarry, tvalid = eng._t(carry), eng._t(valid, dtype=torch.int32)
    plan, info, best = hplanner.icem_plan(eng, prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], c["n"],
                                          noise_beta=beta, keep_elites=c["K"], decay=decay, add_mean_last=True, carry=tcarry, carry_valid=tvalid,
                                          z=None if z is None else [eng._t(x) for x in z], xi=None if xi is None else [eng._t(x) for x in xi],
                                          return_info=True)
    rplan, rinfo, rcarry, rvalid = icem_ref.loop_reference(case, np.float64)
    assert len(info) == len(rinfo) == c["iters"]
    for it in range(c["iters"]):
        acts = _np(info[it]["actions"])
        assert acts.shape == rinfo[it]["actions"].shape
        assert np.abs(acts - rinfo[it]["actions"]).max() <= 1e-5, "candidates of iteration %d" % it
        got, want = _np(info[it]["cand"]), rinfo[it]["cand"]
        scale = np.maximum(np.abs(want), np.sqrt(np.mean(want * want)))
        print("\n[it %d] candidate returns: worst %.2e of their scale" % (it, (np.abs(got - want) / scale).max()), end="")
        assert_close(got, want, 1e-5, "candidate returns, iteration %d" % it)
        np.testing.assert_array_equal(_np(info[it]["elites"]), rinfo[it]["elites"], err_msg="elites of iteration %d" % it)
        el = _np(info[it]["elites"])
        np.testing.assert_array_equal(_np(info[it]["kept"]), acts[np.arange(M)[:, None], el[:, :c["K"]]])
    np.testing.assert_array_equal(_np(info[0]["actions"])[1, :c["K"], :H - 1], carry[1, :, 1:])
    np.testing.assert_array_equal(_np(tcarry), _np(info[-1]["kept"]))
    np.testing.assert_array_equal(_np(tvalid), [1, 1])
    pm, rbest = _np(best["plan_mean"]), _best_plan(case)      # (the loop does not depend on the return mode: both plans of one run)
    print("\nplan (mean) %.2e, plan (best) %.2e" % (np.abs(pm - rplan).max(), np.abs(_np(best["best_seq"]) - rbest).max()))
    assert np.abs(pm - rplan).max() <= 1e-5
    np.testing.assert_array_equal(_np(plan), pm)
    assert np.abs(_np(best["best_seq"]) - rbest).max() <= 1e-5


def _best_plan(case):
    return icem_ref.loop_reference(case, np.float64, return_best=True)[0]


# ---------------------------------------------------------------------------------------------------------------------- 5
FUSED = [      # H, context, beta, decay, return_best, add_mean_last
    (5, False, 0.0, 1.0, False, False),
    (6, True, 2.0, 1.5, True, True),
    (5, True, 2.0, 1.0, False, True),
    (6, False, 0.0, 1.5, True, False),
]


@pytest.mark.parametrize("H,context,beta,decay,best,addmean", FUSED, ids=["H%d-%s-beta%g-decay%g-%s%s" % (r[0], "cadm" if r[1] else "vanilla", r[2], r[3],
                                                                                                "best" if r[4] else "mean", "-addmean" if r[5] else "") for r in FUSED])
def test_fused_equals_stepwise(gpu, H, context, beta, decay, best, addmean):
    """`cadm_icem_plan` with device RNG (probabilistic model: head noise too) == the same launches one at a time, bit for bit: the
    plan, the best return and the carried elites of two consecutive calls -- the second consumes the first's carry."""
    prob, eng = _engine(H, context=context)
    prm = HipEngine.icem_params(noise_beta=beta, keep_elites=K, decay=decay, return_best=best, add_mean_last=addmean)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    z = lambda: zero_carry(eng, M, K, H)
    (ca, va), (cb, vb) = z(), z()
    mean, var = prob["init_mean"], prob["init_var"]
    plans = []
    for call in (1, 2):
        a, ra = eng.icem_plan(prm, *args, mean, var, N, carry=ca, carry_valid=va, seed=4, call=call, want_best_return=True)
        b, _, extra = hplanner.icem_plan(eng, *args, mean, var, N, noise_beta=beta, keep_elites=K, decay=decay, return_best=best,
                                         add_mean_last=addmean, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True)
        a = _np(a)
        assert np.isfinite(a).all() and np.abs(a).max() <= 1.0 and np.abs(a).max() > 0
        np.testing.assert_array_equal(a, _np(b), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_np(ra), _np(extra["best_ret"]))
        np.testing.assert_array_equal(_np(ca), _np(cb), err_msg="carry after call %d" % call)
        np.testing.assert_array_equal(_np(va), [1, 1])
        plans.append(a)
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), np.float32)], axis=1)      # the samplers' warm start
    # the carry is consumed: the same call without it refits another mean (the best sequence of a call may be the same either way)
    if not best:
        (cc, vc) = z()
        c = _np(eng.icem_plan(prm, *args, mean, var, N, carry=cc, carry_valid=vc, seed=4, call=3))
        d = _np(eng.icem_plan(prm, *args, mean, var, N, carry=ca.clone(), carry_valid=va.clone(), seed=4, call=3))
        assert not np.array_equal(c, d)


# ---------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_default_kwargs_take_the_untouched_route(gpu, context):
    """All-default kwargs and the same kwargs spelled out at their defaults: bit-identical get_action results over three calls, and
    neither model holds any iCEM state."""
    H = 5
    a, prob = _model(context, H)
    b, _ = _model(context, H, cem_noise_beta=0.0, cem_keep_elites=0, cem_decay=1.0, cem_return="mean", cem_add_mean=False)
    assert a._opt is None and b._opt is None
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    for _ in range(3):
        pa, pb = _act(a, prob, context, mean, var), _act(b, prob, context, mean, var)
        assert np.isfinite(pa).all()
        np.testing.assert_array_equal(pa, pb)
        # and the engine's own one-call planner on the same (seed, call): the route is today's
        ref = _np(a.engine.cem_plan(prob["obs"], prob["cp_obs"] if context else None, prob["cp_act"] if context else None, mean, var, N,
                                    seed=a.seed, call=a._call))
        np.testing.assert_array_equal(pa, ref)
        mean = np.concatenate([pa[:, 1:], np.zeros((M, 1, A))], axis=1)
    assert a._plan_carry is None and b._plan_carry is None
    a.reset_plan_carry()      # a no-op on a model that carries nothing


def test_refusals_at_construction(gpu, monkeypatch):
    from cadm_amd.envs import make_env_spec
    with pytest.raises(ValueError, match="need use_cem=True"):
        _model(True, 5, use_cem=False, cem_keep_elites=3)
    with pytest.raises(ValueError, match="need use_cem=True"):
        _model(False, 5, use_cem=False, cem_noise_beta=1.0)
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        _model(True, 5, env=make_env_spec("cartpole"), cem_return="best")
    import torch.distributed as dist
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        _model(True, 5, process_group=object(), cem_decay=1.25)
    monkeypatch.undo()
    for bad, msg in ((dict(cem_return="first"), "cem_return"), (dict(cem_decay=0.5), "cem_decay"), (dict(cem_keep_elites=-1), "cem_keep_elites"),
                     (dict(cem_keep_elites=51), "exceeds the planner's 50 elites"), (dict(cem_noise_beta=-1.0), "cem_noise_beta")):
        with pytest.raises(ValueError, match=msg):
            _model(True, 5, **bad)


@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_get_action_carries_elites_across_calls(gpu, context):
    """cem_keep_elites = 3 through the class: after the first get_action the model holds 3 elites per env; the second call equals, bit
    for bit, the stepwise loop on the model's engine started from that carry -- whose iteration 0 holds the carried elites, moved one
    step on, in slots 0..2 -- and differs from the same call without a carry.  reset_plan_carry (all envs, one env), another m, load:
    the next plan is a fresh model's for the same (seed, call)."""
    H = 6
    kw = dict(cem_noise_beta=2.0, cem_keep_elites=K, cem_decay=1.25, cem_return="best", cem_add_mean=True)
    model, prob = _model(context, H, **kw)
    eng = model.engine
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    p1 = _act(model, prob, context, mean, var)
    assert p1.shape == (M, H, A) and np.isfinite(p1).all() and np.abs(p1).max() <= 1.0
    carry1 = model._plan_carry.clone()
    np.testing.assert_array_equal(_np(model._plan_carry_valid), [1, 1])
    assert tuple(carry1.shape) == (M, K, H, A) and np.abs(_np(carry1)).max() > 0
    mean2 = np.concatenate([p1[:, 1:], np.zeros((M, 1, A))], axis=1)
    p2 = _act(model, prob, context, mean2, var)
    cp = (prob["cp_obs"], prob["cp_act"]) if context else (None, None)
    step = dict(noise_beta=2.0, keep_elites=K, decay=1.25, return_best=True, add_mean_last=True, seed=model.seed, call=2, return_info=True)
    c2, v2 = carry1.clone(), torch.ones((M,), dtype=torch.int32, device=eng.device)
    q2, info, _ = hplanner.icem_plan(eng, prob["obs"], cp[0], cp[1], mean2, var, N, carry=c2, carry_valid=v2, **step)
    np.testing.assert_array_equal(_np(info[0]["actions"])[:, :K, :H - 1], _np(carry1)[:, :, 1:])
    np.testing.assert_array_equal(p2, _np(q2))
    np.testing.assert_array_equal(_np(model._plan_carry), _np(c2))
    c0, v0 = torch.zeros_like(carry1), torch.zeros((M,), dtype=torch.int32, device=eng.device)
    q0 = hplanner.icem_plan(eng, prob["obs"], cp[0], cp[1], mean2, var, N, carry=c0, carry_valid=v0, **dict(step, return_info=False))
    assert not np.array_equal(p2, _np(q0))
    # reset: the third call is a fresh model's third call
    fresh, _ = _model(context, H, **kw)
    fresh._call = model._call
    model.reset_plan_carry()
    np.testing.assert_array_equal(_np(model._plan_carry_valid), [0, 0])
    np.testing.assert_array_equal(_act(model, prob, context, mean2, var), _act(fresh, prob, context, mean2, var))
    # a mask resets only its envs: env 1 plans as fresh, env 0 does not
    model.reset_plan_carry(np.array([False, True]))
    np.testing.assert_array_equal(_np(model._plan_carry_valid), [1, 0])
    fresh.reset_plan_carry()
    pm, pf = _act(model, prob, context, mean2, var), _act(fresh, prob, context, mean2, var)
    np.testing.assert_array_equal(pm[1], pf[1])
    assert not np.array_equal(pm[0], pf[0])
    # another number of envs: nothing carried
    one = {k: (v[:1] if isinstance(v, np.ndarray) and v.shape[0] == M else v) for k, v in prob.items()}
    model._call = fresh._call = 10
    fresh.reset_plan_carry()
    fresh._plan_carry = fresh._plan_carry_valid = None
    np.testing.assert_array_equal(_act(model, one, context, mean2[:1], var[:1]), _act(fresh, one, context, mean2[:1], var[:1]))
    assert tuple(model._plan_carry.shape) == (1, K, H, A)


def test_warm_start_resets_reach_the_carry(gpu):
    """CEMWarmStart.reset(idx) and DevicePlannerState.observe(done) / reset() clear the carried elites of the envs they reset."""
    from cadm_amd.caller import DevicePlannerState
    from cadm_amd.policies.mpc_controller import CEMWarmStart
    H = 5
    model, prob = _model(True, H, cem_keep_elites=K)
    ws = CEMWarmStart(M, H, A, model=model)
    _act(model, prob, True, ws.prev_sol, ws.init_var)
    np.testing.assert_array_equal(_np(model._plan_carry_valid), [1, 1])
    ws.reset([1])
    np.testing.assert_array_equal(_np(model._plan_carry_valid), [1, 0])
    CEMWarmStart(M, H, A).reset([0])      # without a model: as before
    state = DevicePlannerState(model, M)
    a = state.act(prob["obs"])
    assert tuple(a.shape) == (M, A) and np.isfinite(_np(a)).all()
    np.testing.assert_array_equal(_np(model._plan_carry_valid), [1, 1])
    state.observe(prob["obs"], a, prob["obs"], done=np.array([1, 0]))
    np.testing.assert_array_equal(_np(model._plan_carry_valid), [0, 1])
    state.reset()
    np.testing.assert_array_equal(_np(model._plan_carry_valid), [0, 0])


def test_device_planner_state_on_another_number_of_envs(gpu):
    """get_action with m = 2, then DevicePlannerState(model, 3).act: the model's carry is reallocated for 3 envs, all invalid when the plan
    starts -- the action is the first step of `icem_plan` from a zero carry under call 2 -- and the two calls moved the counter by 2."""
    from cadm_amd.caller import DevicePlannerState
    H = 5
    model, prob = _model(True, H, cem_keep_elites=K)
    eng = model.engine
    _act(model, prob, True, np.zeros((M, H, A)), np.full((M, H, A), 0.25))
    assert model._call == 1 and tuple(model._plan_carry.shape) == (M, K, H, A) and _np(model._plan_carry_valid).tolist() == [1, 1]
    state, seen, real = DevicePlannerState(model, 3), {}, eng.opt_in_plan

    def spy(opt, *a, **kw):
        seen.update(shape=tuple(kw["carry"].shape), valid=_np(kw["carry_valid"]).copy(), call=kw["call"])
        return real(opt, *a, **kw)
    eng.opt_in_plan = spy
    obs = np.concatenate([prob["obs"], prob["obs"][:1] + np.float32(0.1)])
    a = state.act(obs)
    assert seen["shape"] == (3, K, H, A) and seen["valid"].tolist() == [0, 0, 0] and seen["call"] == 2 and model._call == 2
    np.testing.assert_array_equal(_np(model._plan_carry_valid), [1, 1, 1])
    zero = torch.zeros((3, H, A), dtype=torch.float32, device=eng.device)
    want = eng.icem_plan(model._opt.params, obs, torch.zeros_like(state.hist_obs), torch.zeros_like(state.hist_act), zero, state.init_var, N,
                         *zero_carry(eng, 3, K, H), seed=model.seed, call=2)
    np.testing.assert_array_equal(_np(a), _np(want)[:, 0])


# ---------------------------------------------------------------------------------------------------------------------- 7
def test_argument_checks_return_einval(gpu):
    """Every new export refuses bad arguments with CADM_EINVAL and a message naming itself -- the checks run before any HIP call, so
    null device pointers next to the bad argument are never touched -- and the engine plans normally afterwards."""
    prob, eng = _engine(5)
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(4096, dtype=torch.float32, device=eng.device)
    ibuf = torch.zeros(64, dtype=torch.int32, device=eng.device)
    P, I = ct.c_void_p(buf.data_ptr()), ct.c_void_p(ibuf.data_ptr())

    def einval(rc, name, frag):
        msg = lib.cadm_last_error().decode()
        assert rc == -1, "%s: expected CADM_EINVAL, got %d (%s)" % (name, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    einval(lib.cadm_sample_actions_colored(ctx, P, P, None, -0.5, 0, 0, 0, M, N, P, None), "cadm_sample_actions_colored", "noise_beta")
    einval(lib.cadm_sample_actions_colored(ctx, P, P, None, 1.0, 0, 0, 0, 0, N, P, None), "cadm_sample_actions_colored", "bad arguments")
    einval(lib.cadm_sample_actions_colored(ctx, None, P, None, 1.0, 0, 0, 0, M, N, P, None), "cadm_sample_actions_colored", "bad arguments")
    einval(lib.cadm_sample_actions_colored(ctx, P, P, None, 1.0, 0, 0, -1, M, N, P, None), "cadm_sample_actions_colored", "iteration")
    einval(lib.cadm_icem_keep(ctx, P, I, M, N, KE + 1, P, None), "cadm_icem_keep", "keep_elites")
    einval(lib.cadm_icem_keep(ctx, P, None, M, N, K, P, None), "cadm_icem_keep", "bad arguments")
    einval(lib.cadm_icem_inject(ctx, P, None, M, 2, 3, 0, P, None), "cadm_icem_inject", "keep_elites")
    einval(lib.cadm_icem_inject(ctx, P, None, M, N, K, 2, P, None), "cadm_icem_inject", "shift")
    einval(lib.cadm_icem_inject(ctx, None, None, M, N, K, 0, P, None), "cadm_icem_inject", "bad arguments")
    einval(lib.cadm_icem_track_best(ctx, P, I, P, M, N, None, P, None), "cadm_icem_track_best", "bad arguments")
    einval(lib.cadm_icem_track_best(ctx, P, I, P, 0, N, P, P, None), "cadm_icem_track_best", "bad arguments")
    assert lib.cadm_icem_workspace_bytes(ctx, 0, N, K) == 0 and lib.cadm_icem_workspace_bytes(ctx, M, N, -1) == 0
    assert lib.cadm_icem_workspace_bytes(ctx, M, N, K) > lib.cadm_icem_workspace_bytes(ctx, M, N, 0) > 0

    def plan(prm, c=ctx, n=N, carry=P, valid=I, cp=P):
        return lib.cadm_icem_plan(c, ct.byref(prm), P, cp, cp, P, P, carry, valid, M, n, 0, 1, P, P, None, None)
    einval(plan(HipEngine.icem_params(keep_elites=KE + 1)), "cadm_icem_plan", "keep_elites")
    einval(plan(HipEngine.icem_params(decay=0.9)), "cadm_icem_plan", "decay")
    einval(plan(HipEngine.icem_params(noise_beta=-1.0)), "cadm_icem_plan", "noise_beta")
    einval(plan(HipEngine.icem_params(keep_elites=K), carry=None), "cadm_icem_plan", "carry")
    einval(plan(HipEngine.icem_params(), n=KE - 1), "cadm_icem_plan", "num_elites")
    einval(plan(HipEngine.icem_params(), cp=None), "cadm_icem_plan", "cp_obs/cp_act")
    einval(lib.cadm_icem_plan(ctx, None, P, P, P, P, P, P, I, M, N, 0, 1, P, P, None, None), "cadm_icem_plan", "bad arguments")
    # discrete actions
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=M, H=5, seed=1, hidden_sizes=HID)
    deng = make_engine(dprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    einval(plan(HipEngine.icem_params(), c=deng._ctx), "cadm_icem_plan", "continuous actions only")
    einval(lib.cadm_sample_actions_colored(deng._ctx, P, P, None, 1.0, 0, 0, 0, M, N, P, None), "cadm_sample_actions_colored", "continuous")
    # a candidate-sharded ctx (a host-supplied all-gather registered for two ranks; it is never called)
    _, seng = _engine(5)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(seng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    einval(plan(HipEngine.icem_params(), c=seng._ctx), "cadm_icem_plan", "sharded")
    assert lib.cadm_dist_destroy(seng._ctx) == 0
    # the engine is usable afterwards
    out = _np(eng.icem_plan(HipEngine.icem_params(noise_beta=1.0), prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N,
                            seed=1, call=1))
    assert np.isfinite(out).all() and np.abs(out).max() <= 1.0
