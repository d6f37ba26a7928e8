"""CPU: the restatements of the log-density of given actions (tests/policy_logp_ref.py) against torch.distributions, against each other
under `bars()`, and around the sampler of tests/gauss_policy_ref.py; and every refusal of `cem_policy_logp` that needs no engine."""
import numpy as np
import pytest
import torch
from torch.distributions import AffineTransform, Normal, TanhTransform, TransformedDistribution

import gauss_policy_ref as gref
import policy_logp_ref as lref
from cadm_amd import _lib
from cadm_amd import planner as _planner
from cadm_amd.engine import HipEngine
from cadm_amd.planner import PlanOptions

F = np.float32
D, A, HID, R = 7, 3, (16, 12), 257
LO, HI = -5.0, 2.0
CASES = [(sq, bd) for sq in ("tanh", "none") for bd in gref.BOUNDS]


def setup(squash, bound, lb=-1.0, ub=1.0, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (R, D)).astype(F)
    layers = gref.actor(D, HID, A, "relu", x, LO, HI, seed=seed)
    mid, half = 0.5 * (ub + lb), 0.5 * (ub - lb)
    act = (mid + half * rng.uniform(-0.97, 0.97, (R, A))).astype(F)      # interior actions
    return x, layers, act


@pytest.mark.parametrize("squash,bound", CASES)
@pytest.mark.parametrize("lb,ub", [(-1.0, 1.0), (-0.5, 2.0)])
def test_float64_restatement_is_torch_distributions(squash, bound, lb, ub):
    x, layers, act = setup(squash, bound, lb, ub)
    z = gref.z64(x, layers, "relu")
    ref = lref.logp64(z, act, squash, bound, LO, HI, lb, ub)
    mu, sig = torch.from_numpy(z[:, :A]), torch.from_numpy(ref["sig"])
    base = Normal(mu, sig)
    mid, half = (float(v) for v in gref._mid_half(lb, ub))
    dist = TransformedDistribution(base, [TanhTransform(), AffineTransform(mid, half)]) if squash == "tanh" else base
    want = dist.log_prob(torch.from_numpy(act.astype(np.float64))).sum(-1).numpy()
    assert np.abs(ref["logp"] - want).max() <= 1e-9 * np.maximum(1.0, np.abs(want)).max()
    # pre_squash: the Gaussian's own density of u
    pre = lref.logp64(z, act, squash, bound, LO, HI, lb, ub, space="pre_squash")
    want_pre = base.log_prob(torch.from_numpy(ref["u"])).sum(-1).numpy()
    assert np.abs(pre["logp"] - want_pre).max() <= 1e-9 * np.maximum(1.0, np.abs(want_pre)).max()
    if squash == "none":
        assert np.array_equal(pre["logp"], ref["logp"])


@pytest.mark.parametrize("squash,bound", CASES)
@pytest.mark.parametrize("space", lref.SPACES)
def test_float32_restatement_under_bars(squash, bound, space):
    x, layers, act = setup(squash, bound)
    act[::7, 0] = 1.0            # on a bound, and beyond it: the clamp
    act[3::11, 1] = -1.0
    act[5::13, 2] = 1.75
    z, zf = gref.z64(x, layers, "relu"), gref.z32(x, layers, "relu")
    ref = lref.logp64(z, act, squash, bound, LO, HI, space=space, y=lref.y32(act) if squash == "tanh" else None)
    got = lref.logp32(zf, act, squash, bound, LO, HI, space=space)
    bar = lref.bars(z, ref, squash, bound, LO, HI, space=space)
    ratio = np.abs(got["logp"].astype(np.float64) - ref["logp"]) / bar
    print("float32 restatement %s %s %s: worst |err| / bar = %.3f" % (squash, bound, space, ratio.max()))
    assert np.isfinite(ref["logp"]).all() and ratio.max() <= 1.0
    if squash == "tanh":         # a clamped element sits at atanh(YMAX)
        assert abs(abs(ref["u"][0, 0]) - np.arctanh(float(lref.YMAX))) < 1e-9 and abs(ref["u"][5, 2] - ref["u"][0, 0]) == 0.0


def test_nonfinite_actions_are_nan_in_both():
    x, layers, act = setup("tanh", "clamp")
    act[4, 1], act[9, 0] = np.inf, np.nan
    z = gref.z64(x, layers, "relu")
    for got in (lref.logp64(z, act, "tanh", "clamp", LO, HI)["logp"], lref.logp32(z.astype(F), act, "tanh", "clamp", LO, HI)["logp"]):
        assert np.isnan(got[[4, 9]]).all() and np.isfinite(np.delete(got, [4, 9])).all()


@pytest.mark.parametrize("squash,bound", CASES)
def test_round_trip_through_the_sampler(squash, bound):
    """log pi of the sampler's own actions is the sampler's logp, element by element, where the inverse squash is well conditioned"""
    rng = np.random.default_rng(11)
    lb, ub = (-1.0, 1.0) if squash == "tanh" else (-64.0, 64.0)     # (no squash: bounds the draws do not reach, the clip is no part of the density)
    mu = rng.normal(0.0, 0.7, (R, A))
    l = rng.normal(-1.0, 1.0, (R, A))
    z = np.concatenate([mu, l], axis=-1)
    xi = rng.normal(0.0, 1.0, (R, A)).astype(F)
    s = gref.sample64(z, xi, squash, bound, LO, HI, lb, ub)
    act = s["act"].astype(F)                                       # what the kernel stores
    ref = lref.logp64(z, act, squash, bound, LO, HI, lb, ub)
    keep = np.abs(s["u"]) <= 2.0
    assert keep.mean() >= 0.9, "more than 10 %% of the elements fall outside |u| <= 2 (%.3f kept)" % keep.mean()
    bar = lref.roundtrip_bars(z, ref, act, squash, bound, LO, HI, lb, ub)
    gap = np.abs(ref["term"] - s["term"])
    print("round trip %s %s: kept %.3f, worst gap %.3g, worst gap / bar %.3f" % (squash, bound, keep.mean(), gap[keep].max(),
                                                                              (gap / bar)[keep].max()))
    assert (gap[keep] <= bar[keep]).all()
    if squash == "none":
        assert (gap <= bar).all()


def test_step_sum_restatement():
    rng = np.random.default_rng(0)
    steps = rng.normal(0, 3, (4, 2, 3, 5)).astype(F)
    first = rng.integers(0, 6, (2, 3, 5))
    rows = rng.normal(0, 1, (2, 3, 5)).astype(F)
    S, out = lref.step_sum32(steps, first, -0.37, rows)
    q = (1, 2, 3)
    want = F(0)
    for t in range(min(int(first[q]), 3) + 1):
        want = F(want + steps[(t,) + q])
    assert S[q] == want and out[q] == F(rows[q] + F(F(-0.37) * want))


# ---------------------------------------------------------------------------------------------------------------------- the options
ACTOR = dict(hidden_sizes=(8,), activation="tanh", squash="tanh")


def test_options_accept():
    assert PlanOptions.from_kwargs(cem_policy_logp=None) is None and PlanOptions.from_kwargs(use_cem=True, cem_policy_logp=None) is None
    opt = PlanOptions.from_kwargs(use_cem=True, cem_policy_logp=dict(weight=0.5, space="pre_squash", policy=ACTOR), obs_dim=D, action_dim=A)
    assert opt.logp == (0.5, "pre_squash", ((8,), "tanh", "tanh")) and opt.policy_params is None and opt.critic_params is None
    assert isinstance(opt.logp_params, _lib.PolicyLogpParams) and opt.logp_params.weight == 0.5 and opt.logp_params.space == 1
    ap = opt.actor_params()
    assert (ap.n_hidden, ap.hidden[0], ap.squash, ap.n_samples) == (1, 8, _lib.POLICY_SQUASH["tanh"], 1)
    # one actor: the prior's, or the critics'
    prior = dict(ACTOR, n_samples=2)
    opt = PlanOptions.from_kwargs(use_cem=True, cem_policy_prior=prior, cem_policy_logp=dict(weight=2))
    assert opt.logp == (2.0, "action", ((8,), "tanh", "tanh")) and opt.actor_params() is opt.policy_params
    opt = PlanOptions.from_kwargs(use_cem=True, cem_terminal_q=dict(hidden_sizes=(4,), policy=ACTOR), cem_policy_logp=dict(policy=ACTOR))
    assert opt.logp[2] == opt.critic[5]
    # every other field is what it is without the kwarg
    base = PlanOptions.from_kwargs(use_cem=True, cem_policy_prior=prior)
    with_ = PlanOptions.from_kwargs(use_cem=True, cem_policy_prior=prior, cem_policy_logp=dict())
    for k in PlanOptions._fields:
        if k not in ("logp", "logp_params", "params", "policy_params"):
            assert getattr(base, k) == getattr(with_, k), k
    # the model's check against its head
    head = _planner.policy_head_params(dict(log_std_bounds=(-5.0, 2.0)), has_actor=True)
    assert _planner.policy_logp_setting(None) is None and _planner.policy_logp_setting(base, head_declared=False) is None
    assert _planner.policy_logp_setting(with_, head_declared=True, head=head) is with_.logp_params


@pytest.mark.parametrize("kw,err,match", [
    (dict(cem_policy_logp=dict(policy=ACTOR), use_cem=False), ValueError, "need use_cem=True"),
    (dict(cem_policy_logp=3.0), ValueError, "cem_policy_logp must be dict"),
    (dict(cem_policy_logp=dict(beta=1.0, policy=ACTOR)), ValueError, "cem_policy_logp must be dict"),
    (dict(cem_policy_logp=dict(space="latent", policy=ACTOR)), ValueError, "space must be"),
    (dict(cem_policy_logp=dict(space=2, policy=ACTOR)), ValueError, "space must be"),
    (dict(cem_policy_logp=dict(space=True, policy=ACTOR)), ValueError, "space must be"),
    (dict(cem_policy_logp=dict(weight=float("nan"), policy=ACTOR)), ValueError, "weight must be a finite number"),
    (dict(cem_policy_logp=dict(weight=float("inf"), policy=ACTOR)), ValueError, "weight must be a finite number"),
    (dict(cem_policy_logp=dict(weight=1e39, policy=ACTOR)), ValueError, "weight must be a finite number"),
    (dict(cem_policy_logp=dict(weight=True, policy=ACTOR)), ValueError, "weight must be a finite number"),
    (dict(cem_policy_logp=dict(weight="1", policy=ACTOR)), ValueError, "weight must be a finite number"),
    (dict(cem_policy_logp=dict()), ValueError, "cem_policy_logp needs policy="),
    (dict(cem_policy_logp=dict(policy=dict(ACTOR, n_samples=2))), ValueError, "policy must be dict"),
    (dict(cem_policy_logp=dict(policy=dict(ACTOR, squash="sigmoid"))), ValueError, "policy squash must be"),
    (dict(cem_policy_logp=dict(policy=dict(ACTOR, hidden_sizes=(9,))), cem_policy_prior=dict(ACTOR, n_samples=2)), ValueError,
     "does not agree with the actor"),
    (dict(cem_policy_logp=dict(policy=dict(ACTOR, squash="none")), cem_terminal_q=dict(hidden_sizes=(4,), policy=ACTOR)), ValueError,
     "does not agree with the actor"),
    (dict(cem_policy_logp=dict(policy=ACTOR), obs_dim=_lib.MAX_VALUE_DIMS + 1), ValueError, "observation dims"),
    (dict(cem_policy_logp=dict(policy=ACTOR), action_dim=_lib.MAX_POLICY_ACTIONS + 1), ValueError, "action dims"),
    (dict(cem_policy_logp=dict(policy=ACTOR), discrete=True), NotImplementedError, "discrete"),
])
def test_options_refuse(kw, err, match):
    kw = dict(dict(use_cem=True), **kw)
    with pytest.raises(err, match=match):
        PlanOptions.from_kwargs(**kw)


def test_options_refuse_more_than_one_rank(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="more than"):
        PlanOptions.from_kwargs(use_cem=True, cem_policy_logp=dict(policy=ACTOR), process_group=object())


def test_setting_needs_a_head_within_the_kernel_range():
    opt = PlanOptions.from_kwargs(use_cem=True, cem_policy_logp=dict(policy=ACTOR))
    with pytest.raises(ValueError, match="declare policy_head"):
        _planner.policy_logp_setting(opt, head_declared=False)
    low = _planner.policy_head_params(dict(log_std_bounds=(-10.5, 2.0)), has_actor=True)
    with pytest.raises(ValueError, match="below -10"):
        _planner.policy_logp_setting(opt, head_declared=True, head=low)
    edge = _planner.policy_head_params(dict(log_std_bounds=(-10.0, 2.0)), has_actor=True)
    assert _planner.policy_logp_setting(opt, head_declared=True, head=edge) is opt.logp_params
    # the head's own declaration needs an actor: cem_policy_logp's counts
    assert opt.actor_params() is not None


def test_engine_params():
    p = HipEngine.policy_logp_params()
    assert (p.weight, p.space) == (1.0, _lib.LOGP_SPACES["action"])
    p = HipEngine.policy_logp_params(-0.37, "pre_squash")
    assert (p.weight, p.space) == (float(F(-0.37)), 1) and HipEngine.policy_logp_params(0, 1).space == 1
    assert float(F(_lib.LOGP_YMAX)) == float(lref.YMAX)
    import ctypes
    assert ctypes.sizeof(_lib.PolicyLogpParams) == 8
