"""CPU: the numpy restatement of the terminal value from Q critics (tests/critic_ref.py) is consistent with itself -- the float32
chain against the float64 statement at the bar the GPU tests hold the kernel to, the reduce orders, the NaN and `first` rules -- and
`PlanOptions.from_kwargs` accepts and refuses `cem_terminal_q` as INTEGRATION.md ("Terminal value from Q critics") says."""
import numpy as np
import pytest

import behind_rollout as br
import critic_ref as cref
import policy_ref as pref
import value_ref as vref
from cadm_amd import _lib
from cadm_amd.engine import HipEngine
from cadm_amd.planner import PlanOptions
from helpers import assert_close, floored_rel

F = np.float32
D, A = 11, 3


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _case(hidden, phidden, C, seed, squash="tanh", act="relu", stats=True):
    rng = np.random.default_rng(seed)
    states = (1.5 * rng.standard_normal((37, D))).astype(F)
    actor = dict(layers=pref.he_policy(D, phidden, A, seed + 1, out_scale=0.5), act=act, squash=squash)
    mean = std = None
    if stats:
        actor.update(mean=(0.3 * rng.standard_normal(D)).astype(F), std=rng.uniform(0.5, 2.0, D).astype(F))
        mean, std = (0.3 * rng.standard_normal(D + A)).astype(F), rng.uniform(0.5, 2.0, D + A).astype(F)
    critics = cref.he_critics(D, A, hidden, C, seed + 2)
    return states, actor, critics, mean, std


@pytest.mark.parametrize("hidden", [(), (48,), (64, 48, 200)])
@pytest.mark.parametrize("phidden", [(), (64, 48)])
@pytest.mark.parametrize("reduce", cref.REDUCES)
def test_emulate32_against_q64(hidden, phidden, reduce):
    for ai, act in enumerate(cref.ACTS):
        for squash in pref.SQUASH:
            states, actor, critics, mean, std = _case(hidden, phidden, 3, 10 + ai, squash, act)
            cref.check_live(states, critics, act, actor, mean, std, what="%r %r %s %s" % (hidden, phidden, act, squash))
            q, each = cref.q64(states, critics, act, reduce, actor, mean=mean, std=std, want_each=True)
            g, geach, a = cref.emulate32(states, critics, act, reduce, actor, mean=mean, std=std, want_each=True, want_action=True)
            assert g.dtype == F and geach.shape == (3, 37) and a.shape == (37, A)
            assert_close(geach, each, what="each")
            assert_close(g, q, what="%s of %r behind %r, %s, %s" % (reduce, hidden, phidden, act, squash))
            assert np.abs(a).max() <= 1.0
            # given the actor's own float32 action, the chain behind it has the same bits
            np.testing.assert_array_equal(_bits(cref.emulate32(states, critics, act, reduce, actions=a, mean=mean, std=std)), _bits(g))


@pytest.mark.parametrize("act", cref.ACTS)
def test_the_gpu_kernel_cases_are_live(act):
    """every case of tests/test_gpu_critic.py::test_kernel_against_restatement meets the liveness conditions, and the float32 chain meets
    the float64 statement on it at the bar the kernel is held to"""
    gi = 0
    for hidden in cref.KERNEL_CRITICS:
        for phidden in cref.KERNEL_ACTORS:
            for C, reduce, squash in cref.KERNEL_COMBOS:
                gi += 1
                states = cref.kernel_states(3, 11, 30 + gi)[1]
                actor, critics, mean, std = cref.kernel_case(states, A, hidden, phidden, C, act, squash, 10 + gi)
                what = "%s %r behind %r, C = %d, %s, %s" % (act, hidden, phidden, C, reduce, squash)
                cref.check_live(states, critics, act, actor, mean, std, what=what)
                if gi % 7 == 0:
                    assert_close(cref.emulate32(states, critics, act, reduce, actor, mean=mean, std=std),
                                 cref.q64(states, critics, act, reduce, actor, mean=mean, std=std), what=what)


ENVELOPE = [(name, act) for name in br.CRITIC_ROWS for act in cref.ACTS]


@pytest.mark.parametrize("name,act", ENVELOPE, ids=["%s-%s" % c for c in ENVELOPE])
def test_the_envelope_cases_are_live(name, act):
    """every `critic_ref.ENVELOPE_CASES` entry of tests/test_gpu_critic_envelope.py::test_kernel, on every engine it runs on, meets the
    liveness conditions (a dead net or a saturated squash would pass anything on the GPU), and the float32 chain meets the float64
    statement on it at the bar the kernel is held to, for q and for every critic's q"""
    _, D, A = br.TERM_ENGINES[name][:3]
    m, n = br.CRITIC_ROWS[name][0]
    low = dict(units=1.0, unsaturated=1.0, action=np.inf)
    worst = 0.0
    for gi, (hidden, phidden, C, reduce, squash) in enumerate(cref.ENVELOPE_CASES, 1):
        states = cref.kernel_states(m, n, 30 + gi, name=name)[1]
        assert states.shape[1] == D
        actor, critics, mean, std = cref.kernel_case(states, A, hidden, phidden, C, act, squash, 10 + gi)
        what = "%s %s %r behind %r, C = %d, %s, %s" % (name, act, hidden, phidden, C, reduce, squash)
        live = cref.check_live(states, critics, act, actor, mean, std, what=what)
        low = {k: min(v, live[k]) for k, v in low.items()}
        ref, ref_each = cref.q64(states, critics, act, reduce, actor, mean=mean, std=std, want_each=True)
        got, each = cref.emulate32(states, critics, act, reduce, actor, mean=mean, std=std, want_each=True)
        worst = max(worst, floored_rel(got, ref) / 1e-5, floored_rel(each, ref_each) / 1e-5)
        assert_close(got, ref, what=what)
        assert_close(each, ref_each, what=what + ": each")
    print("\n[%s %s] smallest live share %.2f, unsaturated share %.2f, action effect %.3g; worst |emulate32 - q64| / (1e-5 of scale) %.3f"
          % (name, act, low["units"], low["unsaturated"], low["action"], worst))


def test_the_envelope_cases_cover_what_they_name():
    cases = cref.ENVELOPE_CASES
    assert len(cases) == 18 and {c[0] for c in cases} == set(cref.ENVELOPE_CRITICS) and {c[1] for c in cases} == set(cref.ENVELOPE_ACTORS)
    assert {c[2] for c in cases} == {1, 4, 5} and {c[3] for c in cases} == set(cref.REDUCES) and {c[4] for c in cases} == set(pref.SQUASH)
    for phidden in cref.ENVELOPE_ACTORS:      # every actor depth meets every C, both reduces and both squashes
        mine = [c for c in cases if c[1] == phidden]
        assert {c[2] for c in mine} == {1, 4, 5} and {c[3] for c in mine} == set(cref.REDUCES) and {c[4] for c in mine} == set(pref.SQUASH)
    assert any(len(c[0]) == 4 and len(c[1]) == 4 and c[2] == 5 for c in cases), "four hidden layers under five dense ones at C = 5"
    for name, rows in br.CRITIC_ROWS.items():
        p = br.TERM_ENGINES[name][4]
        assert all((m * n * p) % 16 for m, n in rows) and rows[0][0] * rows[0][1] * p > 16 > rows[1][0] * rows[1][1] * p, name


def test_reduce_orders():
    each = np.array([[1.0, 3.0, F(0.1), -2.0], [2.0, -1.0, F(0.2), -2.0], [0.5, 7.0, F(0.3), F(1e-8)]], F)
    np.testing.assert_array_equal(cref.reduce32(each, "min"), np.array([0.5, -1.0, F(0.1), -2.0], F))
    want = ((each[0] + each[1]) + each[2]) / F(3)
    assert want.dtype == F
    np.testing.assert_array_equal(_bits(cref.reduce32(each, "mean")), _bits(want))
    # C = 1: no division, the critic's own bits under both reduces
    for reduce in cref.REDUCES:
        np.testing.assert_array_equal(_bits(cref.reduce32(each[:1], reduce)), _bits(each[0]))
    # the order matters in float32, and it is the ascending one
    big = np.array([[F(1e8)], [F(1.0)], [F(-1e8)]], F)
    assert cref.reduce32(big, "mean")[0] == F(0.0) and cref.reduce32(big[[0, 2, 1]], "mean")[0] == F(1.0) / F(3)
    assert_close(cref.reduce32(each, "mean"), cref.reduce64(each.astype(np.float64), "mean"))
    np.testing.assert_array_equal(cref.reduce32(each, "min"), cref.reduce64(each.astype(np.float64), "min").astype(F))


@pytest.mark.parametrize("reduce", cref.REDUCES)
def test_two_identical_critics_are_the_single_critic(reduce):
    states, actor, critics, mean, std = _case((64, 48), (64, 48), 1, 5)
    one = cref.emulate32(states, critics, "relu", reduce, actor, mean=mean, std=std)
    two = cref.emulate32(states, critics * 2, "relu", reduce, actor, mean=mean, std=std)
    np.testing.assert_array_equal(_bits(two), _bits(one))      # min(q, q) = q; (q + q) / 2 = q exactly
    np.testing.assert_array_equal(cref.q64(states, critics * 2, "relu", reduce, actor, mean=mean, std=std),
                                  cref.q64(states, critics, "relu", reduce, actor, mean=mean, std=std))


def test_zero_action_rows_give_the_value_net():
    rng = np.random.default_rng(3)
    states = rng.standard_normal((20, D)).astype(F)
    v_layers = vref.he_net(D, (48, 32), 4)
    smean, sstd = rng.standard_normal(D).astype(F), rng.uniform(0.5, 2.0, D).astype(F)
    critic = cref.critic_from_value(v_layers, D, A)
    mean, std = np.concatenate([smean, rng.standard_normal(A).astype(F)]), np.concatenate([sstd, rng.uniform(0.5, 2.0, A).astype(F)])
    actor = dict(layers=pref.he_policy(D, (16,), A, 5), act="tanh")
    q = cref.emulate32(states, [critic], "tanh", "min", actor, mean=mean, std=std)
    np.testing.assert_array_equal(q, vref.emulate32(states, v_layers, "tanh", smean, sstd))      # as numbers: +-0 is the only licence


def test_nan_and_first_rules():
    states, actor, critics, mean, std = _case((48,), (16,), 2, 7)
    clean = cref.emulate32(states, critics, "relu", "min", actor, mean=mean, std=std)
    bad = states.copy()
    bad[3, 2], bad[5, 0], bad[36, D - 1] = np.nan, np.inf, -np.inf
    hit = np.zeros(37, bool)
    hit[[3, 5, 36]] = True
    q, each, a = cref.emulate32(bad, critics, "relu", "min", actor, mean=mean, std=std, want_each=True, want_action=True)
    assert np.isnan(q[hit]).all() and np.isnan(each[:, hit]).all() and np.isnan(cref.q64(bad, critics, "relu", "min", actor, mean=mean, std=std)[hit]).all()
    np.testing.assert_array_equal(_bits(q[~hit]), _bits(clean[~hit]))
    assert (a[hit] == pref.fallback(-1.0, 1.0)).all()      # what act_out shows; no Q is computed from it
    acts = np.zeros((37, A), F)
    acts[8, 1] = np.nan
    assert np.isnan(cref.emulate32(states, critics, "relu", "mean", actions=acts, mean=mean, std=std)[8])
    rows = np.random.default_rng(1).standard_normal(37).astype(F)
    first = np.full(37, 3, np.int32)
    first[[0, 3, 9]] = [0, 2, 1]
    out = cref.update(rows, q, 0.7, first, 3)
    np.testing.assert_array_equal(_bits(out[[0, 3, 9]]), _bits(rows[[0, 3, 9]]))      # first < H: the input bits, NaN state or not
    assert np.isnan(out[5]) and np.isnan(out[36]) and np.isnan(cref.cut(q, first, 3)[[0, 3, 9]]).all()
    live = ~hit & (first >= 3)
    np.testing.assert_array_equal(_bits(out[live]), _bits((rows + F(0.7) * q)[live]))


# ---------------------------------------------------------------------------------------------------------------------- from_kwargs
POL = dict(hidden_sizes=(32,), activation="tanh", squash="tanh")


def _opt(**kw):
    return PlanOptions.from_kwargs(use_cem=True, obs_dim=18, action_dim=6, **kw)


def test_from_kwargs_accepts():
    assert PlanOptions.from_kwargs() is None and _opt() is None and _opt(cem_terminal_q=None) is None
    # the new fields sit in front of the policy ones: existing tests pin the places of everything behind them, counted from the end
    assert PlanOptions._fields[-13:-11] == ("critic", "critic_params") and PlanOptions._fields[-11:-9] == ("policy", "policy_params")
    assert PlanOptions(*range(18)).critic_params is None and PlanOptions(*range(18)).critic is None and PlanOptions(*range(18)).action_advance == 17
    opt = _opt(cem_terminal_q=dict(policy=POL))
    assert opt.critic == ((256, 256), "relu", 2, "min", 1.0, ((32,), "tanh", "tanh"))
    q = opt.critic_params
    assert isinstance(q, _lib.CriticParams) and (q.n_hidden, q.hidden[0], q.hidden[1], q.activation, q.n_critics, q.reduce, q.weight) == \
        (2, 256, 256, 0, 2, 0, 1.0)
    assert opt.policy is None and opt.policy_params is None and opt.value_params is None
    a = opt.actor_params()
    assert (a.n_hidden, a.hidden[0], a.activation, a.squash, a.n_samples, a.noise_std) == (1, 32, 1, 1, 1, 0.0)
    opt = _opt(cem_terminal_q=dict(hidden_sizes=(), activation="swish", n_critics=5, reduce="mean", weight=-0.5, policy=dict(POL, squash="none")))
    assert opt.critic == ((), "swish", 5, "mean", -0.5, ((32,), "tanh", "none"))
    # with a policy prior: `policy` may be left out, the actor is that net; given both, they must agree
    prior = dict(hidden_sizes=(32,), activation="tanh", squash="tanh", n_samples=4)
    opt = _opt(cem_terminal_q=dict(n_critics=1), cem_policy_prior=prior)
    assert opt.critic[5] == ((32,), "tanh", "tanh") and opt.actor_params() is opt.policy_params and opt.policy_params.n_samples == 4
    assert _opt(cem_terminal_q=dict(policy=POL), cem_policy_prior=prior).critic[5] == ((32,), "tanh", "tanh")
    assert _opt(cem_policy_prior=prior).critic_params is None and _opt(cem_policy_prior=prior).actor_params().n_samples == 4
    assert _opt(cem_noise_beta=1.0).actor_params() is None


@pytest.mark.parametrize("bad,match", [
    (dict(policy=POL, hidden_sizes=(8,) * 5), "at most 4 hidden"), (dict(policy=POL, hidden_sizes=(0,)), "hidden widths"),
    (dict(policy=POL, hidden_sizes=(513,)), "hidden widths"), (dict(policy=POL, activation="gelu"), "activation"),
    (dict(policy=POL, n_critics=0), "n_critics"), (dict(policy=POL, n_critics=6), "n_critics"), (dict(policy=POL, n_critics=True), "n_critics"),
    (dict(policy=POL, reduce="max"), "reduce"), (dict(policy=POL, weight=float("nan")), "weight"), (dict(policy=POL, weight=float("inf")), "weight"),
    (dict(policy=POL, wieght=1.0), "cem_terminal_q must be"), ("min", "cem_terminal_q must be"), (dict(), "needs policy"),
    (dict(policy=dict(POL, n_samples=3)), "policy must be"), (dict(policy=dict(POL, squash="clip")), "squash"),
])
def test_from_kwargs_refuses(bad, match):
    with pytest.raises(ValueError, match=match):
        _opt(cem_terminal_q=bad)


def test_from_kwargs_refuses_in_context():
    tq = dict(policy=POL)
    with pytest.raises(ValueError, match="one terminal term"):
        _opt(cem_terminal_q=tq, cem_terminal_value=dict(hidden_sizes=(8,)))
    with pytest.raises(ValueError, match="need use_cem=True"):
        PlanOptions.from_kwargs(cem_terminal_q=tq)
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        PlanOptions.from_kwargs(use_cem=True, discrete=True, cem_terminal_q=tq)
    for prior in (dict(POL, hidden_sizes=(33,)), dict(POL, activation="relu"), dict(POL, squash="none")):
        with pytest.raises(ValueError, match="does not agree"):
            _opt(cem_terminal_q=tq, cem_policy_prior=dict(prior, n_samples=2))
    with pytest.raises(ValueError, match="observation dims"):
        PlanOptions.from_kwargs(use_cem=True, obs_dim=129, action_dim=6, cem_terminal_q=tq)
    with pytest.raises(ValueError, match="action dims"):
        PlanOptions.from_kwargs(use_cem=True, obs_dim=18, action_dim=65, cem_terminal_q=tq)
    assert HipEngine.critic_params((4,), 2, 3, 1, 0.5).reduce == 1      # the CADM_* numbers are taken too
