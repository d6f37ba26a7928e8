"""CPU: what the plan companions of `MLPEnsembleCEMDynamicsModel` must keep, whatever their bodies share -- `uncertainty_cost`,
`tracking_cost`, `plan_terminal_value`, `plan_terminal_q`, `plan_rewards`, `plan_returns` and `constraint_check` on a model that holds
only the attributes they read and an engine that records every call: the calls and their order, the key of the replay (seed, the
last get_action's call, the forecast's iteration word), the TERMINATE cut, which rows every stage receives under a discount, and the
result dict with and without the n axis.  `policy_proposals` and `forecast`, which share the key and the context handling, likewise.

Then the refusals of the four caller-supplied nets (value, reward, policy, critics) and of `_plan_opt_in`, text for text.  The models
there are `object.__new__(Model)` with `_opt` (and the `_*_set` flags where a net is asked for) alone: a refusal that reached for the
engine, or for any other state, would fail on the missing attribute."""
import inspect
import sys

import numpy as np
import pytest
import torch

from cadm_amd import planner
from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as Model
from cadm_amd.engine import HipEngine
from cadm_amd.planner import PlanOptions

M, N, H, A, D, P, HH, E, C = 2, 3, 3, 2, 5, 4, 2, 2, 3
SEED, CALL = (1 << 32) + 5, (2 << 32) + 7      # wider than the 32 bits that key a replay


class Engine:
    """stands where the HipEngine stands: every call is kept as (name, its bound arguments) and answers with CPU tensors of the right
    shape whose values tell the calls apart (the k-th answer starts at 1000 k)"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls, self.D, self.A = [], D, A

    def _t(self, x, dtype=torch.float32):
        return torch.as_tensor(np.ascontiguousarray(x) if not isinstance(x, torch.Tensor) else x).to(dtype).contiguous()

    def _rec(self, **kw):
        self.calls.append((sys._getframe(1).f_code.co_name, kw))
        return len(self.calls)

    def _f(self, k, *shape):
        return torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape) + 1000.0 * k

    def names(self):
        return [c[0] for c in self.calls]

    def only(self, name):
        got = [kw for n, kw in self.calls if n == name]
        assert len(got) == 1, (name, self.names())
        return got[0]

    def set_stats(self, stats):
        self._rec(stats=stats)

    def uncertainty_params(self, kind, weight, w=None, form="var", cap=None, obs_dim=None):
        prm = HipEngine.uncertainty_params(kind, weight, w, form, cap, obs_dim=obs_dim)
        self._rec(w=w, obs_dim=obs_dim, result=prm)
        return prm

    def context_forward(self, cp_obs, cp_act):
        k = self._rec(cp_obs=cp_obs, cp_act=cp_act)
        return self._f(k, E, np.shape(cp_obs)[0], C)

    def rollout_returns(self, obs, ctx_vec, actions, seed=0, call=0, it=0, want_traj=False):
        k = self._rec(obs=obs, ctx_vec=ctx_vec, actions=actions, seed=seed, call=call, it=it, want_traj=want_traj)
        m, n = actions.shape[:2]
        self.rows, self.traj = self._f(k, m, n, P), self._f(k, H, m, n, P, D)
        return self.rows, self.traj

    def constrain_returns(self, traj, rows, constraints, mode="penalty", weight=None, obs=None, actions=None, out=None):
        k = self._rec(traj=traj, rows=rows, constraints=constraints, obs=obs, actions=actions)
        ints = torch.arange(rows.numel(), dtype=torch.int32).reshape(rows.shape)
        self.first = ints % (H + 1)
        return self._f(k, *rows.shape), self.first, ints % 3

    def discount_returns(self, traj, obs, actions, rows, want_steps=False, out=None):
        k = self._rec(traj=traj, obs=obs, actions=actions, rows=rows, want_steps=want_steps)
        self.discounted = self._f(k, *rows.shape)
        return (self.discounted, self._f(k, H, *rows.shape)) if want_steps else self.discounted

    def discount_weights(self):
        self._rec()
        return np.float32(0.5) ** np.arange(H + 1, dtype=np.float32)

    def uncertainty_cost(self, traj, params, first=None, want_steps=False):
        k = self._rec(traj=traj, params=params, first=first, want_steps=want_steps)
        m, n = traj.shape[1:3]
        return (self._f(k, m, n, H), self._f(k, m, n) + 0.5) if want_steps else self._f(k, m, n) + 0.5

    def tracking_returns(self, traj, rows, track, targets, offset=None, first=None, out=None, want_cost=False):
        k = self._rec(traj=traj, rows=rows, track=track, targets=targets, offset=offset, first=first, want_cost=want_cost)
        return (self._f(k, *rows.shape), self._f(k, *rows.shape) + 0.5) if want_cost else self._f(k, *rows.shape)

    def value_returns(self, traj, rows, params, first=None, want_v=False, out=None):
        k = self._rec(traj=traj, rows=rows, params=params, first=first, want=want_v)
        return (self._f(k, *rows.shape), self._f(k, *rows.shape) + 0.5) if want_v else self._f(k, *rows.shape)

    def critic_returns(self, traj, rows, params, first=None, want_q=False, out=None):
        k = self._rec(traj=traj, rows=rows, params=params, first=first, want=want_q)
        return (self._f(k, *rows.shape), self._f(k, *rows.shape) + 0.5) if want_q else self._f(k, *rows.shape)

    def reward_returns(self, traj, obs, actions, rows, params, first=None, want_steps=False, out=None):
        k = self._rec(traj=traj, obs=obs, actions=actions, rows=rows, params=params, first=first, want=want_steps)
        return (self._f(k, *rows.shape), self._f(k, H, *rows.shape), self._f(k, *rows.shape) + 0.5) if want_steps else self._f(k, *rows.shape)

    def policy_propose(self, params, obs, ctx_vec=None, seed=0, call=0, want_states=False):
        k = self._rec(params=params, obs=obs, ctx_vec=ctx_vec, seed=seed, call=call, want_states=want_states)
        m, n = obs.shape[0], params.n_samples
        return (self._f(k, m, n, H, A), self._f(k, H, m, n, P, D)) if want_states else self._f(k, m, n, H, A)

    def plan_forecast(self, obs, cp_obs, cp_act, actions, band_k=1, eps=None, seed=0, call=0):
        k = self._rec(obs=obs, cp_obs=cp_obs, cp_act=cp_act, actions=actions, band_k=band_k, seed=seed, call=call)
        m, n = actions.shape[:2]
        out = {key: self._f(k, m, n, H, D) for key in ("mean", "var_total", "var_epistemic", "var_aleatoric", "lo", "hi")}
        out.update(member_mean=self._f(k, E, m, n, H, D), reward_mean=self._f(k, m, n, H), reward_var=self._f(k, m, n, H),
                   reward_member=self._f(k, E, m, n, H), returns=self._f(k, m, n, P), rollout_returns=self._f(k, m, n, P),
                   diverged_step=torch.full((m, n), H, dtype=torch.int32))
        return out

    # the four nets: what a model registers and evaluates
    def set_value_net(self, params, weights=None, obs_mean=None, obs_std=None):
        self._rec(params=params, weights=weights, mean=obs_mean, std=obs_std)

    def set_reward_net(self, params, weights=None, in_mean=None, in_std=None):
        self._rec(params=params, weights=weights, mean=in_mean, std=in_std)

    def set_policy_net(self, params, weights=None, obs_mean=None, obs_std=None):
        self._rec(params=params, weights=weights, mean=obs_mean, std=obs_std)

    def set_critic_nets(self, params, nets=None, in_mean=None, in_std=None):
        self._rec(params=params, weights=nets, mean=in_mean, std=in_std)

    def opt_in_plan(self, opt, *args, **kw):
        self._rec(opt=opt, args=args, kw=kw)
        return "plan"


TERMS = dict(uncertainty_cost=dict(cem_uncertainty=dict(kind="epistemic", weight=0.1)),
             tracking_cost=dict(cem_tracking=[dict(dim=0), dict(dim=4, kind="abs")]),
             plan_terminal_value=dict(cem_terminal_value=dict(hidden_sizes=(4,))),
             plan_terminal_q=dict(cem_terminal_q=dict(hidden_sizes=(4,), policy=dict(hidden_sizes=(4,)))),
             plan_rewards=dict(cem_reward_net=dict(inputs="next_obs", hidden_sizes=(4,))),
             plan_returns=dict(cem_discount=0.5),
             constraint_check=dict(cem_constraints=[dict(dim=0, lo=-1.0)], cem_constraint_mode="penalty", cem_constraint_weight=2.0))
STAGE = dict(uncertainty_cost="uncertainty_cost", tracking_cost="tracking_returns", plan_terminal_value="value_returns",
             plan_terminal_q="critic_returns", plan_rewards="reward_returns", plan_returns="discount_returns",
             constraint_check="constrain_returns")
CUT = ("uncertainty_cost", "plan_terminal_value", "plan_terminal_q", "plan_rewards")      # the companions under the TERMINATE cut
COMPANIONS = sorted(TERMS)


def options(**kw):
    return PlanOptions.from_kwargs(use_cem=True, n_particles=P, n_forwards=H, action_dim=A, obs_dim=D, **kw)


def model(opt, context=True, **attrs):
    """a model that holds what the companions read, and nothing else"""
    me = object.__new__(Model)
    me._opt, me._call, me.seed, me._stats_dirty, me.engine = opt, CALL, SEED, False, Engine()
    me.obs_space_dims, me.action_space_dims, me.n_forwards, me.history_length, me.context_out_dim = D, A, H, HH, C if context else 0
    me._value_set = me._reward_set = me._policy_set = me._critics_set = True
    me._targets, me._target_offset = torch.zeros(M, 1, 2), torch.zeros(M, dtype=torch.int32)
    for k, v in attrs.items():
        setattr(me, k, v)
    return me


def inputs(context=True, n=N):
    rng = np.random.default_rng(3)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return dict(obs=f(M, D), actions=f(M, H, A) if n is None else f(M, n, H, A), cp_obs=f(M, D * HH) if context else None,
                cp_act=f(M, A * HH) if context else None)


def term_options(name, constraints=None, discount=False):
    kw = dict(TERMS[name])
    if constraints is not None:
        kw.update(cem_constraints=[dict(dim=0, lo=-1.0)], cem_constraint_mode=constraints, cem_constraint_weight=2.0)
    if discount:
        kw.update(cem_discount=0.5)
    return options(**kw)


def np_(t):
    return t.numpy()


# ---------------------------------------------------------------------------------------------------------------------- the engine calls
@pytest.mark.parametrize("context", [True, False])
@pytest.mark.parametrize("seed", [None, (3 << 32) + 11])
@pytest.mark.parametrize("name", COMPANIONS)
def test_a_companion_replays_once_under_the_forecasts_key(name, seed, context):
    me, x = model(term_options(name), context), inputs(context)
    eng = me.engine
    getattr(me, name)(x["obs"], x["actions"], x["cp_obs"], x["cp_act"], seed=seed)
    names = [n for n in eng.names() if n not in ("discount_returns", "discount_weights") or name == "plan_returns"]
    if name == "plan_returns":
        assert names[-1] == "discount_weights"
        names = names[:-1]
    assert names == (["context_forward"] if context else []) + ["rollout_returns", STAGE[name]]
    roll = eng.only("rollout_returns")
    assert (roll["seed"], roll["call"], roll["it"], roll["want_traj"]) == ((SEED if seed is None else seed) & 0xFFFFFFFF, CALL & 0xFFFFFFFF,
                                                                           planner.FORECAST_IT, True)
    assert me._call == CALL
    assert torch.equal(roll["obs"], torch.as_tensor(x["obs"])) and torch.equal(roll["actions"], torch.as_tensor(x["actions"]))
    assert roll["actions"].is_contiguous() and tuple(roll["actions"].shape) == (M, N, H, A)
    if context:
        ctx = eng.only("context_forward")
        assert ctx["cp_obs"] is x["cp_obs"] and ctx["cp_act"] is x["cp_act"] and roll["ctx_vec"].shape == (E, M, C)
    else:
        assert roll["ctx_vec"] is None
    stage = eng.only(STAGE[name])
    assert stage["traj"] is eng.traj
    if name != "uncertainty_cost":
        assert stage["rows"] is eng.rows
    want = dict(uncertainty_cost="uncertainty_params", tracking_cost="track_params", plan_terminal_value="value_params",
                plan_terminal_q="critic_params", plan_rewards="reward_params", constraint_check="constraint_params")
    if name in want:
        key = dict(tracking_cost="track", constraint_check="constraints").get(name, "params")
        assert stage[key] is getattr(me._opt, want[name])
    if name in ("plan_rewards", "plan_returns", "constraint_check"):      # the stages that read the rollout's inputs
        assert stage["obs"] is roll["obs"] and stage["actions"] is roll["actions"]
    if name == "tracking_cost":
        assert stage["targets"] is me._targets and stage["offset"] is me._target_offset and stage["want_cost"] is True
    if name in ("plan_terminal_value", "plan_terminal_q", "plan_rewards"):
        assert stage["want"] is True
    if name in ("uncertainty_cost", "plan_returns"):
        assert stage["want_steps"] is True


def test_a_three_dim_plan_is_rolled_as_one_sequence_per_env():
    me, x = model(term_options("plan_rewards")), inputs(n=None)
    me.plan_rewards(**x)
    acts = me.engine.only("rollout_returns")["actions"]
    assert tuple(acts.shape) == (M, 1, H, A) and acts.is_contiguous() and torch.equal(acts[:, 0], torch.as_tensor(x["actions"]))


# ---------------------------------------------------------------------------------------------------------------------- the TERMINATE cut
@pytest.mark.parametrize("discount", [False, True])
@pytest.mark.parametrize("mode", [None, "penalty", "terminate"])
@pytest.mark.parametrize("name", CUT)
def test_terminate_constraints_cut_the_term_at_the_first_violation(name, mode, discount):
    me, x = model(term_options(name, mode, discount)), inputs()
    eng = me.engine
    res = getattr(me, name)(**x)
    stage = eng.only(STAGE[name])
    if mode != "terminate":
        assert "constrain_returns" not in eng.names() and stage["first"] is None
        if name != "uncertainty_cost":
            assert res["first"] is None
        return
    names = [n for n in eng.names() if n != "discount_returns"]
    assert names[-2:] == ["constrain_returns", STAGE[name]]
    cut, roll = eng.only("constrain_returns"), eng.only("rollout_returns")
    assert cut["traj"] is eng.traj and cut["rows"] is eng.rows and cut["constraints"] is me._opt.constraint_params      # the rollout's own rows
    assert cut["obs"] is roll["obs"] and cut["actions"] is roll["actions"]
    assert stage["first"] is eng.first
    if name != "uncertainty_cost":
        np.testing.assert_array_equal(res["first"], np_(eng.first))


# ---------------------------------------------------------------------------------------------------------------------- rows under a discount
@pytest.mark.parametrize("discount", [False, True])
@pytest.mark.parametrize("name", ["tracking_cost", "constraint_check", "uncertainty_cost"])
def test_a_discounting_model_hands_on_the_discounted_rows(name, discount):
    mode = "terminate" if name == "constraint_check" else None
    me, x = model(term_options(name, mode, discount)), inputs()
    eng = me.engine
    res = getattr(me, name)(**x)
    stage = eng.only(STAGE[name])
    if not discount:
        assert "discount_returns" not in eng.names()
        rows = eng.rows
    else:
        disc, roll = eng.only("discount_returns"), eng.only("rollout_returns")
        assert disc["traj"] is eng.traj and disc["rows"] is eng.rows and disc["obs"] is roll["obs"] and disc["actions"] is roll["actions"]
        assert disc["want_steps"] is False
        rows = eng.discounted
    if name == "uncertainty_cost":
        np.testing.assert_array_equal(res["returns"], np_(rows))
    else:
        assert stage["rows"] is rows
    if name == "tracking_cost":
        np.testing.assert_array_equal(res["returns_untracked"], np_(rows))


@pytest.mark.parametrize("name", CUT[1:])
def test_the_terms_on_the_rows_take_the_rollouts_own_under_a_discount(name):
    """(the discount of a terminal value, Q or learned reward is the stage's own: it reads the engine's weights)"""
    me = model(term_options(name, None, True))
    getattr(me, name)(**inputs())
    assert "discount_returns" not in me.engine.names() and me.engine.only(STAGE[name])["rows"] is me.engine.rows


# ---------------------------------------------------------------------------------------------------------------------- the result
def expected(name, eng, terminate):
    """the result dict for [m,n,H,A] input, out of what the stand-in answered (its k-th answer starts at 1000 k)"""
    k = eng.names().index(STAGE[name]) + 1
    f = lambda *shape: np_(eng._f(k, *shape))
    first = np_(eng.first) if terminate else None
    if name == "uncertainty_cost":
        return dict(step=f(M, eng.n, H), cost=f(M, eng.n) + 0.5, returns=np_(eng.rows))
    if name == "tracking_cost":
        return dict(cost=f(M, eng.n, P) + 0.5, returns=f(M, eng.n, P), returns_untracked=np_(eng.rows))
    if name == "plan_terminal_value":
        return dict(value=f(M, eng.n, P) + 0.5, first=first)
    if name == "plan_terminal_q":
        return dict(q=f(M, eng.n, P) + 0.5, first=first)
    if name == "plan_rewards":
        return dict(reward=f(H, M, eng.n, P).transpose(1, 2, 3, 0), total=f(M, eng.n, P) + 0.5, first=first)
    if name == "plan_returns":
        return dict(returns=f(M, eng.n, P), step_rewards=f(H, M, eng.n, P).transpose(1, 2, 0, 3))
    viol = np_(torch.arange(M * eng.n * P, dtype=torch.int32).reshape(M, eng.n, P) % 3)
    return dict(first_violation=np_(eng.first), violations=viol, returns=f(M, eng.n, P), violation_fraction=(viol > 0).mean(axis=-1))


@pytest.mark.parametrize("n", [N, None])
@pytest.mark.parametrize("name,terminate", [(c, False) for c in COMPANIONS] + [(c, True) for c in CUT])
def test_the_result_and_its_n_axis(name, terminate, n):
    me, x = model(term_options(name, "terminate" if terminate else None)), inputs(n=n)
    eng = me.engine
    eng.n = 1 if n is None else n
    res = getattr(me, name)(**x)
    want = expected(name, eng, terminate)
    if name == "plan_returns":
        weights = res.pop("weights")
        np.testing.assert_array_equal(weights, np.float32(0.5) ** np.arange(H + 1, dtype=np.float32))      # [H + 1], whatever the input
    assert sorted(res) == sorted(want)
    for key, w in want.items():
        if w is None:
            assert res[key] is None, key
            continue
        assert isinstance(res[key], np.ndarray)
        np.testing.assert_array_equal(res[key], w[:, 0] if n is None else w, err_msg=key)


# ---------------------------------------------------------------------------------------------------------------------- the option order
def test_uncertainty_cost_reads_its_options_behind_the_push():
    """the push of new statistics replaces `_opt` with the one that holds the delta_std weights: the stage call gets THAT struct"""
    opt = options(cem_uncertainty=dict(kind="epistemic", weight=0.1, w="delta_std"))
    stats = [np.full((D,), 2.0 + i) for i in range(12)]
    me = model(opt, _stats_dirty=True, _stats12=lambda: stats)
    placeholder = opt.uncertainty_params
    me.uncertainty_cost(**inputs())
    eng = me.engine
    assert eng.names()[:3] == ["set_stats", "uncertainty_params", "context_forward"] and not me._stats_dirty
    built = eng.only("uncertainty_params")
    np.testing.assert_array_equal(built["w"], (1.0 / (np.full((D,), 7.0) + 1e-10) ** 2).astype(np.float32))
    assert built["obs_dim"] == D
    got = eng.only("uncertainty_cost")["params"]
    assert got is built["result"] and got is me._opt.uncertainty_params and got is not placeholder


# ---------------------------------------------------------------------------------------------------------------------- proposals and forecast
@pytest.mark.parametrize("context", [True, False])
@pytest.mark.parametrize("seed", [None, (3 << 32) + 11])
def test_policy_proposals_and_forecast_draw_under_the_same_key(seed, context):
    opt = options(cem_policy_prior=dict(hidden_sizes=(4,), n_samples=3))
    me, x = model(opt, context, discrete=False), inputs(context, n=None)
    eng = me.engine
    out, states = me.policy_proposals(x["obs"], x["cp_obs"], x["cp_act"], seed=seed, return_states=True)
    assert eng.names() == (["context_forward"] if context else []) + ["policy_propose"]
    call = eng.only("policy_propose")
    assert (call["seed"], call["call"]) == ((SEED if seed is None else seed) & 0xFFFFFFFF, CALL & 0xFFFFFFFF)
    assert call["params"] is opt.policy_params and torch.equal(call["obs"], torch.as_tensor(x["obs"])) and call["want_states"] is True
    assert (call["ctx_vec"] is None) == (not context)
    assert out.shape == (M, 3, H, A) and states.shape == (H, M, 3, P, D) and me._call == CALL
    del eng.calls[:]
    res = me.forecast(x["obs"], x["actions"], x["cp_obs"], x["cp_act"], band_k=2, seed=seed)
    assert eng.names() == ["plan_forecast"]
    call = eng.only("plan_forecast")
    assert (call["seed"], call["call"], call["band_k"]) == ((SEED if seed is None else seed) & 0xFFFFFFFF, CALL & 0xFFFFFFFF, 2)
    assert call["obs"] is x["obs"] and call["cp_obs"] is x["cp_obs"] and call["cp_act"] is x["cp_act"]
    assert tuple(call["actions"].shape) == (M, 1, H, A) and me._call == CALL
    assert res["mean"].shape == (M, H, D) and res["member_mean"].shape == (E, M, H, D) and res["reward_member"].shape == (E, M, H)
    assert res["returns"].shape == (M, P) and res["return_mean"].shape == (M,) and res["diverged_step"].shape == (M,)
    np.testing.assert_array_equal(res["std_total"], np.sqrt(np_(eng._f(1, M, 1, H, D)))[:, 0])


# ---------------------------------------------------------------------------------------------------------------------- the four nets
def bare(opt, **attrs):
    me = object.__new__(Model)
    me._opt = opt
    for k, v in attrs.items():
        setattr(me, k, v)
    return me


PLANS = (np.zeros((M, D), np.float32), np.zeros((M, H, A), np.float32))
STATES = np.zeros((M, D), np.float32)
# net -> (option kwargs, the option's name, noun, setter, clearer, engine method, [(method, arguments)] that need the net)
NETS = dict(
    value=(TERMS["plan_terminal_value"], "cem_terminal_value", "value net", "set_terminal_value", "clear_terminal_value", "set_value_net",
           [("terminal_value", (STATES,)), ("plan_terminal_value", PLANS)]),
    reward=(TERMS["plan_rewards"], "cem_reward_net", "reward net", "set_reward_net", "clear_reward_net", "set_reward_net",
            [("reward_net", (STATES,)), ("plan_rewards", PLANS)]),
    policy=(dict(cem_policy_prior=dict(hidden_sizes=(4,), n_samples=3)), "cem_policy_prior", "policy net", "set_policy", "clear_policy",
            "set_policy_net", [("policy_action", (STATES,)), ("policy_proposals", (STATES,))]),
    critics=(TERMS["plan_terminal_q"], "cem_terminal_q", "critics", "set_critics", "clear_critics", "set_critic_nets",
             [("q_value", (STATES,)), ("plan_terminal_q", PLANS)]))
FLAGS = dict(_value_set=False, _reward_set=False, _policy_set=False, _critics_set=False)


@pytest.mark.parametrize("net", sorted(NETS))
def test_a_model_without_the_option_refuses_every_method_of_the_net(net):
    kw, option, noun, setter, clearer, _, needing = NETS[net]
    for opt in (None, options(cem_knots=3)):
        for who, args in [(setter, ([],)), (clearer, ())] + needing:
            tail = " and no cem_terminal_q (and no imagine_policy)" if net == "policy" and who != "policy_proposals" else ""
            with pytest.raises(ValueError) as e:
                getattr(Model, who)(bare(opt), *args)
            assert str(e.value) == "%s: this model has no %s%s" % (who, option, tail)


@pytest.mark.parametrize("net", sorted(NETS))
def test_a_model_without_the_net_refuses_what_needs_it(net):
    kw, option, noun, setter, clearer, _, needing = NETS[net]
    for who, args in needing:
        with pytest.raises(RuntimeError) as e:
            getattr(Model, who)(bare(options(**kw), **FLAGS), *args)
        assert str(e.value) == "%s: this model has no %s (call %s first)" % (who, noun, setter)


def test_the_actor_may_belong_to_the_critics_or_to_imagine():
    q_only = options(**TERMS["plan_terminal_q"])
    for who, args in (("q_value", (STATES,)), ("plan_terminal_q", PLANS)):      # the critics are there, their actor is not
        with pytest.raises(RuntimeError) as e:
            getattr(Model, who)(bare(q_only, **dict(FLAGS, _critics_set=True)), *args)
        assert str(e.value) == "%s: this model has no policy net (call set_policy first)" % who
    with pytest.raises(RuntimeError, match="^q_value: this model has no critics"):      # Q at given actions needs no actor, but critics
        Model.q_value(bare(q_only, **FLAGS), STATES, np.zeros((M, A), np.float32))
    imagining = HipEngine.policy_params((4,), "relu", "tanh", 1, 0.0)
    for me in (bare(q_only, **FLAGS), bare(None, _imagine_policy=imagining, **FLAGS), bare(options(cem_knots=3), _imagine_policy=imagining, **FLAGS)):
        with pytest.raises(RuntimeError) as e:
            Model.policy_action(me, STATES)
        assert str(e.value) == "policy_action: this model has no policy net (call set_policy first)"
        with pytest.raises(ValueError) as e:      # an actor alone is no prior
            Model.policy_proposals(me, STATES)
        assert str(e.value) == "policy_proposals: this model has no cem_policy_prior"
        me.engine = Engine()
        Model.set_policy(me, "w")
        assert me._policy_set is True and me.engine.only("set_policy_net")["params"].n_samples == 1
        Model.clear_policy(me)
        assert me._policy_set is False and me.engine.calls[-1] == ("set_policy_net", dict(params=None, weights=None, mean=None, std=None))


@pytest.mark.parametrize("net", sorted(NETS))
def test_set_and_clear_register_with_the_engine_and_keep_the_flag(net):
    kw, option, noun, setter, clearer, export, _ = NETS[net]
    opt = options(**kw)
    me = bare(opt, engine=Engine(), **FLAGS)
    flag = dict(value="_value_set", reward="_reward_set", policy="_policy_set", critics="_critics_set")[net]
    weights, mean, std = [("W", "b")], np.zeros(3), np.ones(3)
    getattr(me, setter)(weights, mean, std)
    got = me.engine.only(export)
    prm = dict(value=opt.value_params, reward=opt.reward_params, policy=opt.policy_params, critics=opt.critic_params)[net]
    assert got["params"] is prm and got["weights"] is weights and got["mean"] is mean and got["std"] is std
    assert getattr(me, flag) is True and sum(getattr(me, f) for f in FLAGS) == 1
    getattr(me, clearer)()
    assert me.engine.calls[-1] == (export, dict(params=None, weights=None, mean=None, std=None)) and getattr(me, flag) is False
    names = list(inspect.signature(getattr(Model, setter)).parameters)      # the statistics are named as the net names its input
    assert names == ["self", "nets" if net == "critics" else "weights"] + (["obs_mean", "obs_std"] if net in ("value", "policy") else ["in_mean", "in_std"])


# ---------------------------------------------------------------------------------------------------------------------- _plan_opt_in
PLAN_INPUTS = (torch.zeros(M, D), None, None, torch.zeros(M, H, A), torch.ones(M, H, A))
REFUSALS = dict(value="get_action: this model plans under cem_terminal_value and has no value net (call set_terminal_value first)",
                reward="get_action: this model plans under cem_reward_net and has no reward net (call set_reward_net first)",
                policy="get_action: this model plans under cem_policy_prior and has no policy net (call set_policy first)",
                critics="get_action: this model plans under cem_terminal_q and has no critics (call set_critics first)",
                actor="get_action: this model plans under cem_terminal_q and has no policy net (call set_policy first)")


def planning(opt, have):
    flags = {"_%s_set" % k: k in have for k in ("value", "reward", "policy", "critics")}
    return model(opt, False, n_candidates=8, _plan_carry=None, _plan_carry_valid=None, _plan_phase=None, **flags)


@pytest.mark.parametrize("terminal,order", [("plan_terminal_value", ["value", "reward", "policy"]),
                                            ("plan_terminal_q", ["reward", "policy", "critics"])])
def test_plan_opt_in_refuses_a_missing_net_in_order_before_the_call_counter_moves(terminal, order):
    opt = options(cem_policy_prior=NETS["policy"][0]["cem_policy_prior"], **TERMS["plan_rewards"],
                  **(TERMS[terminal] if terminal == "plan_terminal_value" else dict(cem_terminal_q=dict(hidden_sizes=(4,)))))
    for k, missing in enumerate(order):
        me = planning(opt, order[:k])
        with pytest.raises(RuntimeError) as e:
            me._plan_opt_in(*PLAN_INPUTS)
        assert str(e.value) == REFUSALS[missing]
        assert me._call == CALL and me.engine.calls == []
    me = planning(opt, order)
    assert me._plan_opt_in(*PLAN_INPUTS) == "plan"
    plan = me.engine.only("opt_in_plan")
    assert me._call == CALL + 1 and plan["kw"]["call"] == (CALL + 1) & 0xFFFFFFFF and plan["kw"]["seed"] == SEED and plan["opt"] is opt


def test_plan_opt_in_asks_for_the_critics_before_their_actor():
    opt = options(**TERMS["plan_terminal_q"])      # the actor is the critics' own declaration: no prior
    for have, missing in (((), "critics"), (("policy",), "critics"), (("critics",), "actor")):
        me = planning(opt, have)
        with pytest.raises(RuntimeError) as e:
            me._plan_opt_in(*PLAN_INPUTS)
        assert str(e.value) == REFUSALS[missing] and me._call == CALL and me.engine.calls == []
