"""MLPEnsembleCEMDynamicsModel (PE-TS + CaDM) -- MI355X drop-in for the reference class
/root/reference/cadm/dynamics/mlp_cadm_ensemble_cem_dynamics.py:12.

Same constructor kwargs (:26-54) and public methods -- get_action (:344), get_context_pred
(:369), fit (:382), save (:571), load (:579), compute_normalization (:590),
get_normalization_stats (:604) -- so `run_cadm_pets.py` can build it unchanged.  What was one
TensorFlow graph behind `sess.run` is here libcadm_hip.so (hand-written HIP for gfx950)
reached through cadm_amd.engine.HipEngine; host code keeps the reference's numpy-level data
handling (dataset growth, float64 statistics, bootstrap indices, early stopping).

Differences a caller can see (all opt-in except the first):
  * `env` may be a reference env object, a NormalizedEnv wrapper or a cadm_amd.envs.EnvSpec;
    its class selects the compiled-in closures (cadm_amd/envs.py) -- or any env that declares its closures as a
    cadm_amd.env_spec.EnvDecl in a `cadm_env_spec` attribute (the rollout kernel is then built for that spec);
  * extra kwargs: `reference_quirks` (default True: reproduce the context-layout quirks Q1/Q2
    of core/utils.py:434-435), `seed` (device Philox key; the reference never seeds TF),
    `device`, `process_group` (OPT-IN: shard candidates over the ranks of that torch.distributed group; every
    rank must then call get_action with the same observations -- None, the default, never shards.  The GUARD against ranks
    that drift apart (different obs / history / warm start -> different elite sets -> silently different plans): the first
    `check_replicated_calls` (2) sharded calls AND every `check_replicated_every`-th (256th) one after them compare a checksum
    of the inputs with one extra all-reduce and raise on a mismatch; all other calls run only the path's own collectives.
    `check_replicated_every=0` switches the periodic check OFF -- then nothing detects divergence after the first calls);
  * `cem_noise_beta`, `cem_keep_elites`, `cem_decay`, `cem_return`, `cem_add_mean`: the iCEM planner (Pinneri et al. 2020; INTEGRATION.md
    "iCEM planner").  At their defaults (0.0, 0, 1.0, "mean", False) `get_action` is the reference's CEM, unchanged; any other value
    plans with `cadm_icem_plan` -- coloured action noise, elites kept between CEM iterations and (moved one step on) between
    consecutive calls, `reset_plan_carry` to forget them at an episode boundary;
  * `cem_update="mppi"`, `cem_temperature`, `cem_temperature_relative`: the MPPI update (INTEGRATION.md "MPPI update") in that loop --
    every candidate refits the mean and variance with weight exp(return / temperature) instead of the top `num_elites` alone;
    `cem_update="mppi"` alone takes the opt-in route, the default "cem" leaves everything as it is;
    (what the ten `cem_*` kwargs mean is held in ONE attribute, `_opt`: None at the defaults, else a cadm_amd.planner.PlanOptions)
  * `cem_score="mean_std" | "member_std" | "cvar"`, `cem_risk`: risk-aware candidate scores in that loop (INTEGRATION.md "Risk-aware
    scoring") -- a candidate's particle returns become mean - cem_risk * std, mean - cem_risk * (std of the ensemble members' means), or
    the mean of the worst cem_risk fraction of them, instead of their plain mean; a non-default `cem_score` alone takes the opt-in route;
  * `cem_constraints=[dict(dim=d, lo=..., hi=...), ...]`, `cem_constraint_mode="penalty" | "terminate"`, `cem_constraint_weight`: state
    constraints in that loop (INTEGRATION.md "State constraints and termination") -- a predicted state is healthy while lo < obs[d] < hi
    for every entry; "penalty" takes cem_constraint_weight off a particle's return per violating step, "terminate" ends its return at
    the first one (that step still pays) and takes the weight off once; `cem_constraints` alone takes the opt-in route, and a constraint
    that never binds leaves every plan as it is.  `constraint_check(obs, actions, ...)`: which particles of given plans violate, and when;
  * `cem_knots=r`, `cem_knot_interp="hold" | "linear"`, `cem_knot_anchor="call" | "episode"`: plans on knots in that loop (INTEGRATION.md
    "Plans on knots") -- every candidate is piecewise constant ("hold": action repeat r) or piecewise linear on knot steps r apart, so the
    search runs over H / r decisions per action dim instead of H; "call" hangs the grid on every call's first step, "episode" keeps
    the breakpoints fixed in episode time (the model advances a per-env phase by one per call, `reset_plan_carry` puts it back to 0);
    `cem_knots` > 1 alone takes the opt-in route, the default 1 leaves everything as it is;
  * `cem_tracking=[dict(dim=d, kind="square" | "abs" | "huber", w=..., delta=...), ...]`, `cem_target_advance`: targets set at run time in
    that loop (INTEGRATION.md "Tracking targets at run time") -- `set_targets(targets, offset=None)` gives every env a goal [m,K] or a
    reference [m,T,K] for the K terms, and every candidate's particle returns lose sum_t sum_k w_k c(x_t[d_k] - target) before they are
    scored; NaN in the targets: no target there; the model moves every env's place in its reference on by one per planned call
    (`cem_target_advance=False`: the caller does), `reset_plan_carry` puts it back to 0; `clear_targets()`; `tracking_cost(obs, actions,
    ...)`: what the terms cost given plans.  `cem_tracking` alone takes the opt-in route; targets that are all NaN change no plan;
  * `cem_action_delay=d`, `cem_action_rate_limit`, `cem_action_rate_cost`, `cem_action_advance`: an actuator model in that loop
    (INTEGRATION.md "Actuator model") -- the plan's first d steps are the ones earlier calls committed, every other step stays within
    `cem_action_rate_limit` (a scalar or [A]) of the step before it, step 0 of the action applied last, and sum_t sum_a w_a (u_t - u_{t-1})^2
    (`cem_action_rate_cost`, a scalar or [A]) comes off every candidate's score; the model keeps the applied action and the committed
    steps per env on the device and moves them on after every planned call (`cem_action_advance=False`: the caller does, with
    `set_applied_actions`), `reset_plan_carry` forgets them; `actuator_state()`; `action_cost(actions)`: what the model makes of given
    plans.  Any of the three alone takes the opt-in route;
  * `cem_uncertainty=dict(kind="epistemic" | "total", weight=lambda, w=None | float | [D] | "delta_std", form="var" | "std", cap=None)`:
    the ensemble's disagreement about the states a candidate visits, per step, as a cost (lambda > 0) or a bonus (lambda < 0) in that
    loop's candidate score (INTEGRATION.md "Pricing model uncertainty"); `w="delta_std"` weighs every dim by 1 / sigma_delta^2 of the
    current normalisation statistics (picked up again after every `fit`), `set_uncertainty_weights(w)` replaces the weights at run time,
    `uncertainty_cost(obs, actions, ...)`: what the term makes of given plans.  It alone takes the opt-in route;
  * `cem_terminal_value=dict(hidden_sizes=(256, 256), activation="relu" | "tanh" | "swish", weight=1.0)`: a value net V on the last
    state of every particle in that loop, so that a candidate is scored by return + weight * V(s_H) (INTEGRATION.md "Terminal value").
    The kwarg declares the net's shape; `set_terminal_value(weights, obs_mean=None, obs_std=None)` hands over a critic at run time (a
    list of (W [in,out], b [out]) or a torch.nn.Sequential), as often as it is retrained and with nothing rebuilt,
    `clear_terminal_value()` removes it, `terminal_value(states)` evaluates V through the planner's kernel,
    `plan_terminal_value(obs, actions, ...)`: what the term adds for given plans.  It alone takes the opt-in route;
  * `cem_reward_net=dict(inputs="next_obs" | "obs_act" | "obs_act_next_obs", hidden_sizes=(128, 128), activation=, weight=1.0)`: a
    learned reward net R on every step of every particle in that loop, so that a candidate is scored by return + weight * sum_t R_t
    (INTEGRATION.md "Learned reward").  The kwarg declares the net's shape; `set_reward_net(weights, in_mean=None, in_std=None)` hands
    over the net at run time (a list of (W [in,out], b [out]) or a torch.nn.Sequential) with nothing rebuilt, `clear_reward_net()`
    removes it, `reward_net(obs, act, next_obs)` evaluates R through the planner's kernel, `plan_rewards(obs, actions, ...)`: the step
    rewards of given plans.  It alone takes the opt-in route;
  * `cem_policy_prior=dict(hidden_sizes=(256, 256), activation="relu", squash="tanh" | "none", n_samples=24, noise_std=0.0,
    proposals="noise" | "head", std_scale=1.0)`: the learner's actor as a prior in that loop (INTEGRATION.md "Policy prior";
    "Proposals drawn from the head" for the last two keys) -- once per call the policy is rolled through the model
    on `n_samples` sequences per env (sequence 0 without noise), and every iteration's candidates hold those sequences behind the kept
    elites and the mean candidate.  The kwarg declares the net's shape; `set_policy(weights, obs_mean=None, obs_std=None)` hands over
    an actor at run time (a list of (W [in,out], b [out]) or a torch.nn.Sequential) with nothing rebuilt, `clear_policy()` removes it,
    `policy_action(states)` evaluates it through the planner's kernel, `policy_proposals(obs, ...)`: the sequences a call would
    inject.  It alone takes the opt-in route; `fit` does not touch the policy;
  * `cem_terminal_q=dict(hidden_sizes=(256, 256), activation="relu", n_critics=2, reduce="min" | "mean", weight=1.0,
    policy=dict(hidden_sizes=, activation=, squash=))`: the terminal value of a learner that has an actor and Q critics but no V
    (INTEGRATION.md "Terminal value from Q critics") -- weight * reduce_c Q_c(s_H, pi(s_H)) on the last state of every particle, one
    fused launch per iteration.  The kwarg declares the shapes (`policy` may be left out with a `cem_policy_prior`: the actor is then
    that net); `set_critics(nets, in_mean=None, in_std=None)` hands over the C critics (each as `set_terminal_value` takes a net, with
    D + A inputs) and `set_policy(...)` the actor, at run time and with nothing rebuilt; `clear_critics()`, `q_value(states,
    actions=None)`, `plan_terminal_q(obs, actions, ...)`.  Not together with `cem_terminal_value`.  It alone takes the opt-in route;
  * `policy_head=dict(kind="gaussian", log_std_bounds=(-5.0, 2.0), log_std_bound="clamp" | "tanh")`: the model's one actor
    (whichever option declares it) is a SAC actor (INTEGRATION.md "Stochastic actor head") -- `set_policy` then takes a net whose last
    layer has 2 A outputs, the mean and the log standard deviation; the planner and `policy_action` keep the mode action, bit for bit
    (with `cem_policy_prior`'s `proposals="head"` the prior's sequences 1 .. P - 1 are trajectories of the policy itself, drawn at
    std_scale times the standard deviation the head predicts at every state, instead of the mode plus `noise_std`);
    `imagine(...)` draws its actions from the policy and returns their `logp`, `policy_sample(states)` draws for given states,
    `policy_log_prob(states, actions)` is the density of actions the caller brings;
  * `cem_policy_logp=dict(weight=1.0, space="action" | "pre_squash", policy=dict(hidden_sizes=, activation=, squash=))`: the actor as
    a preference, not only a source of candidates (INTEGRATION.md "Actor-regularised planning") -- weight * sum_t log pi(a_t | s_t) on
    every step of every particle joins the particle's return.  Needs `policy_head`; `policy` may be left out beside
    `cem_policy_prior` or `cem_terminal_q`'s policy (one actor).  `plan_policy_log_prob(obs, actions, ...)`: the term of given plans.
    It alone takes the opt-in route;
  * `cem_discount=gamma` in (0, 1]: a discount over the horizon in that loop (INTEGRATION.md "Discount over the horizon") -- every
    quantity that enters a candidate's score is weighted by gamma^t at step t: the env's own step rewards, the constraint penalty, the
    tracking, uncertainty and rate costs and the learned reward, and a terminal value or Q by gamma^H on top of its `weight` (which
    then no longer carries gamma ** n_forwards).  `plan_returns(obs, actions, ...)`: the discounted returns of given plans; the other
    diagnostics report discounted figures too; `forecast` does not.  Any value other than 1.0 takes the opt-in route;
  * `forecast(obs, actions, ...)` and `get_action(..., return_forecast=True)`: the model's per-step predicted states, rewards and
    their spread under a plan (INTEGRATION.md "Forecasting a plan"); the default `return_forecast=False` is today's path, unchanged;
  * `predict(obs, act, cp_obs, cp_act)` -- thin alias the north-star asks for: one-step mean
    prediction of every ensemble member (the reference has no public predict).
"""
import time
from collections import OrderedDict, namedtuple

import joblib
import numpy as np
import torch

from .. import planner as _planner
from ..engine import HipEngine
from ..envs import resolve_env_kind
from ..utils import log as logger

_ACTIVATIONS = (None, "relu", "tanh", "sigmoid", "softmax", "swish")   # reference :17-24


class FitIndexStream(object):
    """Every random index `fit` consumes, in the order the reference draws them from the global `np.random`
    (/root/reference/cadm/dynamics/mlp_cadm_ensemble_cem_dynamics.py:444, :465, :472-474 + :483):

        permutation(N)             -> [N]        train / validation split of the windows
        bootstrap(E, n_train)      -> [E, n]     each member's bootstrap sample of training rows (E > 1 only)
        epoch_order(E, n_train)    -> [E, n]     `shuffle_rows`: per-member argsort of uniforms, once per epoch

    The default draws them on the host from a numpy Generator.  A caller (or a parity test) may pass any object with
    these three methods as `fit(..., index_stream=...)`, e.g. `ReplayIndexStream` with arrays captured elsewhere."""

    def __init__(self, rng):
        self.rng = rng

    def permutation(self, n):
        return self.rng.permutation(n)

    def bootstrap(self, E, n_train):
        return self.rng.integers(0, n_train, size=(E, n_train))

    def epoch_order(self, E, n_train):
        return np.argsort(self.rng.uniform(size=(E, n_train)), axis=-1)


class RecordingIndexStream(object):
    """Wraps a stream and keeps what it handed out (`.log`: list of (kind, array))."""

    def __init__(self, inner):
        self.inner, self.log = inner, []

    def _rec(self, kind, arr):
        self.log.append((kind, np.array(arr)))
        return arr

    def permutation(self, n):
        return self._rec("permutation", self.inner.permutation(n))

    def bootstrap(self, E, n_train):
        return self._rec("bootstrap", self.inner.bootstrap(E, n_train))

    def epoch_order(self, E, n_train):
        return self._rec("epoch_order", self.inner.epoch_order(E, n_train))


class ReplayIndexStream(object):
    """Replays a recorded log; raises if `fit` asks for something else than what was recorded."""

    def __init__(self, log):
        self.log, self.pos = list(log), 0

    def _next(self, kind, shape):
        if self.pos >= len(self.log) or self.log[self.pos][0] != kind or tuple(self.log[self.pos][1].shape) != tuple(shape):
            raise ValueError("index stream exhausted or out of order at draw %d (%s %r)" % (self.pos, kind, shape))
        arr = self.log[self.pos][1]
        self.pos += 1
        return arr

    def permutation(self, n):
        return self._next("permutation", (n,))

    def bootstrap(self, E, n_train):
        return self._next("bootstrap", (E, n_train))

    def epoch_order(self, E, n_train):
        return self._next("epoch_order", (E, n_train))


def _checked_shapes(model, *inputs):
    """The shape set of get_action's (obs, cp_obs, cp_act, cem_init_mean, cem_init_var), checked once per set (the reference would raise a
    TF shape error; raw device pointers would not).  A function of the model: the CPU tests of get_action run it on a stand-in object."""
    sig = tuple(None if x is None else tuple(np.shape(x)) for x in inputs)
    if sig != model._checked_sig:
        model._check_planner_inputs(*inputs)
        model._checked_sig = sig
    return sig


def calibration_summary(out):
    """The sums and counts of `cadm_calibration_stats` (numpy arrays) -> what `evaluate_calibration` returns (see there): the means,
    and coverage / nominal / calibration_error derived from rank_hist.  NaN where the divisor is 0."""
    res = {k: out[k].astype(np.int64) for k in ("rank_hist", "rank_hist_member", "ties", "degenerate", "count", "diverged")}
    hist, count = res["rank_hist"], res["count"]
    p = hist.shape[-1] - 1
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(count > 0, count, np.nan)[:, None]
        res["crps"] = out["crps"].astype(np.float64) / n
        used = count[:, None] - res["degenerate"]
        nd = np.where(used > 0, used, np.nan)
        res["z2"] = out["z2"].astype(np.float64) / nd
        res["nll"] = out["nll"].astype(np.float64) / nd
        res["z2_ideal"] = (p + 1.0) / (p - 3.0) if p > 3 else float("nan")
        ks = np.arange(p // 2)
        res["nominal"] = (p - 1.0 - 2.0 * ks) / (p + 1.0)
        csum = np.concatenate([np.zeros(hist.shape[:-1] + (1,), np.int64), np.cumsum(hist, axis=-1)], axis=-1)      # [.., r]: ranks below r
        res["coverage"] = (csum[..., p - ks] - csum[..., ks + 1]) / n[:, :, None]          # ranks k + 1 .. p - 1 - k
        cdf = csum[..., 1:] / n[:, :, None]
        res["calibration_error"] = np.abs(cdf - np.arange(1, p + 2) / (p + 1.0)).max(axis=-1).mean(axis=-1)
    return res


# The four nets a caller hands a model at run time: the PlanOptions field that declares one, the kwarg behind that field, the model's
# "the engine holds one" attribute, what the messages call it, its setter, and the engine method that registers it (None clears it).
_Net = namedtuple("_Net", "field kwarg flag noun setter register")
_NETS = dict(value=_Net("value_params", "cem_terminal_value", "_value_set", "value net", "set_terminal_value", "set_value_net"),
             reward=_Net("reward_params", "cem_reward_net", "_reward_set", "reward net", "set_reward_net", "set_reward_net"),
             policy=_Net("policy_params", "cem_policy_prior", "_policy_set", "policy net", "set_policy", "set_policy_net"),
             critics=_Net("critic_params", "cem_terminal_q", "_critics_set", "critics", "set_critics", "set_critic_nets"))


def _need_net(model, net, who, under=None):
    """Refuse for `who` while the model holds no `net`; under: the option the call plans under (get_action's wording)."""
    row = _NETS[net]
    if not getattr(model, row.flag):
        raise RuntimeError("%s: this model %shas no %s (call %s first)" % (who, "plans under %s and " % under if under else "", row.noun, row.setter))


def _require_net(model, net, who, need_net=False, need_actor=False):
    """The model's options, for a method of `net` -- refused without the option that declares it, with need_net while none is
    registered, with need_actor while no policy net is.  (Functions of the model: a refusal reads `_opt` and the flags alone.)"""
    opt = getattr(model, "_opt", None)
    if opt is None or getattr(opt, _NETS[net].field) is None:
        raise ValueError("%s: this model has no %s" % (who, _NETS[net].kwarg))
    if need_net:
        _need_net(model, net, who)
    if need_actor:
        _need_net(model, "policy", who)
    return opt


def _require_policy(model, who, need_net=False):
    """`_require_net` for the methods of the policy net that need no prior: the actor of `cem_terminal_q` will do, and so will the
    one of `imagine_policy` (no planner option: the options may then be None)."""
    opt = getattr(model, "_opt", None)
    declared = opt is not None and (opt.policy_params is not None or opt.critic_params is not None or opt.logp_params is not None)
    if not declared and getattr(model, "_imagine_policy", None) is None:
        raise ValueError("%s: this model has no cem_policy_prior and no cem_terminal_q (and no imagine_policy)" % who)
    if need_net:
        _need_net(model, "policy", who)
    return opt


def _register_net(model, net, params, *given):
    """`set_*` (params and what the caller gave: weights, mean, std) and `clear_*` (None) of a net: the engine's copy and the flag."""
    getattr(model.engine, _NETS[net].register)(params, *given)
    setattr(model, _NETS[net].flag, params is not None)


class MLPEnsembleCEMDynamicsModel(object):
    """Probabilistic-ensemble MLP dynamics model with a context encoder and a CEM / RS planner."""

    def __init__(self,
                 name,
                 env,
                 hidden_sizes=(200, 200, 200, 200),
                 hidden_nonlinearity="swish",       # (the reference's default, tf.nn.relu, is not a key of its own `_activations` table:
                 output_nonlinearity=None,          #  dynamics.py:30 vs :104 raises KeyError on a defaulted call; every script passes 'swish')
                 batch_size=128,
                 learning_rate=0.001,
                 normalize_input=True,
                 optimizer=None,
                 valid_split_ratio=0.2,
                 rolling_average_persitency=0.99,
                 n_forwards=30,
                 n_candidates=2500,
                 ensemble_size=5,
                 n_particles=20,
                 use_cem=False,
                 deterministic=False,
                 weight_decays=(0., 0., 0., 0., 0.),
                 weight_decay_coeff=0.0,
                 cp_hidden_sizes=(256, 128, 64),
                 context_weight_decays=(0., 0., 0., 0.),
                 context_out_dim=10,
                 context_hidden_nonlinearity="relu",
                 history_length=10,
                 future_length=10,
                 state_diff=False,
                 back_coeff=0.0,
                 # ---- extensions (not in the reference) ----
                 reference_quirks=True,
                 seed=0,
                 device=None,
                 process_group=None,
                 check_replicated_calls=2,
                 check_replicated_every=256,
                 cem_noise_beta=0.0,
                 cem_keep_elites=0,
                 cem_decay=1.0,
                 cem_return="mean",
                 cem_add_mean=False,
                 cem_update="cem",
                 cem_temperature=1.0,
                 cem_temperature_relative=False,
                 cem_score="mean",
                 cem_risk=None,
                 cem_constraints=None,
                 cem_constraint_mode="penalty",
                 cem_constraint_weight=None,
                 cem_knots=1,
                 cem_knot_interp="hold",
                 cem_knot_anchor="call",
                 cem_tracking=None,
                 cem_target_advance=True,
                 cem_action_delay=0,
                 cem_action_rate_limit=None,
                 cem_action_rate_cost=None,
                 cem_action_advance=True,
                 cem_uncertainty=None,
                 cem_terminal_value=None,
                 cem_reward_net=None,
                 cem_policy_prior=None,
                 cem_terminal_q=None,
                 cem_discount=1.0,
                 cem_policy_logp=None,
                 imagine_policy=None,
                 policy_head=None,
                 engine_lib=None,
                 ):
        self.env = env
        self.name = name
        self._dataset = None

        if hidden_nonlinearity not in _ACTIVATIONS or output_nonlinearity not in _ACTIVATIONS:
            raise KeyError("unknown nonlinearity %r / %r" % (hidden_nonlinearity, output_nonlinearity))
        if hidden_nonlinearity == "softmax" or output_nonlinearity is not None:
            # reference: `_activations` (dynamics.py:17-24) offers both; `output_nonlinearity` would be applied to BOTH heads and to the
            # context encoder's output (core/utils.py:327,333,609), 'softmax' row-wise over a hidden layer's units.  No script of the
            # reference passes either (run_cadm_pets.py:221, run_pets.py: 'swish' / None).
            raise NotImplementedError(
                "the HIP kernels implement hidden_nonlinearity in (swish, relu, tanh, sigmoid, None) and output_nonlinearity=None "
                "(reference: _activations, cadm/dynamics/mlp_cadm_ensemble_cem_dynamics.py:17-24; its scripts pass 'swish' / None: "
                "run_cadm_pets.py:221); got hidden_nonlinearity=%r, output_nonlinearity=%r" % (hidden_nonlinearity, output_nonlinearity))
        # context_hidden_nonlinearity is accepted and ignored exactly like the reference
        # (always ReLU: dynamics.py:49 vs :141-156, layers.py:34).
        if optimizer is not None and getattr(optimizer, "__name__", "") not in ("AdamOptimizer",):
            raise NotImplementedError("only Adam (TF1 semantics) is implemented")

        self.deterministic = deterministic
        self.n_forwards = n_forwards
        self.n_candidates = n_candidates
        self.use_cem = use_cem
        self.weight_decays = weight_decays
        self.weight_decay_coeff = weight_decay_coeff
        self.normalization = None
        self.normalize_input = normalize_input
        self.batch_size = batch_size
        self.learning_rate = learning_rate
        self.valid_split_ratio = valid_split_ratio
        self.rolling_average_persitency = rolling_average_persitency
        self.ensemble_size = ensemble_size
        self.n_particles = n_particles
        self.cp_hidden_sizes = cp_hidden_sizes
        self.context_out_dim = context_out_dim
        self.history_length = history_length
        self.future_length = future_length
        self.context_weight_decays = context_weight_decays
        self.state_diff = state_diff
        self.back_coeff = back_coeff

        self.obs_space_dims = obs_space_dims = env.observation_space.shape[0]
        self.proc_obs_space_dims = env.proc_observation_space_dims
        if len(env.action_space.shape) == 0:
            self.action_space_dims = env.action_space.n
            self.discrete = True
        else:
            self.action_space_dims = env.action_space.shape[0]
            self.discrete = False

        if n_particles % ensemble_size != 0:
            raise ValueError("n_particles must be a multiple of ensemble_size (core/utils.py:447 int(p/E))")

        # the opt-in planner's switches (planner.PlanOptions), checked before the engine is built; None, every cem_* kwarg at its default:
        # the reference's CEM, and get_action never looks further
        self._opt = _planner.PlanOptions.from_kwargs(cem_noise_beta, cem_keep_elites, cem_decay, cem_return, cem_add_mean, cem_update,
                                                     cem_temperature, cem_temperature_relative, cem_score, cem_risk, use_cem=use_cem,
                                                     discrete=self.discrete, process_group=process_group, n_particles=n_particles,
                                                     cem_constraints=cem_constraints, cem_constraint_mode=cem_constraint_mode,
                                                     cem_constraint_weight=cem_constraint_weight, cem_knots=cem_knots,
                                                     cem_knot_interp=cem_knot_interp, cem_knot_anchor=cem_knot_anchor,
                                                     cem_tracking=cem_tracking, cem_target_advance=cem_target_advance,
                                                     cem_action_delay=cem_action_delay, cem_action_rate_limit=cem_action_rate_limit,
                                                     cem_action_rate_cost=cem_action_rate_cost, cem_action_advance=cem_action_advance,
                                                     n_forwards=n_forwards, action_dim=None if self.discrete else self.action_space_dims,
                                                     cem_uncertainty=cem_uncertainty, obs_dim=obs_space_dims,
                                                     cem_terminal_value=cem_terminal_value, cem_reward_net=cem_reward_net,
                                                     cem_policy_prior=cem_policy_prior, cem_terminal_q=cem_terminal_q,
                                                     cem_discount=cem_discount, cem_policy_logp=cem_policy_logp)
        if self._opt is not None and self._opt.constraint_params is not None:
            cp = self._opt.constraint_params
            if max(cp.dim[:cp.n]) >= obs_space_dims:
                raise ValueError("cem_constraints read observation dim %d, this env has %d" % (max(cp.dim[:cp.n]), obs_space_dims))
        if self._opt is not None and self._opt.track_params is not None:
            tp = self._opt.track_params
            if max(tp.dim[:tp.n]) >= obs_space_dims:
                raise ValueError("cem_tracking reads observation dim %d, this env has %d" % (max(tp.dim[:tp.n]), obs_space_dims))
        # the actor of `imagine` on a model whose planner declares none (planner.imagine_policy_params): never part of `_opt`, so
        # get_action of such a model stays on the route its cem_* kwargs select
        self._imagine_policy = _planner.imagine_policy_params(imagine_policy, self._opt, obs_dim=obs_space_dims,
                                                              action_dim=self.action_space_dims, discrete=self.discrete)
        # the Gaussian head of that one actor (planner.policy_head_params): None, and every path is as it is without the kwarg
        world = 1
        if process_group is not None and policy_head is not None:
            import torch.distributed as dist
            world = dist.get_world_size(process_group)
        self._policy_head = _planner.policy_head_params(policy_head, has_actor=self._actor_params() is not None, discrete=self.discrete,
                                                        world=world)
        # where the policy prior's proposals come from (planner.policy_proposals_setting): None without a prior; "head" needs the head
        self._proposals = _planner.policy_proposals_setting(self._opt, head_declared=self._policy_head is not None)
        # the actor's log-density as a term of the score (planner.policy_logp_setting): None without cem_policy_logp; it needs the head
        _planner.policy_logp_setting(self._opt, head_declared=self._policy_head is not None, head=self._policy_head)
        self._head_set = False                                # whether the engine holds the head's log-std layer: `set_policy`
        self._sample_call = 0           # policy_sample's own noise counter, as imagine's
        self._plan_carry = self._plan_carry_valid = None      # device tensors [m,K,H,A] float32 / [m] int32 (keep_elites > 0)
        self._plan_phase = None                               # device tensor [m] int32: the knot grid's phase (cem_knot_anchor="episode")
        self._targets = self._target_offset = None            # device tensors [m,T,K] float32 / [m] int32 (cem_tracking): `set_targets`
        self._act_prev = self._act_prefix = None              # device tensors [m,A] / [m,delay,A] float32, NaN = unknown (the actuator model)
        self._value_set = False                               # whether the engine holds a value net (cem_terminal_value): `set_terminal_value`
        self._reward_set = False                              # whether the engine holds a reward net (cem_reward_net): `set_reward_net`
        self._policy_set = False                              # whether the engine holds a policy net (cem_policy_prior, cem_terminal_q): `set_policy`
        self._critics_set = False                             # whether the engine holds Q critics (cem_terminal_q): `set_critics`

        self.env_kind = resolve_env_kind(env)
        self.seed = int(seed)
        self._call = 0
        self._eval_call = 0             # evaluate_horizon's own noise counter: evaluations never shift get_action's draws
        self._imagine_call = 0          # imagine's own noise counter, likewise: the key of a call is (seed, _imagine_call), then it moves on
        self._checked_sig = None        # shape set of the last get_action whose inputs were checked
        self._group = process_group
        self._shard1 = None
        self._check_replicated_left = int(check_replicated_calls)   # sharded get_action calls that still verify replicated inputs
        self._check_replicated_every = int(check_replicated_every)  # ... and every N-th sharded call after those (0: never again)
        self._sharded_calls = 0
        self.engine = HipEngine(self.env_kind, ensemble_size, n_particles, obs_space_dims, self.action_space_dims,
                                self.proc_obs_space_dims, context_out_dim, hidden_sizes, n_forwards,
                                deterministic=deterministic, discrete=self.discrete,
                                reference_quirks=reference_quirks, history_length=history_length,
                                cp_hidden_sizes=cp_hidden_sizes, back_model=back_coeff > 0.0, device=device,
                                hidden_nonlinearity=hidden_nonlinearity,
                                lib=engine_lib)      # engine_lib: developer builds only (tools/ab.sh); None = the product library
        # tf.global_variables_initializer() equivalent (mb_trainer.py:164)
        self.engine.init_weights(np.random.default_rng(self.seed))
        if self._opt is not None and self._opt.discount != 1.0:
            self.engine.set_discount(self._opt.discount)      # state of the engine, set once: every stage and diagnostic reads it there
        if self._proposals is not None:
            self.engine.set_policy_proposals(*self._proposals)      # likewise: the roll of every plan and of `policy_proposals` reads it there
        self._train_ready = False
        self._stats_dirty = True
        self._dist_failed = False
        # The rollout kernel is compiled per geometry: the reference defaults are in the library, anything else
        # (`--hidden_size`, `--context_out_dim`, depth, nonlinearity) is built now (cadm_amd.jit, ~30 s once, then cached),
        # and a launch that cannot fit the hardware (LDS for this horizon) raises here -- not at the first get_action.
        self.engine.ensure_rollout(None, 1, max(1, n_candidates))
        if self._opt is not None and self._opt.keep_elites > self.engine.num_elites:
            raise ValueError("cem_keep_elites=%d exceeds the planner's %d elites" % (self._opt.keep_elites, self.engine.num_elites))
        if self._opt is not None and self._opt.policy_params is not None:
            K, P = self._opt.keep_elites, self._opt.policy_params.n_samples
            least = _planner.policy_min_candidates(n_candidates, self._opt.decay, self.engine.num_elites, K, self.engine.num_cem_iters)
            if K + 1 + P > least:
                raise ValueError("cem_policy_prior: %d kept elites, the mean candidate and %d proposals need %d candidate slots, the smallest "
                                 "iteration has %d" % (K, P, K + 1 + P, least))

    # ------------------------------------------------------------------ planning
    def _push_stats(self):
        if self._stats_dirty:
            keys = ("obs_mean", "obs_std", "act_mean", "act_std", "delta_mean", "delta_std", "cp_obs_mean",
                    "cp_obs_std", "cp_act_mean", "cp_act_std", "back_delta_mean", "back_delta_std")
            stats = self._stats12()
            self.engine.set_stats(dict(zip(keys, stats)))
            self._stats_dirty = False
            opt = getattr(self, "_opt", None)
            if opt is not None and opt.uncertainty is not None and opt.uncertainty[2] == "delta_std":
                # the spread in units of the model's own one-step target scale: w_d = 1 / (sigma_delta_d + 1e-10)^2 of THESE statistics
                sd = np.asarray(stats[5], dtype=np.float64).reshape(-1) + 1e-10
                self._set_uncertainty_w((1.0 / (sd * sd)).astype(np.float32))

    def _set_uncertainty_w(self, w):
        kind, lam, _, form, cap = self._opt.uncertainty
        self._opt = self._opt._replace(uncertainty_params=self.engine.uncertainty_params(kind, lam, w, form, cap, obs_dim=self.obs_space_dims))

    def _require_uncertainty(self, who):
        opt = getattr(self, "_opt", None)
        if opt is None or opt.uncertainty_params is None:
            raise ValueError("%s: this model has no cem_uncertainty" % who)
        return opt

    def set_uncertainty_weights(self, w):
        """Replace the per-dim weights of `cem_uncertainty` from the next call on: None (1 for every dim), a number, or [D] (finite, >= 0, at
        least one > 0; dims with 0 are never read).  A model built with w="delta_std" stops following its statistics: the weights are
        then the caller's."""
        opt = self._require_uncertainty("set_uncertainty_weights")
        if isinstance(w, str):
            raise ValueError("set_uncertainty_weights: w must be None, a number or [D] numbers, got %r" % (w,))
        kind, lam, _, form, cap = opt.uncertainty
        key = None if w is None else (float(w) if np.ndim(w) == 0 else tuple(float(x) for x in np.asarray(w).reshape(-1)))
        self._opt = opt._replace(uncertainty=(kind, lam, key, form, cap))
        self._set_uncertainty_w(w)

    def uncertainty_cost(self, obs, actions, cp_obs=None, cp_act=None, seed=None):
        """What this model's `cem_uncertainty` term makes of `actions` ([m,H,A], or [m,n,H,A]; numpy or tensor) -- the companion of
        `tracking_cost` / `constraint_check`: the context encoder, one rollout that records its trajectories and the uncertainty kernels,
        as numpy arrays (for [m,H,A] input the n axis is dropped):
          step [m,n,H]      the step cost u_t (weighted variance or its square root, capped) of every step
          cost [m,n]        their sum over the counted steps: what the planner multiplies by lambda and takes off the candidate score
          returns [m,n,p]   the rollout's particle returns: what lambda has to be weighed against
        If the model has `cem_constraints` in terminate mode their first violations cut the sum, as in the loop.  The noise is drawn as
        `forecast` draws it: (seed, the last get_action's call) under the forecast's iteration word; no counter moves.  On a model with
        `cem_discount` the cost and the returns are the discounted ones; step stays undiscounted."""
        self._require_uncertainty("uncertainty_cost")
        obs, acts, rows, traj, squeeze = self._replay("uncertainty_cost", obs, actions, cp_obs, cp_act, seed)
        # (the options are read behind the replay: its push of new statistics replaces them with the ones that hold the delta_std weights)
        step, cost = self.engine.uncertainty_cost(traj, self._opt.uncertainty_params, first=self._terminate_first(traj, rows, obs, acts),
                                                  want_steps=True)
        return self._result(squeeze, step=step, cost=cost, returns=self._env_rows(traj, obs, acts, rows))

    def _next_call(self):
        self._call += 1
        return self._call & 0xFFFFFFFF

    def _check_planner_inputs(self, obs, cp_obs, cp_act, cem_init_mean, cem_init_var):
        """Host-side shape checks (the reference would raise a TF shape error; raw device pointers would not)."""
        D, A, Hh, H = self.obs_space_dims, self.action_space_dims, self.history_length, self.n_forwards
        shp = lambda x: tuple(int(v) for v in x.shape)
        m = shp(obs)[0]
        want = {"obs": (obs, (m, D)), "cem_init_mean": (cem_init_mean, (m, H, A)), "cem_init_var": (cem_init_var, (m, H, A))}
        if self.context_out_dim > 0:
            want["cp_obs"] = (cp_obs, (m, D * Hh))
            want["cp_act"] = (cp_act, (m, A * Hh))
            if cp_obs is None or cp_act is None:
                raise ValueError("get_action: cp_obs and cp_act are required for a context model")
        for name, (x, expect) in want.items():
            if x is not None and shp(x) != expect:
                raise ValueError("get_action: %s has shape %r, expected %r" % (name, shp(x), expect))
        if (cem_init_mean is None) != (cem_init_var is None):
            raise ValueError("get_action: cem_init_mean and cem_init_var must be given together")

    def _sharding(self):
        """Candidate shard of this rank.  The sharded planner is the library's loop on every rank; what is negotiated on first use is
        only its collective: the ctx's own RCCL communicator when EVERY rank of the group can build one (backend nccl, one GPU per
        rank), else -- all ranks together -- torch.distributed's all-gather through `cadm_dist_init_external`.  (The second element,
        always True, is kept for callers that asked "is the plan one library call?")"""
        if self._group is None:         # never sharded (the default): nothing to negotiate
            if self._shard1 is None or self._shard1.n != self.n_candidates:
                self._shard1 = _planner.Shard(self.n_candidates)
            return self._shard1, True
        shard = _planner.Shard.from_group(self.n_candidates, self._group)
        if shard.world > 1 and self.engine.dist_world == 1:
            import torch.distributed as dist
            backend = dist.get_backend(self._group)
            ok = 0.0
            if backend == "nccl" and not self._dist_failed:
                ok = 1.0
                try:       # in-library RCCL communicator: the whole sharded planner stays on the stream
                    self.engine.dist_init(self._group)
                except Exception as exc:
                    ok = 0.0
                    logger.log("cadm_amd: in-library RCCL init failed on this rank (%s)" % exc)
            # every rank must take the SAME collective, or some would wait in ncclAllGather and others in torch's
            flag = torch.tensor([ok], device=self.engine.device if backend == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self._group)
            if float(flag.item()) < 1.0:
                if self.engine.dist_world > 1:
                    self.engine.dist_destroy()
                if backend == "nccl":
                    self._dist_failed = True
                    logger.log("cadm_amd: a rank failed in-library RCCL init; all ranks plug torch.distributed's all_gather into the same planner")
                self.engine.dist_init_external(self._group)
        return shard, True

    def _replication_check_due(self, peek=False):
        """Sharded calls only.  Counts the call (unless `peek`: the same call asking again further down) and says whether this one
        verifies that every rank was fed the same inputs: the first `check_replicated_calls` calls, then every
        `check_replicated_every`-th.  Every rank makes the same sequence of calls, so every rank takes the same decision."""
        if not peek:
            self._sharded_calls += 1
        if self._check_replicated_left > 0:
            return True
        return self._check_replicated_every > 0 and self._sharded_calls % self._check_replicated_every == 0

    def get_action(self, obs, cp_obs, cp_act, cem_init_mean=None, cem_init_var=None, return_forecast=False):
        """reference :344-367.  CEM: returns the whole plan [m,H,A]; RS: the first action [m,A]
        (ints [m] for discrete envs).  Continuous outputs are clipped to [-1,1].
        return_forecast=True (an extension; CEM routes only): returns (plan, forecast) -- `forecast` of the returned plan, drawn with
        this call's own (seed, call)."""
        if return_forecast:
            return self._get_action_with_forecast(obs, cp_obs, cp_act, cem_init_mean, cem_init_var)
        if self._stats_dirty:
            self._push_stats()
        if getattr(self, "_opt", None) is not None and cem_init_mean is not None:      # the opt-in planner; None (or a CPU test's stand-in object): today's route
            return self._get_action_opt_in(obs, cp_obs, cp_act, cem_init_mean, cem_init_var)
        nd = np.ndarray
        counted = False
        if (type(obs) is nd and type(cem_init_mean) is nd and type(cem_init_var) is nd and (cp_obs is None or type(cp_obs) is nd)
                and (cp_act is None or type(cp_act) is nd) and obs.shape[0] > 0):
            # the samplers' call, shapes read off the arrays (np.shape / isinstance over five arguments cost ~4 us of a 0.9 ms call)
            sig = (obs.shape, None if cp_obs is None else cp_obs.shape, None if cp_act is None else cp_act.shape, cem_init_mean.shape,
                   cem_init_var.shape)
            if sig == self._checked_sig:
                shard, fused = self._sharding()
                due = False
                if shard.world > 1:      # the call is counted HERE, whatever path it then takes (the torch.distributed
                    due = self._replication_check_due()      # fallback used to re-ask with peek=True without ever having counted)
                    counted = True
                if not due:
                    self._call += 1
                    return self.engine.cem_plan_host((obs, cp_obs, cp_act, cem_init_mean, cem_init_var), self.n_candidates, seed=self.seed,
                                                     call=self._call & 0xFFFFFFFF, shapes=sig)
        m = int(np.shape(obs)[0])
        if m == 0:      # an empty batch of environments: the reference's graph returns empty arrays
            if cem_init_mean is not None:
                return np.zeros((0, self.n_forwards, self.action_space_dims), np.float32)
            return np.zeros((0,), np.int32) if self.discrete else np.zeros((0, self.action_space_dims), np.float32)
        host_in = not any(isinstance(x, torch.Tensor) for x in (obs, cp_obs, cp_act, cem_init_mean, cem_init_var))
        sig = _checked_shapes(self, obs, cp_obs, cp_act, cem_init_mean, cem_init_var)
        call = self._next_call()
        shard, fused = self._sharding()
        check_due = shard.world > 1 and self._replication_check_due(peek=counted)
        if host_in and cem_init_mean is not None and not check_due:
            # the hot path of the samplers' loop: one library call from host arrays to the host plan (clipped in the last kernel)
            return self.engine.cem_plan_host((obs, cp_obs, cp_act, cem_init_mean, cem_init_var), self.n_candidates, seed=self.seed, call=call,
                                             shapes=sig)
        if host_in:
            obs, cp_obs, cp_act, cem_init_mean, cem_init_var = self.engine.stage((obs, cp_obs, cp_act, cem_init_mean, cem_init_var))
        if check_due:      # first calls + every N-th: one blocking all-reduce + a host sync
            self._check_replicated_left = max(0, self._check_replicated_left - 1)
            _planner.check_replicated([self.engine._t(x) for x in (obs, cp_obs, cp_act, cem_init_mean) if x is not None], shard)
        if cem_init_mean is not None:
            # the plan lands in a persistent pinned host buffer (written by the last refit kernel): one stream
            # synchronisation instead of an allocation + D2H copy per call
            eng = self.engine
            host = eng.host_out((m, self.n_forwards, self.action_space_dims))
            eng.cem_plan(obs, cp_obs, cp_act, cem_init_mean, cem_init_var, self.n_candidates, seed=self.seed, call=call, out=host)
            torch.cuda.current_stream(eng.device).synchronize()
            action = host.numpy().copy()
            if shard.world > 1 and eng.dist_mismatch():      # (the sharded refit checks every rank's input checksum on every call)
                raise RuntimeError(eng.MISMATCH_MSG)
            return action if self.discrete else np.minimum(np.maximum(action, -1.0), 1.0)
        action = self.engine.rs_plan(obs, cp_obs, cp_act, self.n_candidates, seed=self.seed, call=call)
        action = action.cpu().numpy()
        if not self.discrete:
            action = np.minimum(np.maximum(action, -1.0), 1.0)
        return action

    def _plan_opt_in(self, obs, cp_obs, cp_act, cem_init_mean, cem_init_var, out=None):
        """One planned call of the opt-in loop under this model's switches (`HipEngine.opt_in_plan`: `cadm_icem_plan`, `cadm_mppi_plan` with
        cem_update="mppi", `cadm_scored_plan` with a non-default cem_score), for get_action and caller.DevicePlannerState alike: the elites
        it keeps for the next call stay on the device, here; it draws the call number."""
        eng, K, m = self.engine, self._opt.keep_elites, int(np.shape(obs)[0])
        if K > 0 and (self._plan_carry is None or self._plan_carry.shape[0] != m):      # first call, or another number of envs: nothing carried
            self._plan_carry = torch.zeros((m, K, self.n_forwards, self.action_space_dims), dtype=torch.float32, device=eng.device)
            self._plan_carry_valid = torch.zeros((m,), dtype=torch.int32, device=eng.device)
        episode = self._opt.knots is not None and self._opt.knots[2] == "episode"
        if episode and (self._plan_phase is None or self._plan_phase.shape[0] != m):      # likewise: the grid hangs on this call's first step
            self._plan_phase = torch.zeros((m,), dtype=torch.int32, device=eng.device)
        extra = dict(phase=self._plan_phase) if episode else {}
        tracked = self._opt.track_params is not None
        if tracked:
            if self._targets is None:
                raise RuntimeError("get_action: this model plans under cem_tracking and has no targets (call set_targets first)")
            if self._targets.shape[0] != m or self._targets.shape[2] != self._opt.track_params.n:
                raise ValueError("get_action: the targets are %r, this call has %d envs and cem_tracking %d terms: expected [%d,T,%d]"
                                 % (tuple(self._targets.shape), m, self._opt.track_params.n, m, self._opt.track_params.n))
            extra.update(targets=self._targets, target_offset=self._target_offset)
        if self._opt.actuator_params is not None:      # first call, or another number of envs: nothing applied, nothing committed; the
            self._actuator_tensors(m)                  # library moves both on behind the plan, on the engine's stream (cem_action_advance)
            extra.update(act_prev=self._act_prev, act_prefix=self._act_prefix)
        for net, row in _NETS.items():      # value, reward, policy, critics: every declared net is registered ...
            if getattr(self._opt, row.field) is not None:
                _need_net(self, net, "get_action", under=row.kwarg)
        if self._opt.critic_params is not None:      # ... and so is the actor the critics are evaluated at
            _need_net(self, "policy", "get_action", under="cem_terminal_q")
        if self._opt.logp_params is not None:        # ... and the actor whose density scores the plans, with its head
            _need_net(self, "policy", "get_action", under="cem_policy_logp")
            if not self._head_set:
                raise RuntimeError("get_action: this model plans under cem_policy_logp and has no registered Gaussian head (call set_policy first)")
        call = self._next_call()
        if not any(isinstance(x, torch.Tensor) for x in (obs, cp_obs, cp_act, cem_init_mean, cem_init_var)):
            obs, cp_obs, cp_act, cem_init_mean, cem_init_var = eng.stage((obs, cp_obs, cp_act, cem_init_mean, cem_init_var))
        if self.context_out_dim == 0:
            cp_obs = cp_act = None
        plan = eng.opt_in_plan(self._opt, obs, cp_obs, cp_act, cem_init_mean, cem_init_var, self.n_candidates, carry=self._plan_carry,
                               carry_valid=self._plan_carry_valid, seed=self.seed, call=call, out=out, **extra)
        if episode:      # the horizon recedes by one step per call, the breakpoints stay where they are in episode time (torch ops on the
            self._plan_phase.add_(1).remainder_(self._opt.knots[0])      # engine's stream, behind the plan: no host synchronisation)
        if tracked and self._opt.target_advance:      # likewise: the next call's step 0 is this call's step 1 of the reference
            self._target_offset.add_(1)
        return plan

    # ------------------------------------------------------------------ actuator model (INTEGRATION.md "Actuator model")
    def _actuator_tensors(self, m):
        """The actuator state for m envs, allocated on first use and again -- all NaN -- for another number of envs."""
        if self._act_prev is None or self._act_prev.shape[0] != m:
            nan = float("nan")
            self._act_prev = torch.full((m, self.action_space_dims), nan, dtype=torch.float32, device=self.engine.device)
            self._act_prefix = torch.full((m, self._opt.actuator_params.delay, self.action_space_dims), nan, dtype=torch.float32,
                                          device=self.engine.device)

    def _require_actuator(self, who):
        opt = getattr(self, "_opt", None)
        if opt is None or opt.actuator_params is None:
            raise ValueError("%s: this model has no actuator model (cem_action_delay / cem_action_rate_limit / cem_action_rate_cost)" % who)
        return opt.actuator_params

    def set_applied_actions(self, prev=None, committed=None, mask=None):
        """Tell the actuator model what the device was really told: prev [m,A], the action applied immediately before the next plan's
        step 0, and / or committed [m,delay,A], the actions already decided for its steps 0 .. delay-1 -- for a caller whose executed
        action differs from the plan, who starts an episode with a known command, or who advances the state themselves
        (`cem_action_advance=False`).  NaN: unknown / that step is free.  None leaves that part as it is; mask [m]: only the envs where
        it is set are written."""
        prm = self._require_actuator("set_applied_actions")
        given = [np.shape(x)[0] for x in (prev, committed) if x is not None]
        if not given:
            return
        m, A, d = int(given[0]), self.action_space_dims, prm.delay
        for name, x, shp in (("prev", prev, (m, A)), ("committed", committed, (m, d, A))):
            if x is not None and tuple(int(v) for v in np.shape(x)) != shp:
                raise ValueError("set_applied_actions: %s %r, expected %r" % (name, tuple(np.shape(x)), shp))
        eng = self.engine
        self._actuator_tensors(m)
        mk = None
        if mask is not None:
            mk = eng._t(np.asarray(mask) if not isinstance(mask, torch.Tensor) else mask, dtype=torch.bool).reshape(-1)
            if mk.shape[0] != m:
                raise ValueError("set_applied_actions: mask has %d entries, expected %d" % (mk.shape[0], m))
        for x, dst in ((prev, self._act_prev), (committed, self._act_prefix)):
            if x is None:
                continue
            src = eng._t(x)
            if mk is None:
                dst.copy_(src)
            else:
                dst.copy_(torch.where(mk.reshape((m,) + (1,) * (dst.dim() - 1)), src, dst))

    def actuator_state(self):
        """dict(prev [m,A], committed [m,delay,A]) as numpy copies (NaN: unknown / free), or None before the first planned call."""
        self._require_actuator("actuator_state")
        if self._act_prev is None:
            return None
        return dict(prev=self._act_prev.cpu().numpy(), committed=self._act_prefix.cpu().numpy())

    def action_cost(self, actions):
        """What the actuator model makes of `actions` ([m,H,A], or [m,n,H,A]; numpy or tensor) under the current state and parameters, and
        what that costs -- the companion of `tracking_cost`: dict(cost [m,n], actions [m,n,H,A]) as numpy arrays (for [m,H,A] input the n
        axis is dropped).  Moves no counter and no state; the caller's array is not written.  On a model with `cem_discount` the cost is
        the discounted one."""
        prm = self._require_actuator("action_cost")
        eng = self.engine
        acts = eng._t(actions)
        if acts.dim() not in (3, 4) or tuple(acts.shape[-2:]) != (self.n_forwards, self.action_space_dims):
            raise ValueError("action_cost: actions %r, expected [m,%d,%d] or [m,n,%d,%d]"
                             % (tuple(acts.shape), self.n_forwards, self.action_space_dims, self.n_forwards, self.action_space_dims))
        acts = acts.contiguous().clone()
        m = acts.shape[0]
        prev = prefix = None
        if self._act_prev is not None:
            if self._act_prev.shape[0] != m:
                raise ValueError("action_cost: actions for %d envs, the actuator state holds %d" % (m, self._act_prev.shape[0]))
            prev, prefix = self._act_prev, self._act_prefix
        acts, cost = eng.actuate_actions(acts, prm, prev=prev, prefix=prefix, want_cost=True)
        return dict(cost=cost.cpu().numpy(), actions=acts.cpu().numpy())

    # ------------------------------------------------------------------ tracking targets (INTEGRATION.md "Tracking targets at run time")
    def set_targets(self, targets, offset=None):
        """The targets `cem_tracking`'s terms are held against from the next get_action on: [m,K] (a constant goal per env) or [m,T,K] (a
        reference of T rows per env; K: the number of terms, in their order), numpy or tensor, kept on the device.  NaN: no target for
        that term at that row.  Step t of a plan is compared with row clamp(offset + t, 0, T - 1) of its env; offset [m] ints (None:
        zeros) -- with `cem_target_advance=True` the model moves every env's on by one per planned call, `reset_plan_carry(mask)` puts
        the masked envs' back to 0."""
        opt = getattr(self, "_opt", None)
        if opt is None or opt.track_params is None:
            raise ValueError("set_targets: this model has no cem_tracking")
        K = opt.track_params.n
        shp = tuple(int(v) for v in np.shape(targets))
        if len(shp) not in (2, 3) or shp[0] < 1 or shp[-1] != K or (len(shp) == 3 and shp[1] < 1):
            raise ValueError("set_targets: targets %r, expected [m,%d] or [m,T,%d] with m, T >= 1 (one column per cem_tracking term)" % (shp, K, K))
        if offset is not None and tuple(int(v) for v in np.shape(offset)) != (shp[0],):
            raise ValueError("set_targets: offset %r, expected [%d]" % (tuple(np.shape(offset)), shp[0]))
        eng = self.engine
        t = eng._t(targets)
        self._targets = (t[:, None] if t.dim() == 2 else t).contiguous().clone()      # (the model's own copy: a later edit of the caller's tensor changes no plan)
        if offset is None:
            self._target_offset = torch.zeros((shp[0],), dtype=torch.int32, device=eng.device)
        else:
            self._target_offset = eng._t(offset, dtype=torch.int32).clone()

    def clear_targets(self):
        """Forget the targets and their offsets: get_action on a model with `cem_tracking` then raises until `set_targets` is called."""
        self._targets = self._target_offset = None

    def tracking_cost(self, obs, actions, cp_obs=None, cp_act=None, seed=None):
        """What this model's `cem_tracking` terms cost `actions` ([m,H,A], or [m,n,H,A]; numpy or tensor) against the current targets and
        offsets -- the companion of `constraint_check`: the context encoder, one rollout that records its trajectories and the tracking
        kernel, as numpy arrays (for [m,H,A] input the n axis is dropped):
          cost [m,n,p]               the tracking cost per particle
          returns [m,n,p]            the tracked particle returns (returns_untracked - cost), as the planner scores them without constraints
          returns_untracked [m,n,p]  the rollout's own returns: what `w` has to be weighed against
        The noise is drawn as `forecast` draws it: (seed, the last get_action's call) under the forecast's iteration word; the planner's
        call counter and the offsets do not move.  On a model with `cem_discount` the cost and both returns are the discounted ones."""
        if self._opt is None or self._opt.track_params is None:
            raise ValueError("tracking_cost: this model has no cem_tracking")
        if self._targets is None:
            raise RuntimeError("tracking_cost: this model has no targets (call set_targets first)")
        obs, acts, raw, traj, squeeze = self._replay("tracking_cost", obs, actions, cp_obs, cp_act, seed)
        raw = self._env_rows(traj, obs, acts, raw)
        rows, cost = self.engine.tracking_returns(traj, raw, self._opt.track_params, self._targets, offset=self._target_offset, want_cost=True)
        return self._result(squeeze, cost=cost, returns=rows, returns_untracked=raw)

    # ------------------------------------------------------------------ terminal value (INTEGRATION.md "Terminal value")
    def set_terminal_value(self, weights, obs_mean=None, obs_std=None):
        """The value net of `cem_terminal_value` from the next call on: `weights` a list of (W [in,out], b [out]) per layer, numpy or
        torch, or a torch.nn.Sequential of Linear and ReLU / Tanh / SiLU modules (Linear.weight is transposed on import) -- of the
        declared layer sizes and activation, else it is refused; obs_mean / obs_std [D] (None: 0 / 1, std finite and > 0): the net reads
        (obs - obs_mean) / obs_std of the raw observation.  Everything is copied: a later edit of the caller's tensors changes no plan.
        Replacing the net rebuilds nothing."""
        opt = _require_net(self, "value", "set_terminal_value")
        _register_net(self, "value", opt.value_params, weights, obs_mean, obs_std)

    def clear_terminal_value(self):
        """Remove the value net: get_action on a model with `cem_terminal_value` then raises until `set_terminal_value` is called."""
        _require_net(self, "value", "clear_terminal_value")
        _register_net(self, "value", None)

    def terminal_value(self, states):
        """V of raw observations `states` [..., D] (numpy or tensor) through the planner's kernel -> numpy [...]; NaN for a state with a
        non-finite value."""
        _require_net(self, "value", "terminal_value", need_net=True)
        return self.engine.value_eval(states).cpu().numpy()

    def plan_terminal_value(self, obs, actions, cp_obs=None, cp_act=None, seed=None):
        """What this model's terminal value adds for `actions` ([m,H,A], or [m,n,H,A]; numpy or tensor) -- the companion of
        `tracking_cost`: the context encoder, one rollout that records its trajectories and the value kernel, as numpy arrays (for [m,H,A]
        input the n axis is dropped):
          value [m,n,p]     V of every particle's last state (NaN: a diverged particle, or one the constraints ended before the horizon);
                            the planner adds weight * value to the particle's return
          first [m,n,p]     with `cem_constraints` in terminate mode their first violations (a particle with first < H gets no value), else None
        The noise is drawn as `forecast` draws it: (seed, the last get_action's call) under the forecast's iteration word; no counter moves.
        On a model with `cem_discount` the planner adds weight * gamma^H * value (`plan_returns`' weights[H]); value itself is V."""
        opt = _require_net(self, "value", "plan_terminal_value", need_net=True)
        obs, acts, rows, traj, squeeze = self._replay("plan_terminal_value", obs, actions, cp_obs, cp_act, seed)
        first = self._terminate_first(traj, rows, obs, acts)
        _, v = self.engine.value_returns(traj, rows, opt.value_params, first=first, want_v=True)
        return self._result(squeeze, value=v, first=first)

    # ------------------------------------------------------------------ terminal value from Q critics (INTEGRATION.md "Terminal value from Q critics")
    def set_critics(self, nets, in_mean=None, in_std=None):
        """The Q critics of `cem_terminal_q` from the next call on: `nets` a list of n_critics nets, each what `set_terminal_value` takes
        (a list of (W [in,out], b [out]) per layer or a torch.nn.Sequential) with D + A inputs -- of the declared layer sizes and
        activation, else it is refused; in_mean / in_std [D + A] (None: 0 / 1): every critic reads ([obs ; act] - in_mean) / in_std of
        the raw observation and the actor's clipped action.  Everything is copied; replacing the critics rebuilds nothing."""
        opt = _require_net(self, "critics", "set_critics")
        _register_net(self, "critics", opt.critic_params, nets, in_mean, in_std)

    def clear_critics(self):
        """Remove the critics: get_action on a model with `cem_terminal_q` then raises until `set_critics` is called."""
        _require_net(self, "critics", "clear_critics")
        _register_net(self, "critics", None)

    def q_value(self, states, actions=None, return_each=False):
        """The reduced Q of raw observations `states` [..., D] (numpy or tensor) through the planner's kernel -> numpy [...]: at the
        policy net's action (actions None; `set_policy` first), or at `actions` [..., A].  NaN for a state (or action) with a non-finite
        value.  return_each: (q, each [n_critics, ...]), every critic's own value."""
        _require_net(self, "critics", "q_value", need_net=True, need_actor=actions is None)
        out = self.engine.critic_eval(states, actions, want_each=return_each)
        return (out[0].cpu().numpy(), out[1].cpu().numpy()) if return_each else out.cpu().numpy()

    def plan_terminal_q(self, obs, actions, cp_obs=None, cp_act=None, seed=None):
        """What this model's terminal Q adds for `actions` ([m,H,A], or [m,n,H,A]; numpy or tensor) -- the companion of
        `plan_terminal_value`: the context encoder, one rollout that records its trajectories and the fused actor / critics kernel, as
        numpy arrays (for [m,H,A] input the n axis is dropped):
          q [m,n,p]         reduce_c Q_c(s_H, pi(s_H)) of every particle's last state (NaN: a diverged particle, or one the constraints
                            ended before the horizon); the planner adds weight * q to the particle's return
          first [m,n,p]     with `cem_constraints` in terminate mode their first violations (a particle with first < H gets no q), else None
        The noise is drawn as `forecast` draws it: (seed, the last get_action's call) under the forecast's iteration word; no counter moves.
        On a model with `cem_discount` the planner adds weight * gamma^H * q (`plan_returns`' weights[H]); q itself is the reduced Q."""
        opt = _require_net(self, "critics", "plan_terminal_q", need_net=True, need_actor=True)
        obs, acts, rows, traj, squeeze = self._replay("plan_terminal_q", obs, actions, cp_obs, cp_act, seed)
        first = self._terminate_first(traj, rows, obs, acts)
        _, q = self.engine.critic_returns(traj, rows, opt.critic_params, first=first, want_q=True)
        return self._result(squeeze, q=q, first=first)

    # ------------------------------------------------------------------ policy prior (INTEGRATION.md "Policy prior")
    def _actor_params(self):
        """the `PolicyParams` this model's actor is registered under: the planner's declaration, else `imagine_policy`'s; None without one"""
        opt = getattr(self, "_opt", None)
        prm = None if opt is None else opt.actor_params()
        return prm if prm is not None else getattr(self, "_imagine_policy", None)

    def set_policy(self, weights, obs_mean=None, obs_std=None):
        """The policy net of `cem_policy_prior` (or the actor of `cem_terminal_q` / `imagine_policy`) from the next call on: `weights` as `set_terminal_value` takes them (a list of (W [in,out],
        b [out]) per layer or a torch.nn.Sequential of Linear and ReLU / Tanh / SiLU modules, the last Linear with A outputs) -- of the
        declared layer sizes and activation, else it is refused; obs_mean / obs_std [D] (None: 0 / 1): the net reads (obs - obs_mean) /
        obs_std of the raw observation.  Everything is copied; replacing the net rebuilds nothing."""
        _require_policy(self, "set_policy")      # (the actor of cem_terminal_q or imagine_policy alone: registered with n_samples = 1)
        head = getattr(self, "_policy_head", None)
        if head is None:
            _register_net(self, "policy", self._actor_params(), weights, obs_mean, obs_std)
            return
        # a SAC actor: the mean columns are the mode actor every existing path reads, the log-std columns hang on it as the head
        prm = self._actor_params()
        layers, act = HipEngine.value_weights(weights)
        if act is not None and _planner._lib.VALUE_ACTS[act] != prm.activation:
            raise ValueError("set_policy: the module's activation %r is not the declared one" % (act,))
        mean_layers, W_ls, b_ls = _planner.split_gaussian_layers(layers, self.action_space_dims)
        self._head_set = False
        _register_net(self, "policy", prm, mean_layers, obs_mean, obs_std)
        self.engine.set_policy_head(head, W_ls, b_ls)
        self._head_set = True

    def clear_policy(self):
        """Remove the policy net: get_action on a model with `cem_policy_prior` then raises until `set_policy` is called."""
        _require_policy(self, "clear_policy")
        _register_net(self, "policy", None)      # (the library drops the head with the net)
        self._head_set = False

    def policy_action(self, states):
        """The policy's action of raw observations `states` [..., D] (numpy or tensor) through the planner's kernel -> numpy [..., A]:
        squashed and clipped to the action bounds, no noise; clip(0, lb, ub) for a state with a non-finite value."""
        _require_policy(self, "policy_action", need_net=True)
        return self.engine.policy_eval(states).cpu().numpy()

    def policy_sample(self, states, seed=None, numpy=True):
        """Actions drawn from the stochastic actor (`policy_head`) for raw observations `states` [..., D] -> dict(act [..., A], logp
        [...], mode [..., A]): a ~ pi(. | s) squashed and clipped as the actor is, its log-density (the unclipped Gaussian's for
        squash="none"), and `policy_action`'s action.  A state with a non-finite value: act = mode = clip(0, lb, ub), logp = NaN.  The
        draws are keyed (seed, a counter of policy_sample's own): get_action's and imagine's draws never move."""
        _require_policy(self, "policy_sample", need_net=True)
        if getattr(self, "_policy_head", None) is None or not getattr(self, "_head_set", False):
            raise ValueError("policy_sample: this model has no registered Gaussian head (declare policy_head, then set_policy)")
        call = self._sample_call & 0xFFFFFFFF
        self._sample_call += 1
        out = self.engine.policy_sample(states, seed=int(self.seed if seed is None else seed) & 0xFFFFFFFF, call=call)
        return {k: v.cpu().numpy() for k, v in out.items()} if numpy else out

    def _require_head(self, who):
        """Refuse for `who` while the model has no actor with a registered Gaussian head."""
        _require_policy(self, who, need_net=True)
        if getattr(self, "_policy_head", None) is None or not getattr(self, "_head_set", False):
            raise ValueError("%s: this model has no registered Gaussian head (declare policy_head, then set_policy)" % who)

    def policy_log_prob(self, states, actions, space="action", numpy=True):
        """log pi(a | s) of GIVEN `actions` [..., A] at raw observations `states` [..., D] under the stochastic actor (`policy_head`)
        -> [...]: the density `policy_sample` reports for its own draws, evaluated at actions the caller brings (stored transitions
        under the current actor, a planner's actions before they are distilled).  space "action": the squashed actor's density;
        "pre_squash": the Gaussian's density of atanh of the normalised action, without the Jacobian (for squash="none" the two agree).
        An action on or beyond a bound is clamped to |y| = 0.999999 first.  NaN for a row with a non-finite state or action.  Works on
        any model with a registered head, with or without `cem_policy_logp`; nothing is drawn and no counter moves."""
        self._require_head("policy_log_prob")
        out = self.engine.policy_log_prob(states, actions, space)
        return out.cpu().numpy() if numpy else out

    def plan_policy_log_prob(self, obs, actions, cp_obs=None, cp_act=None, seed=None):
        """The actor's log-density along `actions` ([m,H,A], or [m,n,H,A]; numpy or tensor) -- the companion of `plan_rewards` for
        `cem_policy_logp`: the context encoder, one rollout that records its trajectories and the log-density kernels, as numpy arrays
        (for [m,H,A] input the n axis is dropped):
          logp [m,n,p,H]    log pi(a_t | s_t) of every step of every particle (NaN: a step with a non-finite state or action, or one
                            behind a particle's first violation)
          total [m,n,p]     the sum over the counted steps in ascending t; the planner adds weight * total to the particle's return
          first [m,n,p]     with `cem_constraints` in terminate mode their first violations (steps t <= first count), else None
        The noise is drawn as `forecast` draws it: (seed, the last get_action's call) under the forecast's iteration word; no counter moves.
        On a model with `cem_discount` total is the discounted sum (gamma^t * logp_t); logp stays undiscounted."""
        opt = getattr(self, "_opt", None)
        if opt is None or opt.logp_params is None:
            raise ValueError("plan_policy_log_prob: this model has no cem_policy_logp")
        self._require_head("plan_policy_log_prob")
        obs, acts, rows, traj, squeeze = self._replay("plan_policy_log_prob", obs, actions, cp_obs, cp_act, seed)
        first = self._terminate_first(traj, rows, obs, acts)
        _, steps, total = self.engine.policy_logp_returns(traj, obs, acts, rows, self._opt.logp_params, first=first, want_steps=True)
        return self._result(squeeze, logp=steps.permute(1, 2, 3, 0), total=total, first=first)

    def policy_proposals(self, obs, cp_obs=None, cp_act=None, seed=None, return_states=False):
        """The sequences the policy prior would inject for `obs` [m,D] (with a context model its history cp_obs / cp_act) -> numpy
        [m,n_samples,H,A]: the context encoder and the proposal roll, drawn under (seed, the last get_action's call); no counter moves.
        return_states: (proposals, states [H,m,n_samples,p,D]), the particle states every step's actions were computed from."""
        opt = _require_net(self, "policy", "policy_proposals", need_net=True)
        self._push_stats()
        D, m = self.obs_space_dims, int(np.shape(obs)[0])
        if tuple(np.shape(obs)) != (m, D) or m == 0:
            raise ValueError("policy_proposals: obs %r, expected [m,%d] with m >= 1" % (tuple(np.shape(obs)), D))
        if self.context_out_dim > 0 and (cp_obs is None or cp_act is None):
            raise ValueError("policy_proposals: cp_obs and cp_act are required for a context model")
        eng = self.engine
        out = eng.policy_propose(opt.policy_params, eng._t(obs).contiguous(), self._context_vec(cp_obs, cp_act), want_states=return_states,
                                 **self._replay_key(seed))
        return (out[0].cpu().numpy(), out[1].cpu().numpy()) if return_states else out.cpu().numpy()

    # ------------------------------------------------------------------ imagined rollouts (INTEGRATION.md "Imagined rollouts for a learner")
    def imagine(self, obs, cp_obs=None, cp_act=None, horizon=1, branches=1, actions=None, noise_std=0.0, disagreement_w=None, seed=None,
                numpy=False, sample=None):
        """Model-generated experience for a learner (MBPO / Dyna): `branches` independent rollouts of `horizon` steps from each start state
        obs [m,D] (with a context model each state's own history cp_obs / cp_act, as `policy_proposals` takes them), as transitions.
        Actions: the registered actor (`set_policy`) on every row's own state, perturbed by noise_std * xi and clipped on EVERY row; or
        `actions` [m,branches,horizon,A], raw and clipped to the bounds, with no policy registered -- one source per call.  Every step is a
        one-step rollout of the planner's kernels, so horizon is independent of n_forwards; of the n_particles predictions of a row
        (every member n_particles / E times) ONE is kept, drawn uniformly (MBPO's scheme).  Returns a dict of device tensors (numpy=True:
        numpy copies) of static shape, k = horizon, n = branches:
          states [k+1,m,n,D]   with the views obs = states[:-1] and next_obs = states[1:]
          act [k,m,n,A]; rew [k,m,n]   the action taken; the rollout's own step reward of the kept particle -- what the planner scores by
          done, valid [k,m,n] uint8    valid: a transition to train on; done: it ended the row (the state left `cem_constraints`)
          member [k,m,n] int32         the ensemble member that predicted it (-1: the row was dead)
          disagreement [k,m,n]         sum_d w_d * (epistemic variance of dim d over the row's particles) as `cem_uncertainty` computes it
                                       (kind="epistemic", form="var", no cap); w: disagreement_w -- None (1), [D], or "delta_std"; +inf if not finite
          length [m,n] int32; n_valid  the valid transitions of a row; of the call (a 0-dim tensor; numpy=True: an int)
        A row whose kept particle is not finite stops without a valid transition; a row behind its end is frozen at its last state with
        valid = 0, rew = 0, member = -1, disagreement = 0.  Nothing is compacted: out["obs"][out["valid"].bool()] is the flat batch.
        `cem_constraints` (either mode) define termination; `cem_reward_net` with a registered net adds weight * R(s, a, s') to rew, and the
        dict then also holds rew_env and rew_net (0 where not valid).  The other planner options -- knots, tracking, the actuator model,
        uncertainty pricing, the discount, the terminal value or Q -- change nothing here.  A deterministic model draws no head noise and
        still draws the kept particle.  The noise is keyed (seed, a counter of imagine's own): get_action's draws never move.
        sample (models with `policy_head`): None -- True exactly when a head is declared and `actions` is None; True: every action is
        drawn from the actor's Gaussian head on the row's own state, and the dict also holds logp [k,m,n], the log-density of act[t] at
        states[t] (computed on every row, meaningful where valid); False: the mode action plus noise_std, as without a head."""
        import torch.distributed as dist
        world = dist.get_world_size(self._group) if self._group is not None else 1
        a = _planner.imagine_args(obs, cp_obs, cp_act, horizon, branches, actions, noise_std, disagreement_w, obs_dim=self.obs_space_dims,
                                  action_dim=self.action_space_dims, n_particles=self.n_particles, context=self.context_out_dim > 0,
                                  history_length=self.history_length, discrete=self.discrete, world=world,
                                  policy_registered=self._policy_set, sample=sample,
                                  head_declared=getattr(self, "_policy_head", None) is not None, head_registered=getattr(self, "_head_set", False))
        self._push_stats()
        eng, opt = self.engine, getattr(self, "_opt", None)
        w = a.w
        if isinstance(w, str):      # the spread in units of the model's own one-step target scale, as cem_uncertainty's "delta_std"
            sd = np.asarray(self._stats12()[5], dtype=np.float64).reshape(-1) + 1e-10
            w = (1.0 / (sd * sd)).astype(np.float32)
        ctx_vec = eng.context_forward(cp_obs, cp_act) if self.context_out_dim > 0 else None
        call = self._imagine_call & 0xFFFFFFFF
        self._imagine_call += 1
        out = eng.imagine(eng._t(obs).contiguous(), ctx_vec, a.k, a.n, actions, a.noise_std,
                          None if opt is None else opt.constraint_params, w, int(self.seed if seed is None else seed) & 0xFFFFFFFF, call,
                          sample=a.sample)
        out.pop("alive")
        out["obs"], out["next_obs"] = out["states"][:-1], out["states"][1:]
        out["n_valid"] = out["valid"].sum()
        if opt is not None and opt.reward_params is not None and self._reward_set:
            parts = {"next_obs": (out["next_obs"],), "obs_act": (out["obs"], out["act"]),
                     "obs_act_next_obs": (out["obs"], out["act"], out["next_obs"])}[opt.reward[0]]
            r = eng.reward_eval(torch.cat(parts, dim=-1))
            out["rew_env"] = out["rew"]
            out["rew_net"] = torch.where(out["valid"].bool(), r, torch.zeros_like(r))
            out["rew"] = out["rew_env"] + out["rew_net"] * float(np.float32(opt.reward_params.weight))      # (one multiply, then one add: two launches)
        if numpy:
            out = {k: (int(v) if k == "n_valid" else v.cpu().numpy()) for k, v in out.items()}
        return out

    def imagine_targets(self, batch, gamma, lam=0.95, bootstrap="auto", penalty=0.0, max_disagreement=None, steve=None, numpy=False):
        """What a critic is trained on, out of the dict `batch` that `imagine` returned (device tensors are taken as they are, numpy arrays
        are uploaded) and bootstrap values of its states, in one launch (INTEGRATION.md "Value-expansion targets").  bootstrap: "value" --
        V of the registered value net on batch["states"] (`cem_terminal_value`); "q" -- the critics at the actor's action
        (`cem_terminal_q`); a [k+1,m,n] tensor or array -- the caller's own values, e.g. a target network's, on any model; "auto" --
        value or q, whichever the model declares.  penalty: rew - penalty * disagreement is the step reward (MOPO); max_disagreement: a
        row is cut in front of the first step whose disagreement exceeds it (M2AC).  Returns a dict of device tensors (numpy=True: numpy
        copies), k = horizon, n = branches:
          lambda_return [k,m,n]        the lambda-return of states[t] (Dreamer, TD-MPC); 0 where the step is not used
          nstep, nstep_ok [k,m,n]      the h = t + 1 step target of the START state and whether it exists (MVE)
          used [k,m,n] uint8           the steps in front of the row's end: valid and within max_disagreement
          boot [k+1,m,n]               the bootstrap values that were used
        and with steve=dict(var_floor=): steve [m], the n-step targets of a start state averaged over the horizons with weights inverse
        to their variance over the branches (STEVE); steve_weight, steve_mean, steve_var [k,m]; steve_count [k,m] int32;
        steve_fallback [m] uint8 (no horizon had two targets: steve is boot[0]).  A diverged row bootstraps from its last finite state,
        a terminated row does not bootstrap.  Draws no noise and moves no counter."""
        opt = getattr(self, "_opt", None)
        a = _planner.imagine_targets_args(batch, gamma, lam, bootstrap, penalty, max_disagreement, steve,
                                          has_value=opt is not None and opt.value_params is not None,
                                          has_q=opt is not None and opt.critic_params is not None)
        eng = self.engine
        if a.bootstrap == "value":
            _require_net(self, "value", "imagine_targets", need_net=True)
            boot = eng.value_eval(batch["states"])
        elif a.bootstrap == "q":
            _require_net(self, "critics", "imagine_targets", need_net=True, need_actor=True)
            boot = eng.critic_eval(batch["states"])
        else:
            boot = eng._t(bootstrap)
        out = eng.imagine_targets(eng._t(batch["rew"]), eng._t(batch["valid"], dtype=torch.uint8), eng._t(batch["done"], dtype=torch.uint8),
                                  eng._t(batch["disagreement"]), boot.contiguous(), a.gamma, a.lam, a.penalty, a.max_disagreement, a.var_floor)
        out["boot"] = boot
        if numpy:
            out = {k: v.cpu().numpy() for k, v in out.items()}
        return out

    # ------------------------------------------------------------------ learned reward (INTEGRATION.md "Learned reward")
    def set_reward_net(self, weights, in_mean=None, in_std=None):
        """The reward net of `cem_reward_net` from the next call on: `weights` as `set_terminal_value` takes them (a list of (W [in,out],
        b [out]) per layer, or a torch.nn.Sequential of Linear and ReLU / Tanh / SiLU modules) -- of the declared input, layer sizes and
        activation, else it is refused; in_mean / in_std [K] over the concatenated input (None: 0 / 1, std finite and > 0): the net reads
        (input - in_mean) / in_std of the raw observations and actions.  Everything is copied; replacing the net rebuilds nothing."""
        opt = _require_net(self, "reward", "set_reward_net")
        _register_net(self, "reward", opt.reward_params, weights, in_mean, in_std)

    def clear_reward_net(self):
        """Remove the reward net: get_action on a model with `cem_reward_net` then raises until `set_reward_net` is called."""
        _require_net(self, "reward", "clear_reward_net")
        _register_net(self, "reward", None)

    def reward_net(self, obs=None, act=None, next_obs=None):
        """R of raw transitions through the planner's kernel -> numpy [...]: obs [..., D], act [..., A], next_obs [..., D] (numpy or
        tensor), of which the declared `inputs` says which are read and concatenated (the others may be None); NaN for an input with a
        non-finite value."""
        opt = _require_net(self, "reward", "reward_net", need_net=True)
        eng = self.engine
        need = {"next_obs": (("next_obs", next_obs, eng.D),), "obs_act": (("obs", obs, eng.D), ("act", act, eng.A)),
                "obs_act_next_obs": (("obs", obs, eng.D), ("act", act, eng.A), ("next_obs", next_obs, eng.D))}[opt.reward[0]]
        parts = []
        for name, x, dim in need:
            if x is None or np.ndim(x) < 1 or np.shape(x)[-1] != dim:
                raise ValueError("reward_net: inputs %r need %s [..., %d], got %r" % (opt.reward[0], name, dim, None if x is None else tuple(np.shape(x))))
            parts.append(eng._t(x))
        if any(t.shape[:-1] != parts[0].shape[:-1] for t in parts):
            raise ValueError("reward_net: the leading shapes %r do not agree" % ([tuple(t.shape) for t in parts],))
        return eng.reward_eval(torch.cat(parts, dim=-1)).cpu().numpy()

    def plan_rewards(self, obs, actions, cp_obs=None, cp_act=None, seed=None):
        """The learned step rewards of `actions` ([m,H,A], or [m,n,H,A]; numpy or tensor) -- the companion of `plan_terminal_value`: the
        context encoder, one rollout that records its trajectories and the reward kernels, as numpy arrays (for [m,H,A] input the n axis
        is dropped):
          reward [m,n,p,H]  R of every step of every particle (NaN: a step with a non-finite input, or one behind a particle's first violation)
          total [m,n,p]     the sum over the counted steps in ascending t; the planner adds weight * total to the particle's return
          first [m,n,p]     with `cem_constraints` in terminate mode their first violations (steps t <= first count), else None
        The noise is drawn as `forecast` draws it: (seed, the last get_action's call) under the forecast's iteration word; no counter moves.
        On a model with `cem_discount` total is the discounted sum (gamma^t * R_t); reward stays undiscounted."""
        opt = _require_net(self, "reward", "plan_rewards", need_net=True)
        obs, acts, rows, traj, squeeze = self._replay("plan_rewards", obs, actions, cp_obs, cp_act, seed)
        first = self._terminate_first(traj, rows, obs, acts)
        _, steps, total = self.engine.reward_returns(traj, obs, acts, rows, opt.reward_params, first=first, want_steps=True)
        return self._result(squeeze, reward=steps.permute(1, 2, 3, 0), total=total, first=first)

    def _get_action_opt_in(self, obs, cp_obs, cp_act, cem_init_mean, cem_init_var):
        """The opt-in route of get_action: `_plan_opt_in` into the pinned host buffer."""
        m = int(np.shape(obs)[0])
        if m == 0:
            return np.zeros((0, self.n_forwards, self.action_space_dims), np.float32)
        _checked_shapes(self, obs, cp_obs, cp_act, cem_init_mean, cem_init_var)
        host = self.engine.host_out((m, self.n_forwards, self.action_space_dims))
        self._plan_opt_in(obs, cp_obs, cp_act, cem_init_mean, cem_init_var, out=host)
        torch.cuda.current_stream(self.engine.device).synchronize()
        return host.numpy().copy()

    # ------------------------------------------------------------------ discount over the horizon (INTEGRATION.md "Discount over the horizon")
    def _env_rows(self, traj, obs, acts, rows):
        """The env's own particle returns as the planner scores them: on a model with `cem_discount` the rollout's undiscounted sums
        are replaced by the discounted ones (`HipEngine.discount_returns`), as the loop does directly behind its rollout."""
        opt = getattr(self, "_opt", None)
        if opt is None or opt.discount == 1.0:
            return rows
        return self.engine.discount_returns(traj, obs, acts, rows)

    def plan_returns(self, obs, actions, cp_obs=None, cp_act=None, seed=None):
        """The discounted env returns of `actions` ([m,H,A], or [m,n,H,A]; numpy or tensor) under this model's `cem_discount` -- the
        companion of `plan_rewards` and `tracking_cost`: the context encoder, one rollout that records its trajectories and the discount
        kernel, as numpy arrays (for [m,H,A] input the n axis is dropped):
          returns [m,n,p]         sum_t weights[t] * step_rewards[..., t] in ascending t: what the planner scores in the place of the
                                  rollout's undiscounted sum
          step_rewards [m,n,H,p]  the undiscounted step rewards, from the recorded states
          weights [H+1]           gamma^t, the floats the kernels read (weights[H]: what a terminal value or Q is multiplied by)
        The noise is drawn as `forecast` draws it: (seed, the last get_action's call) under the forecast's iteration word; no counter moves."""
        opt = getattr(self, "_opt", None)
        if opt is None or opt.discount == 1.0:
            raise ValueError("plan_returns: this model has no cem_discount")
        obs, acts, rows, traj, squeeze = self._replay("plan_returns", obs, actions, cp_obs, cp_act, seed)
        out, steps = self.engine.discount_returns(traj, obs, acts, rows, want_steps=True)
        return dict(self._result(squeeze, returns=out, step_rewards=steps.permute(1, 2, 0, 3)), weights=self.engine.discount_weights())

    # ------------------------------------------------------------------ forecast of a plan (INTEGRATION.md "Forecasting a plan")
    def _forecast_refuse(self, what):
        if self.discrete:
            raise ValueError("%s: discrete actions are not forecast (random shooting returns no plan)" % what)

    def _get_action_with_forecast(self, obs, cp_obs, cp_act, cem_init_mean, cem_init_var):
        """get_action on today's route, whichever it is, then the forecast of the plan it returned under the same (seed, call)."""
        self._forecast_refuse("get_action(return_forecast=True)")
        if cem_init_mean is None:
            raise ValueError("get_action(return_forecast=True): the random-shooting route returns one action, not a plan to forecast")
        plan = MLPEnsembleCEMDynamicsModel.get_action(self, obs, cp_obs, cp_act, cem_init_mean, cem_init_var)      # (not a subclass's signature)
        return plan, self._forecast(obs, plan, cp_obs, cp_act, 1, **self._replay_key())

    def _replay_key(self, seed=None):
        """The words a diagnostic's noise is keyed by: `seed`, the model's by default, and the last get_action's call.  No counter moves."""
        return dict(seed=int(self.seed if seed is None else seed) & 0xFFFFFFFF, call=self._call & 0xFFFFFFFF)

    def _context_vec(self, cp_obs, cp_act):
        """The context encoder's output for a checked history; None for a model without context, whatever history it was given."""
        return self.engine.context_forward(cp_obs, cp_act) if self.context_out_dim > 0 else None

    def _replay(self, who, obs, actions, cp_obs, cp_act, seed):
        """What the plan companions share: the statistics pushed, the inputs checked and staged, the context encoder and ONE rollout of
        `actions` that records its trajectories, drawn as `forecast` draws it -> (obs [m,D], actions [m,n,H,A], rows [m,n,p], traj
        [H,m,n,p,D], squeeze: the input was [m,H,A] and the results drop their n axis).  The push may replace `self._opt`."""
        self._push_stats()
        cp_obs, cp_act = self._rollout_inputs(who, obs, actions, cp_obs, cp_act)
        eng = self.engine
        ctx_vec = self._context_vec(cp_obs, cp_act)
        acts = eng._t(actions)
        squeeze = acts.dim() == 3
        acts = (acts[:, None] if squeeze else acts).contiguous()
        obs = eng._t(obs)
        rows, traj = eng.rollout_returns(obs, ctx_vec, acts, it=_planner.FORECAST_IT, want_traj=True, **self._replay_key(seed))
        return obs, acts, rows, traj, squeeze

    def _terminate_first(self, traj, rows, obs, acts):
        """The first violations [m,n,p] of a replay under this model's `cem_constraints` in terminate mode -- what cuts a term's sum, as in
        the loop --, else None."""
        prm = self._opt.constraint_params
        if prm is None or prm.mode != _planner._lib.CONSTRAIN_MODES["terminate"]:
            return None
        return self.engine.constrain_returns(traj, rows, prm, obs=obs, actions=acts)[1]

    @staticmethod
    def _result(squeeze, **tensors):
        """A companion's result: its device tensors [m,n,...] as numpy arrays, without the n axis for [m,H,A] input; None stays None."""
        res = {k: None if v is None else v.cpu().numpy() for k, v in tensors.items()}
        return {k: None if v is None else v[:, 0] for k, v in res.items()} if squeeze else res

    def _rollout_inputs(self, who, obs, actions, cp_obs, cp_act):
        """The input checks `forecast` and the plan companions (`_replay`) share -> (cp_obs, cp_act), None for a model without context."""
        D, A, H = self.obs_space_dims, self.action_space_dims, self.n_forwards
        shp = tuple(int(v) for v in np.shape(actions))
        m = int(np.shape(obs)[0])
        if tuple(np.shape(obs)) != (m, D) or m == 0 or len(shp) not in (3, 4) or shp[0] != m or shp[-2:] != (H, A):
            raise ValueError("%s: obs %r, actions %r: expected [m,%d] with m >= 1 and [m,%d,%d] or [m,n,%d,%d]"
                             % (who, tuple(np.shape(obs)), shp, D, H, A, H, A))
        if self.context_out_dim == 0:
            return None, None
        if cp_obs is None or cp_act is None:
            raise ValueError("%s: cp_obs and cp_act are required for a context model" % who)
        Hh = self.history_length
        if tuple(np.shape(cp_obs)) != (m, D * Hh) or tuple(np.shape(cp_act)) != (m, A * Hh):
            raise ValueError("%s: cp_obs %r / cp_act %r, expected %r / %r" % (who, tuple(np.shape(cp_obs)), tuple(np.shape(cp_act)),
                                                                             (m, D * Hh), (m, A * Hh)))
        return cp_obs, cp_act

    def _forecast(self, obs, actions, cp_obs, cp_act, band_k, seed, call):
        self._push_stats()
        cp_obs, cp_act = self._rollout_inputs("forecast", obs, actions, cp_obs, cp_act)
        eng = self.engine
        acts = eng._t(actions)
        squeeze = acts.dim() == 3
        out = eng.plan_forecast(obs, cp_obs, cp_act, acts[:, None] if squeeze else acts, band_k=band_k, seed=seed, call=call)
        r = {k: v.cpu().numpy() for k, v in out.items()}
        res = dict(mean=r["mean"], member_mean=r["member_mean"], std_total=np.sqrt(r["var_total"]), std_epistemic=np.sqrt(r["var_epistemic"]),
                   std_aleatoric=np.sqrt(r["var_aleatoric"]), lo=r["lo"], hi=r["hi"], reward_mean=r["reward_mean"],
                   reward_std=np.sqrt(r["reward_var"]), reward_member=r["reward_member"], returns=r["returns"],
                   return_mean=r["returns"].mean(axis=-1), rollout_returns=r["rollout_returns"], diverged_step=r["diverged_step"])
        if squeeze:
            res = {k: v[:, :, 0] if k in ("member_mean", "reward_member") else v[:, 0] for k, v in res.items()}
        return res

    def forecast(self, obs, actions, cp_obs=None, cp_act=None, band_k=1, seed=None):
        """What the model predicts under `actions` ([m,H,A], or [m,n,H,A]: n sequences per env; numpy or tensor), step by step, as
        numpy arrays (for [m,H,A] input the n axis is dropped):
          mean, std_total, std_epistemic, std_aleatoric, lo, hi [m,n,H,D]; member_mean [E,m,n,H,D]   predicted states: particle mean,
              spread over the particles, its part from member disagreement / from noise inside a member (total^2 = epistemic^2 +
              aleatoric^2), and the band_k-th smallest / largest particle value
          reward_mean, reward_std [m,n,H]; reward_member [E,m,n,H]   the step reward
          returns, rollout_returns [m,n,p]; return_mean [m,n]        per-particle returns (the forecast's own sum of step rewards, and
              the rollout kernel's), and the particle mean of `returns`
          diverged_step [m,n]   the first step with a non-finite predicted value (H: none); from it on the statistics are NaN
        The noise is the device generator's under (seed, call) -- seed: the model's by default, call: the last get_action's -- with an
        iteration word no planner loop uses.  The planner's call counter does not move: planning is the same with or without forecasts
        in between, and `forecast` of the plan `get_action` just returned reproduces `get_action(..., return_forecast=True)`'s."""
        self._forecast_refuse("forecast")
        return self._forecast(obs, actions, cp_obs, cp_act, band_k, **self._replay_key(seed))

    def constraint_check(self, obs, actions, cp_obs=None, cp_act=None, seed=None):
        """Which particles of `actions` ([m,H,A], or [m,n,H,A]; numpy or tensor) leave the region this model's `cem_constraints` declare
        healthy, and when -- the companion of `forecast`: the context encoder, one rollout that records its trajectories, and the
        constraint kernel under the model's mode and weight, as numpy arrays (for [m,H,A] input the n axis is dropped):
          first_violation, violations [m,n,p]   the first violating step (H: none) and the number of violating steps, per particle
          violation_fraction [m,n]              the share of a sequence's particles with any violation
          returns [m,n,p]                       the constrained particle returns, as the planner would score them
        The noise is drawn as `forecast` draws it: (seed, the last get_action's call) under the forecast's iteration word; the planner's
        call counter does not move.  On a model with `cem_discount` the returns and the penalty are the discounted ones."""
        if self._opt is None or self._opt.constraint_params is None:
            raise ValueError("constraint_check: this model has no cem_constraints")
        obs, acts, rows, traj, squeeze = self._replay("constraint_check", obs, actions, cp_obs, cp_act, seed)
        rows, first, viol = self.engine.constrain_returns(traj, self._env_rows(traj, obs, acts, rows), self._opt.constraint_params, obs=obs,
                                                          actions=acts)
        res = self._result(squeeze, first_violation=first, violations=viol, returns=rows)
        res["violation_fraction"] = (res["violations"] > 0).mean(axis=-1)
        return res

    def reset_plan_carry(self, mask=None):
        """Forget the elites the iCEM planner carries from one get_action to the next (`cem_keep_elites` > 0): for every env, or for
        those where `mask` [m] is set -- at an episode boundary, so that a new episode never starts from the previous one's plans --
        and put their knot grids back on the call's first step (`cem_knot_anchor="episode"`) and their tracking references back on row 0
        (`cem_tracking`: the target offsets; the targets themselves stay); the actuator model's applied action and committed steps become
        unknown (NaN, not zero: a new episode's first step is not limited against the last episode's command).  A no-op for a model
        that carries nothing."""
        held = [t for t in (self._plan_carry_valid, getattr(self, "_plan_phase", None), getattr(self, "_target_offset", None)) if t is not None]
        unknown = [t for t in (getattr(self, "_act_prev", None), getattr(self, "_act_prefix", None)) if t is not None]
        if not held and not unknown:
            return
        if mask is None:
            for t in held:
                t.zero_()
            for t in unknown:
                t.fill_(float("nan"))
            return
        mk = self.engine._t(np.asarray(mask) if not isinstance(mask, torch.Tensor) else mask, dtype=torch.bool).reshape(-1)
        for t in held + unknown:
            if mk.shape[0] != t.shape[0]:
                raise ValueError("reset_plan_carry: mask has %d entries, the planner carries elites for %d envs" % (mk.shape[0], t.shape[0]))
        for t in held:
            t.masked_fill_(mk, 0)
        for t in unknown:
            t.masked_fill_(mk.reshape((-1,) + (1,) * (t.dim() - 1)), float("nan"))

    def get_context_pred(self, cp_obs, cp_act):
        """reference :369-380 -> [E,m,C]."""
        self._push_stats()
        return self.engine.context_forward(cp_obs, cp_act).cpu().numpy()

    def predict(self, obs, act, cp_obs=None, cp_act=None, return_std=False):
        """One-step prediction of every ensemble member (no reference twin; the north-star's `predict()`):
        obs [m,D], act [m,A] (+ history for the CaDM model) -> mean next observation [E,m,D]
        (`obs_postproc(obs, denormalize(mu))`), optionally with the predictive std of the delta [E,m,D]."""
        self._push_stats()
        E = self.ensemble_size
        tile = lambda x: None if x is None else np.tile(np.asarray(x, dtype=np.float32)[None], (E, 1, 1))
        mu, lv = self.engine.predict_heads(tile(obs), tile(act), tile(cp_obs), tile(cp_act))
        stats = self._stats12()
        dmean, dstd = np.asarray(stats[4], np.float32), np.asarray(stats[5], np.float32)
        delta = mu.cpu().numpy() * (dstd + 1e-10) + dmean
        nxt = self.env.obs_postproc(np.broadcast_to(np.asarray(obs, np.float32)[None], delta.shape), delta)
        if return_std:
            if lv is None:
                raise ValueError("a deterministic model has no predictive variance")
            return nxt, np.exp((lv.cpu().numpy() + 2.0 * np.log(dstd)) / 2.0)
        return nxt

    # ------------------------------------------------------------------ training
    def _ensure_train(self):
        if not self._train_ready:
            self.engine.train_configure(self.learning_rate, self.weight_decays, self.context_weight_decays,
                                        self.weight_decay_coeff, self.back_coeff, max_batch=0)
            self._train_ready = True

    def fit(self, obs, act, obs_next, cp_obs, cp_act, future_bool, epochs=1000, compute_normalization=True,
            valid_split_ratio=None, rolling_average_persitency=None, verbose=False, log_tabular=False,
            max_logging=5000, rng=None, index_stream=None, keep_trace=None):
        """reference :382-569.  `rng` (numpy Generator) replaces the reference's global np.random; `index_stream`
        (see FitIndexStream) replaces the draws themselves -- without one, the per-epoch shuffles are drawn ON THE DEVICE
        (an [E, n_train] argsort per epoch is ~1 s of host time and an 80 MB copy at 2 M rows).  `self.last_fit_trace` keeps
        the per-epoch validation losses and, with `keep_trace` (default: only when an index stream is injected), one
        [steps, 3] array of training losses [mse, back_mse, recon] per epoch."""
        D, A, F, Hh = self.obs_space_dims, self.action_space_dims, self.future_length, self.history_length
        # torch tensors (ModelSampleProcessor.process_samples(as_device=True)) come to the host here, as float64 -- the dtype of the
        # processor's own numpy output: the dataset is kept on the host (it grows by np.concatenate) and uploaded again below
        obs, act, obs_next, cp_obs, cp_act, future_bool = (
            x.detach().cpu().numpy().astype(np.float64, copy=False) if isinstance(x, torch.Tensor) else x
            for x in (obs, act, obs_next, cp_obs, cp_act, future_bool))
        assert obs.ndim == 2 and obs.shape[1] == D * F
        assert obs_next.ndim == 2 and obs_next.shape[1] == D * F
        assert act.ndim == 2 and act.shape[1] == A * F
        assert cp_obs.ndim == 2 and cp_obs.shape[1] == D * Hh
        assert cp_act.ndim == 2 and cp_act.shape[1] == A * Hh
        assert future_bool.ndim == 2 and future_bool.shape[1] == F
        if valid_split_ratio is None:
            valid_split_ratio = self.valid_split_ratio
        if rolling_average_persitency is None:
            rolling_average_persitency = self.rolling_average_persitency
        assert 1 > valid_split_ratio >= 0
        if getattr(self, "_plan_carry_valid", None) is not None:      # elites planned under the old weights (getattr: the CPU tests' fit on a bare object)
            self._plan_carry_valid.zero_()
        injected = index_stream is not None
        if index_stream is None:
            index_stream = FitIndexStream(rng if rng is not None else np.random.default_rng(self.seed + 7919 * (self._call + 1)))
        if keep_trace is None:
            keep_trace = injected

        obs = obs.reshape(-1, D)
        obs_next = obs_next.reshape(-1, D)
        delta = self.env.targ_proc(obs, obs_next)
        back_delta = self.env.targ_proc(obs_next, obs)
        obs = obs.reshape(-1, F * D)
        obs_next = obs_next.reshape(-1, F * D)
        delta = delta.reshape(-1, F * D)
        back_delta = back_delta.reshape(-1, F * D)
        new = dict(obs=obs, act=act, delta=delta, cp_obs=cp_obs, cp_act=cp_act, future_bool=future_bool,
                   obs_next=obs_next, back_delta=back_delta, single_obs=obs[:, :D], single_act=act[:, :A],
                   single_delta=delta[:, :D], single_back_delta=back_delta[:, :D])
        if self._dataset is None:
            self._dataset = new
        else:
            for k, v in new.items():
                self._dataset[k] = np.concatenate([self._dataset[k], v])
        ds = self._dataset
        self.compute_normalization(ds["single_obs"], ds["single_act"], ds["single_delta"], ds["cp_obs"],
                                   ds["cp_act"], ds["single_back_delta"])
        self._push_stats()

        N = ds["obs"].shape[0]
        n_valid = min(int(N * valid_split_ratio), max_logging)
        perm = np.asarray(index_stream.permutation(N))
        # The reference explodes every window into F rows on the host (`_preprocess_inputs`, :676-696: reshape, tile the
        # history F times, mask by future_bool) and feeds numpy batches.  Here the windowed dataset goes to HBM once and
        # a row is the pair (window, future offset): batches gather straight from the windows, the history is never tiled.
        dev = self._upload_dataset(ds)
        train_rows = self._row_index(ds["future_bool"], perm[n_valid:])
        valid_rows = self._row_index(ds["future_bool"], perm[:n_valid]) if n_valid > 0 else None
        return self._fit_loop(dev, train_rows, valid_rows, epochs, rolling_average_persitency, verbose, log_tabular, index_stream,
                              device_shuffle=not injected, keep_trace=keep_trace)

    def _eval_windows(self, who, obs, act, obs_next, cp_obs, cp_act, future_bool, seed):
        """What evaluate_horizon and evaluate_calibration share: the asserts, the F <= n_forwards check, the statistics push, the upload
        and the evaluations' own call counter -> (engine, device dataset, N, F, dict(seed=, call=))."""
        D, A, F, Hh = self.obs_space_dims, self.action_space_dims, self.future_length, self.history_length
        assert obs.ndim == 2 and obs.shape[1] == D * F
        assert obs_next.ndim == 2 and obs_next.shape[1] == D * F
        assert act.ndim == 2 and act.shape[1] == A * F
        assert cp_obs.ndim == 2 and cp_obs.shape[1] == D * Hh
        assert cp_act.ndim == 2 and cp_act.shape[1] == A * Hh
        assert future_bool.ndim == 2 and future_bool.shape[1] == F
        if F > self.n_forwards:
            raise ValueError("%s: future_length %d exceeds the planning horizon n_forwards %d" % (who, F, self.n_forwards))
        N = obs.shape[0]
        if N == 0:
            raise ValueError("%s: no windows" % who)
        self._stats12()                 # (raises RuntimeError when no statistics are set)
        self._push_stats()
        eng = self.engine
        dev = {k: eng._t(v) for k, v in (("obs", obs), ("act", act), ("obs_next", obs_next), ("cp_obs", cp_obs), ("cp_act", cp_act))}
        dev["future_bool"] = eng._t(np.asarray(future_bool) > 0)
        self._eval_call += 1
        return eng, dev, N, F, dict(seed=(self.seed if seed is None else int(seed)) & 0xFFFFFFFF, call=self._eval_call & 0xFFFFFFFF)

    def evaluate_horizon(self, obs, act, obs_next, cp_obs, cp_act, future_bool, seed=None, chunk=4096):
        """Open-loop prediction error along the horizon on held-out windows (no reference twin).  Takes the arrays `fit` takes
        (future windows of F = future_length steps, F <= n_forwards).  Every window is rolled out from its first observation
        through its recorded actions, F steps without correction, with the rows the planner scores (n_particles particles over
        the ensemble, planning-time context layout and noise) -- all on the device; the trajectories never reach the host.
        Step h of a window counts while future_bool[:, :h + 1] is all set.  Returns numpy arrays (NaN where count == 0):
            mse [F,D]         squared error of the particle mean, averaged over the counted windows
            member_mse [E,F,D]   the same for each member's own particles
            spread [F,D]      mean biased variance over the particles (what the ensemble BELIEVES its error is)
            rmse [F]          sqrt(mean over dims of mse)
            count, diverged [F]   windows counted / left out because their trajectory was not finite
        Uses the current normalisation statistics (RuntimeError when unset); leaves the dataset, weights, optimiser state and
        get_action's noise sequence alone.  `seed`: Philox key of the noise (default: the model's, with a call counter of its own)."""
        eng, dev, N, F, kw = self._eval_windows("evaluate_horizon", obs, act, obs_next, cp_obs, cp_act, future_bool, seed)
        out = eng.eval_horizon(dev, N, F, chunk=int(chunk), **kw)
        out = {k: v.cpu().numpy() for k, v in out.items()}
        count = out["count"].astype(np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            n = np.where(count > 0, count, np.nan)[:, None]
            mse = out["se"].astype(np.float64) / n
            res = dict(mse=mse, member_mse=out["se_member"].astype(np.float64) / n[None], spread=out["spread"].astype(np.float64) / n,
                       count=count, diverged=out["diverged"].astype(np.int64))
            res["rmse"] = np.sqrt(mse.mean(axis=1))
        return res

    def evaluate_calibration(self, obs, act, obs_next, cp_obs, cp_act, future_bool, seed=None, chunk=4096):
        """Is the ensemble's predictive distribution calibrated?  Takes what `evaluate_horizon` takes and rolls the same particles out
        the same way (same statistics push, same call counter, same noise keys), then asks, per counted (window, step) and dim,
        where the recorded next observation y falls among the p = n_particles particles x_j -- on the device.  Returns numpy arrays,
        NaN where the divisor is 0:
            rank_hist [F,D,p+1]            int64: windows whose y exceeds exactly r particles (Talagrand histogram; flat when calibrated,
                                           U-shaped when over-confident, dome-shaped when under-confident, skewed when biased)
            rank_hist_member [E,F,D,p/E+1] int64: the same against each member's own particles
            ties, degenerate [F,D]         int64: windows where y equals a particle / where the biased particle variance is exactly 0
            count, diverged [F]            int64: as evaluate_horizon's
            crps [F,D]                     mean of (1/p) sum |x_j - y| - (1/(2 p^2)) sum |x_j - x_k|: in the units of the state, lower is better
            z2 [F,D]                       mean of (xbar - y)^2 / v over the non-degenerate windows, v the biased particle variance
            nll [F,D]                      mean of 0.5 (log 2 pi + log v + (xbar - y)^2 / v) over the same
            z2_ideal                       (p + 1) / (p - 3), NaN for p <= 3: for a Gaussian predictive distribution of which the p particles and
                                           the truth are independent draws, E[(xbar - y)^2 / v_biased] = (1 + 1/p) p / (p - 3) -- 21/17 at p = 20.
                                           z2 above it: over-confident; below it: under-confident
            coverage [F,D,K], nominal [K]  K = p // 2: the share of windows whose y lies between order statistics k and p - 1 - k of the
                                           particles (k + 1 <= rank <= p - 1 - k), and that interval's nominal level (p - 1 - 2 k) / (p + 1)
            calibration_error [F]          mean over dims of max_r |empirical CDF of the rank at r - (r + 1) / (p + 1)|
        Leaves the dataset, weights, optimiser state and get_action's noise sequence alone."""
        eng, dev, N, F, kw = self._eval_windows("evaluate_calibration", obs, act, obs_next, cp_obs, cp_act, future_bool, seed)
        out = eng.eval_calibration(dev, N, F, chunk=int(chunk), **kw)
        return calibration_summary({k: v.cpu().numpy() for k, v in out.items()})

    _BATCH_KEYS = ("obs", "act", "delta", "obs_next", "back_delta", "cp_obs", "cp_act")

    def _upload_dataset(self, ds):
        eng = self.engine
        return {k: eng._t(ds[k]) for k in self._BATCH_KEYS}

    @staticmethod
    def _row_index(future_bool, windows):
        """Rows of `_preprocess_inputs(ds[windows])` as (window id, future offset), in the same order
        (window-major, masked by future_bool)."""
        wl, f = np.nonzero(future_bool[windows] > 0)
        return np.asarray(windows)[wl].astype(np.int64), f.astype(np.int64)

    def _gather_rows(self, dev, w, f):
        """[..] index tensors -> the batch dict of `cadm_train_step` ([.., dim] each)."""
        D, A, F = self.obs_space_dims, self.action_space_dims, self.future_length
        N = dev["obs"].shape[0]
        out = {}
        for k in ("obs", "delta", "obs_next", "back_delta"):
            out[k] = dev[k].view(N, F, D)[w, f]
        out["act"] = dev["act"].view(N, F, A)[w, f]
        out["cp_obs"] = dev["cp_obs"][w]
        out["cp_act"] = dev["cp_act"][w]
        return out

    def _fit_loop(self, dev, train_rows, valid_rows, epochs, persistency, verbose, log_tabular, stream,
                  device_shuffle=False, keep_trace=True):
        """Epoch / batch loop (reference :460-569): bootstrap indices, shuffle_rows, one fused
        fwd/bwd/Adam step per batch, validation, rolling-average early stop."""
        self._ensure_train()
        eng, E = self.engine, self.ensemble_size
        row_w = torch.as_tensor(train_rows[0], device=eng.device)
        row_f = torch.as_tensor(train_rows[1], device=eng.device)
        n_train = int(row_w.shape[0])
        if E > 1:
            bootstrap_idx = np.asarray(stream.bootstrap(E, n_train))            # :465
        else:
            bootstrap_idx = np.tile(np.arange(n_train, dtype="int64"), (E, 1))  # :467
        didx = torch.as_tensor(bootstrap_idx.astype(np.int64), device=eng.device)
        trace = self.last_fit_trace = dict(train=[], valid=[])
        gen = None
        if device_shuffle:      # keyed by the host stream, so a seeded `rng` still fixes the whole fit
            gen = torch.Generator(device=eng.device)
            gen.manual_seed(int(stream.rng.integers(0, 2 ** 62)))
        dev_valid = None
        if valid_rows is not None and valid_rows[0].shape[0] > 0:
            vw = torch.as_tensor(valid_rows[0], device=eng.device)
            vf = torch.as_tensor(valid_rows[1], device=eng.device)
            dev_valid = {k: v[None].expand(E, -1, -1).contiguous() for k, v in self._gather_rows(dev, vw, vf).items()}  # :470,515-521
        rolling, rolling_prev = None, None
        epoch = -1
        for epoch in range(epochs):
            t0 = time.time()
            # shuffle_rows (:472-474,483): independent permutation of every member's index row (argsort of uniforms) --
            # on the device by default; from the host stream when one is injected (parity tests replay the reference's draws)
            if gen is not None:
                order = torch.argsort(torch.rand((E, n_train), device=eng.device, generator=gen), dim=-1)
            else:
                order = torch.as_tensor(np.asarray(stream.epoch_order(E, n_train)).astype(np.int64), device=eng.device)
            didx = torch.gather(didx, 1, order)
            losses = []
            for b in range(int(np.ceil(n_train / self.batch_size))):
                bi = didx[:, b * self.batch_size:(b + 1) * self.batch_size]    # [E,B] row ids
                # the step reads its rows through (row id -> window, offset) inside the kernels: no gathered batch
                losses.append(eng.train_step_rows(dev, self.future_length, row_w, row_f, bi, train=True))
            step_losses = torch.stack(losses).cpu().numpy() if losses else np.zeros((0, 3))
            if keep_trace:
                trace["train"].append(step_losses)          # one [steps, 3] array per epoch
            tl = step_losses.mean(0) if losses else np.zeros(3)
            if dev_valid is not None:
                v_mse, v_back, v_recon = eng.train_step(dev_valid, train=False).cpu().numpy()
                trace["valid"].append((v_mse, v_back, v_recon))
                if verbose:
                    logger.log("Training DynamicsModel - finished epoch %i --"
                               "[Training] mse loss: %.4f  back mse loss: %.4f  recon loss:  %.4f "
                               "[Validation] mse loss: %.4f  back mse loss: %.4f  recon loss:  %.4f  epoch time: %.2f"
                               % (epoch, tl[0], tl[1], tl[2], v_mse, v_back, v_recon, time.time() - t0))
                if rolling is None:                                             # :544-549
                    rolling, rolling_prev = 1.5 * v_recon, 2 * v_recon
                    if v_recon < 0:
                        rolling, rolling_prev = v_recon / 1.5, v_recon / 2
                rolling = persistency * rolling + (1.0 - persistency) * v_recon  # :551-552
                if rolling_prev < rolling:                                      # :554-556
                    logger.log("Stopping Training of Model since its valid_loss_rolling_average decreased")
                    break
            elif verbose:
                logger.log("Training DynamicsModel - finished epoch %i --[Training] mse loss: %.4f  back mse loss: "
                           "%.4f  recon loss: %.4f  epoch time: %.2f" % (epoch, tl[0], tl[1], tl[2], time.time() - t0))
            rolling_prev = rolling                                              # :564
        eng.repack()   # planner weight streams follow the updated master weights
        if log_tabular:
            logger.logkv("AvgModelEpochTime", float("nan"))   # reference logs mean([]) (Appendix C)
            logger.logkv("Epochs", epoch)

    def _preprocess_inputs(self, obs, act, delta, cp_obs, cp_act, future_bool, obs_next, back_delta):
        """reference :676-696: explode the future window into rows, tile the history, mask.  Kept as the host-side
        definition of a "row" (tests compare the device gather of `fit` against it); `fit` itself no longer calls it."""
        D, A, Hh, F = self.obs_space_dims, self.action_space_dims, self.history_length, self.future_length
        fb = future_bool.reshape(-1) > 0
        rows = lambda x, w: x.reshape((-1, w))[fb]
        if Hh > 0:
            _cp_obs = np.tile(cp_obs, (1, F)).reshape((-1, D * Hh))[fb]
            _cp_act = np.tile(cp_act, (1, F)).reshape((-1, A * Hh))[fb]
        else:       # vanilla model: no history window
            _cp_obs = np.zeros((int(fb.sum()), 0))
            _cp_act = np.zeros((int(fb.sum()), 0))
        return (rows(obs, D), rows(act, A), rows(delta, D), rows(obs_next, D), rows(back_delta, D), _cp_obs, _cp_act)

    # ------------------------------------------------------------------ checkpoint
    def save(self, save_path):
        """reference :571-577: joblib list of arrays in tf.trainable_variables() order + '_norm_stats'."""
        joblib.dump(self.engine.params_list(), save_path)
        if self.normalization is not None:
            joblib.dump(self.normalization, save_path + "_norm_stats")

    def load(self, load_path):
        """reference :579-588 (positional assignment)."""
        self.engine.load_params_list(joblib.load(load_path))
        self.reset_plan_carry()
        if self.normalize_input:
            self.normalization = joblib.load(load_path + "_norm_stats")
            self._stats_dirty = True

    # ------------------------------------------------------------------ statistics
    def compute_normalization(self, obs, act, delta, cp_obs, cp_act, back_delta):
        """reference :590-602 (population statistics in float64 on the host)."""
        assert obs.shape[0] == delta.shape[0] == act.shape[0]
        proc_obs = self.env.obs_preproc(obs)
        n = OrderedDict()
        n["obs"] = (np.mean(proc_obs, axis=0), np.std(proc_obs, axis=0))
        n["delta"] = (np.mean(delta, axis=0), np.std(delta, axis=0))
        n["act"] = (np.mean(act, axis=0), np.std(act, axis=0))
        n["cp_obs"] = (np.mean(cp_obs, axis=0), np.std(cp_obs, axis=0))
        n["cp_act"] = (np.mean(cp_act, axis=0), np.std(cp_act, axis=0))
        n["back_delta"] = (np.mean(back_delta, axis=0), np.std(back_delta, axis=0))
        self.normalization = n
        self._stats_dirty = True

    def set_normalization(self, normalization):
        """Install precomputed statistics (same OrderedDict layout as `self.normalization`)."""
        self.normalization = normalization
        self._stats_dirty = True

    def get_normalization_stats(self):
        """reference :604-645."""
        return self._stats12()

    def _stats12(self):
        """The 12 statistic vectors in STAT_KEYS order (what the engine consumes)."""
        D, A, P, Hh = self.obs_space_dims, self.action_space_dims, self.proc_obs_space_dims, self.history_length
        if self.normalize_input:
            if self.normalization is None:
                raise RuntimeError("normalization statistics are not set: call fit(), load() or set_normalization()")
            nz = self.normalization
            om, os_ = nz["obs"]
            dm, ds = nz["delta"]
            am, as_ = (np.zeros((A,)), np.ones((A,))) if self.discrete else nz["act"]
            # the reference's VANILLA model saves only obs / delta / act (mlp_ensemble_cem_dynamics.py:343-351): a model
            # without history window / backward net never reads the other three, so they default to (0, 1)
            com, cos = (np.zeros((D * Hh,)), np.ones((D * Hh,))) if (self.state_diff or "cp_obs" not in nz) else nz["cp_obs"]
            cam, cas = (np.zeros((A * Hh,)), np.ones((A * Hh,))) if (self.discrete or "cp_act" not in nz) else nz["cp_act"]
            bm, bs = nz["back_delta"] if "back_delta" in nz else (np.zeros((D,)), np.ones((D,)))
        else:
            om, os_ = np.zeros((P,)), np.ones((P,))
            am, as_ = np.zeros((A,)), np.ones((A,))
            dm, ds = np.zeros((D,)), np.ones((D,))
            com, cos = np.zeros((D * Hh,)), np.ones((D * Hh,))
            cam, cas = np.zeros((A * Hh,)), np.ones((A * Hh,))
            bm, bs = np.zeros((D,)), np.ones((D,))
        return (om, os_, am, as_, dm, ds, com, cos, cam, cas, bm, bs)
