"""Host-side pieces of the CEM / random-shooting planners.

The planner itself is ONE implementation, in the library: ``HipEngine.cem_plan`` / ``cem_plan_host`` / ``rs_plan`` (`cadm_cem_plan`,
`cadm_cem_plan_staged`, `cadm_rs_plan`).  Candidate-sharded over several GPUs it is still that loop -- every rank draws and rolls out
its own contiguous shard, ONE all-gather of the per-candidate returns per CEM iteration ([m, n/G] floats + a checksum word per rank)
gives every rank the full vector, every rank runs the identical top-k + refit and regenerates the elite sequences by id.
Only the collective is a plug: the RCCL communicator the ctx owns (`HipEngine.dist_init`), or -- same loop, same payload, same
checks -- an all-gather this module supplies over any torch.distributed backend (`ExternalAllGather`, registered with
`cadm_dist_init_external`; "gloo" in the CPU tests and in the two-ranks-on-one-GPU test).

What is left here:
  * `Shard`: a rank's contiguous candidate range;  `check_replicated`: the host-side guard of the first sharded calls;
  * `ExternalAllGather`: the host-supplied collective;
  * `PlanOptions`: what a model's `cem_*` kwargs mean -- their checks, the switches, and the ctypes structs `HipEngine.opt_in_plan` hands to the library;
  * `icem_plan`: the opt-in iCEM loop (`cadm_icem_plan`, csrc/icem.hip; `update="mppi"`: `cadm_mppi_plan`; `score=`: `cadm_scored_plan`; `constraints=`: `cadm_constrained_plan`; `knots=`: `cadm_knot_plan`; `tracking=`: `cadm_tracking_plan`; `actuator=`: `cadm_actuated_plan`; `uncertainty=`: `cadm_uncertain_plan`; `value=`: `cadm_valued_plan`; `reward=`: `cadm_rewarded_plan`; `policy=`: `cadm_guided_plan`; `critic=`: `cadm_critic_plan`; `policy_logp=`: `cadm_anchored_plan`) one launch at a time, for the same purposes;
  * `cem_plan` / `rs_plan`: the per-iteration, SINGLE-RANK form over the engine's primitives, for parity tests with injected ``z`` /
    ``eps`` and for diagnostics (`return_info`) -- the reference's TF RNG streams are unseeded.
Reference: /root/reference/cadm/dynamics/core/utils.py:398-488 (CEM), :490-561 (RS).
"""
import collections

import numpy as np
import torch

from . import _lib
from .engine import HipEngine


POLICY_IT = _lib.POLICY_IT  # the iteration word of the proposal roll's first one-step rollout: csrc/planner.h CADM_POLICY_IT (tests/test_policy_ref.py pairs the two)
FORECAST_IT = 0xFC0000      # the iteration word of a forecast's rollout: csrc/planner.h CADM_FORECAST_IT (tests/test_constraint_ref.py pairs the two)


class PlanOptions(collections.namedtuple("PlanOptions", "noise_beta keep_elites decay return_best add_mean_last update temperature relative score "
                                                       "params score_params constraints constraint_params knots knot_params actuator actuator_params "
                                                       "action_advance proposals std_scale discount logp logp_params critic critic_params policy policy_params reward reward_params value value_params uncertainty "
                                                       "uncertainty_params tracking track_params target_advance",
                                                       defaults=(None, None, None, None, True, "noise", 1.0, 1.0, None, None, None, None, None, None, None, None, None, None, None, None,
                                                                 None, None, True))):
    """The opt-in planner's switches (a model's `cem_*` kwargs), immutable, with the structs the library reads built once: `params` -- an
    `IcemParams` (update "cem") or a `MppiParams` ("mppi") -- and `score_params` (a `ScoreParams`, or None: the particle mean).
    `score`: None, or (mode name, kappa, k).  `constraints`: None, or (the list of dict(dim=, lo=, hi=), mode name, weight), with
    `constraint_params` the `ConstraintParams` built from it (None: no state constraints, and the loop records no trajectory).
    `knots`: None, or (spacing, interp name, anchor name), with `knot_params` the `KnotParams` built from it (None: every step is a decision).
    `tracking`: None, or the tuple of dict(dim=, kind=, w=, delta=), with `track_params` the `TrackParams` built from it (None: no run-time
    targets); `target_advance`: whether a model moves its per-env target offsets on by one after every plan.
    `actuator`: None, or (delay, the rate limits, the rate costs) -- each of the two a tuple of A floats or one float -- with
    `actuator_params` the `ActuatorParams` built from it (None: no actuator model); `action_advance`: whether a planned call ends with the
    actuator state moved on by one step (prev <- plan[:,0], the committed prefix <- plan[:,1 .. delay]).
    `uncertainty`: None, or (kind name, lambda, w -- None, a float, a tuple of D floats or "delta_std" --, form name, cap or None), with
    `uncertainty_params` the `UncertaintyParams` built from it (None: no uncertainty term; for w="delta_std" a placeholder with w = 1
    that the model replaces whenever it pushes its normalisation statistics).
    `value`: None, or (the tuple of hidden widths, activation name, weight), with `value_params` the `ValueParams` built from it (None: no
    terminal value).  The net itself is not an option: a model registers it at run time (`set_terminal_value`).
    `reward`: None, or (inputs name, the tuple of hidden widths, activation name, weight), with `reward_params` the `RewardParams` built
    from it (None: no learned reward); the net is registered at run time too (`set_reward_net`).
    `policy`: None, or (the tuple of hidden widths, activation name, squash name, n_samples, noise_std), with `policy_params` the
    `PolicyParams` built from it (None: no policy prior); the net is registered at run time too (`set_policy`).  `proposals` / `std_scale`:
    where the prior's sequences 1 .. P - 1 come from -- "noise", the mode action plus noise_std, or "head", draws of the actor's Gaussian
    head at std_scale times its own standard deviation (a model hands both to its engine once, `HipEngine.set_policy_proposals`;
    `policy_proposals_setting` is the check against the model's `policy_head`).
    `critic`: None, or (the tuple of hidden widths, activation name, n_critics, reduce name, weight, actor), with `critic_params` the
    `CriticParams` built from it (None: no terminal Q); actor = (the tuple of hidden widths, activation name, squash name) of the policy
    net the critics are evaluated at -- the policy prior's when one is declared (`actor_params` builds its `PolicyParams`); critics
    and actor are registered at run time (`set_critics`, `set_policy`).
    `logp`: None, or (weight, space name, actor), with `logp_params` the `PolicyLogpParams` built from it (None: the actor's log-density
    is no term of the score); actor = (the tuple of hidden widths, activation name, squash name) of the policy net whose density it is
    -- the one actor of the model, as `critic`'s.
    `discount`: gamma in (0, 1], the discount over the horizon every term of a candidate's score is weighted by per step (1.0: none); a
    model hands it to its engine once (`HipEngine.set_discount`), it is not a parameter of a plan call."""
    __slots__ = ()

    def actor_params(self):
        """The `PolicyParams` a model registers its actor under: the policy prior's, or -- for a model whose only actor declaration is
        `cem_terminal_q`'s or `cem_policy_logp`'s `policy` -- one built from it with n_samples = 1 (the value is not used); None without
        any."""
        if self.policy_params is not None:
            return self.policy_params
        if self.critic is not None:
            hs, act, squash = self.critic[5]
        elif self.logp is not None:
            hs, act, squash = self.logp[2]
        else:
            return None
        return HipEngine.policy_params(hs, act, squash, 1, 0.0)

    @staticmethod
    def from_kwargs(cem_noise_beta=0.0, cem_keep_elites=0, cem_decay=1.0, cem_return="mean", cem_add_mean=False, cem_update="cem",
                    cem_temperature=1.0, cem_temperature_relative=False, cem_score="mean", cem_risk=None, use_cem=False, discrete=False,
                    process_group=None, n_particles=20, cem_constraints=None, cem_constraint_mode="penalty", cem_constraint_weight=None, *,
                    cem_knots=1, cem_knot_interp="hold", cem_knot_anchor="call", cem_tracking=None, cem_target_advance=True,
                    cem_action_delay=0, cem_action_rate_limit=None, cem_action_rate_cost=None, cem_action_advance=True, n_forwards=None,
                    action_dim=None, cem_uncertainty=None, obs_dim=None, cem_terminal_value=None, cem_reward_net=None,
                    cem_policy_prior=None, cem_terminal_q=None, cem_discount=1.0, cem_policy_logp=None):
        """None when every `cem_*` kwarg is at its default (the reference's CEM: nothing else is looked at); else the kwargs checked --
        everything that needs no engine -- and folded into a `PlanOptions`.  n_forwards / action_dim: the model's horizon and action
        dims, what `cem_action_delay` and the lengths of `cem_action_rate_limit` / `cem_action_rate_cost` are checked against (None: the
        library checks them against the engine's).  cem_uncertainty: None, or dict(kind="epistemic" | "total", weight=lambda, w=None |
        float | [D] | "delta_std", form="var" | "std", cap=None) (`HipEngine.uncertainty_params`); obs_dim: the model's observation dims,
        what a list `w` is checked against.  cem_terminal_value: None, or dict(hidden_sizes=(..), activation="relu" | "tanh" | "swish",
        weight=1.0) (`HipEngine.value_params`): the shape of the value net a model is given at run time.  cem_reward_net: None, or
        dict(inputs="next_obs" | "obs_act" | "obs_act_next_obs", hidden_sizes=(..), activation=, weight=1.0) (`HipEngine.reward_params`):
        the shape of the reward net a model is given at run time; obs_dim / action_dim: what its input dims are checked against.
        cem_policy_prior: None, or dict(hidden_sizes=(..), activation=, squash="tanh" | "none", n_samples=24, noise_std=0.0,
        proposals="noise" | "head", std_scale=1.0) (`HipEngine.policy_params`, `HipEngine.policy_proposals_args`): the shape of the
        policy net a model is given at run time, how many proposals it makes (whether they fit the smallest iteration's candidates is
        the model's check, once it knows its engine's elites: `policy_min_candidates`) and where they come from: "head" draws them from
        the actor's Gaussian head at std_scale times its standard deviation (no noise_std with it: one source; std_scale belongs to
        "head" alone; whether the model declares a `policy_head` is the model's check: `policy_proposals_setting`).
        cem_terminal_q: None, or dict(hidden_sizes=(256, 256), activation="relu", n_critics=2, reduce="min" | "mean", weight=1.0,
        policy=dict(hidden_sizes=, activation=, squash=)) (`HipEngine.critic_params`): the shape of the Q critics and of the actor they
        are evaluated at; `policy` may be left out when cem_policy_prior is declared (the actor is then that net; given both, they must
        agree); not together with cem_terminal_value: a plan has one terminal term.  cem_discount: gamma in (0, 1], the discount over
        the horizon (`HipEngine.set_discount`); 1.0: none.  With it the `weight` of cem_terminal_value / cem_terminal_q no longer carries
        gamma ** n_forwards: the library multiplies it in.
        cem_policy_logp: None, or dict(weight=1.0, space="action" | "pre_squash", policy=dict(hidden_sizes=, activation=, squash=))
        (`HipEngine.policy_logp_params`): weight * sum_t log pi(a_t | s_t) of the model's actor joins every particle's return; `policy`
        may be left out beside cem_policy_prior or cem_terminal_q's policy (one actor: given both, they must agree).  Whether the model
        declares the `policy_head` the density needs is the model's check: `policy_logp_setting`."""
        if isinstance(cem_discount, (bool, np.bool_)) or not isinstance(cem_discount, (int, float, np.integer, np.floating)) \
                or not 0.0 < float(cem_discount) <= 1.0:      # (NaN: false)
            raise ValueError("cem_discount must be a number in (0, 1] (1.0: no discount over the horizon), got %r" % (cem_discount,))
        discount = float(np.float32(cem_discount))      # what the library is handed
        if not 0.0 < discount <= 1.0:
            raise ValueError("cem_discount must be a number in (0, 1] in float32, got %r" % (cem_discount,))
        act_off = (cem_action_rate_limit is None and cem_action_rate_cost is None and isinstance(cem_action_delay, (int, np.integer))
                   and not isinstance(cem_action_delay, bool) and int(cem_action_delay) == 0)
        if (float(cem_noise_beta), int(cem_keep_elites), float(cem_decay), cem_return, bool(cem_add_mean), cem_update, float(cem_temperature),
                bool(cem_temperature_relative), cem_score, cem_risk, cem_constraints, cem_constraint_mode,
                cem_constraint_weight) == (0.0, 0, 1.0, "mean", False, "cem", 1.0, False, "mean", None, None, "penalty", None) \
                and (cem_knot_interp, cem_knot_anchor) == ("hold", "call") and isinstance(cem_knots, (int, np.integer)) \
                and not isinstance(cem_knots, bool) and int(cem_knots) == 1 and cem_tracking is None and cem_target_advance is True \
                and act_off and cem_action_advance is True and cem_uncertainty is None and cem_terminal_value is None \
                and cem_reward_net is None and cem_policy_prior is None and cem_terminal_q is None and float(cem_discount) == 1.0 \
                and cem_policy_logp is None:
            return None
        if not use_cem:
            raise ValueError("cem_noise_beta / cem_keep_elites / cem_decay / cem_return / cem_add_mean / cem_update / cem_temperature / "
                             "cem_score / cem_risk / cem_constraints / cem_knots / cem_tracking / cem_action_delay / cem_action_rate_limit / "
                             "cem_action_rate_cost / cem_uncertainty / cem_terminal_value / cem_reward_net / cem_policy_prior / cem_terminal_q / cem_discount / cem_policy_logp configure the CEM planner: they need "
                             "use_cem=True")
        if float(cem_discount) != 1.0:
            if discrete:
                raise ValueError("cem_discount needs continuous actions: this env's action space is discrete (discrete actions are planned "
                                 "by random shooting, which sums the step rewards undiscounted)")
            if process_group is not None:
                import torch.distributed as dist
                if dist.get_world_size(process_group) > 1:
                    raise ValueError("cem_discount is not supported on a process group of more than one rank: the candidate-sharded planner "
                                     "sums the step rewards undiscounted")
        value = vparams = None
        if cem_terminal_value is not None:
            if not isinstance(cem_terminal_value, dict) or set(cem_terminal_value) - {"hidden_sizes", "activation", "weight"}:
                raise ValueError("cem_terminal_value must be dict(hidden_sizes=, activation=, weight=), got %r" % (cem_terminal_value,))
            if obs_dim is not None and not 1 <= int(obs_dim) <= _lib.MAX_VALUE_DIMS:
                raise ValueError("a terminal value net reads up to %d observation dims, got %r" % (_lib.MAX_VALUE_DIMS, obs_dim))
            v = dict(hidden_sizes=(), activation="relu", weight=1.0)
            v.update(cem_terminal_value)
            vparams = HipEngine.value_params(v["hidden_sizes"], v["activation"], v["weight"])
            value = (tuple(int(vparams.hidden[l]) for l in range(vparams.n_hidden)),
                     [k for k, x in _lib.VALUE_ACTS.items() if x == vparams.activation][0], float(vparams.weight))
        policy = pparams = None
        proposals, std_scale = "noise", 1.0
        if cem_policy_prior is not None:
            if not isinstance(cem_policy_prior, dict) or set(cem_policy_prior) - {"hidden_sizes", "activation", "squash", "n_samples", "noise_std",
                                                                                  "proposals", "std_scale"}:
                raise ValueError("cem_policy_prior must be dict(hidden_sizes=, activation=, squash=, n_samples=, noise_std=, proposals=, "
                                 "std_scale=), got %r" % (cem_policy_prior,))
            if obs_dim is not None and not 1 <= int(obs_dim) <= _lib.MAX_VALUE_DIMS:
                raise ValueError("a policy net reads up to %d observation dims, got %r" % (_lib.MAX_VALUE_DIMS, obs_dim))
            if action_dim is not None and not 1 <= int(action_dim) <= _lib.MAX_POLICY_ACTIONS:
                raise ValueError("a policy net writes up to %d action dims, got %r" % (_lib.MAX_POLICY_ACTIONS, action_dim))
            q = dict(hidden_sizes=(256, 256), activation="relu", squash="tanh", n_samples=24, noise_std=0.0, proposals="noise", std_scale=1.0)
            q.update(cem_policy_prior)
            pparams = HipEngine.policy_params(q["hidden_sizes"], q["activation"], q["squash"], q["n_samples"], q["noise_std"])
            proposals, std_scale = q["proposals"], HipEngine.policy_proposals_args(q["proposals"], q["std_scale"])[1]
            if proposals == "head" and pparams.noise_std > 0.0:
                raise ValueError("cem_policy_prior: proposals=\"head\" draws the proposals from the policy itself; noise_std=%r perturbs the "
                                 "mode action (proposals=\"noise\"): one source of proposals" % (q["noise_std"],))
            if proposals == "noise" and std_scale != 1.0:
                raise ValueError("cem_policy_prior: std_scale=%r scales the head's standard deviation (proposals=\"head\"); the noise route's "
                                 "scale is noise_std" % (q["std_scale"],))
            policy = (tuple(int(pparams.hidden[l]) for l in range(pparams.n_hidden)),
                      [k for k, x in _lib.VALUE_ACTS.items() if x == pparams.activation][0],
                      [k for k, x in _lib.POLICY_SQUASH.items() if x == pparams.squash][0], int(pparams.n_samples), float(pparams.noise_std))
        critic = qparams = None
        if cem_terminal_q is not None:
            if not isinstance(cem_terminal_q, dict) or set(cem_terminal_q) - {"hidden_sizes", "activation", "n_critics", "reduce", "weight", "policy"}:
                raise ValueError("cem_terminal_q must be dict(hidden_sizes=, activation=, n_critics=, reduce=, weight=, policy=), got %r"
                                 % (cem_terminal_q,))
            if cem_terminal_value is not None:
                raise ValueError("cem_terminal_q and cem_terminal_value are both given: a plan has one terminal term")
            if obs_dim is not None and not 1 <= int(obs_dim) <= _lib.MAX_VALUE_DIMS:
                raise ValueError("Q critics read up to %d observation dims, got %r" % (_lib.MAX_VALUE_DIMS, obs_dim))
            if action_dim is not None and not 1 <= int(action_dim) <= _lib.MAX_POLICY_ACTIONS:
                raise ValueError("Q critics read up to %d action dims, got %r" % (_lib.MAX_POLICY_ACTIONS, action_dim))
            c = dict(hidden_sizes=(256, 256), activation="relu", n_critics=2, reduce="min", weight=1.0, policy=None)
            c.update(cem_terminal_q)
            qparams = HipEngine.critic_params(c["hidden_sizes"], c["activation"], c["n_critics"], c["reduce"], c["weight"])
            actor = None
            if c["policy"] is not None:
                if not isinstance(c["policy"], dict) or set(c["policy"]) - {"hidden_sizes", "activation", "squash"}:
                    raise ValueError("cem_terminal_q: policy must be dict(hidden_sizes=, activation=, squash=), got %r" % (c["policy"],))
                a = dict(hidden_sizes=(256, 256), activation="relu", squash="tanh")
                a.update(c["policy"])
                ap = HipEngine.policy_params(a["hidden_sizes"], a["activation"], a["squash"], 1, 0.0)
                actor = (tuple(int(ap.hidden[l]) for l in range(ap.n_hidden)), [k for k, x in _lib.VALUE_ACTS.items() if x == ap.activation][0],
                         [k for k, x in _lib.POLICY_SQUASH.items() if x == ap.squash][0])
            if policy is not None:
                if actor is not None and actor != policy[:3]:
                    raise ValueError("cem_terminal_q: policy %r does not agree with cem_policy_prior's net %r (one actor: hidden_sizes, "
                                     "activation and squash must be the same)" % (actor, policy[:3]))
                actor = policy[:3]
            if actor is None:
                raise ValueError("cem_terminal_q needs policy=dict(hidden_sizes=, activation=, squash=), the actor the critics are evaluated at "
                                 "(or a cem_policy_prior, whose net it then is)")
            critic = (tuple(int(qparams.hidden[l]) for l in range(qparams.n_hidden)),
                      [k for k, x in _lib.VALUE_ACTS.items() if x == qparams.activation][0], int(qparams.n_critics),
                      [k for k, x in _lib.CRITIC_REDUCES.items() if x == qparams.reduce][0], float(qparams.weight), actor)
        logp = lparams = None
        if cem_policy_logp is not None:
            if not isinstance(cem_policy_logp, dict) or set(cem_policy_logp) - {"weight", "space", "policy"}:
                raise ValueError("cem_policy_logp must be dict(weight=, space=, policy=), got %r" % (cem_policy_logp,))
            if obs_dim is not None and not 1 <= int(obs_dim) <= _lib.MAX_VALUE_DIMS:
                raise ValueError("a policy net reads up to %d observation dims, got %r" % (_lib.MAX_VALUE_DIMS, obs_dim))
            if action_dim is not None and not 1 <= int(action_dim) <= _lib.MAX_POLICY_ACTIONS:
                raise ValueError("a policy net writes up to %d action dims, got %r" % (_lib.MAX_POLICY_ACTIONS, action_dim))
            g = dict(weight=1.0, space="action", policy=None)
            g.update(cem_policy_logp)
            lparams = HipEngine.policy_logp_params(g["weight"], g["space"])
            lactor = None
            if g["policy"] is not None:
                if not isinstance(g["policy"], dict) or set(g["policy"]) - {"hidden_sizes", "activation", "squash"}:
                    raise ValueError("cem_policy_logp: policy must be dict(hidden_sizes=, activation=, squash=), got %r" % (g["policy"],))
                a = dict(hidden_sizes=(256, 256), activation="relu", squash="tanh")
                a.update(g["policy"])
                ap = HipEngine.policy_params(a["hidden_sizes"], a["activation"], a["squash"], 1, 0.0)
                lactor = (tuple(int(ap.hidden[l]) for l in range(ap.n_hidden)), [k for k, x in _lib.VALUE_ACTS.items() if x == ap.activation][0],
                          [k for k, x in _lib.POLICY_SQUASH.items() if x == ap.squash][0])
            declared = policy[:3] if policy is not None else None if critic is None else critic[5]      # the model's one actor, so far
            if declared is not None:
                if lactor is not None and lactor != declared:
                    raise ValueError("cem_policy_logp: policy %r does not agree with the actor %r that cem_policy_prior / cem_terminal_q "
                                     "declare (one actor: hidden_sizes, activation and squash must be the same)" % (lactor, declared))
                lactor = declared
            if lactor is None:
                raise ValueError("cem_policy_logp needs policy=dict(hidden_sizes=, activation=, squash=), the actor whose density it is "
                                 "(or a cem_policy_prior / cem_terminal_q, whose actor it then is)")
            logp = (float(lparams.weight), [k for k, x in _lib.LOGP_SPACES.items() if x == lparams.space][0], lactor)
        reward = rparams = None
        if cem_reward_net is not None:
            if not isinstance(cem_reward_net, dict) or set(cem_reward_net) - {"inputs", "hidden_sizes", "activation", "weight"}:
                raise ValueError("cem_reward_net must be dict(inputs=, hidden_sizes=, activation=, weight=), got %r" % (cem_reward_net,))
            r = dict(inputs="obs_act_next_obs", hidden_sizes=(), activation="relu", weight=1.0)
            r.update(cem_reward_net)
            rparams = HipEngine.reward_params(r["inputs"], r["hidden_sizes"], r["activation"], r["weight"])
            if obs_dim is not None and action_dim is not None:
                K = HipEngine.reward_input_dims(rparams.inputs, int(obs_dim), int(action_dim))
                if not 1 <= K <= _lib.MAX_REWARD_DIMS:
                    raise ValueError("a reward net reads up to %d input dims, %r on %r observation and %r action dims are %d"
                                     % (_lib.MAX_REWARD_DIMS, r["inputs"], obs_dim, action_dim, K))
            reward = ([k for k, x in _lib.REWARD_INPUTS.items() if x == rparams.inputs][0],
                      tuple(int(rparams.hidden[l]) for l in range(rparams.n_hidden)),
                      [k for k, x in _lib.VALUE_ACTS.items() if x == rparams.activation][0], float(rparams.weight))
        uncertainty = uparams = None
        if cem_uncertainty is not None:
            if not isinstance(cem_uncertainty, dict) or not {"kind", "weight"} <= set(cem_uncertainty) \
                    or set(cem_uncertainty) - {"kind", "weight", "w", "form", "cap"}:
                raise ValueError("cem_uncertainty must be dict(kind=, weight=, w=, form=, cap=) with kind and weight given, got %r" % (cem_uncertainty,))
            u = dict(w=None, form="var", cap=None)
            u.update(cem_uncertainty)
            delta = isinstance(u["w"], str)
            if delta and u["w"] != "delta_std":
                raise ValueError("cem_uncertainty: w must be None, a number, a list of them or 'delta_std', got %r" % (u["w"],))
            uparams = HipEngine.uncertainty_params(u["kind"], u["weight"], None if delta else u["w"], u["form"], u["cap"], obs_dim=obs_dim)
            names = lambda table, v: [k for k, x in table.items() if x == v][0]
            w_key = "delta_std" if delta else None if u["w"] is None else (float(u["w"]) if np.ndim(u["w"]) == 0
                                                                           else tuple(float(x) for x in np.asarray(u["w"]).reshape(-1)))
            uncertainty = (names(_lib.UNC_KINDS, uparams.kind), float(uparams.weight), w_key, names(_lib.UNC_FORMS, uparams.form),
                           None if u["cap"] is None else float(uparams.cap))
        if not isinstance(cem_action_advance, (bool, np.bool_)):
            raise ValueError("cem_action_advance must be True or False, got %r" % (cem_action_advance,))
        actuator = aparams = None
        if act_off:
            if not cem_action_advance:
                raise ValueError("cem_action_advance configures the actuator model: it needs cem_action_delay, cem_action_rate_limit or "
                                 "cem_action_rate_cost")
        else:
            aparams = HipEngine.actuator_params(cem_action_delay, cem_action_rate_limit, cem_action_rate_cost, action_dim=action_dim,
                                                horizon=n_forwards)
            as_key = lambda v: None if v is None else (float(v) if np.ndim(v) == 0 else tuple(float(x) for x in np.asarray(v).reshape(-1)))
            actuator = (int(cem_action_delay), as_key(cem_action_rate_limit), as_key(cem_action_rate_cost))
        if not isinstance(cem_target_advance, (bool, np.bool_)):
            raise ValueError("cem_target_advance must be True or False, got %r" % (cem_target_advance,))
        tracking = tparams = None
        if cem_tracking is None:
            if not cem_target_advance:
                raise ValueError("cem_target_advance configures tracking targets: it needs cem_tracking")
        else:
            tparams = HipEngine.track_params(cem_tracking)
            tracking = tuple(dict(c) for c in ([cem_tracking] if isinstance(cem_tracking, dict) else cem_tracking))
        if isinstance(cem_knots, bool) or not isinstance(cem_knots, (int, np.integer)) or int(cem_knots) < 1:
            raise ValueError("cem_knots must be an integer >= 1 (the spacing of the knot steps), got %r" % (cem_knots,))
        if cem_knot_interp not in ("hold", "linear"):
            raise ValueError("cem_knot_interp must be 'hold' or 'linear', got %r" % (cem_knot_interp,))
        if cem_knot_anchor not in ("call", "episode"):
            raise ValueError("cem_knot_anchor must be 'call' or 'episode', got %r" % (cem_knot_anchor,))
        if int(cem_knots) == 1 and (cem_knot_interp, cem_knot_anchor) != ("hold", "call"):
            raise ValueError("cem_knot_interp / cem_knot_anchor configure knots: they need cem_knots > 1")
        knots = None if int(cem_knots) == 1 else (int(cem_knots), cem_knot_interp, cem_knot_anchor)
        constraints = cparams = None
        if cem_constraints is None:
            if cem_constraint_mode != "penalty" or cem_constraint_weight is not None:
                raise ValueError("cem_constraint_mode / cem_constraint_weight configure state constraints: they need cem_constraints")
        else:
            if cem_constraint_weight is None:
                raise ValueError("cem_constraints need a cem_constraint_weight (finite, >= 0): the penalty per violating step, or at termination")
            cparams = HipEngine.constraint_params(cem_constraints, cem_constraint_mode, cem_constraint_weight)
            cons = [cem_constraints] if isinstance(cem_constraints, dict) else list(cem_constraints)
            constraints = (tuple(dict(c) for c in cons), cem_constraint_mode, float(cem_constraint_weight))
        score = None
        if cem_score not in ("mean", "mean_std", "member_std", "cvar"):
            raise ValueError("cem_score must be 'mean', 'mean_std', 'member_std' or 'cvar', got %r" % (cem_score,))
        if cem_score == "mean":
            if cem_risk is not None:
                raise ValueError("cem_risk configures a risk-aware score: it needs cem_score='mean_std', 'member_std' or 'cvar'")
        else:
            if cem_risk is None or not np.isfinite(float(cem_risk)):
                raise ValueError("cem_score=%r needs a finite cem_risk, got %r" % (cem_score, cem_risk))
            if cem_score == "cvar":
                if not 0.0 < float(cem_risk) <= 1.0:
                    raise ValueError("cem_score='cvar': cem_risk is the tail fraction, in (0, 1]; got %r" % (cem_risk,))
                score = ("cvar", 0.0, HipEngine.cvar_k(cem_risk, n_particles))
            else:
                score = (cem_score, float(cem_risk), None)
        if cem_update not in ("cem", "mppi"):
            raise ValueError("cem_update must be 'cem' or 'mppi', got %r" % (cem_update,))
        if not (np.isfinite(float(cem_temperature)) and float(cem_temperature) > 0.0):
            raise ValueError("cem_temperature must be finite and > 0, got %r" % (cem_temperature,))
        if cem_update == "cem" and (float(cem_temperature) != 1.0 or bool(cem_temperature_relative)):
            raise ValueError("cem_temperature / cem_temperature_relative configure the MPPI update: they need cem_update='mppi'")
        if cem_return not in ("mean", "best"):
            raise ValueError("cem_return must be 'mean' or 'best', got %r" % (cem_return,))
        if not 0.0 <= float(cem_noise_beta) <= 16.0:
            raise ValueError("cem_noise_beta must lie in [0, 16], got %r" % (cem_noise_beta,))
        if not float(cem_decay) >= 1.0:
            raise ValueError("cem_decay must be >= 1, got %r" % (cem_decay,))
        if int(cem_keep_elites) < 0:
            raise ValueError("cem_keep_elites must be >= 0, got %r" % (cem_keep_elites,))
        if discrete:
            raise NotImplementedError("the iCEM planner (cem_* kwargs) plans continuous actions only; this env's action space is discrete")
        if process_group is not None:
            import torch.distributed as dist
            if dist.get_world_size(process_group) > 1:
                raise NotImplementedError("the iCEM planner (cem_* kwargs) does not shard candidates over a process group of more than "
                                          "one rank: carried elites cannot be regenerated by id")
        icem = dict(noise_beta=float(cem_noise_beta), keep_elites=int(cem_keep_elites), decay=float(cem_decay), return_best=cem_return == "best",
                    add_mean_last=bool(cem_add_mean))
        mppi = dict(temperature=float(cem_temperature), relative=bool(cem_temperature_relative))
        params = HipEngine.mppi_params(**mppi, **icem) if cem_update == "mppi" else HipEngine.icem_params(**icem)
        return PlanOptions(update=cem_update, score=score, params=params, score_params=None if score is None else HipEngine.score_params(*score),
                           constraints=constraints, constraint_params=cparams, knots=knots,
                           knot_params=None if knots is None else HipEngine.knot_params(knots[0], knots[1]), tracking=tracking,
                           track_params=tparams, target_advance=bool(cem_target_advance), actuator=actuator, actuator_params=aparams,
                           action_advance=bool(cem_action_advance), uncertainty=uncertainty, uncertainty_params=uparams, value=value, value_params=vparams, reward=reward,
                           reward_params=rparams, policy=policy, policy_params=pparams, critic=critic, critic_params=qparams, discount=discount, proposals=proposals,
                           std_scale=std_scale, logp=logp, logp_params=lparams, **mppi, **icem)


def policy_slot(keep_elites, last, add_mean_last):
    """The first candidate slot of the policy prior's proposals in an iteration: behind the kept elites and, in the last iteration of a
    loop with add_mean_last, the mean candidate (csrc/icem.hip)."""
    return int(keep_elites) + (1 if last and add_mean_last else 0)


def policy_min_candidates(n, decay, num_elites, keep_elites, iters=5):
    """The candidate count of the smallest iteration of a loop of `iters` iterations, min over it of min(n, max(floor(n / decay^it),
    2 num_elites, keep_elites + 1)) (csrc/icem.hip icem_n_it; decay rounded to float32 as the library receives it): what keep_elites + 1
    + n_samples of a policy prior must fit."""
    d = float(np.float32(decay))
    return min(min(int(n), max(int(np.floor(float(n) / d ** it)), 2 * int(num_elites), int(keep_elites) + 1)) for it in range(int(iters)))


def policy_proposals_setting(opt, head_declared=False):
    """What a model hands `HipEngine.set_policy_proposals` once, at construction -> (source name, std_scale), or None for a model without
    a policy prior (nothing is set: the engine's default is the noise route).  opt: the model's `PlanOptions` (or None); head_declared:
    whether the model declares a `policy_head`.  proposals="head" without one is a ValueError: there is no head to draw from.  Needs no
    GPU."""
    if opt is None or opt.policy_params is None:
        return None
    if opt.proposals == "head" and not head_declared:
        raise ValueError("cem_policy_prior: proposals=\"head\" draws the proposals from the actor's Gaussian head: declare policy_head")
    return opt.proposals, float(opt.std_scale)


def policy_logp_setting(opt, head_declared=False, head=None):
    """The model's check of `cem_policy_logp` against its `policy_head` -> the options' `PolicyLogpParams`, or None for a model without
    the term.  opt: the model's `PlanOptions` (or None); head_declared: whether the model declares a `policy_head`; head: its
    `PolicyHeadParams` when the caller has them.  Without a head there is no density to evaluate, and a head whose log_std lower bound
    is below -10 is refused as the library refuses it (exp(-log_std) must stay finite with a margin): both ValueError.  Needs no GPU."""
    if opt is None or opt.logp_params is None:
        return None
    if not head_declared:
        raise ValueError("cem_policy_logp scores plans by the density of the actor's Gaussian head: declare policy_head")
    if head is not None and head.log_std_min < _lib.LOGSTD_MIN:
        raise ValueError("cem_policy_logp: policy_head log_std_bounds: lo %r is below %g (exp(-log_std) must stay finite with a margin)"
                         % (head.log_std_min, _lib.LOGSTD_MIN))
    return opt.logp_params


def imagine_policy_params(imagine_policy, opt=None, obs_dim=None, action_dim=None, discrete=False):
    """What a model's `imagine_policy` kwarg means -> the `PolicyParams` its actor is registered under (`set_policy`), or None for None.
    imagine_policy: dict(hidden_sizes=, activation=, squash=), the shape of the actor `imagine` rolls out on a model that PLANS without
    one; `opt`: the model's `PlanOptions` (None: the reference planner) -- a planner-declared actor (`cem_policy_prior`, or
    `cem_terminal_q`'s policy) is the one actor of a model, so giving both is refused.  Touches no planner option.  Needs no GPU."""
    if imagine_policy is None:
        return None
    if not isinstance(imagine_policy, dict) or set(imagine_policy) - {"hidden_sizes", "activation", "squash"}:
        raise ValueError("imagine_policy must be dict(hidden_sizes=, activation=, squash=), got %r" % (imagine_policy,))
    if opt is not None and opt.actor_params() is not None:
        raise ValueError("imagine_policy is given together with a planner-declared actor (cem_policy_prior / cem_terminal_q): a model has one "
                         "actor, and imagine() rolls that one out")
    if discrete:
        raise NotImplementedError("imagine_policy declares a continuous actor: this env's action space is discrete")
    if obs_dim is not None and not 1 <= int(obs_dim) <= _lib.MAX_VALUE_DIMS:
        raise ValueError("a policy net reads up to %d observation dims, got %r" % (_lib.MAX_VALUE_DIMS, obs_dim))
    if action_dim is not None and not 1 <= int(action_dim) <= _lib.MAX_POLICY_ACTIONS:
        raise ValueError("a policy net writes up to %d action dims, got %r" % (_lib.MAX_POLICY_ACTIONS, action_dim))
    q = dict(hidden_sizes=(256, 256), activation="relu", squash="tanh")
    q.update(imagine_policy)
    return HipEngine.policy_params(q["hidden_sizes"], q["activation"], q["squash"], 1, 0.0)


def policy_head_params(policy_head, has_actor=False, discrete=False, world=1):
    """What a model's `policy_head` kwarg means -> the `PolicyHeadParams` the actor's log-std layer is registered under (`set_policy`),
    or None for None.  policy_head: dict(kind="gaussian", log_std_bounds=(lo, hi), log_std_bound="clamp" | "tanh") -- the model's one
    actor (has_actor: `cem_policy_prior`, `cem_terminal_q`'s policy or `imagine_policy` declares it) is then a SAC actor whose last layer
    has 2 A outputs, the mean and the log standard deviation; log_std_bound says how the raw log-std reaches (lo, hi): clamped, or lo +
    0.5 (hi - lo) (tanh(l) + 1).  ValueError for a model without an actor, unknown keys, an unknown kind or bound, bounds that are not
    finite, lo >= hi, hi > 10 (exp must stay finite with a margin); NotImplementedError for discrete actions and for more than one rank,
    as `imagine_policy`.  Touches no planner option.  Needs no GPU."""
    if policy_head is None:
        return None
    if not isinstance(policy_head, dict) or set(policy_head) - {"kind", "log_std_bounds", "log_std_bound"}:
        raise ValueError("policy_head must be dict(kind=, log_std_bounds=, log_std_bound=), got %r" % (policy_head,))
    if discrete:
        raise NotImplementedError("policy_head declares a continuous stochastic actor: this env's action space is discrete")
    if int(world) > 1:
        raise NotImplementedError("policy_head is not supported on a process group of more than one rank")
    if not has_actor:
        raise ValueError("policy_head needs a declared actor (cem_policy_prior, cem_terminal_q's policy or imagine_policy): it is that net's head")
    q = dict(kind="gaussian", log_std_bounds=(-5.0, 2.0), log_std_bound="clamp")
    q.update(policy_head)
    if not isinstance(q["kind"], str) or q["kind"] not in _lib.HEAD_KINDS:
        raise ValueError("policy_head kind must be %s, got %r" % (" or ".join(repr(k) for k in _lib.HEAD_KINDS), q["kind"]))
    if not isinstance(q["log_std_bound"], str) or q["log_std_bound"] not in _lib.LOGSTD_BOUNDS:
        raise ValueError("policy_head log_std_bound must be %s, got %r" % (" or ".join(repr(k) for k in _lib.LOGSTD_BOUNDS), q["log_std_bound"]))
    try:
        lo, hi = (float(np.float32(v)) for v in q["log_std_bounds"])
    except (TypeError, ValueError):
        raise ValueError("policy_head log_std_bounds must be two finite numbers (lo, hi), got %r" % (q["log_std_bounds"],)) from None
    if any(isinstance(v, (bool, np.bool_)) for v in q["log_std_bounds"]) or not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError("policy_head log_std_bounds must be two finite numbers (lo, hi), got %r" % (q["log_std_bounds"],))
    if not lo < hi:
        raise ValueError("policy_head log_std_bounds need lo < hi, got %r" % (q["log_std_bounds"],))
    if hi > _lib.LOGSTD_MAX:
        raise ValueError("policy_head log_std_bounds: hi %r is beyond %g (exp must stay finite with a margin)" % (hi, _lib.LOGSTD_MAX))
    prm = _lib.PolicyHeadParams()
    prm.kind, prm.bound, prm.log_std_min, prm.log_std_max = _lib.HEAD_KINDS[q["kind"]], _lib.LOGSTD_BOUNDS[q["log_std_bound"]], lo, hi
    return prm


def split_gaussian_layers(layers, A):
    """The layers [(W [in,out], b [out])] of a SAC actor whose last layer has 2 A outputs -> (the mode actor's layers: the mean columns
    [0, A) of the last layer; W_ls, b_ls: its log-std columns [A, 2 A)) -- torch's chunk(2, -1), as contiguous float32 arrays."""
    if not layers:
        raise ValueError("set_policy: no layers given")
    W, b = layers[-1]
    if W.ndim != 2 or W.shape[1] != 2 * A or b.shape != (2 * A,):
        raise ValueError("set_policy: with a policy_head the last layer has 2 A = %d outputs (mean, then log-std), got W %r and b %r"
                         % (2 * A, tuple(W.shape), tuple(b.shape)))
    mean = list(layers[:-1]) + [(np.ascontiguousarray(W[:, :A]), np.ascontiguousarray(b[:A]))]
    return mean, np.ascontiguousarray(W[:, A:]), np.ascontiguousarray(b[A:])


IMAGINE_IT = _lib.IMAGINE_IT      # the iteration word of imagine's first one-step rollout: csrc/planner.h CADM_IMAGINE_IT
IMAGINE_MAX_STEPS = (POLICY_IT - IMAGINE_IT) // 2      # steps whose even words IMAGINE_IT + 2 t stay below the proposal roll's
ImagineArgs = collections.namedtuple("ImagineArgs", "m n k noise_std w sample", defaults=(False,))


def imagine_args(obs, cp_obs=None, cp_act=None, horizon=1, branches=1, actions=None, noise_std=0.0, disagreement_w=None, sample=None, *, obs_dim,
                 action_dim, n_particles, context=False, history_length=0, discrete=False, world=1, policy_registered=False, head_declared=False,
                 head_registered=False):
    """The parsing and the refusals of `model.imagine`'s arguments, before anything is launched -> ImagineArgs(m, n, k, noise_std, w, sample): m
    start states, n branches, k steps, the noise as the float32 the library is handed, w -- None (1 for every dim), "delta_std", or the
    float32 [D] weights of the disagreement --, and sample: whether the actions are drawn from the actor's Gaussian head (`policy_head`).
    sample None means True exactly when a head is declared and actions is None; True with noise_std > 0, with actions or without a
    registered head is a ValueError; False on a model with a head is the mode action plus noise_std.
    Arrays may be numpy or torch.  ValueError for horizon / branches < 1, neither a registered
    policy nor actions or both, wrong shapes, non-finite obs, a missing history on a context model, m * n * p rows beyond one rollout
    launch, k beyond the iteration words; NotImplementedError for a discrete action space or more than one rank.  Needs no GPU."""
    D, A, p = int(obs_dim), int(action_dim), int(n_particles)
    if discrete:
        raise NotImplementedError("imagine: discrete actions are not rolled out (the actor and the open-loop actions are continuous)")
    if int(world) > 1:
        raise NotImplementedError("imagine is not sharded over a process group of more than one rank")
    for name, v in (("horizon", horizon), ("branches", branches)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 1:
            raise ValueError("imagine: %s must be an int >= 1, got %r" % (name, v))
    k, n = int(horizon), int(branches)
    if k > IMAGINE_MAX_STEPS:
        raise ValueError("imagine: horizon %d is beyond the %d steps the rollouts' iteration words hold" % (k, IMAGINE_MAX_STEPS))
    shp = tuple(int(v) for v in np.shape(obs))
    if len(shp) != 2 or shp[1] != D or shp[0] < 1:
        raise ValueError("imagine: obs %r, expected [m,%d] with m >= 1" % (shp, D))
    m = shp[0]
    if m * n * p * max(D, A) >= 1 << 31:
        raise ValueError("imagine: m * branches * n_particles = %d rows are more than one rollout launch takes" % (m * n * p))
    finite = bool(torch.isfinite(obs).all()) if isinstance(obs, torch.Tensor) else bool(np.isfinite(np.asarray(obs, dtype=np.float64)).all())
    if not finite:
        raise ValueError("imagine: obs holds a non-finite value (a rollout cannot start from it)")
    if (actions is None) == (not policy_registered):
        raise ValueError("imagine: %s" % ("neither a registered policy (set_policy) nor actions" if actions is None else
                                          "actions are given and a policy is registered: clear_policy() first, one source of actions per call"))
    if actions is not None and tuple(int(v) for v in np.shape(actions)) != (m, n, k, A):
        raise ValueError("imagine: actions %r, expected [m,branches,horizon,A] = %r" % (tuple(np.shape(actions)), (m, n, k, A)))
    if context:
        if cp_obs is None or cp_act is None:
            raise ValueError("imagine: cp_obs and cp_act are required for a context model (each start state's own history)")
        want = ((m, D * int(history_length)), (m, A * int(history_length)))
        if (tuple(np.shape(cp_obs)), tuple(np.shape(cp_act))) != want:
            raise ValueError("imagine: cp_obs %r / cp_act %r, expected %r / %r" % ((tuple(np.shape(cp_obs)), tuple(np.shape(cp_act))) + want))
    elif cp_obs is not None or cp_act is not None:
        raise ValueError("imagine: this model has no context encoder, cp_obs / cp_act must be None")
    try:
        std = float(np.float32(noise_std))
    except (TypeError, ValueError):
        raise ValueError("imagine: noise_std must be a finite number >= 0, got %r" % (noise_std,)) from None
    if isinstance(noise_std, bool) or not np.isfinite(std) or std < 0.0:
        raise ValueError("imagine: noise_std must be a finite number >= 0, got %r" % (noise_std,))
    if actions is not None and std != 0.0:
        raise ValueError("imagine: noise_std perturbs the policy's actions; open-loop actions are taken as given")
    w = disagreement_w
    if isinstance(w, str):
        if w != "delta_std":
            raise ValueError("imagine: disagreement_w must be None, [D] numbers or 'delta_std', got %r" % (w,))
    elif w is not None:
        w = np.asarray(w, dtype=np.float32)
        if w.shape != (D,) or not bool(np.all(np.isfinite(w) & (w >= 0.0))) or not bool(np.any(w > 0.0)):
            raise ValueError("imagine: disagreement_w must be [%d] finite numbers >= 0 with at least one > 0" % D)
    if sample is not None and not isinstance(sample, (bool, np.bool_)):
        raise ValueError("imagine: sample must be None, True or False, got %r" % (sample,))
    sample = bool(head_declared and actions is None) if sample is None else bool(sample)
    if sample:
        if actions is not None:
            raise ValueError("imagine: sample=True draws the actions from the actor's head; open-loop actions are taken as given")
        if not head_registered:
            raise ValueError("imagine: sample=True needs a registered Gaussian head (declare policy_head, then set_policy)")
        if std != 0.0:
            raise ValueError("imagine: sample=True draws from the policy itself; noise_std perturbs the mode action (sample=False)")
    return ImagineArgs(m, n, k, std, w, sample)


TargetArgs = collections.namedtuple("TargetArgs", "m n k gamma lam penalty max_disagreement var_floor bootstrap")
TARGET_BOOTSTRAPS = ("value", "q", "a [horizon+1,m,branches] tensor or array of the caller's own values")


def _target_number(name, v, ok, what):
    """v as the float32 the library is handed; ValueError unless it is a number for which ok(value) holds"""
    try:
        x = float(np.float32(v))
    except (TypeError, ValueError):
        x = None
    if x is None or isinstance(v, (bool, np.bool_)) or not ok(x):
        raise ValueError("imagine_targets: %s must be %s, got %r" % (name, what, v))
    return x


def imagine_targets_args(batch, gamma, lam=0.95, bootstrap="auto", penalty=0.0, max_disagreement=None, steve=None, *, has_value=False,
                         has_q=False):
    """The parsing and the refusals of `model.imagine_targets`' arguments, before anything is launched -> TargetArgs(m, n, k, gamma, lam,
    penalty, max_disagreement, var_floor, bootstrap): the shape of `batch` (the dict `imagine` returned: rew, valid, done, disagreement
    [k,m,n] and states [k+1,m,n,D]; numpy or torch), the numbers as the float32 the library is handed (max_disagreement None: +inf;
    var_floor None: no STEVE outputs) and where the bootstrap values come from -- "value", "q" or "given".  bootstrap "auto" is whichever
    of value and q the model declares (has_value / has_q: its cem_terminal_value / cem_terminal_q), value where it declares both.
    ValueError for a batch that lacks a key or whose shapes disagree, gamma outside (0, 1], lam outside [0, 1], a penalty negative or not
    finite, a max_disagreement not > 0, a steve that is not dict(var_floor= a finite number > 0), steve with fewer than two branches, a
    bootstrap the model does not declare, or a given one of another shape.  A pure function of its inputs: it draws no noise, moves no
    counter and does not care how many ranks there are.  Needs no GPU."""
    need = ("rew", "valid", "done", "disagreement", "states")
    if not isinstance(batch, dict) or any(key not in batch for key in need):
        raise ValueError("imagine_targets: batch must be the dict imagine() returned, with %s%s"
                         % (", ".join(need), "" if not isinstance(batch, dict) else "; it lacks %s" % ", ".join(k_ for k_ in need if k_ not in batch)))
    shp = tuple(int(v) for v in np.shape(batch["rew"]))
    if len(shp) != 3 or min(shp) < 1:
        raise ValueError("imagine_targets: batch['rew'] %r, expected [horizon,m,branches] with every size >= 1" % (shp,))
    k, m, n = shp
    for key in ("valid", "done", "disagreement"):
        if tuple(int(v) for v in np.shape(batch[key])) != shp:
            raise ValueError("imagine_targets: batch[%r] %r, expected %r as batch['rew']" % (key, tuple(np.shape(batch[key])), shp))
    st = tuple(int(v) for v in np.shape(batch["states"]))
    if len(st) != 4 or st[:3] != (k + 1, m, n):
        raise ValueError("imagine_targets: batch['states'] %r, expected [horizon+1,m,branches,D] = (%d, %d, %d, D)" % (st, k + 1, m, n))
    g = _target_number("gamma", gamma, lambda x: 0.0 < x <= 1.0, "a number in (0, 1]")
    l_ = _target_number("lam", lam, lambda x: 0.0 <= x <= 1.0, "a number in [0, 1]")
    beta = _target_number("penalty", penalty, lambda x: np.isfinite(x) and x >= 0.0, "a finite number >= 0")
    maxd = float("inf") if max_disagreement is None else _target_number("max_disagreement", max_disagreement, lambda x: x > 0.0,
                                                                        "None or a number > 0")
    floor = None
    if steve is not None:
        if not isinstance(steve, dict) or set(steve) != {"var_floor"}:
            raise ValueError("imagine_targets: steve must be None or dict(var_floor=), got %r" % (steve,))
        floor = _target_number("steve var_floor", steve["var_floor"], lambda x: np.isfinite(x) and x > 0.0, "a finite number > 0")
        if n < 2:
            raise ValueError("imagine_targets: steve weighs the horizons by the variance over the branches and needs branches >= 2, "
                             "the batch has %d" % n)
    if isinstance(bootstrap, str):
        if bootstrap not in ("auto", "value", "q"):
            raise ValueError("imagine_targets: bootstrap must be 'auto' or one of %s, got %r" % (", ".join(map(repr, TARGET_BOOTSTRAPS[:2]))
                                                                                                + " or " + TARGET_BOOTSTRAPS[2], bootstrap))
        kind = bootstrap
        if kind == "auto":
            kind = "value" if has_value else "q" if has_q else None
            if kind is None:
                raise ValueError("imagine_targets: bootstrap='auto' needs a model that declares cem_terminal_value or cem_terminal_q; this "
                                 "one declares neither.  The choices are 'value' (V of the registered value net), 'q' (the critics at the "
                                 "actor's action) or %s" % TARGET_BOOTSTRAPS[2])
        if kind == "value" and not has_value:
            raise ValueError("imagine_targets: bootstrap='value' needs a model with cem_terminal_value")
        if kind == "q" and not has_q:
            raise ValueError("imagine_targets: bootstrap='q' needs a model with cem_terminal_q")
    else:
        if bootstrap is None or tuple(int(v) for v in np.shape(bootstrap)) != (k + 1, m, n):
            raise ValueError("imagine_targets: bootstrap %r, expected 'auto', 'value', 'q' or values of shape [horizon+1,m,branches] = %r"
                             % (None if bootstrap is None else tuple(np.shape(bootstrap)), (k + 1, m, n)))
        kind = "given"
    return TargetArgs(m, n, k, g, l_, beta, maxd, floor, kind)


class Shard:
    """Contiguous candidate shard of one rank."""

    def __init__(self, n, rank=0, world=1, group=None):
        if n % world != 0:
            raise ValueError("n_candidates (%d) must be divisible by the number of ranks (%d)" % (n, world))
        self.n, self.rank, self.world, self.group = n, rank, world, group
        self.n_local = n // world
        self.offset = rank * self.n_local

    @staticmethod
    def from_group(n, group):
        """Shard over the ranks of an EXPLICIT torch.distributed group.  Sharding is opt-in: a process that merely has
        torch.distributed initialised (parallel samplers planning for different observations, say) must not have its
        candidates mixed with other ranks'.  Every rank of `group` must call the planner with identical observations,
        weights and statistics (replicated state; checked by `check_replicated`)."""
        if group is None:
            return Shard(n)
        import torch.distributed as dist
        return Shard(n, dist.get_rank(group), dist.get_world_size(group), group)


def check_replicated(tensors, shard):
    """Guard for sharded planning: the replicated inputs must be the same on every rank of the group.  ONE all-reduce (MAX of
    [h, -h] gives max and -min of a position-weighted, NaN-aware checksum) plus a host sync -- so the planner runs it on the
    first few sharded calls of a model only (`MLPEnsembleCEMDynamicsModel(check_replicated_calls=...)`), not on every
    `get_action`: the steady-state call has exactly the path's own collectives (one all-gather per CEM iteration)."""
    if shard.world == 1:
        return
    import torch.distributed as dist
    sums = []
    for t in tensors:
        if t is None:
            continue
        x = torch.nan_to_num(t.double().reshape(-1), nan=12345.678, posinf=1.0e300, neginf=-1.0e300)
        w = torch.arange(1, x.numel() + 1, device=x.device, dtype=torch.float64)      # position-weighted: permutations differ
        sums.append((x * w).sum())
        sums.append(x.sum())
    h = torch.stack(sums)
    both = torch.cat([h, -h])
    if both.is_cuda and dist.get_backend(shard.group) != "nccl":      # (gloo moves host tensors)
        both = both.cpu()
    dist.all_reduce(both, op=dist.ReduceOp.MAX, group=shard.group)
    hi, lo = both[:h.numel()], -both[h.numel():]
    if not torch.equal(lo, hi):
        raise RuntimeError("candidate-sharded planning needs identical obs / history / warm start on every rank of the "
                           "group (checksums differ: %s vs %s)" % (lo.tolist(), hi.tolist()))


class ExternalAllGather:
    """The all-gather the library calls where the RCCL path calls ncclAllGather (include/cadm_hip.h: cadm_allgather_fn), over a
    torch.distributed group of any backend.  `resolve(ptr, nbytes)` maps a raw pointer of the call to a float32 torch tensor viewing
    that memory -- both pointers lie inside the planner's workspace, which the caller owns as a tensor.  Backend "nccl": the collective
    is enqueued on the current stream like every kernel of the plan.  Any other backend (gloo): the payload -- m * n/G + 1 floats per
    rank -- takes a synchronous round trip through host memory.  An exception inside the callback cannot cross the C frames: it is kept
    in `.error` (the library call then fails and `HipEngine._check` re-raises it)."""

    def __init__(self, group, resolve):
        import torch.distributed as dist
        from . import _lib
        self.group, self.resolve = group, resolve
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        self.backend = dist.get_backend(group)
        self.error, self.calls = None, 0
        self.cfunc = _lib.ALLGATHER_FN(self._call)      # (kept alive with the object: the library holds the raw function pointer)

    def _call(self, user, send, recv, count, stream):
        try:
            self.gather(self.resolve(send, 4 * count), self.resolve(recv, 4 * count * self.world))
            self.calls += 1
            return 0
        except BaseException as exc:      # noqa: B902 -- nothing may propagate into the C caller
            self.error = exc
            return 1

    def gather(self, send, recv):
        """[count] floats of every rank -> [world * count] floats, rank-major, on every rank"""
        import torch.distributed as dist
        if send.is_cuda and self.backend != "nccl":
            host = torch.empty(recv.shape, dtype=recv.dtype)
            dist.all_gather_into_tensor(host, send.cpu(), group=self.group)      # (.cpu() waits for the stream's work on `send`)
            recv.copy_(host)
        else:
            dist.all_gather_into_tensor(recv, send.contiguous(), group=self.group)


def cem_plan(engine, obs, cp_obs, cp_act, init_mean, init_var, n, seed=0, call=0, z=None, eps=None, return_info=False):
    """Single rank, one iteration at a time over the engine's primitives.  z [iters,m,n,H,A] / eps [iters,H,m,n,p,D]: optional injected draws."""
    obs = engine._t(obs)
    mean = engine._t(init_mean).clone()
    var = engine._t(init_var).clone()
    ctx_vec = engine.context_forward(cp_obs, cp_act) if engine.C > 0 else None
    info = []
    for it in range(engine.num_cem_iters):
        actions = engine.sample_actions(mean, var, n, z=None if z is None else z[it], seed=seed, call=call, it=it)
        rows = engine.rollout_returns(obs, ctx_vec, actions, eps=None if eps is None else eps[it], seed=seed, call=call, it=it)
        cand = engine.particle_mean(rows).unsqueeze(0)
        elites = engine.cem_refit(cand, actions, mean, var, want_elites=return_info)
        if return_info:
            info.append(dict(actions=actions, rows=rows, cand=cand, elites=elites, mean=mean.clone(), var=var.clone()))
    plan = mean if engine.discrete else mean.clamp(float(engine.cfg.lower_bound), float(engine.cfg.upper_bound))   # dynamics.py:365-366
    return (plan, info, ctx_vec) if return_info else plan


def rs_plan(engine, obs, cp_obs, cp_act, n, seed=0, call=0, actions=None, raw=None, eps=None):
    obs = engine._t(obs)
    m = obs.shape[0]
    ctx_vec = engine.context_forward(cp_obs, cp_act) if engine.C > 0 else None
    if actions is None:
        actions, raw = engine.sample_uniform(m, n, seed=seed, call=call)
    else:
        actions = engine._t(actions)
    rows = engine.rollout_returns(obs, ctx_vec, actions, eps=eps, norm_actions=not engine.discrete, seed=seed, call=call, it=0)
    cand = engine.particle_mean(rows).unsqueeze(0)
    first, best = engine.rs_select(cand, actions)
    if engine.discrete:
        raw = engine._t(raw, dtype=torch.int32)
        return raw[torch.arange(m, device=raw.device), best.long(), 0], cand
    return first.clamp(float(engine.cfg.lower_bound), float(engine.cfg.upper_bound)), cand


def icem_plan(engine, obs, cp_obs, cp_act, init_mean, init_var, n, noise_beta=0.0, keep_elites=0, decay=1.0, return_best=False,
              add_mean_last=False, carry=None, carry_valid=None, seed=0, call=0, z=None, xi=None, eps=None, return_info=False,
              update="cem", temperature=1.0, relative=False, score=None, constraints=None, knots=None, phase=None, tracking=None, actuator=None,
              action_advance=False, uncertainty=None, value=None, reward=None, policy=None, critic=None, policy_logp=None):
    """The iCEM loop of `cadm_icem_plan` (csrc/icem.hip) one launch at a time over the engine's primitives, single rank: for parity
    tests with injected draws and for diagnostics.  update="mppi": the loop of `cadm_mppi_plan` -- the elite ids come from an elite
    refit into copies of mean / var, the distribution from `mppi_refit`.  score: a `HipEngine.score_params` (`cadm_scored_plan`; None: the
    particle mean) -- `cand`, the elites and the best return are then by score.  constraints: a `HipEngine.constraint_params`
    (`cadm_constrained_plan`; None: none) -- every rollout then records its trajectories and `constrain_returns` rewrites `rows` before the
    score; `return_info` carries `traj`, `first_violation`, `violations` and the rollout's own `rows_raw`.  z / xi / eps: optional per-iteration lists of injected truncated-normal draws
    [m,n_it,H,A] (noise_beta == 0), spectral draws [m,n_it,A,H] (noise_beta > 0) and head noise [H,m,n_it,p,D].  carry [m,K,H,A] /
    carry_valid [m] int32 are read at iteration 0 and rewritten IN PLACE after the last refit, as the library does.  knots: a
    `HipEngine.knot_params` (`cadm_knot_plan`; None or spacing 1: none) with phase [m] int32 (None: 0) -- the copy of init_mean and every
    iteration's candidates, behind the injections, are shaped onto the grid (`shape_actions`); `return_info` carries the shaped `actions`.
    tracking: (a `HipEngine.track_params`, targets [m,T,K] or [m,K], offset [m] int32 or None) (`cadm_tracking_plan`; None: none) -- every
    rollout then records its trajectories and `tracking_returns` takes the cost off `rows` behind `constrain_returns` (whose first
    violations it reads in terminate mode) and before the score; `return_info` carries `track_cost` and `rows_untracked`.
    actuator: (a `HipEngine.actuator_params`, prev [m,A], prefix [m,delay,A] or None) (`cadm_actuated_plan`; None: none) -- every
    iteration's candidates pass `actuate_actions` behind the knot shaping, their cost comes off `cand` behind the score, and the plan takes
    one more pass with n = 1; `return_info` carries the actuated `actions`, `action_cost` [m,n_it] and `score`, the candidates' score
    before the subtraction.  action_advance: then prev and prefix are moved on by one step IN PLACE, as the library does.
    uncertainty: a `HipEngine.uncertainty_params` (`cadm_uncertain_plan`; None: none) -- every rollout then records its trajectories,
    `uncertainty_cost` prices them (under TERMINATE constraints with their first violations) and float32(lambda * cost) comes off `cand`
    behind the actuator's cost; `return_info` carries `unc_steps` [m,n_it,H], `unc_cost` [m,n_it] and `unc_score`, the candidates' score
    before that subtraction.
    value: a `HipEngine.value_params` describing the engine's registered value net (`cadm_valued_plan`; None: none) -- every rollout then
    records its trajectories and `value_returns` adds weight * V(last state) to the particle rows behind the constraints (under TERMINATE
    with their first violations) and the tracking terms, before the score; `return_info` carries `value` [m,n_it,p], V of every row (NaN
    where skipped), and `value_rows`, the rows before the addition.
    reward: a `HipEngine.reward_params` describing the engine's registered reward net (`cadm_rewarded_plan`; None: none) -- every rollout
    then records its trajectories and `reward_returns` adds weight * (the sum of R over the counted steps) to the particle rows behind the
    constraints (under TERMINATE with their first violations) and the tracking terms, in front of the terminal value; `return_info`
    carries `reward_steps` [H,m,n_it,p] (NaN where not counted), `reward_sum` [m,n_it,p] and `reward_rows`, the rows before the addition.
    policy: a `HipEngine.policy_params` describing the engine's registered policy net (`cadm_guided_plan`; None: none) -- one
    `policy_propose` behind the context encoder, and in every iteration its sequences are injected at `policy_slot`, in front of the knot
    shaping and the actuator pass; the third return value of `return_info` carries `proposals` [m,P,H,A].
    critic: a `HipEngine.critic_params` describing the engine's registered critics (`cadm_critic_plan`; None: none; not with `value`) --
    every rollout then records its trajectories and `critic_returns` adds weight * reduce_c Q_c(s, pi(s)) of the last state to the
    particle rows behind the reward stage, before the score; `return_info` carries `q` [m,n_it,p] (NaN where skipped) and `q_rows`, the
    rows before the addition.
    policy_logp: a `HipEngine.policy_logp_params` (`cadm_anchored_plan`; None: none) -- every rollout then records its trajectories and
    `policy_logp_returns` adds weight * (the sum of log pi(a_t | s_t) over the counted steps) to the particle rows behind the learned
    reward and in front of the terminal value / Q; `return_info` carries `logp_steps` [H,m,n_it,p] (NaN where not counted), `logp_sum`
    [m,n_it,p] and `logp_rows`, the rows before the addition.
    On an engine with a discount over the horizon (`HipEngine.set_discount`) every rollout records its trajectories and
    `discount_returns` rewrites `rows` directly behind it, in front of the constraints; the stage calls above pick the engine's table up
    themselves; `return_info` carries `rows_undiscounted`, the rollout's own sums, and `rows_discounted` (`rows_raw` is then the
    discounted rows the constraints read)."""
    if critic is not None and value is not None:
        raise ValueError("icem_plan: critic and value are both given: a plan has one terminal term")
    obs = engine._t(obs)
    mean, var = engine._t(init_mean).clone(), engine._t(init_var).clone()
    if knots is not None and knots.spacing == 1:
        knots = None
    if knots is not None:
        engine.shape_actions(mean, knots, phase)
    m, K, iters = obs.shape[0], int(keep_elites), engine.num_cem_iters
    lo, hi = float(engine.cfg.lower_bound), float(engine.cfg.upper_bound)
    ctx_vec = engine.context_forward(cp_obs, cp_act) if engine.C > 0 else None
    proposals = None if policy is None else engine.policy_propose(policy, obs, ctx_vec, seed=seed, call=call)
    best_ret = torch.full((m,), float("nan"), dtype=torch.float32, device=engine.device)      # NaN: nothing scored yet (icem_best_init_kernel)
    best_seq = torch.full((m, engine.H, engine.A), float("nan"), dtype=torch.float32, device=engine.device)
    kept, info = None, []
    discounted = engine.discount_weights() is not None
    for it in range(iters):
        last = it + 1 == iters
        ni = engine.icem_candidates(n, decay, it, K)
        if noise_beta > 0:
            actions = engine.sample_actions_colored(mean, var, ni, noise_beta, xi=None if xi is None else xi[it], seed=seed, call=call, it=it)
        else:
            actions = engine.sample_actions(mean, var, ni, z=None if z is None else z[it], seed=seed, call=call, it=it)
        if K > 0 and it == 0:
            engine.icem_inject(actions, carry, valid=carry_valid, shift=1)
        elif K > 0:
            engine.icem_inject(actions, kept)
        if last and add_mean_last:
            engine.icem_inject(actions, mean.clamp(lo, hi).unsqueeze(1).contiguous(), slot0=K)
        if proposals is not None:
            engine.icem_inject(actions, proposals, slot0=policy_slot(K, last, add_mean_last))
        if knots is not None:
            engine.shape_actions(actions, knots, phase)
        action_cost = None
        if actuator is not None:
            _, action_cost = engine.actuate_actions(actions, actuator[0], prev=actuator[1], prefix=actuator[2], want_cost=True)
        extra = {}
        if constraints is None and tracking is None and uncertainty is None and value is None and reward is None and critic is None \
                and policy_logp is None and not discounted:
            rows = engine.rollout_returns(obs, ctx_vec, actions, eps=None if eps is None else eps[it], seed=seed, call=call, it=it)
        else:
            rows, traj = engine.rollout_returns(obs, ctx_vec, actions, eps=None if eps is None else eps[it], seed=seed, call=call, it=it,
                                                want_traj=True)
            first = None
            if discounted:
                undiscounted = rows
                rows = engine.discount_returns(traj, obs, actions, undiscounted)
                extra = dict(traj=traj, rows_undiscounted=undiscounted, rows_discounted=rows)
            if constraints is not None:
                raw = rows
                rows, first, viol = engine.constrain_returns(traj, raw, constraints, obs=obs, actions=actions)
                extra.update(traj=traj, first_violation=first, violations=viol, rows_raw=raw)
                if constraints.mode != _lib.CONSTRAIN_MODES["terminate"]:
                    first = None
            if tracking is not None:
                untracked = rows
                rows, cost = engine.tracking_returns(traj, untracked, tracking[0], tracking[1], offset=tracking[2], first=first, want_cost=True)
                extra.update(traj=traj, track_cost=cost, rows_untracked=untracked)
            if reward is not None:
                unrewarded = rows
                rows, steps, rsum = engine.reward_returns(traj, obs, actions, unrewarded, reward, first=first, want_steps=True)
                extra.update(traj=traj, reward_steps=steps, reward_sum=rsum, reward_rows=unrewarded)
            if policy_logp is not None:
                logp_rows = rows
                rows, lsteps, lsum = engine.policy_logp_returns(traj, obs, actions, logp_rows, policy_logp, first=first, want_steps=True)
                extra.update(traj=traj, logp_steps=lsteps, logp_sum=lsum, logp_rows=logp_rows)
            if value is not None:
                unvalued = rows
                rows, v = engine.value_returns(traj, unvalued, value, first=first, want_v=True)
                extra.update(traj=traj, value=v, value_rows=unvalued)
            if critic is not None:
                q_rows = rows
                rows, q = engine.critic_returns(traj, q_rows, critic, first=first, want_q=True)
                extra.update(traj=traj, q=q, q_rows=q_rows)
        cand = engine.particle_mean(rows) if score is None else engine.particle_score(rows, score)
        if actuator is not None:
            extra.update(action_cost=action_cost, score=cand)
            cand = cand - action_cost
        if uncertainty is not None:
            unc_steps, unc_cost = engine.uncertainty_cost(traj, uncertainty, first=first, want_steps=True)
            extra.update(traj=traj, unc_steps=unc_steps, unc_cost=unc_cost, unc_score=cand)
            cand = cand - unc_cost * torch.tensor(uncertainty.weight, dtype=torch.float32, device=cand.device)      # (two roundings, as the kernel's)
        if update == "mppi":
            elites = engine.cem_refit(cand.unsqueeze(0), actions, mean.clone(), var.clone(), want_elites=True)
            engine.mppi_refit(cand, actions, mean, var, temperature=temperature, relative=relative)
        else:
            elites = engine.cem_refit(cand.unsqueeze(0), actions, mean, var, want_elites=True)
        engine.icem_track_best(cand, elites, actions, best_ret, best_seq)
        if K > 0:
            kept = engine.icem_keep(actions, elites, K)
            if last:
                carry.copy_(kept)
                carry_valid.fill_(1)
        if return_info:
            info.append(dict(actions=actions, rows=rows, cand=cand, elites=elites, kept=kept, mean=mean.clone(), var=var.clone(), **extra))
    plan_mean = mean.clamp(lo, hi)
    plan = best_seq if return_best else plan_mean
    if actuator is not None:
        plan = engine.actuate_actions(plan.clone(), actuator[0], prev=actuator[1], prefix=actuator[2])
        if action_advance:
            d = actuator[0].delay
            actuator[1].copy_(plan[:, 0])
            if d > 0:
                actuator[2].copy_(plan[:, 1:1 + d])
    return (plan, info, dict(best_ret=best_ret, best_seq=best_seq, plan_mean=plan_mean, proposals=proposals)) if return_info else plan
