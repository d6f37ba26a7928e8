"""MLPEnsembleCEMDynamicsModel (Vanilla DM / PE-TS, no context) -- MI355X drop-in for
/root/reference/cadm/dynamics/mlp_ensemble_cem_dynamics.py:11.

Same constructor kwargs (:25-45) and methods: get_action(obs, cem_init_mean, cem_init_var)
(:191-207), fit(obs, act, obs_next, ...) (:209-323), save/load (:325-341).  Shares the HIP
path of the CaDM model with context_dim = 0 and no backward model.
"""
from collections import OrderedDict

import numpy as np

from .mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as _CaDMModel


class MLPEnsembleCEMDynamicsModel(_CaDMModel):
    def __init__(self, name, env, hidden_sizes=(200, 200, 200, 200), hidden_nonlinearity="swish",
                 output_nonlinearity=None, batch_size=128, learning_rate=0.001, normalize_input=True,
                 optimizer=None, valid_split_ratio=0.2, rolling_average_persitency=0.99, n_forwards=30,
                 n_candidates=2500, ensemble_size=5, n_particles=20, use_cem=False, deterministic=False,
                 weight_decays=(0., 0., 0., 0., 0.), weight_decay_coeff=0.0, **extensions):
        """The reference's own kwargs (:25-45); `extensions`: the CaDM class's, checked by its signature -- but its context kwargs."""
        for kw in ("cp_hidden_sizes", "context_weight_decays", "context_out_dim", "context_hidden_nonlinearity", "history_length",
                   "future_length", "state_diff", "back_coeff"):
            if kw in extensions:
                raise TypeError("__init__() got an unexpected keyword argument %r" % kw)
        super().__init__(name, env, hidden_sizes=hidden_sizes, hidden_nonlinearity=hidden_nonlinearity,
                         output_nonlinearity=output_nonlinearity, batch_size=batch_size, learning_rate=learning_rate,
                         normalize_input=normalize_input, optimizer=optimizer, valid_split_ratio=valid_split_ratio,
                         rolling_average_persitency=rolling_average_persitency, n_forwards=n_forwards,
                         n_candidates=n_candidates, ensemble_size=ensemble_size, n_particles=n_particles,
                         use_cem=use_cem, deterministic=deterministic, weight_decays=weight_decays,
                         weight_decay_coeff=weight_decay_coeff, cp_hidden_sizes=(), context_weight_decays=(),
                         context_out_dim=0, history_length=0, future_length=1, state_diff=False, back_coeff=0.0, **extensions)

    def get_action(self, obs, cem_init_mean=None, cem_init_var=None, return_forecast=False):
        if return_forecast:
            return super().get_action(obs, None, None, cem_init_mean, cem_init_var, return_forecast=True)
        return super().get_action(obs, None, None, cem_init_mean, cem_init_var)

    def forecast(self, obs, actions, band_k=1, seed=None):
        """The model's per-step prediction under `actions` (see the CaDM class; a vanilla model has no history)."""
        return super().forecast(obs, actions, None, None, band_k=band_k, seed=seed)

    def constraint_check(self, obs, actions, seed=None):
        """Which particles of `actions` violate this model's `cem_constraints`, and when (see the CaDM class; a vanilla model has no history)."""
        return super().constraint_check(obs, actions, None, None, seed=seed)

    def tracking_cost(self, obs, actions, seed=None):
        """What this model's `cem_tracking` terms cost `actions` against the current targets (see the CaDM class; a vanilla model has no history)."""
        return super().tracking_cost(obs, actions, None, None, seed=seed)

    def uncertainty_cost(self, obs, actions, seed=None):
        """What this model's `cem_uncertainty` term makes of `actions` (see the CaDM class; a vanilla model has no history)."""
        return super().uncertainty_cost(obs, actions, None, None, seed=seed)

    def plan_terminal_value(self, obs, actions, seed=None):
        """What this model's `cem_terminal_value` adds for `actions` (see the CaDM class; a vanilla model has no history)."""
        return super().plan_terminal_value(obs, actions, None, None, seed=seed)

    def plan_rewards(self, obs, actions, seed=None):
        """The learned step rewards of `actions` under this model's `cem_reward_net` (see the CaDM class; a vanilla model has no history)."""
        return super().plan_rewards(obs, actions, None, None, seed=seed)

    def plan_terminal_q(self, obs, actions, seed=None):
        """What this model's `cem_terminal_q` adds for `actions` (see the CaDM class; a vanilla model has no history)."""
        return super().plan_terminal_q(obs, actions, None, None, seed=seed)

    def plan_policy_log_prob(self, obs, actions, seed=None):
        """The actor's log-density along `actions` under this model's `cem_policy_logp` (see the CaDM class; a vanilla model has no history)."""
        return super().plan_policy_log_prob(obs, actions, None, None, seed=seed)

    def plan_returns(self, obs, actions, seed=None):
        """The discounted env returns of `actions` under this model's `cem_discount` (see the CaDM class; a vanilla model has no history)."""
        return super().plan_returns(obs, actions, None, None, seed=seed)

    def policy_proposals(self, obs, seed=None, return_states=False):
        """The sequences this model's `cem_policy_prior` would inject for `obs` (see the CaDM class; a vanilla model has no history)."""
        return super().policy_proposals(obs, None, None, seed=seed, return_states=return_states)

    def predict(self, obs, act, return_std=False):
        return super().predict(obs, act, None, None, return_std=return_std)

    def get_context_pred(self, *a, **k):
        raise AttributeError("the vanilla model has no context encoder")

    def compute_normalization(self, obs, act, delta, *unused):
        """reference :343-351: the vanilla model keeps obs / delta / act statistics only.  (The extra positional
        arguments are what the shared `fit` passes for the CaDM model; a vanilla model has no history / backward net.)"""
        assert obs.shape[0] == delta.shape[0] == act.shape[0]
        proc_obs = self.env.obs_preproc(obs)
        n = OrderedDict()
        n["obs"] = (np.mean(proc_obs, axis=0), np.std(proc_obs, axis=0))
        n["delta"] = (np.mean(delta, axis=0), np.std(delta, axis=0))
        n["act"] = (np.mean(act, axis=0), np.std(act, axis=0))
        self.normalization = n
        self._stats_dirty = True

    def get_normalization_stats(self):
        """reference :353-373: (obs_mean, obs_std, act_mean, act_std, delta_mean, delta_std)."""
        return self._stats12()[:6]

    def evaluate_horizon(self, obs, act, obs_next, seed=None, chunk=4096):
        """Prediction error on held-out samples with the planner's particles (see the CaDM class; a vanilla model's windows hold
        one step, so F = 1)."""
        N = obs.shape[0]
        D, A = self.obs_space_dims, self.action_space_dims
        assert obs.ndim == 2 and obs.shape[1] == D
        assert obs_next.ndim == 2 and obs_next.shape[1] == D
        assert act.ndim == 2 and act.shape[1] == A
        return super().evaluate_horizon(obs, act, obs_next, np.zeros((N, 0)), np.zeros((N, 0)), np.ones((N, 1)), seed=seed, chunk=chunk)

    def evaluate_calibration(self, obs, act, obs_next, seed=None, chunk=4096):
        """Calibration of the predictive distribution on held-out samples (see the CaDM class; a vanilla model's windows hold one
        step, so F = 1)."""
        N = obs.shape[0]
        D, A = self.obs_space_dims, self.action_space_dims
        assert obs.ndim == 2 and obs.shape[1] == D
        assert obs_next.ndim == 2 and obs_next.shape[1] == D
        assert act.ndim == 2 and act.shape[1] == A
        return super().evaluate_calibration(obs, act, obs_next, np.zeros((N, 0)), np.zeros((N, 0)), np.ones((N, 1)), seed=seed, chunk=chunk)

    def fit(self, obs, act, obs_next, epochs=1000, compute_normalization=True, valid_split_ratio=None,
            rolling_average_persitency=None, verbose=False, log_tabular=False, max_logging=5000, rng=None, index_stream=None):
        """reference :209-323 (single-step samples, no history window)."""
        N = obs.shape[0]
        D, A = self.obs_space_dims, self.action_space_dims
        assert obs.ndim == 2 and obs.shape[1] == D
        assert obs_next.ndim == 2 and obs_next.shape[1] == D
        assert act.ndim == 2 and act.shape[1] == A
        return super().fit(obs, act, obs_next, np.zeros((N, 0)), np.zeros((N, 0)), np.ones((N, 1)), epochs=epochs,
                           compute_normalization=compute_normalization, valid_split_ratio=valid_split_ratio,
                           rolling_average_persitency=rolling_average_persitency, verbose=verbose,
                           log_tabular=log_tabular, max_logging=max_logging, rng=rng, index_stream=index_stream)
