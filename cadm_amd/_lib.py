"""ctypes binding of libcadm_hip.so (the C ABI declared in include/cadm_hip.h).

The library is the product: there is NO Python / PyTorch fallback for any planner or
training arithmetic.  If the shared object is missing or a call fails, this module
raises -- loudly -- instead of computing anything on the host.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcadm_hip.so")              # the product; nothing in the environment redirects it
DEV_LIB_PATH = os.path.join(_HERE, "libcadm_hip_dev.so")      # product objects + csrc/dev/ (comparison kernel, developer hooks)
CSRC = os.path.join(_HERE, "csrc")

ABI_VERSION = 2
MAX_HIDDEN_LAYERS = 8
MAX_CP_LAYERS = 8

ENV_KINDS = {"halfcheetah": 0, "cripple_halfcheetah": 0, "ant": 1, "slim_humanoid": 2,
             "cartpole": 3, "pendulum": 4}
ENV_SPEC = 5              # CADM_ENV_SPEC: a user-declared env (cadm_amd/env_spec.py EnvDecl)
SPEC_MAX_D, SPEC_MAX_TERMS = 48, 32
NET_FF, NET_BACK, NET_CTX = 0, 1, 2
# hidden nonlinearity codes (include/cadm_hip.h CADM_ACT_*; the reference's `_activations`, dynamics.py:17-24)
ACT_KINDS = {"swish": 0, "relu": 1, "tanh": 2, "sigmoid": 3, None: 4}
NOISE_PHILOX, NOISE_INJECT, NOISE_NONE = 0, 1, 2


class CadmError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("env_kind", C.c_int32), ("ensemble_size", C.c_int32),
        ("n_particles", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32),
        ("proc_obs_dim", C.c_int32), ("context_dim", C.c_int32), ("n_hidden", C.c_int32),
        ("hidden", C.c_int32), ("horizon", C.c_int32), ("deterministic", C.c_int32),
        ("discrete", C.c_int32), ("reference_quirks", C.c_int32), ("history_length", C.c_int32),
        ("n_cp_hidden", C.c_int32), ("cp_hidden", C.c_int32 * MAX_CP_LAYERS),
        ("num_elites", C.c_int32), ("num_cem_iters", C.c_int32), ("alpha", C.c_float),
        ("lower_bound", C.c_float), ("upper_bound", C.c_float), ("back_model", C.c_int32),
        ("hidden_act", C.c_int32), ("reserved", C.c_int32 * 6),
    ]


class EnvSpecC(C.Structure):          # include/cadm_hip.h cadm_env_spec
    _fields_ = [
        ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("proc_obs_dim", C.c_int32),
        ("preproc", C.c_int32 * SPEC_MAX_D), ("postproc", C.c_int32 * SPEC_MAX_D), ("n_terms", C.c_int32),
        ("term_kind", C.c_int32 * SPEC_MAX_TERMS), ("term_dim", C.c_int32 * SPEC_MAX_TERMS), ("term_when", C.c_int32 * SPEC_MAX_TERMS),
        ("term_w", C.c_float * SPEC_MAX_TERMS), ("term_lo", C.c_float * SPEC_MAX_TERMS), ("term_hi", C.c_float * SPEC_MAX_TERMS),
        ("ctrl_cost", C.c_float), ("bonus", C.c_float), ("hash_lo", C.c_uint32), ("hash_hi", C.c_uint32),
    ]


class IcemParams(C.Structure):          # include/cadm_hip.h cadm_icem_params
    _fields_ = [("noise_beta", C.c_float), ("keep_elites", C.c_int32), ("decay", C.c_float), ("return_best", C.c_int32),
                ("add_mean_last", C.c_int32)]


class MppiParams(C.Structure):          # include/cadm_hip.h cadm_mppi_params
    _fields_ = [("icem", IcemParams), ("temperature", C.c_float), ("relative", C.c_int32)]


class ScoreParams(C.Structure):         # include/cadm_hip.h cadm_score_params
    _fields_ = [("mode", C.c_int32), ("kappa", C.c_float), ("k", C.c_int32)]


class ForecastOut(C.Structure):         # include/cadm_hip.h cadm_forecast_out: device pointers
    _fields_ = [(k, C.c_void_p) for k in ("mean", "member_mean", "var_total", "var_epistemic", "var_aleatoric", "lo", "hi", "reward_mean",
                                          "reward_var", "reward_member", "returns", "diverged_step", "rollout_returns")]


class CalibrationOut(C.Structure):     # include/cadm_hip.h cadm_calibration_out: device pointers
    _fields_ = [(k, C.c_void_p) for k in ("rank_hist", "rank_hist_member", "ties", "degenerate", "crps", "z2", "nll", "count", "diverged")]


SCORE_MODES = {"mean": 0, "mean_std": 1, "member_std": 2, "cvar": 3}      # CADM_SCORE_*
MAX_CONSTRAINTS = 16                                                       # CADM_MAX_CONSTRAINTS
CONSTRAIN_MODES = {"penalty": 0, "terminate": 1}                           # CADM_CONSTRAIN_*


class ConstraintParams(C.Structure):    # include/cadm_hip.h cadm_constraint_params
    _fields_ = [("n", C.c_int32), ("mode", C.c_int32), ("weight", C.c_float), ("dim", C.c_int32 * MAX_CONSTRAINTS),
                ("lo", C.c_float * MAX_CONSTRAINTS), ("hi", C.c_float * MAX_CONSTRAINTS)]


KNOT_INTERPS = {"hold": 0, "linear": 1}                                    # CADM_KNOT_*


class KnotParams(C.Structure):          # include/cadm_hip.h cadm_knot_params
    _fields_ = [("spacing", C.c_int32), ("interp", C.c_int32)]


MAX_TRACK_TERMS = 16                                                       # CADM_MAX_TRACK_TERMS
TRACK_KINDS = {"square": 0, "abs": 1, "huber": 2}                          # CADM_TRACK_*


class TrackParams(C.Structure):         # include/cadm_hip.h cadm_track_params
    _fields_ = [("n", C.c_int32), ("dim", C.c_int32 * MAX_TRACK_TERMS), ("kind", C.c_int32 * MAX_TRACK_TERMS),
                ("w", C.c_float * MAX_TRACK_TERMS), ("delta", C.c_float * MAX_TRACK_TERMS)]


MAX_ACT_DIMS = 32                                                          # CADM_MAX_ACT_DIMS


class ActuatorParams(C.Structure):      # include/cadm_hip.h cadm_actuator_params
    _fields_ = [("delay", C.c_int32), ("n_dims", C.c_int32), ("rate_limit", C.c_float * MAX_ACT_DIMS), ("rate_w", C.c_float * MAX_ACT_DIMS)]


MAX_UNC_DIMS = 128                                                         # CADM_MAX_UNC_DIMS
UNC_KINDS = {"epistemic": 0, "total": 1}                                   # CADM_UNC_EPISTEMIC / CADM_UNC_TOTAL
UNC_FORMS = {"var": 0, "std": 1}                                           # CADM_UNC_VAR / CADM_UNC_STD


class UncertaintyParams(C.Structure):   # include/cadm_hip.h cadm_uncertainty_params
    _fields_ = [("kind", C.c_int32), ("form", C.c_int32), ("weight", C.c_float), ("cap", C.c_float), ("n_dims", C.c_int32),
                ("w", C.c_float * MAX_UNC_DIMS)]


MAX_VALUE_LAYERS, MAX_VALUE_WIDTH, MAX_VALUE_DIMS = 4, 512, 128            # CADM_MAX_VALUE_LAYERS / _WIDTH / _DIMS
VALUE_ACTS = {"relu": 0, "tanh": 1, "swish": 2}                            # CADM_VALUE_RELU / _TANH / _SWISH


class ValueParams(C.Structure):         # include/cadm_hip.h cadm_value_params
    _fields_ = [("n_hidden", C.c_int32), ("hidden", C.c_int32 * MAX_VALUE_LAYERS), ("activation", C.c_int32), ("weight", C.c_float)]


MAX_REWARD_DIMS = 256                                                      # CADM_MAX_REWARD_DIMS
REWARD_INPUTS = {"next_obs": 0, "obs_act": 1, "obs_act_next_obs": 2}       # CADM_REWARD_NEXT_OBS / _OBS_ACT / _OBS_ACT_NEXT_OBS


class RewardParams(C.Structure):        # include/cadm_hip.h cadm_reward_params (the layer conventions are the value net's)
    _fields_ = [("n_hidden", C.c_int32), ("hidden", C.c_int32 * MAX_VALUE_LAYERS), ("activation", C.c_int32), ("inputs", C.c_int32),
                ("weight", C.c_float)]


MAX_POLICY_ACTIONS = 64                                                    # CADM_MAX_POLICY_ACTIONS
POLICY_SQUASH = {"none": 0, "tanh": 1}                                     # CADM_POLICY_NONE / _TANH
IMAGINE_IT = 0xF00000                                                      # csrc/planner.h CADM_IMAGINE_IT: imagine's one-step rollouts run under IMAGINE_IT + 2 t, below POLICY_IT
IMAGINE_VIEWS = 9                                                          # include/cadm_hip.h CADM_IMAGINE_VIEWS: the outputs cadm_imagine_workspace_bytes reports offsets of
STREAM_IMAGINE, STREAM_IMAGINE_ACT = 6, 7                                  # csrc/common.h: the Philox stream words of imagine's particle draw and action noise
POLICY_IT = 0xFA0000                                                       # csrc/planner.h CADM_POLICY_IT: the roll's one-step rollouts run under POLICY_IT + 2 t


TARGET_VIEWS = 10                                                          # include/cadm_hip.h CADM_TARGET_VIEWS: the outputs cadm_imagine_targets_workspace_bytes reports offsets of


class TargetParams(C.Structure):        # include/cadm_hip.h cadm_target_params
    _fields_ = [("gamma", C.c_float), ("lam", C.c_float), ("penalty", C.c_float), ("max_disagreement", C.c_float), ("var_floor", C.c_float),
                ("want_steve", C.c_int32)]


class PolicyParams(C.Structure):       # include/cadm_hip.h cadm_policy_params (the layer conventions are the value net's)
    _fields_ = [("n_hidden", C.c_int32), ("hidden", C.c_int32 * MAX_VALUE_LAYERS), ("activation", C.c_int32), ("squash", C.c_int32),
                ("n_samples", C.c_int32), ("noise_std", C.c_float)]


HEAD_KINDS = {"gaussian": 1}                                               # CADM_HEAD_GAUSSIAN
LOGSTD_BOUNDS = {"clamp": 0, "tanh": 1}                                    # CADM_LOGSTD_CLAMP / _TANH
LOGSTD_MAX = 10.0                                                          # the largest log_std_max a head takes: expf stays finite with a margin
STREAM_POLICY_SAMPLE = 8                                                   # csrc/common.h: the Philox stream word of the Gaussian head's draws
PROPOSALS = {"noise": 0, "head": 1}                                        # CADM_PROPOSE_NOISE / _HEAD: where the policy prior's proposals come from
IMAGINE_SAMPLED_VIEWS = 10                                                 # include/cadm_hip.h CADM_IMAGINE_SAMPLED_VIEWS: cadm_imagine's nine, then logp


class PolicyHeadParams(C.Structure):   # include/cadm_hip.h cadm_policy_head_params
    _fields_ = [("kind", C.c_int32), ("bound", C.c_int32), ("log_std_min", C.c_float), ("log_std_max", C.c_float)]


LOGP_SPACES = {"action": 0, "pre_squash": 1}                               # CADM_LOGP_ACTION / _PRE_SQUASH
LOGP_YMAX = 0.999999                                                       # CADM_LOGP_YMAX: where |y| is clamped before atanh
LOGSTD_MIN = -10.0                                                         # the smallest log_std_min the log-density takes: expf(-ls) stays finite with a margin


class PolicyLogpParams(C.Structure):   # include/cadm_hip.h cadm_policy_logp_params
    _fields_ = [("weight", C.c_float), ("space", C.c_int32)]


MAX_CRITICS = 5                                                            # CADM_MAX_CRITICS
CRITIC_REDUCES = {"min": 0, "mean": 1}                                     # CADM_CRITIC_MIN / _MEAN


class CriticParams(C.Structure):        # include/cadm_hip.h cadm_critic_params (the layer conventions are the value net's)
    _fields_ = [("n_hidden", C.c_int32), ("hidden", C.c_int32 * MAX_VALUE_LAYERS), ("activation", C.c_int32), ("n_critics", C.c_int32),
                ("reduce", C.c_int32), ("weight", C.c_float)]


class TrainHParams(C.Structure):
    _fields_ = [
        ("learning_rate", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float),
        ("back_coeff", C.c_float), ("weight_decay_coeff", C.c_float),
        ("weight_decays", C.c_float * (MAX_HIDDEN_LAYERS + 1)),
        ("context_weight_decays", C.c_float * (MAX_CP_LAYERS + 1)),
    ]


_P = C.c_void_p
_u32, _i = C.c_uint32, C.c_int

# The nest of opt-in plan exports, inner to outer: what cadm_<level>_plan takes in front of the level below (behind ctx).  Every level
# ends with the tail of cadm_icem_plan behind its params: obs, cp_obs, cp_act, init_mean, init_var, carry_io, carry_valid_io, m, n, seed,
# call, workspace, plan_out, best_return_out, stream.
_PLAN_TAIL = [_P, _P, _P, _P, _P, _P, _P, _i, _i, _u32, _u32, _P, _P, _P, _P]
_PLAN_NEST = (
    ("scored", [C.POINTER(ScoreParams), _i, C.POINTER(MppiParams)]),          # score, update, prm
    ("constrained", [C.POINTER(ConstraintParams)]),
    ("knot", [C.POINTER(KnotParams), _P]),                                    # knots, phase
    ("tracking", [C.POINTER(TrackParams), _P, _i, _P]),                       # track, targets, T, offset
    ("actuated", [C.POINTER(ActuatorParams), _P, _P, _i]),                    # act, prev_io, prefix_io, advance
    ("uncertain", [C.POINTER(UncertaintyParams)]),
    ("valued", [C.POINTER(ValueParams)]),
    ("rewarded", [C.POINTER(RewardParams)]),
    ("guided", [C.POINTER(PolicyParams)]),
    ("critic", [C.POINTER(CriticParams)]),
    ("anchored", [C.POINTER(PolicyLogpParams)]),
)
_PLAN_ARGS, _args = {}, _PLAN_TAIL      # level -> argtypes of cadm_<level>_plan: ctx, every level's own arguments from it inwards, the tail
for _level, _front in _PLAN_NEST:
    _args = _front + _args
    _PLAN_ARGS[_level] = [_P] + _args

# name -> (restype, argtypes); must list every symbol include/cadm_hip.h declares
SIGNATURES = {
    "cadm_last_error": (C.c_char_p, []),
    "cadm_abi_version": (_i, []),
    "cadm_build_id": (C.c_char_p, []),
    "cadm_ctx_create": (_i, [C.POINTER(Config), C.POINTER(_P)]),
    "cadm_ctx_destroy": (_i, [_P]),
    "cadm_set_env_spec": (_i, [_P, C.POINTER(EnvSpecC)]),
    "cadm_set_weights": (_i, [_P, _i, _i, _P, _P]),
    "cadm_set_logvar_bounds": (_i, [_P, _i, _P, _P]),
    "cadm_repack": (_i, [_P, _P]),
    "cadm_set_norm_stats": (_i, [_P, C.POINTER(_P), _P]),
    "cadm_context_forward": (_i, [_P, _P, _P, _i, _i, _P, _P]),
    "cadm_sample_actions": (_i, [_P, _P, _P, _P, _u32, _u32, _i, _i, _i, _P, _P]),
    "cadm_sample_actions_shard": (_i, [_P, _P, _P, _P, _u32, _u32, _i, _i, _i, _i, _i, _P, _P]),
    "cadm_sample_uniform": (_i, [_P, _u32, _u32, _i, _i, _P, _P, _P]),
    "cadm_rollout_returns": (_i, [_P, _P, _P, _P, _P, _P, _i, _u32, _u32, _i, _i, _i, _i, _i, _P, _P, _P]),
    "cadm_rollout_builtin": (_i, [_P]),
    "cadm_register_rollout": (_i, [_P, _i, _P, C.POINTER(_i)]),
    "cadm_rollout_check": (_i, [_P, _i, _i, _i]),
    "cadm_particle_mean": (_i, [_P, _P, _i, _i, _P, _P]),
    "cadm_cem_refit": (_i, [_P, _P, _i, _i, _P, _i, _P, _P, _P, _P]),
    "cadm_cem_refit_regen": (_i, [_P, _P, _i, _i, _i, _P, _P, _u32, _u32, _i, _P, _P]),
    "cadm_rs_select": (_i, [_P, _P, _i, _i, _P, _i, _P, _P, _P]),
    "cadm_plan_workspace_bytes": (C.c_size_t, [_P, _i, _i]),
    "cadm_cem_plan": (_i, [_P, _P, _P, _P, _P, _P, _i, _i, _u32, _u32, _P, _P, _P]),
    "cadm_cem_plan_staged": (_i, [_P, _P, _P, C.POINTER(C.c_int32), _i, _i, _i, _u32, _u32, _P, _P, _i, _P]),
    "cadm_sample_actions_colored": (_i, [_P, _P, _P, _P, C.c_float, _u32, _u32, _i, _i, _i, _P, _P]),
    "cadm_icem_keep": (_i, [_P, _P, _P, _i, _i, _i, _P, _P]),
    "cadm_icem_inject": (_i, [_P, _P, _P, _i, _i, _i, _i, _P, _P]),
    "cadm_icem_track_best": (_i, [_P, _P, _P, _P, _i, _i, _P, _P, _P]),
    "cadm_icem_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i]),
    "cadm_icem_plan": (_i, [_P, C.POINTER(IcemParams), _P, _P, _P, _P, _P, _P, _P, _i, _i, _u32, _u32, _P, _P, _P, _P]),
    "cadm_mppi_refit": (_i, [_P, _P, _P, _i, _i, C.c_float, _i, _P, _P, _P, _P]),
    "cadm_mppi_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i]),
    "cadm_mppi_plan": (_i, [_P, C.POINTER(MppiParams), _P, _P, _P, _P, _P, _P, _P, _i, _i, _u32, _u32, _P, _P, _P, _P]),
    "cadm_particle_score": (_i, [_P, _P, _i, _i, C.POINTER(ScoreParams), _P, _P]),
    "cadm_scored_plan": (_i, _PLAN_ARGS["scored"]),
    "cadm_constrain_returns": (_i, [_P, C.POINTER(ConstraintParams), _P, _P, _P, _P, _i, _i, _P, _P, _P, _P]),
    "cadm_constrained_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i, _i]),
    "cadm_constrained_plan": (_i, _PLAN_ARGS["constrained"]),
    "cadm_shape_actions": (_i, [_P, C.POINTER(KnotParams), _P, _i, _i, _P, _P]),
    "cadm_knot_plan": (_i, _PLAN_ARGS["knot"]),
    "cadm_tracking_returns": (_i, [_P, C.POINTER(TrackParams), _P, _P, _i, _P, _P, _P, _i, _i, _P, _P, _P]),
    "cadm_tracking_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i, _i, _i]),
    "cadm_tracking_plan": (_i, _PLAN_ARGS["tracking"]),
    "cadm_actuate_actions": (_i, [_P, C.POINTER(ActuatorParams), _P, _P, _i, _i, _P, _P, _P]),
    "cadm_actuated_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i, _i, _i, _i]),
    "cadm_actuated_plan": (_i, _PLAN_ARGS["actuated"]),
    "cadm_uncertainty_cost": (_i, [_P, C.POINTER(UncertaintyParams), _P, _P, _i, _i, _P, _P, _P]),
    "cadm_uncertain_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i, _i, _i, _i]),
    "cadm_uncertain_plan": (_i, _PLAN_ARGS["uncertain"]),
    "cadm_set_value_net": (_i, [_P, C.POINTER(ValueParams), C.POINTER(_P), C.POINTER(_P), _P, _P, _P]),
    "cadm_value_eval": (_i, [_P, _P, _i, _P, _P]),
    "cadm_value_returns": (_i, [_P, C.POINTER(ValueParams), _P, _P, _i, _i, _P, _P, _P, _P]),
    "cadm_valued_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i, _i, _i, _i, _i]),
    "cadm_valued_plan": (_i, _PLAN_ARGS["valued"]),
    "cadm_set_reward_net": (_i, [_P, C.POINTER(RewardParams), C.POINTER(_P), C.POINTER(_P), _P, _P, _P]),
    "cadm_reward_eval": (_i, [_P, _P, _i, _P, _P]),
    "cadm_reward_workspace_bytes": (C.c_size_t, [_P, _i, _i]),
    "cadm_reward_returns": (_i, [_P, C.POINTER(RewardParams), _P, _P, _P, _P, _i, _i, _P, _P, _P, _P, _P, _P]),
    "cadm_rewarded_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i, _i, _i, _i, _i]),
    "cadm_rewarded_plan": (_i, _PLAN_ARGS["rewarded"]),
    "cadm_set_policy_net": (_i, [_P, C.POINTER(PolicyParams), C.POINTER(_P), C.POINTER(_P), _P, _P, _P]),
    "cadm_policy_eval": (_i, [_P, _P, _i, _P, _P]),
    "cadm_policy_workspace_bytes": (C.c_size_t, [_P, _i, _i]),
    "cadm_policy_propose": (_i, [_P, C.POINTER(PolicyParams), _P, _P, _i, _u32, _u32, _P, _P, _P, _P]),
    "cadm_guided_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i, _i, _i, _i, _i, _i]),
    "cadm_guided_plan": (_i, _PLAN_ARGS["guided"]),
    "cadm_set_critic_nets": (_i, [_P, C.POINTER(CriticParams), C.POINTER(_P), C.POINTER(_P), _P, _P, _P]),
    "cadm_critic_eval": (_i, [_P, _P, _P, _i, _P, _P, _P, _P]),
    "cadm_critic_returns": (_i, [_P, C.POINTER(CriticParams), _P, _P, _i, _i, _P, _P, _P, _P]),
    "cadm_critic_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i, _i, _i, _i, _i, _i]),
    "cadm_critic_plan": (_i, _PLAN_ARGS["critic"]),
    "cadm_set_discount": (_i, [_P, C.c_float, _P]),
    "cadm_discount_weights": (_i, [_P, C.POINTER(C.c_float), C.POINTER(_i)]),
    "cadm_discount_returns": (_i, [_P, _P, _P, _P, _i, _i, _P, _P, _P, _P]),
    "cadm_imagine_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i, C.POINTER(C.c_uint64)]),
    "cadm_imagine": (_i, [_P, _P, _P, _P, _i, _i, _i, C.c_float, C.POINTER(ConstraintParams), C.POINTER(UncertaintyParams), _u32, _u32, _P, _P]),
    "cadm_imagine_select": (_i, [_P, _P, _P, _P, _P, _i, _i, C.POINTER(ConstraintParams), C.POINTER(UncertaintyParams), _u32, _u32, _P, _P, _P,
                                 _P, _P, _P, _P, _P, _P, _P]),
    "cadm_set_policy_head": (_i, [_P, C.POINTER(PolicyHeadParams), _P, _P, _P]),
    "cadm_policy_sample": (_i, [_P, _P, _i, _u32, _i, _u32, _u32, _P, _P, _P, _P]),
    "cadm_imagine_sampled_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i, C.POINTER(C.c_uint64)]),
    "cadm_imagine_sampled": (_i, [_P, _P, _P, _i, _i, _i, C.POINTER(ConstraintParams), C.POINTER(UncertaintyParams), _u32, _u32, _P, _P]),
    "cadm_set_policy_proposals": (_i, [_P, C.c_int32, C.c_float]),
    "cadm_policy_logp": (_i, [_P, _P, _P, _i, _i, _P, _P]),
    "cadm_policy_logp_workspace_bytes": (C.c_size_t, [_P, _i, _i]),
    "cadm_policy_logp_returns": (_i, [_P, C.POINTER(PolicyLogpParams), _P, _P, _P, _P, _i, _i, _P, _P, _P, _P, _P, _P]),
    "cadm_anchored_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i, _i, _i, _i, _i, _i]),
    "cadm_anchored_plan": (_i, _PLAN_ARGS["anchored"]),
    "cadm_imagine_targets_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i, _i, C.POINTER(C.c_uint64)]),
    "cadm_imagine_targets": (_i, [_P, _P, _P, _P, _P, _P, _i, _i, _i, C.POINTER(TargetParams), _P, _P]),
    "cadm_rs_plan": (_i, [_P, _P, _P, _P, _i, _i, _u32, _u32, _P, _P, _P, _P]),
    "cadm_train_configure": (_i, [_P, C.POINTER(TrainHParams), _i]),
    "cadm_train_step": (_i, [_P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _P, _P]),
    "cadm_train_step_rows": (_i, [_P, _P, _P, _P, _P, _P, _P, _P, _i, _P, _P, _P, C.c_longlong, _i, _i, _P, _P]),
    "cadm_train_reset": (_i, [_P, _P]),
    "cadm_predict": (_i, [_P, _P, _P, _P, _P, _i, _P, _P, _P]),
    "cadm_profile_enable": (_i, [_P, _i]),
    "cadm_profile_read": (_i, [_P, C.POINTER(C.c_float), C.POINTER(_i)]),
    "cadm_profile_read_collective": (_i, [_P, C.POINTER(C.c_float), C.POINTER(_i)]),
    "cadm_warm_start_shift": (_i, [_P, _P, _i, _P, _P, _P]),
    "cadm_history_update": (_i, [_P, _P, _P, _P, _P, _i, _i, _P, _P, _P, _P, _P]),
    "cadm_build_windows": (_i, [_P, _P, _P, _P, _i, _i, _i, _i, _i, _P, _P, _P, _i, _i, _P, _P, _P, _P, _P, _P, _P]),
    "cadm_horizon_error": (_i, [_P, _P, C.c_longlong, _P, _i, _i, _i, _i, _i, C.c_longlong, _P, C.c_longlong, _P, _P, _P, _P, _P, _i, _P]),
    "cadm_eval_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i]),
    "cadm_eval_horizon": (_i, [_P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _u32, _u32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "cadm_calibration_stats": (_i, [_P, _P, C.c_longlong, _P, _i, _i, _i, _i, _i, C.c_longlong, _P, C.c_longlong, C.POINTER(CalibrationOut), _i, _P]),
    "cadm_eval_calibration_workspace_bytes": (C.c_size_t, [_P, _i, _i, _i]),
    "cadm_eval_calibration": (_i, [_P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _u32, _u32, _P, _P, C.POINTER(CalibrationOut), _P]),
    "cadm_forecast_stats": (_i, [_P, _P, _P, _P, _i, _i, _i, _i, _i, _i, C.POINTER(ForecastOut), _P]),
    "cadm_forecast_workspace_bytes": (C.c_size_t, [_P, _i, _i]),
    "cadm_plan_forecast": (_i, [_P, _P, _P, _P, _P, _P, _i, _i, _i, _u32, _u32, _P, C.POINTER(ForecastOut), _P]),
    "cadm_dist_unique_id": (_i, [C.c_char_p]),
    "cadm_dist_init": (_i, [_P, C.c_char_p, _i, _i]),
    "cadm_dist_destroy": (_i, [_P]),
    "cadm_dist_info": (_i, [_P, C.POINTER(_i), C.POINTER(_i)]),
    "cadm_dist_init_external": (_i, [_P, _i, _i, C.c_void_p, _P]),
    "cadm_dist_mismatch": (_i, [_P, C.POINTER(_i), _P]),
}
# int fn(void* user, const void* send, void* recv, size_t count, void* stream)  (include/cadm_hip.h: cadm_allgather_fn)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

# developer entry points (csrc/dev/dev_api.h): only in libcadm_hip_dev.so, typed by load_dev()
DEV_SIGNATURES = {
    "cadm_dev_set_rollout": (_i, [_P, _i, _i]),
    "cadm_dev_set_timing_buffer": (_i, [_P, _P]),
    "cadm_dev_read_adam_moment": (_i, [_P, _i, _i, _i, _i, _P, C.c_long, _P]),
    "cadm_dev_rollout_plan": (_i, [_i, _i, _i, C.POINTER(_i)]),
    "cadm_dev_rollout_plan_for": (_i, [_i, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(C.c_float)]),
    "cadm_dev_set_train_flavour": (_i, [_P, _i]),
    "cadm_dev_refit_sharded": (_i, [_P, _P, _i, _i, _i, _i, _P, _P, _u32, _u32, _i, _P, _P]),
    "cadm_dev_input_checksum": (_i, [_P, _P, _P, _P, _P, _P, _i, _P, _P]),
}
DEV_ROLLOUT_XDL, DEV_ROLLOUT_F32 = 0, 1

_lib = None
_dev_libs = {}


def build(verbose=False):
    """Compile libcadm_hip.so (+ the developer library) for gfx950 with hipcc (cross-compiles without a GPU).  Returns
    {"up_to_date_before": bool, "compiled": [objects hipcc produced in this call], "build_id": str} and prints one line saying
    so: an incremental `make` on a tree that already holds current objects compiles nothing, and the caller should be able
    to tell that from a build that exercised the compiler."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    before = subprocess.run(["make", "-C", CSRC, "-q", "HIPCC=" + hipcc], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    jobs = int(os.environ.get("MAX_JOBS") or min(os.cpu_count() or 4, 16))     # os.cpu_count() is the host's, not this job's share
    r = subprocess.run(["make", "-C", CSRC, "-j", str(jobs), "HIPCC=" + hipcc],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout)
    if r.returncode != 0:
        raise CadmError("building libcadm_hip.so failed (see output above)")
    compiled = [ln.split(" -o ")[-1].strip() for ln in r.stdout.splitlines() if " -c " in ln and " -o " in ln]
    linked = [ln.split(" -o ")[-1].strip() for ln in r.stdout.splitlines() if " -shared " in ln]
    try:
        bid = open(os.path.join(CSRC, "build_id.h")).read().split('"')[1]
    except Exception:
        bid = "?"
    print("cadm_amd build: %s; hipcc compiled %d object(s), linked %d librar(ies); build id %s"
          % ("tree was up to date" if before else "tree was stale", len(compiled), len(linked), bid))
    return {"up_to_date_before": before, "compiled": compiled, "linked": linked, "build_id": bid}


def load():
    """dlopen the library and type every entry point.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CadmError(
            "libcadm_hip.so is not built (%s missing). Run `python -c \"import __graft_entry__ as g; "
            "g.build()\"` or `make -C cadm_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm bundles its own libamdhip64: it has to be in the process BEFORE this library's dependency on
    # libamdhip64.so is resolved, or two HIP runtimes coexist and the second one sees no device
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    _lib = _open(LIB_PATH, SIGNATURES)
    return _lib


def _open(path, signatures):
    lib = C.CDLL(path)
    for name, (res, args) in signatures.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.cadm_abi_version() != ABI_VERSION:
        raise CadmError("%s ABI %d != binding ABI %d" % (os.path.basename(path), lib.cadm_abi_version(), ABI_VERSION))
    return lib


def load_dev(path=None):
    """The DEVELOPER library (tests and tools/ only; no product module calls this): the product's objects plus the
    fp32-MFMA comparison kernel and the hooks of csrc/dev/dev_api.h.  A separate dlopen handle -- an engine is bound
    to it explicitly with HipEngine(..., lib=load_dev()); the product library and its engines are unaffected."""
    path = os.path.abspath(path or DEV_LIB_PATH)
    if path not in _dev_libs:
        if not os.path.exists(path):
            raise CadmError("%s is not built (make -C cadm_amd/csrc dev)" % path)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        sigs = dict(SIGNATURES)
        sigs.update(DEV_SIGNATURES)
        _dev_libs[path] = _open(path, sigs)
    return _dev_libs[path]


def check(rc, what="", lib=None):
    if rc != 0:
        msg = (lib or load()).cadm_last_error()
        raise CadmError("%s failed (code %d): %s" % (what or "libcadm_hip call", rc,
                                                     msg.decode() if msg else "?"))


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())
