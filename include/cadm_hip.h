/*
 * cadm_hip.h -- C ABI of libcadm_hip.so: the MI355X (gfx950) implementation of
 * CaDM's CEM-planning / ensemble-training hot path.
 *
 * The reference (younggyoseo/CaDM) has NO FFI layer: its seam is the Python class
 * MLPEnsembleCEMDynamicsModel (cadm/dynamics/mlp_cadm_ensemble_cem_dynamics.py:12)
 * whose methods call sess.run on one TensorFlow graph (cadm/utils/tensor_utils.py:6-11).
 * Every entry point below replaces one piece of that graph; the reference lines it
 * replaces are cited per function (paths relative to /root/reference).  The Python
 * mirror of the class lives in cadm_amd/dynamics/ and binds these with ctypes
 * (see INTEGRATION.md).
 *
 * Conventions
 *   - every pointer argument is a DEVICE pointer to row-major float32 unless noted;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously;
 *   - every function returns 0 on success or a negative CADM_E* code and never throws;
 *     cadm_last_error() returns a thread-local message for the last failure;
 *   - no global state beyond the opaque cadm_ctx;
 *   - a cadm_ctx is bound to the HIP device that was current at cadm_ctx_create.
 */
#ifndef CADM_HIP_H
#define CADM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CADM_ABI_VERSION 2

#define CADM_OK 0
#define CADM_EINVAL (-1)      /* bad argument / unsupported configuration */
#define CADM_ENOMEM (-2)      /* device allocation failed */
#define CADM_EHIP (-3)        /* HIP runtime error (see cadm_last_error) */
#define CADM_ESTATE (-4)      /* weights / stats not set */
#define CADM_ENOTBUILT (-5)   /* no rollout kernel for this geometry in this build (cadm_amd.jit builds one: cadm_register_rollout) */

/* hidden nonlinearity (the reference's `_activations` table, dynamics.py:17-24; ctor default relu :30, the scripts pass swish) */
#define CADM_ACT_SWISH 0
#define CADM_ACT_RELU 1
#define CADM_ACT_TANH 2
#define CADM_ACT_SIGMOID 3
#define CADM_ACT_NONE 4

/* env kinds: the closures obs_preproc / obs_postproc / tf_reward_fn that the reference
 * compiles into its graph (cadm/envs/<env>.py) are compiled into the kernels */
#define CADM_ENV_HALFCHEETAH 0   /* half_cheetah_env.py:46-59,82-88; cripple: half_cheetah_cripple_env.py:60-73,90-96 */
#define CADM_ENV_ANT 1           /* ant_env.py:52-62,89-98 */
#define CADM_ENV_SLIM_HUMANOID 2 /* slim_humanoid_env.py:39-46,95-111 */
#define CADM_ENV_CARTPOLE 3      /* classic_control.py:94-101,154-166 */
#define CADM_ENV_PENDULUM 4      /* classic_control.py:209-218,284-291 */
#define CADM_ENV_SPEC 5          /* a user-declared env (cadm_env_spec below): rollouts come from a module built for the spec (cadm_amd/jit.py) */

#define CADM_NET_FF 0    /* variable scope 'ff_model'        (dynamics.py:159) */
#define CADM_NET_BACK 1  /* variable scope 'backward_model'  (dynamics.py:213) */
#define CADM_NET_CTX 2   /* variable scope 'context_model'   (dynamics.py:140) */

#define CADM_MAX_HIDDEN_LAYERS 8
#define CADM_MAX_CP_LAYERS 8

typedef struct cadm_ctx cadm_ctx;

/* Mirrors the ctor kwargs of MLPEnsembleCEMDynamicsModel (dynamics.py:26-54) that shape the graph. */
typedef struct cadm_config {
    int32_t abi_version;       /* CADM_ABI_VERSION */
    int32_t env_kind;          /* CADM_ENV_* */
    int32_t ensemble_size;     /* E */
    int32_t n_particles;       /* p, p % E == 0 (core/utils.py:447) */
    int32_t obs_dim;           /* D  (must match the env kind) */
    int32_t act_dim;           /* A */
    int32_t proc_obs_dim;      /* P */
    int32_t context_dim;       /* C = context_out_dim, 0 for the vanilla PE-TS model */
    int32_t n_hidden;          /* number of hidden layers (4; 1 .. CADM_MAX_HIDDEN_LAYERS) */
    int32_t hidden;            /* hidden width, all layers equal (200) */
    int32_t horizon;           /* n_forwards H */
    int32_t deterministic;     /* dynamics.py:43 */
    int32_t discrete;          /* discrete action space (cartpole) */
    int32_t reference_quirks;  /* 1: reproduce context-layout quirks Q1/Q2 (core/utils.py:434-435) */
    int32_t history_length;    /* Hh */
    int32_t n_cp_hidden;       /* context encoder hidden layers (3) */
    int32_t cp_hidden[CADM_MAX_CP_LAYERS]; /* (256,128,64) */
    int32_t num_elites;        /* 50  (core/utils.py:391) */
    int32_t num_cem_iters;     /* 5   (core/utils.py:392) */
    float alpha;               /* 0.1 (core/utils.py:393) */
    float lower_bound;         /* -1  (core/utils.py:395) */
    float upper_bound;         /* +1  (core/utils.py:396) */
    int32_t back_model;        /* 1: backward model present (back_coeff > 0, dynamics.py:212) */
    int32_t hidden_act;        /* CADM_ACT_*: hidden_nonlinearity of both dynamics nets (dynamics.py:104; 0 = swish) */
    int32_t reserved[6];       /* CADM_ENV_SPEC: [0], [1] = low / high word of the spec's 64-bit hash (cadm_env_spec.hash); else 0 */
} cadm_config;

/* A user-declared env (env_kind CADM_ENV_SPEC, cadm_amd/env_spec.py): the closures obs_preproc / obs_postproc / targ_proc / reward
 * as tables.  Continuous actions only.  Envelope (checked by cadm_ctx_create before any HIP call):
 * 1 <= D <= CADM_SPEC_MAX_D, 1 <= A <= CADM_SPEC_MAX_A, 1 <= P <= CADM_SPEC_MAX_P, discrete == 0.
 *   preproc[d]   CADM_SPEC_PRE_*: the features of obs dim d, in dim order (sincos: sin then cos); P = their count
 *   postproc[d]  CADM_SPEC_POST_*: next[d] = obs[d] + delta[d] (add) or delta[d] (replace); targ_proc follows
 *   terms        reward = sum over terms of w * f(x), x = obs[dim] (when OBS: the pre-step state) or next_obs[dim] (NEXT_OBS);
 *                f = x, x^2, |x|, [lo < x < hi] or [x > hi] + [x < lo]; then - ctrl_cost * sum(a^2) + bonus */
#define CADM_SPEC_MAX_D 48
#define CADM_SPEC_MAX_A 24
#define CADM_SPEC_MAX_P 64
#define CADM_SPEC_MAX_TERMS 32
#define CADM_SPEC_PRE_ID 0
#define CADM_SPEC_PRE_DROP 1
#define CADM_SPEC_PRE_SINCOS 2
#define CADM_SPEC_POST_ADD 0
#define CADM_SPEC_POST_REPLACE 1
#define CADM_SPEC_TERM_LINEAR 0
#define CADM_SPEC_TERM_SQUARE 1
#define CADM_SPEC_TERM_ABS 2
#define CADM_SPEC_TERM_INSIDE 3
#define CADM_SPEC_TERM_OUTSIDE 4
#define CADM_SPEC_WHEN_OBS 0
#define CADM_SPEC_WHEN_NEXT_OBS 1
typedef struct cadm_env_spec {
    int32_t obs_dim, act_dim, proc_obs_dim;
    int32_t preproc[CADM_SPEC_MAX_D];
    int32_t postproc[CADM_SPEC_MAX_D];
    int32_t n_terms;
    int32_t term_kind[CADM_SPEC_MAX_TERMS];
    int32_t term_dim[CADM_SPEC_MAX_TERMS];
    int32_t term_when[CADM_SPEC_MAX_TERMS];
    float term_w[CADM_SPEC_MAX_TERMS];
    float term_lo[CADM_SPEC_MAX_TERMS];
    float term_hi[CADM_SPEC_MAX_TERMS];
    float ctrl_cost, bonus;
    uint32_t hash_lo, hash_hi;   /* hash of the spec's canonical serialisation: must equal the ctx config's reserved[0..1] */
} cadm_env_spec;

const char* cadm_last_error(void);
int cadm_abi_version(void);
/* 16 hex digits: sha256 over the kernel sources (csrc/ *.hip, *.h, include/cadm_hip.h) this binary was compiled from.  Profiling
 * artefacts (profiles/ *pmc*.json) record it, and bench.py only quotes counters whose build id equals the loaded library's. */
const char* cadm_build_id(void);

/* Build / free the per-model device state (replaces graph construction, dynamics.py:107-342). */
int cadm_ctx_create(const cadm_config* cfg, cadm_ctx** out);
int cadm_ctx_destroy(cadm_ctx* ctx);
/* CADM_ENV_SPEC only, right after cadm_ctx_create: validate the spec's tables against the ctx (dims, feature count P, hash),
 * keep them and upload the per-feature (source dim, op) table the training / prediction input assembly reads.  Training and
 * prediction on a spec ctx fail with CADM_ESTATE until it is set.  Synchronous. */
int cadm_set_env_spec(cadm_ctx* ctx, const cadm_env_spec* spec);

/* Register one dense layer's master weights (raw TF layout W [E,in,out], b [E,1,out];
 * create_dense_layer, core/utils.py:635-641).  The pointers stay owned by the caller and must
 * outlive the ctx; the planner's MFMA-fragment weight streams are (re)packed from them.
 * layer index: CADM_NET_FF/BACK: 0..n_hidden-1 hidden, n_hidden = output_mu, n_hidden+1 = output_logvar;
 *              CADM_NET_CTX:     0..n_cp_hidden-1 hidden, n_cp_hidden = cp_output. */
int cadm_set_weights(cadm_ctx* ctx, int net, int layer, float* W, float* b);
/* max_logvar / min_logvar [1,D] (core/utils.py:338-339). */
int cadm_set_logvar_bounds(cadm_ctx* ctx, int net, float* max_logvar, float* min_logvar);
/* The caller has written master weights in place (load(), a manual assign; ANY net): re-pack the planner's weight streams
 * now and mark the training chains' packed operand copies stale (rebuilt at the next cadm_train_step / cadm_predict;
 * training steps themselves keep them current).  Writing registered weights without this call leaves both on old values.
 * Fails with CADM_EINVAL if a dynamics weight cannot be split for the f16 matrix pipe: non-finite, or |w| > 65000 AS PACKED -- swish
 * nets carry log2(e) in layer 0 (limit 45052 in the model's units) and 1 / log2(e) in the heads (93780); biases: any finite value.
 * The planner's other range limits (inputs clamped at +-65000, hidden pre-activations at 60000 = 41589 for swish nets in the model's
 * units) are listed in INTEGRATION.md, "Numeric envelope of the planner". */
int cadm_repack(cadm_ctx* ctx, void* stream);

/* The 12 normalisation vectors fed per call in the reference (dynamics.py:344-347,604-645), order:
 * obs_mean[P] obs_std[P] act_mean[A] act_std[A] delta_mean[D] delta_std[D] cp_obs_mean[D*Hh]
 * cp_obs_std[D*Hh] cp_act_mean[A*Hh] cp_act_std[A*Hh] back_delta_mean[D] back_delta_std[D].
 * HOST pointers (float32); copied. */
int cadm_set_norm_stats(cadm_ctx* ctx, const float* const host_stats[12], void* stream);

/* Context encoder inference (core/utils.py:401-406,614-617): cp_obs [m,D*Hh], cp_act [m,A*Hh]
 * -> ctx_out [E,m,C].  With bs != 0 the inputs are already [E,m,.] (get_context_pred,
 * dynamics.py:369-380 / training graph :619-622). */
int cadm_context_forward(cadm_ctx* ctx, const float* cp_obs, const float* cp_act, int m, int bs,
                         float* ctx_out, void* stream);

/* Candidate action sequences (core/utils.py:425-429):
 * actions[m,n_global,H,A] = mean + sqrt(min(min(((mean-lb)/2)^2,((ub-mean)/2)^2),var)) * z.
 * z = injected truncated-normal draws [m,n_global,H,A], or NULL to draw them on device from
 * Philox4x32-10 keyed (seed, call) with counters (element, attempt, STREAM_ACT | it<<8). */
int cadm_sample_actions(cadm_ctx* ctx, const float* mean, const float* var, const float* z,
                        uint32_t seed, uint32_t call, int it, int m, int n_global,
                        float* actions_out, void* stream);
/* The same for candidates [cand_offset, cand_offset + n_local) only, written at their GLOBAL positions of actions_out
 * [m,n_global,H,A]: the draws are keyed by the global element index, so a rank of a candidate-sharded planner that draws only its own
 * shard writes exactly what any other rank would have written there (the other positions are left untouched). */
int cadm_sample_actions_shard(cadm_ctx* ctx, const float* mean, const float* var, const float* z,
                              uint32_t seed, uint32_t call, int it, int m, int n_global, int cand_offset, int n_local,
                              float* actions_out, void* stream);
/* Random-shooting draws (core/utils.py:498-503): U[-1,1) actions (continuous) or one-hot rows of
 * uniform integer actions (discrete; raw ints also written to raw_out [m,n,H] if non-NULL). */
int cadm_sample_uniform(cadm_ctx* ctx, uint32_t seed, uint32_t call, int m, int n_global,
                        float* actions_out, int32_t* raw_out, void* stream);

/* THE hot kernel: trajectory-sampling rollout of candidates [cand_offset, cand_offset+n_local)
 * through the ensemble over the whole horizon (core/utils.py:431-472, one CEM iteration's inner
 * loop; vanilla :138-170).  One launch = H steps x (m*n_local*p) rows.
 *   obs          [m,D]            start state (tiled over n,p as :432)
 *   obs_rows     [m,n_local,p,D]  optional per-row start state (teacher forcing), else NULL
 *   ctx_vec      [E,m,C]          context encoder output (NULL when C == 0)
 *   actions      [m,n_global,H,A] candidate actions; normalised in-kernel (:443) unless
 *                                 norm_actions == 0 (discrete RS feeds one-hot rows, :500)
 *   eps          [H,m,n_local,p,D] injected N(0,1) for the Gaussian head (:365), or NULL to draw
 *                                 from Philox keyed (seed, call), counters (global row, t, d/2,
 *                                 STREAM_EPS | it<<8) -- independent of the candidate sharding
 *   it           CEM iteration (selects the context layout of quirk Q2, :434)
 *   returns_rows [m,n_local,p]    out: per-row returns before the particle mean (:471)
 *   traj_out     [H,m,n_local,p,D] optional out: next observation after every step, else NULL
 * The state after the LAST step is computed only when something reads it: with traj_out, or for an env whose reward reads the next
 * observation (cartpole; a CADM_ENV_SPEC env with a CADM_SPEC_WHEN_NEXT_OBS term).  Otherwise the launch evaluates the model H - 1
 * times per row (not at all at H = 1) and never reads eps[H-1]; returns_rows are bit-identical either way. */
int cadm_rollout_returns(cadm_ctx* ctx, const float* obs, const float* obs_rows, const float* ctx_vec,
                         const float* actions, const float* eps, int norm_actions,
                         uint32_t seed, uint32_t call, int it,
                         int cand_offset, int n_global, int m, int n_local,
                         float* returns_rows, float* traj_out, void* stream);

/* Rollout kernels are compile-time specialised per (env kind, hidden width, number of hidden layers, context width,
 * nonlinearity).  The library carries the reference's defaults (4 x {128,200,256,512} swish, context 0 / 10); for anything else
 * (`--hidden_size`, `--context_out_dim`, run_cadm_pets.py:122-135) the caller builds cadm_amd/csrc/rollout_jit.hip with hipcc
 * (cadm_amd/jit.py does) and registers the module's entry point for a noise mode (0 device Philox, 1 injected eps, 2 deterministic).
 *   cadm_rollout_builtin   1 if the ctx's geometry is compiled in, else 0
 *   cadm_register_rollout  fn = the module's `cadm_jit_rollout`; describe = its `cadm_jit_describe` output (checked against the ctx;
 *                          CADM_ENV_SPEC: describe[8], describe[9] = the spec hash the module was built for, refused unless it is the ctx's)
 *   cadm_rollout_check     validates that a rollout of m x n_local candidates can be launched (kernel present, LDS fits the
 *                          horizon) WITHOUT launching -- construction-time instead of first-get_action failure */
int cadm_rollout_builtin(cadm_ctx* ctx);
int cadm_register_rollout(cadm_ctx* ctx, int noise_mode, void* fn, const int describe[10]);
int cadm_rollout_check(cadm_ctx* ctx, int noise_mode, int m, int n_local);

/* Mean over particles (core/utils.py:474): returns_rows [m,n_local,p] -> cand_returns [m,n_local]. */
int cadm_particle_mean(cadm_ctx* ctx, const float* returns_rows, int m, int n_local,
                       float* cand_returns, void* stream);

/* Elite refit (core/utils.py:475-486): top-k (sorted, ties -> lower index), gather, mean /
 * biased variance over elites, EMA with alpha.
 *   cand_returns  [G,m,n_local]  the all-gathered per-candidate returns of G ranks (G = 1: [m,n]);
 *                                global candidate ni lives at [ni / n_local][mi][ni % n_local]
 *   actions       [m,G*n_local,H,A]
 *   mean_io/var_io [m,H,A]       updated in place
 *   elites_out    [m,num_elites] optional int32 out (global candidate ids), else NULL */
int cadm_cem_refit(cadm_ctx* ctx, const float* cand_returns, int G, int n_local, const float* actions,
                   int m, float* mean_io, float* var_io, int32_t* elites_out, void* stream);

/* cadm_cem_refit without the candidates' action sequences: the <= num_elites elites' sequences are DRAWN AGAIN from the device RNG by
 * global candidate id -- (seed, call, it) and mean_io / var_io (before the update) are the distribution iteration `it` was sampled
 * from -- so a rank that sampled only its own shard (cadm_sample_actions_shard) refits over the global set without any exchange of
 * actions.  Bit-identical to cadm_cem_refit on the fully sampled buffer. */
int cadm_cem_refit_regen(cadm_ctx* ctx, const float* cand_returns, int G, int n_local, int m, float* mean_io, float* var_io,
                         uint32_t seed, uint32_t call, int it, int32_t* elites_out, void* stream);

/* Random-shooting selection (core/utils.py:554-561): argmax over candidates (first maximum),
 * out[m,A] = actions[mi, best, 0, :].  best_out [m] optional. */
int cadm_rs_select(cadm_ctx* ctx, const float* cand_returns, int G, int n_local, const float* actions,
                   int m, float* first_action_out, int32_t* best_out, void* stream);

/* Whole single-GPU CEM planner = one `sess.run(optimal_action_var)` (dynamics.py:349-356,
 * core/utils.py:398-488): context encoder once, then num_cem_iters x (sample, rollout, refit);
 * the result [m,H,A] is clipped to [lb,ub] as get_action does (dynamics.py:365-366) unless discrete.
 * workspace: device scratch of cadm_plan_workspace_bytes(ctx, m, n) bytes. */
size_t cadm_plan_workspace_bytes(cadm_ctx* ctx, int m, int n);
int cadm_cem_plan(cadm_ctx* ctx, const float* obs, const float* cp_obs, const float* cp_act,
                  const float* init_mean, const float* init_var, int m, int n,
                  uint32_t seed, uint32_t call, void* workspace, float* plan_out, void* stream);
/* The same planner fed from the HOST, as the class's get_action is (numpy in -> numpy out, dynamics.py:344-367): `host_block`
 * is a pinned host buffer of `nfloats` floats holding obs / cp_obs / cp_act / init_mean / init_var at float offsets off[0..4]
 * (-1 = absent); it is copied to `dev_block` (device, >= nfloats floats) with one async copy on `stream`, the planner runs, and
 * the last refit kernel writes the plan into `plan_out_host` (pinned, device-visible host memory: [m,H,A] floats followed by m
 * 32-bit completion flags).  sync != 0: returns when plan_out_host is readable (the flags are polled; no sleep in the runtime). */
int cadm_cem_plan_staged(cadm_ctx* ctx, const float* host_block, float* dev_block, const int32_t off[5], int nfloats,
                         int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out_host, int sync,
                         void* stream);
/* Random-shooting planner (core/utils.py:490-561): out [m,A] (continuous) or raw_best_out [m] ints. */
int cadm_rs_plan(cadm_ctx* ctx, const float* obs, const float* cp_obs, const float* cp_act,
                 int m, int n, uint32_t seed, uint32_t call, void* workspace,
                 float* action_out, int32_t* raw_best_out, void* stream);

/* iCEM planner (Pinneri et al. 2020; no reference twin, OPT-IN beside cadm_cem_plan, which is untouched): temporally correlated
 * candidate noise, elites carried over between CEM iterations and -- moved one step on -- between consecutive calls, optionally the
 * best sequence seen as the plan, and a decaying candidate count.  Single rank, continuous actions.
 *
 * cadm_sample_actions_colored: one noise sequence z_0 .. z_{H-1} per (env mi, candidate c, action dim a) from spectral draws
 * x_k, y_k ~ N(0,1):
 *   z_t = c_b [ x_0 / sqrt2 + sum_{1 <= k < H/2} k^(-b/2) (x_k cos th_kt - y_k sin th_kt) + [H even] (H/2)^(-b/2) x_{H/2} (-1)^t / sqrt2 ],
 *   th_kt = 2 pi ((k t) mod H) / H,   c_b = (1/2 + sum_{1 <= k < H/2} k^(-b) + [H even] (H/2)^(-b) / 2)^(-1/2)
 * (Var z_t = 1 for every t, b; b = 0: an orthonormal transform of iid normals, white; b > 0: low frequencies weigh more), and
 *   actions[mi,c,t,a] = clip(mean + sd z_t, lb, ub),  sd = sqrt(min(min(((mean-lb)/2)^2, ((ub-mean)/2)^2), var))  as cadm_sample_actions;
 * no rejection step.  The spectral draws are injected -- xi [m,n,A,H]: slot 0 = x_0, then (x_k, y_k) in k order, x_{H/2} last when H
 * is even: H numbers per sequence -- or, xi NULL, drawn from Philox4x32-10 keyed (seed, call) with counters (global sequence index
 * (mi n + c) A + a, k, STREAM_ICEM | it<<8) and Box-Muller on the first two words (x_k = r cos, y_k = r sin).  0 <= beta <= 16;
 * the horizon must fit the kernel's LDS (H <= 246). */
typedef struct cadm_icem_params {
    float noise_beta;       /* 0: the truncated-normal sampler of cadm_sample_actions, unchanged; > 0: coloured noise */
    int32_t keep_elites;    /* K, 0 <= K <= num_elites */
    float decay;            /* >= 1: iteration it uses min(n, max(floor(n / decay^it), 2 num_elites, K + 1)) candidates */
    int32_t return_best;    /* 1: the plan is the best sequence of this call; 0: the refitted mean, clipped */
    int32_t add_mean_last;  /* 1: candidate slot K of the last iteration is the current mean, clipped */
} cadm_icem_params;
int cadm_sample_actions_colored(cadm_ctx* ctx, const float* mean, const float* var, const float* xi, float beta,
                                uint32_t seed, uint32_t call, int it, int m, int n, float* actions_out, void* stream);
/* gather: kept_out[mi,j] = actions[mi, elites[mi,j]] for j < K; actions [m,n,H,A], elites [m,num_elites] as cadm_cem_refit's
 * elites_out (return descending, ties to the lower index), kept_out [m,K,H,A] */
int cadm_icem_keep(cadm_ctx* ctx, const float* actions, const int32_t* elites, int m, int n, int K, float* kept_out, void* stream);
/* scatter: candidate slots [0,K) of actions_io [m,n,H,A] take kept [m,K,H,A]; shift = 1 (across calls): steps [0,H-1) take kept
 * steps [1,H) and step H-1 keeps its value; valid [m] int32 (or NULL = all): envs with valid[mi] == 0 are left untouched */
int cadm_icem_inject(cadm_ctx* ctx, const float* kept, const int32_t* valid, int m, int n, int K, int shift, float* actions_io,
                     void* stream);
/* per env: the iteration's best candidate is the one with the greatest NON-NaN return (+inf and -inf count), ties (-0.0 against
 * +0.0 included) to the lower index: the first of elites[mi, 0 .. num_elites) whose return is not NaN (cadm_cem_refit's elites_out
 * ranks a NaN return above +inf, so NaN returns come first), or, when all of them are NaN, the arg-max over cand_returns[mi, :].
 * An elite id outside [0, n) ends the walk and leaves the env as it is.  Where best_ret_io[mi] is NaN (nothing stored yet) or that
 * return is STRICTLY greater than it (a tie is not), the return and the candidate's sequence replace best_ret_io [m] /
 * best_seq_io [m,H,A].  Over a cadm_icem_plan call: the plan under return_best is the sequence with the greatest non-NaN return
 * scored in the call, ties to the earliest iteration, then the lowest index; it (and best_return_out) is NaN only if every return
 * of the call is NaN. */
int cadm_icem_track_best(cadm_ctx* ctx, const float* cand_returns, const int32_t* elites, const float* actions, int m, int n,
                         float* best_ret_io, float* best_seq_io, void* stream);
/* The loop: context encoder once, then per iteration `it` with n_it candidates: sample (white or coloured), write the kept sequences
 * into slots [0,K) -- iteration 0: carry_io [m,K,H,A] of envs with carry_valid_io[mi] != 0, moved one step on; later: the K best of
 * the previous iteration -- and (last iteration, add_mean_last) the clipped mean into slot K; rollout; particle mean; refit; track the
 * best; gather the K best (after the last refit into carry_io, setting carry_valid_io[mi] = 1).  plan_out [m,H,A]; best_return_out
 * [m] optional: the best candidate return of the call.  carry_io / carry_valid_io are caller-owned and may be NULL when K == 0.
 * CADM_EINVAL (before any HIP call) for a sharded ctx, discrete actions, K > num_elites, decay < 1, n < num_elites.
 * workspace: cadm_icem_workspace_bytes(ctx, m, n, K) bytes (0 for bad arguments).  Everything is enqueued on `stream`. */
size_t cadm_icem_workspace_bytes(cadm_ctx* ctx, int m, int n, int K);
int cadm_icem_plan(cadm_ctx* ctx, const cadm_icem_params* params, const float* obs, const float* cp_obs, const float* cp_act,
                   const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m, int n,
                   uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream);

/* MPPI update (Williams et al. 2017; no reference twin, OPT-IN): a softmax-weighted refit over ALL candidates in place of the top-k
 * elite refit.  Per env, with F = the candidates whose return is finite (NaN, +inf and -inf get weight 0):
 *   R* = max_F R,   lambda_eff = temperature (relative == 0)   or   temperature (R* - min_F R) (relative != 0);
 *   w_c = exp((R_c - R*) / lambda_eff)   (relative and lambda_eff == 0, all finite returns equal: w_c = 1),   W = sum_c w_c >= 1,
 *   mu = sum_c w_c a_c / W,   v = sum_c w_c (a_c - mu)^2 / W   (the mean first, then the variance around it),
 *   mean <- alpha mean + (1 - alpha) mu,   var <- alpha var + (1 - alpha) v   (the ctx's alpha, the blend of cadm_cem_refit),
 *   plan_out [m,H,A] (optional; device or pinned host memory) = clip(new mean, lower_bound, upper_bound).
 * An env without any finite return keeps mean_io / var_io bit for bit, and its plan is clip(mean).  The action sequences must be
 * finite.  Sums are taken in a fixed order (csrc/mppi.hip, "Reduction contract"): the same bits run to run, and per env whatever m.
 *   cand_returns [m,n], actions [m,n,H,A], mean_io / var_io [m,H,A] updated in place
 * CADM_EINVAL (before any HIP call) for a temperature that is not finite and > 0, discrete actions, a sharded ctx. */
int cadm_mppi_refit(cadm_ctx* ctx, const float* cand_returns, const float* actions, int m, int n, float temperature, int relative,
                    float* mean_io, float* var_io, float* plan_out, void* stream);
/* The loop of cadm_icem_plan with this update in place of the elite refit; everything else composes unchanged: white or coloured
 * sampling, kept elites across iterations and calls, the candidate-count decay, add_mean_last, return_best, best_return_out.  The
 * elites that are kept and tracked are still the top num_elites by return (descending, ties to the lower index).  Refusals: those of
 * cadm_icem_plan, and the temperature check.  workspace: cadm_mppi_workspace_bytes(ctx, m, n, K) bytes (0 for bad arguments). */
typedef struct cadm_mppi_params {
    cadm_icem_params icem;
    float temperature;      /* lambda > 0 */
    int32_t relative;       /* != 0: lambda is a fraction of the env's return range R* - min_F R */
} cadm_mppi_params;
size_t cadm_mppi_workspace_bytes(cadm_ctx* ctx, int m, int n, int K);
int cadm_mppi_plan(cadm_ctx* ctx, const cadm_mppi_params* params, const float* obs, const float* cp_obs, const float* cp_act,
                   const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m, int n,
                   uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream);

/* Risk-aware candidate scores (no reference twin, OPT-IN): what a candidate's p particle returns become before the update of the
 * opt-in loop ranks or weighs it.  The rollout writes every particle's return (returns_rows [m,n_local,p]) -- a probabilistic ensemble
 * with trajectory sampling computes them to expose model uncertainty -- and the plain mean averages that uncertainty away.  Per
 * candidate, with mu = the mean exactly as cadm_particle_mean computes it (one fp32 chain over j = 0 .. p-1, then / p):
 *   CADM_SCORE_MEAN        mu: cadm_particle_mean itself is enqueued (the same kernel, grid and bits)
 *   CADM_SCORE_MEAN_STD    mu - kappa sigma,    sigma   = sqrt(sum_j (r_j - mu)^2 / p)        (mu first, then the deviations from it)
 *   CADM_SCORE_MEMBER_STD  mu - kappa sigma_E,  sigma_E = sqrt(sum_e (mu_e - mu)^2 / E),  mu_e = the mean of member e's q = p / E
 *                          particles (particle j belongs to member j / q, as in the rollout): what the MEMBERS disagree about
 *   CADM_SCORE_CVAR        the mean of the k lowest returns, 1 <= k <= p: particle j counts iff rank_j < k,
 *                          rank_j = #{i : r_i < r_j or (r_i == r_j and i < j)}; the counted r_j are added in particle order, then / k
 * kappa: any finite float (> 0 pessimistic, < 0 optimistic, 0: mu's bits).  k = p: the mean up to rounding; k = 1: the minimum.
 * Every sum is one chain in index order: the same bits run to run, whatever m, n_local and the candidate's position.
 * A candidate with a NaN or +-inf particle return scores, in every mode, exactly what cadm_particle_mean gives it: a diverged row
 * meets the elite ranking, cadm_icem_track_best and MPPI's zero weight as it does under the mean.
 * cadm_particle_score is rank-local (it works on a sharded ctx, like cadm_particle_mean) and needs no workspace.
 * CADM_EINVAL (before any HIP call) for an unknown mode, a kappa that is not finite (the std modes), k outside [1, p] (CVAR).
 * score NULL = CADM_SCORE_MEAN. */
#define CADM_SCORE_MEAN 0
#define CADM_SCORE_MEAN_STD 1
#define CADM_SCORE_MEMBER_STD 2
#define CADM_SCORE_CVAR 3
typedef struct cadm_score_params {
    int32_t mode;           /* CADM_SCORE_* */
    float kappa;            /* MEAN_STD, MEMBER_STD: the weight of the standard deviation */
    int32_t k;              /* CVAR: the number of lowest particle returns averaged */
} cadm_score_params;
int cadm_particle_score(cadm_ctx* ctx, const float* returns_rows, int m, int n_local, const cadm_score_params* score,
                        float* cand_returns, void* stream);
/* The loop of cadm_icem_plan (update == 0: the elite refit; only params->icem is read) or of cadm_mppi_plan (update == 1) with this
 * score in place of the particle mean; everything else composes unchanged.  The elites, the tracked best plan and best_return_out
 * are by SCORE (best_return_out is the best score, not the best mean).  score NULL or CADM_SCORE_MEAN: exactly the launches of
 * cadm_icem_plan / cadm_mppi_plan.  Refusals: those of the loop with that update, the score's, and an update that is not 0 or 1.
 * workspace: cadm_icem_workspace_bytes (update 0) / cadm_mppi_workspace_bytes (update 1); scoring needs none of its own. */
int cadm_scored_plan(cadm_ctx* ctx, const cadm_score_params* score, int update, const cadm_mppi_params* params, const float* obs,
                     const float* cp_obs, const float* cp_act, const float* init_mean, const float* init_var, float* carry_io,
                     int32_t* carry_valid_io, int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out,
                     float* best_return_out, void* stream);

/* State constraints and early termination (no reference twin, OPT-IN): tell the opt-in loop "do not go there".  A constraint reads ONE
 * observation dim: a state is healthy iff x[dim[k]] > lo[k] && x[dim[k]] < hi[k] for every k < n, compared in float32 (a missing side
 * is -inf / +inf).  A value equal to a bound violates; NaN or +-inf in a constrained dim violates; a non-finite value in any other dim
 * is not looked at.  Checked is the POST-step state of every step t = 0 .. H-1 of a recorded trajectory (traj [H,m,n,p,D], the layout
 * of cadm_rollout_returns' traj_out, H and p the ctx's); the observation a call starts from is never checked.  Per particle row:
 *   violations [m,n,p]       int32: the number of steps whose post-step state violates
 *   first_violation [m,n,p]  int32: the first such step, H if there is none
 *   CADM_CONSTRAIN_PENALTY    rows_out = rows_in - weight * (float)violations     (one fp32 multiply and one subtract)
 *   CADM_CONSTRAIN_TERMINATE  rows_out = (r_0 + ... + r_tau) - weight, tau = first_violation < H: r_t the particle's step reward as
 *                             cadm_forecast_stats evaluates it (pre-step state: obs at t = 0, else traj[t-1]; post-step state
 *                             traj[t]; the raw action), added in step order from r_0.  The step that leaves the region still pays;
 *                             whatever traj holds after tau, a blow-up included, does not reach the return.
 * A row without a violation keeps rows_in's bits in both modes: a constraint that never binds changes no plan.
 * cadm_constrain_returns: rows_in / rows_out [m,n,p] (rows_out may alias rows_in); first_violation_out / violations_out may each be
 * NULL; obs [m,D] and actions [m,n,H,A] (raw) are read in TERMINATE mode only and may be NULL in PENALTY mode.  traj is read at most
 * once; a row's counters and partial sum are one thread's chain in step order (csrc/constrain.hip), no floating-point atomics: the
 * same bits run to run, whatever m, n and the row's position.  Needs no workspace.
 * Refusals, before any HIP call: CADM_EINVAL for n outside 1 .. CADM_MAX_CONSTRAINTS, a dim outside 0 .. D-1, lo >= hi, a NaN bound,
 * both sides infinite, an unknown mode, a weight that is negative or not finite, a discrete ctx (cartpole), a sharded ctx, a D whose
 * LDS tiles (2 x 64 x D floats) exceed 48 KiB; CADM_ESTATE for a CADM_ENV_SPEC ctx before cadm_set_env_spec in TERMINATE mode. */
#define CADM_MAX_CONSTRAINTS 16
#define CADM_CONSTRAIN_PENALTY 0
#define CADM_CONSTRAIN_TERMINATE 1
typedef struct cadm_constraint_params {
    int32_t n;              /* 1 .. CADM_MAX_CONSTRAINTS */
    int32_t mode;           /* CADM_CONSTRAIN_* */
    float weight;           /* finite, >= 0 */
    int32_t dim[CADM_MAX_CONSTRAINTS];
    float lo[CADM_MAX_CONSTRAINTS];
    float hi[CADM_MAX_CONSTRAINTS];
} cadm_constraint_params;
int cadm_constrain_returns(cadm_ctx* ctx, const cadm_constraint_params* params, const float* traj, const float* obs,
                           const float* actions, const float* rows_in, int m, int n, float* rows_out, int32_t* first_violation_out,
                           int32_t* violations_out, void* stream);
/* The loop of cadm_scored_plan under constraints: every iteration's rollout records its trajectories into a view of the workspace,
 * and cadm_constrain_returns rewrites the particle returns in place before cadm_particle_score sees them; everything else composes
 * unchanged (the elites, the best plan and best_return_out are by the constrained score).  constraints NULL: exactly the launches of
 * cadm_scored_plan.  Refusals: those of cadm_scored_plan and of cadm_constrain_returns.
 * workspace: cadm_constrained_workspace_bytes(ctx, m, n, K, mppi) bytes -- cadm_icem_workspace_bytes (mppi == 0) or
 * cadm_mppi_workspace_bytes (mppi != 0) plus one view of H m n p D floats at the end (0 for bad arguments). */
size_t cadm_constrained_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi);
int cadm_constrained_plan(cadm_ctx* ctx, const cadm_constraint_params* constraints, const cadm_score_params* score, int update,
                          const cadm_mppi_params* params, const float* obs, const float* cp_obs, const float* cp_act,
                          const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m, int n,
                          uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream);

/* Plans on knots (no reference twin, OPT-IN): the opt-in loop searches over fewer decisions than the horizon has steps -- action repeat
 * (HOLD) or linear interpolation (LINEAR) between knot steps `spacing` = r >= 1 apart.  Per env a phase phi, taken modulo r with a
 * non-negative result (a negative or >= r phase is legal), moves the grid; H is the ctx's horizon.
 *   step t belongs to segment j = (t + phi) div r;  the segment's knot step is k_j = max(0, j r - phi);  the next knot is
 *   k_{j+1} = (j+1) r - phi.  The knot steps are k_0 = 0 < k_1 < ..., J = (H - 1 + phi) div r + 1 of them, all inside [0, H).
 *   H = 7, r = 3: phi = 0 -> {0, 3, 6}; phi = 1 -> {0, 2, 5}; phi = 2 -> {0, 1, 4}.   H = 5, r = 8, phi = 5 -> {0, 3}.
 * Shaping a sequence a[0 .. H), per action dim:
 *   a knot step keeps its bits;
 *   any other step t under CADM_KNOT_HOLD takes a[k_j] (a copy: the same bits);
 *   any other step t under CADM_KNOT_LINEAR with k_{j+1} <= H - 1 takes fmaf(w, a[k_{j+1}] - a[k_j], a[k_j]),
 *       w = (float)(t - k_j) / (float)(k_{j+1} - k_j) in fp32 (one rounded difference, one rounded quotient, one fused multiply-add);
 *   any other step t under CADM_KNOT_LINEAR in a last segment without a next knot inside the horizon holds a[k_j].
 * Shaping is idempotent; shaped values of a sequence inside [lb, ub] stay inside [lb, ub]; r = 1 is the identity (nothing is enqueued);
 * a HOLD-shaped sequence moved one step on (cadm_icem_inject, shift = 1) lies on the grid of phase phi + 1 -- carried elites and a
 * phase that advances by one per call fit together.  Reads come from knot steps only, writes go to the other steps only.
 * cadm_shape_actions: seqs_io [m,n,H,A] shaped IN PLACE, n the packed candidate count of the buffer (n = 1: means [m,1,H,A]); phase [m]
 * int32 on the device, or NULL = 0 for every env.  One thread per element, no atomics, no workspace.
 * CADM_EINVAL (before any HIP call) for spacing < 1, an unknown interp.  spacing >= H is legal: one knot (a constant plan), or two with
 * a non-zero phase. */
#define CADM_KNOT_HOLD 0
#define CADM_KNOT_LINEAR 1
typedef struct cadm_knot_params {
    int32_t spacing;        /* r >= 1: knot steps are r apart; 1: every step is a knot */
    int32_t interp;         /* CADM_KNOT_* */
} cadm_knot_params;
int cadm_shape_actions(cadm_ctx* ctx, const cadm_knot_params* knots, const int32_t* phase, int m, int n, float* seqs_io, void* stream);
/* The loop of cadm_constrained_plan on a grid of knots.  Before iteration 0, init_mean is copied into the workspace and shaped (n = 1):
 * that copy is iteration 0's mean; the caller's init_mean is not written, init_var is used as it is.  In every iteration, behind the
 * sampler, the kept-elite injection and the add_mean_last injection and before the rollout, the iteration's n_it candidates are shaped
 * in place: the rollout, the constraints, the score, either refit, the tracked best, the kept elites and the carry written after the
 * last refit see sequences on the grid, and their per-step statistics at the knot steps are those of a CEM run in knot space.  The draws
 * are those of the loop without knots.  knots NULL or spacing == 1: exactly the launches of cadm_constrained_plan.  Refusals: those of
 * cadm_constrained_plan and of cadm_shape_actions.  workspace: that of the loop underneath -- cadm_constrained_workspace_bytes with
 * constraints, else cadm_icem_workspace_bytes (update 0) / cadm_mppi_workspace_bytes (update 1). */
int cadm_knot_plan(cadm_ctx* ctx, const cadm_knot_params* knots, const int32_t* phase, const cadm_constraint_params* constraints,
                   const cadm_score_params* score, int update, const cadm_mppi_params* params, const float* obs, const float* cp_obs,
                   const float* cp_act, const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m,
                   int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream);

/* Tracking targets at run time (no reference twin, OPT-IN): tell the opt-in loop "go there" -- a cost on the predicted states that the
 * caller sets per env and per step when it calls, with no new env spec and no rebuild.  A term k < n reads ONE observation dim of the
 * POST-step state of every step t = 0 .. H-1 of a recorded trajectory (traj [H,m,n,p,D], the layout of cadm_rollout_returns' traj_out, H
 * and p the ctx's); the observation a call starts from is never read.  targets [m,T,K] float32 on the device, K = n terms, T >= 1 rows
 * per env; offset [m] int32 on the device, or NULL = 0.  Step t of env mi is compared with
 *   g = targets[mi, clamp(offset[mi] + t, 0, T-1), k]
 * -- T = 1 is a constant goal, a reference shorter than the horizon holds its last row, a negative offset holds the first.  A NaN g
 * means "no target for this term at this step": the (step, term) is skipped (a terminal cost, sparse waypoints).  Per particle row, one
 * chain over t = 0 .. H-1 in step order, k ascending inside a step, every operation rounded to float32 (nothing is fused):
 *   e = x[dim[k]] - g;   c = e*e (CADM_TRACK_SQUARE), |e| (CADM_TRACK_ABS), or |e| <= delta[k] ? 0.5 e*e : delta[k] (|e| - 0.5 delta[k])
 *   (CADM_TRACK_HUBER);   cost += w[k] * c;   rows_out = rows_in - cost
 * A row whose every (step, term) was skipped keeps rows_in's bits: targets that are all NaN change no plan.  A non-finite value in a
 * tracked dim at a counted step makes the row's return non-finite (it then meets the score, the elite ranking and MPPI's zero weight as
 * a diverged rollout's row does); other dims are not looked at.  Not done: wrapping an angle's e, targets on actions.  On a ctx with a discount
 * over the horizon (cadm_set_discount): cost += disc[t] * (w_k * c).
 * cadm_tracking_returns: rows_in / rows_out [m,n,p] (rows_out may alias rows_in).  first [m,n,p] int32, or NULL: cadm_constrain_returns'
 * first_violation_out -- steps t > first[row] are not counted: the step that leaves the region still pays, as it does for the reward in
 * TERMINATE mode, and nothing traj holds after it reaches the return.  cost_out [m,n,p], or NULL: the cost alone (0 for a row with
 * nothing counted).  traj is read at most once; a row's cost is one thread's chain (csrc/tracking.hip), no floating-point atomics: the
 * same bits run to run, whatever m, n and the row's position.  Needs no workspace.
 * Refusals, before any HIP call: CADM_EINVAL for n outside 1 .. CADM_MAX_TRACK_TERMS, a dim outside 0 .. D-1, an unknown kind, a w that
 * is negative or not finite, a Huber delta that is not finite or <= 0, T < 1, NULL targets, a discrete ctx (cartpole), a sharded ctx, a
 * D whose LDS tile (64 x D floats, plus 4.5 KiB of targets, offsets and terms) exceeds 48 KiB. */
#define CADM_MAX_TRACK_TERMS 16
#define CADM_TRACK_SQUARE 0
#define CADM_TRACK_ABS 1
#define CADM_TRACK_HUBER 2
typedef struct cadm_track_params {
    int32_t n;              /* 1 .. CADM_MAX_TRACK_TERMS */
    int32_t dim[CADM_MAX_TRACK_TERMS];
    int32_t kind[CADM_MAX_TRACK_TERMS];     /* CADM_TRACK_* */
    float w[CADM_MAX_TRACK_TERMS];          /* finite, >= 0 */
    float delta[CADM_MAX_TRACK_TERMS];      /* CADM_TRACK_HUBER only: finite, > 0 */
} cadm_track_params;
int cadm_tracking_returns(cadm_ctx* ctx, const cadm_track_params* track, const float* traj, const float* targets, int T,
                          const int32_t* offset, const int32_t* first, const float* rows_in, int m, int n, float* rows_out,
                          float* cost_out, void* stream);
/* The loop of cadm_knot_plan under tracking targets.  With track set, every iteration's rollout records its trajectories into the
 * workspace whether or not there are constraints, and the order is rollout -> cadm_constrain_returns (if any) -> cadm_tracking_returns
 * -> cadm_particle_score, the particle returns rewritten in place.  Under TERMINATE constraints the constraint kernel also writes its
 * first_violation into an [m,n,p] int32 view of the workspace and the tracking kernel reads it as `first`; under PENALTY constraints or
 * none, first is NULL.  The elites, the tracked best plan, best_return_out, the kept elites and the carry are by the tracked score.
 * targets [m,T,K] / offset [m] (or NULL) are read, never written: advancing the offsets between calls is the caller's.
 * track NULL: exactly the launches of cadm_knot_plan (targets, T and offset are not looked at).  Refusals: those of cadm_knot_plan and
 * of cadm_tracking_returns.
 * workspace: cadm_tracking_workspace_bytes(ctx, m, n, K, mppi, terminate) bytes with track set -- cadm_constrained_workspace_bytes(ctx,
 * m, n, K, mppi) plus, for terminate != 0 (TERMINATE constraints), the first_violation view (0 for bad arguments); with track NULL that
 * of cadm_knot_plan. */
size_t cadm_tracking_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate);
int cadm_tracking_plan(cadm_ctx* ctx, const cadm_track_params* track, const float* targets, int T, const int32_t* offset,
                       const cadm_knot_params* knots, const int32_t* phase, const cadm_constraint_params* constraints,
                       const cadm_score_params* score, int update, const cadm_mppi_params* params, const float* obs, const float* cp_obs,
                       const float* cp_act, const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m,
                       int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream);

/* Actuator model (no reference twin, OPT-IN): what the device that executes a plan can do with it -- an action delay (a committed
 * prefix), per-dim rate limits, and a per-dim cost on the change of the action.  It acts on action sequences [m,n,H,A] (H, A and the box
 * [lb, ub] the ctx's), never on trajectories.
 * Parameters: delay d, 0 <= d < H;  per action dim a a rate limit delta_a > 0 (+inf: none) and a rate-cost weight w_a, finite, >= 0.
 * Device state, per env mi (float32, NaN = absent, as in cadm_tracking_returns' targets):
 *   prev[mi, a]       the action applied immediately before the plan's step 0; NaN: unknown.            [m,A], or NULL: all NaN
 *   prefix[mi, j, a]  j < d: the action already committed for the plan's step j; NaN: that step is free.  [m,d,A], or NULL: all NaN
 * Any per-env pattern can be pinned by writing values and NaNs into prefix (a latch for the rest of a knot segment, say).
 * Actuate, IN PLACE, an independent chain per (env, candidate, action dim), steps ascending, every operation rounded to float32:
 *   last = prev[mi,a]
 *   for t in 0 .. H-1:
 *       x = u[t]
 *       if t < d and prefix[mi,t,a] is not NaN:     y = prefix[mi,t,a]                      (a fact: neither limited nor clipped)
 *       elif delta_a is finite and last is not NaN:  y = clip(clip(x, last - delta_a, last + delta_a), lb, ub)
 *       else:                                        y = x
 *       if last is not NaN:                          c_a += w_a * (y - last)^2              (pinned steps count too)
 *       u[t] = y;  last = y
 *   cost[mi,c] = ((c_0 + c_1) + c_2) + ...   (ascending a)
 * clip(x, lo, hi) = min(max(x, lo), hi) by comparisons: v = x < lo ? lo : x;  v > hi ? hi : v -- a NaN x stays NaN.  last - delta_a and
 * last + delta_a are one rounding each; the difference, the square, the product and each add of the cost are one rounding each (nothing
 * is fused): the new sequences are reproducible bit for bit in numpy float32.  With last inside the box both bounds hold; with last
 * outside it (a prev the caller reports from outside) the box wins.  Actuate is idempotent bit for bit.  With d = 0, every delta = +inf
 * and every w = 0 it copies its input and the cost is 0.  A chain is one thread's and a candidate's dims are added by one thread
 * (csrc/actuator.hip), no floating-point atomics: nothing depends on the grid, on m or n, or on the row's position.
 * cadm_actuate_actions: seqs_io [m,n,H,A], n the packed candidate count of the buffer; cost_out [m,n], or NULL.  No workspace.
 * n_dims: the number of action dims the arrays were filled for, or 0 when every entry holds the same broadcast value.
 * Refusals, before any HIP call: CADM_EINVAL for a delay outside [0, H), a limit that is <= 0 or NaN, a cost that is negative or not
 * finite, n_dims that is neither 0 nor A, A > CADM_MAX_ACT_DIMS, a discrete ctx (cartpole), a candidate-sharded ctx. */
#define CADM_MAX_ACT_DIMS 32
typedef struct cadm_actuator_params {
    int32_t delay;                          /* d: 0 .. H-1 */
    int32_t n_dims;                         /* 0, or the ctx's A */
    float rate_limit[CADM_MAX_ACT_DIMS];    /* > 0; +inf: none */
    float rate_w[CADM_MAX_ACT_DIMS];        /* finite, >= 0 */
} cadm_actuator_params;
int cadm_actuate_actions(cadm_ctx* ctx, const cadm_actuator_params* params, const float* prev, const float* prefix, int m, int n,
                         float* seqs_io, float* cost_out, void* stream);
/* The loop of cadm_tracking_plan under an actuator model.  Per iteration: sampler -> kept-elite injection -> add_mean_last injection ->
 * knot shaping -> ACTUATE (the iteration's n_it candidates in place, their cost into the workspace) -> rollout -> constraints ->
 * tracking -> score -> cand[mi,c] = cand[mi,c] - cost[mi,c] -> the refit (elite or MPPI), track-best, keep.  Everything behind actuate
 * sees feasible sequences: the rollout, the elites, the tracked best, the kept elites and the carry.  The cost is deterministic per
 * candidate, so it comes off the candidate score and not off the particle rows: a risk score of the returns is unaffected by it; a
 * non-finite score stays non-finite.  A mean of feasible sequences (the elite mean, the MPPI weighted mean) is feasible only up to
 * rounding, so the plan is written to the workspace, takes one more actuate pass with n = 1 there, and is then written to plan_out
 * (which may be pinned host memory): the returned plan obeys pins and limits exactly as defined above.  For return_best that pass is a
 * bitwise no-op.  advance != 0: behind the plan, on the same stream, prev_io <- plan[:,0] and prefix_io[:,j] <- plan[:,1+j] for j < d.
 * prev_io [m,A] is required, prefix_io [m,d,A] with d > 0.
 * params NULL: exactly the launches of cadm_tracking_plan (prev_io, prefix_io and advance are not looked at).  Refusals: those of
 * cadm_tracking_plan and of cadm_actuate_actions.
 * workspace: cadm_actuated_workspace_bytes(ctx, m, n, K, mppi, traj, terminate) with params set -- traj != 0: with constraints or
 * tracking terms (the trajectory view); terminate != 0: tracking terms under TERMINATE constraints -- that is the loop underneath's plus
 * the cost [m,n] and the plan copy [m,H,A] (0 for bad arguments); with params NULL that of cadm_tracking_plan. */
size_t cadm_actuated_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int traj, int terminate);
int cadm_actuated_plan(cadm_ctx* ctx, const cadm_actuator_params* params, float* prev_io, float* prefix_io, int advance,
                       const cadm_track_params* track, const float* targets, int T, const int32_t* offset, const cadm_knot_params* knots,
                       const int32_t* phase, const cadm_constraint_params* constraints, const cadm_score_params* score, int update,
                       const cadm_mppi_params* mppi_params, const float* obs, const float* cp_obs, const float* cp_act,
                       const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m, int n,
                       uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream);

/* Pricing model uncertainty (no reference twin, OPT-IN): a cost, or with a negative weight a bonus, on the ensemble's disagreement about
 * the STATES a candidate's plan visits, per step -- cadm_forecast_stats' var_epistemic / var_total as a term of the candidate score.
 * (cadm_score_params' MEMBER_STD is not this: it measures disagreement about the summed reward, is blind to every observation dim the
 * reward does not read, and sees nothing of a disagreement that cancels over the horizon.)
 * For a candidate (env mi, candidate c), a step t and an observation dim d with weight w_d > 0, over x_j = traj[t,mi,c,j,d] (traj
 * [H,m,n,p,D]: a rollout's traj_out; particle j belongs to member j / q, q = p / E; H, p, E, D the ctx's), the variance is formed by
 * the chain of cadm_forecast_stats, every operation rounded to float32 and nothing fused:
 *   x0  = x_0
 *   s_e = sum_{j<q} (x_{e q + j} - x0)        j ascending, from 0.0f        (e = 0 .. E-1)
 *   tot = sum_e s_e                           e ascending, from 0.0f
 *   md  = tot / (float)p
 *   CADM_UNC_TOTAL:      var = sum_j ((x_j - x0) - md)^2   j ascending;   v = var / (float)p
 *   CADM_UNC_EPISTEMIC:  de = s_e / (float)q - md;  epi = sum_e de*de   e ascending;   v = epi / (float)E
 * so a one-hot w reproduces cadm_forecast_stats' var_total / var_epistemic bit for bit.  The step cost is
 *   u_t = sum_d w_d * v[t,d]   over the dims with w_d > 0, ascending d, from the first such term (one product and one add per dim);
 *   form CADM_UNC_STD: u_t = sqrtf(u_t);     then  u_t = u_t > cap ? cap : u_t   (a comparison, not fminf: NaN stays NaN; +inf: no cap)
 * and the candidate's cost is  cost[mi,c] = sum_t u_t  over the COUNTED steps, in step order, from 0.0f: every step 0 .. H-1, or with
 * first [m,n,p] (cadm_constrain_returns' first_violation, TERMINATE mode) the steps t <= min_j first[mi,c,j] -- the step at which the
 * first particle leaves still counts, as it does for the reward and for tracking; behind it the particles are a mix of dead and live
 * ones, and whatever traj holds there never reaches the cost.  Dims with w_d == 0 are never read.  A non-finite value in a weighted dim
 * at a counted step makes u_t and the cost non-finite by the arithmetic above; an overflowed, infinite u_t is a value like any other.
 * A planner with weight < 0 (a bonus) should set a cap: an unbounded bonus rewards a diverging rollout.
 * Every v, every u_t and every cost is one thread's chain (csrc/uncertainty.hip), no floating-point atomics: nothing depends on the
 * grid, on m or n, or on the candidate's position; the same bits run to run and inside any batch.
 * cadm_uncertainty_cost: n the packed candidate count of traj; step_out [m,n,H] (u_t of EVERY step, counted or not) or NULL -- the same
 * cost_out bits either way; cost_out [m,n].  No workspace.  Rank-local arithmetic, but refused on a candidate-sharded ctx, like
 * cadm_tracking_returns.  `weight` (lambda) is not applied here: it is what cadm_uncertain_plan multiplies the cost by.
 * Refusals, before any HIP call: CADM_EINVAL for an unknown kind or form, a weight that is not finite, a cap that is NaN or <= 0, a w
 * that is negative, NaN or infinite, all w zero, n_dims that is neither 0 nor D, D > CADM_MAX_UNC_DIMS, a discrete ctx (cartpole), a
 * candidate-sharded ctx, a p * D tile beyond the kernel's LDS budget (p * D + 2 D floats, each count rounded up to 4, above 48 KiB). */
#define CADM_MAX_UNC_DIMS 128
#define CADM_UNC_EPISTEMIC 0
#define CADM_UNC_TOTAL 1
#define CADM_UNC_VAR 0
#define CADM_UNC_STD 1
typedef struct cadm_uncertainty_params {
    int32_t kind, form;              /* CADM_UNC_EPISTEMIC | CADM_UNC_TOTAL;  CADM_UNC_VAR | CADM_UNC_STD */
    float weight;                    /* lambda: finite, any sign (> 0: a penalty, < 0: a bonus) */
    float cap;                       /* > 0; +inf: none */
    int32_t n_dims;                  /* 0: w[0] for every dim; else the ctx's D */
    float w[CADM_MAX_UNC_DIMS];      /* finite, >= 0, at least one > 0 */
} cadm_uncertainty_params;
int cadm_uncertainty_cost(cadm_ctx* ctx, const cadm_uncertainty_params* params, const float* traj, const int32_t* first, int m, int n,
                          float* step_out, float* cost_out, void* stream);
/* The loop of cadm_actuated_plan with that cost in the candidate score.  Every iteration's rollout records its trajectories, as it does
 * for constraints and tracking terms; TERMINATE constraints write their first violations into the workspace with or without tracking
 * terms.  Per iteration: rollout -> constraints -> tracking -> cadm_particle_score -> the actuator's cand -= cost ->
 * cand[mi,c] = cand[mi,c] - weight * cost[mi,c] (one multiply, one subtract; n_it, the iteration's packed candidate count) -> the
 * refit (elite or MPPI) -> track-best -> keep.  The cost is a statistic over the particles, so it comes off the candidate score, not off
 * the particle rows: a risk score of the returns is unaffected by it.  The elites, the tracked best, best_return_out, the kept elites
 * and the carry are by the final score; a candidate whose cost is not finite meets them as a diverged rollout's does.
 * params NULL: exactly the launches of cadm_actuated_plan.  Refusals: those of cadm_actuated_plan and of cadm_uncertainty_cost.
 * workspace: cadm_uncertain_workspace_bytes(ctx, m, n, K, mppi, terminate, actuator) with params set -- terminate != 0: TERMINATE
 * constraints; actuator != 0: an actuator model -- that is the loop underneath's WITH the trajectory view (and under TERMINATE the
 * first-violation view), and behind everything else u [m,n,H] and the cost [m,n] (0 for bad arguments); with params NULL that of
 * cadm_actuated_plan. */
size_t cadm_uncertain_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate, int actuator);
int cadm_uncertain_plan(cadm_ctx* ctx, const cadm_uncertainty_params* params, const cadm_actuator_params* actuator, float* prev_io,
                        float* prefix_io, int advance, const cadm_track_params* track, const float* targets, int T, const int32_t* offset,
                        const cadm_knot_params* knots, const int32_t* phase, const cadm_constraint_params* constraints,
                        const cadm_score_params* score, int update, const cadm_mppi_params* mppi_params, const float* obs,
                        const float* cp_obs, const float* cp_act, const float* init_mean, const float* init_var, float* carry_io,
                        int32_t* carry_valid_io, int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out,
                        float* best_return_out, void* stream);

/* Terminal value (no reference twin, OPT-IN): a caller-supplied value net V on the LAST state of every particle's trajectory, so that a
 * plan is scored by  return + weight * V(s_H)  and sees beyond its H steps (POLO, LOOP, TD-MPC).  `weight` carries a discount gamma^H -- unless the ctx has a discount
 * over the horizon (cadm_set_discount): the library then multiplies disc[H] in, and `weight` no longer carries it.
 * V is an MLP  D -> h_1 -> .. -> h_L -> 1,  L = n_hidden in 0 .. CADM_MAX_VALUE_LAYERS (0: a linear V), every width in
 * 1 .. CADM_MAX_VALUE_WIDTH, one hidden activation for the net, a linear output, D <= CADM_MAX_VALUE_DIMS.  For a state s [D], all in
 * float32 (csrc/value.hip):
 *   x_k = (s_k - mean_k) * std_inv_k                                        one subtract, one multiply
 *   layer with K inputs, unit u:  acc = b[u];  for k = 0 .. K4-1 ascending:  acc = fmaf(W[k][u], x_k, acc)
 *       (K4: K rounded up to 4; W and x are exact zeros for K <= k < K4; the bias seeds the accumulator)
 *   hidden:  CADM_VALUE_RELU max(z, 0) | CADM_VALUE_TANH tanhf(z) | CADM_VALUE_SWISH z / (1 + expf(-z));   output: the sum itself.
 * A state with any non-finite value has V = NaN, set explicitly.  V of a state is one chain in ascending k, no floating-point
 * atomics: the same bits run to run, in any batch, at any row position, for any m or n, from cadm_value_eval as from the planner.
 * cadm_set_value_net: W[l] [in,out] row-major and b[l] [out] (l = 0 .. n_hidden), mean [D] and std_inv [D] are DEVICE pointers; they are
 * copied and packed into memory the ctx owns, on `stream` -- the caller may free its tensors afterwards.  A second call replaces the
 * net; params NULL clears it.  params->weight is not kept: every call below brings its own.
 * cadm_value_eval: v_out[r] = V(states[r]) for states [R,D].
 * cadm_value_returns: for row q of rows [m,n,p] with the terminal state traj[H-1,q,:] (traj [H,m,n,p,D]: a rollout's traj_out, n its
 * packed candidate count):  rows_out[q] = rows_in[q] + weight * V  (one multiply, then one add, no fma; a NaN V gives a NaN return, as a
 * diverged rollout's is).  With first [m,n,p] (cadm_constrain_returns' first_violation, TERMINATE mode) a row with first[q] < H keeps its
 * input bits and its terminal state is not read: an ended episode has no future.  rows_out may alias rows_in.  v_out [m,n,p] or NULL:
 * V of every row, NaN for the rows `first` skipped.  params must describe the registered net (layer count, widths, activation), else
 * CADM_EINVAL; no registered net: CADM_ESTATE.
 * Refusals, before any HIP call: CADM_EINVAL for null pointers, n_hidden outside 0 .. 4, a width outside 1 .. 512, an unknown
 * activation, a weight that is not finite, D > CADM_MAX_VALUE_DIMS, a discrete ctx (cartpole), a candidate-sharded ctx, activation
 * tiles (two regions of 16 rows x the widest layers, each width rounded up to 4) beyond the 160 KiB of LDS. */
#define CADM_MAX_VALUE_LAYERS 4
#define CADM_MAX_VALUE_WIDTH 512
#define CADM_MAX_VALUE_DIMS 128
#define CADM_VALUE_RELU 0
#define CADM_VALUE_TANH 1
#define CADM_VALUE_SWISH 2
typedef struct cadm_value_params {
    int32_t n_hidden;                          /* L: 0 .. CADM_MAX_VALUE_LAYERS */
    int32_t hidden[CADM_MAX_VALUE_LAYERS];     /* h_1 .. h_L, each 1 .. CADM_MAX_VALUE_WIDTH */
    int32_t activation;                        /* CADM_VALUE_RELU | CADM_VALUE_TANH | CADM_VALUE_SWISH */
    float weight;                              /* finite */
} cadm_value_params;
int cadm_set_value_net(cadm_ctx* ctx, const cadm_value_params* params, const float* const* W, const float* const* b, const float* mean,
                       const float* std_inv, void* stream);
int cadm_value_eval(cadm_ctx* ctx, const float* states, int R, float* v_out, void* stream);
int cadm_value_returns(cadm_ctx* ctx, const cadm_value_params* params, const float* traj, const int32_t* first, int m, int n,
                       const float* rows_in, float* rows_out, float* v_out, void* stream);
/* The loop of cadm_uncertain_plan with that term in the particle returns.  Every iteration's rollout records its trajectories;
 * TERMINATE constraints write their first violations into the workspace.  Per iteration: rollout -> constraints -> tracking ->
 * rows[q] += weight * V(traj[H-1,q]) on the particle rows [m,n_it,p] -> cadm_particle_score (a risk-aware score sees return + value per
 * particle) -> the actuator's and the uncertainty term's costs off the candidate score, unchanged -> the refit.  PENALTY constraints do
 * not gate the value.  params NULL: exactly the launches of cadm_uncertain_plan.  Refusals: those of cadm_uncertain_plan and of
 * cadm_value_returns.  workspace: cadm_valued_workspace_bytes(ctx, m, n, K, mppi, terminate, actuator, uncertainty) with params set --
 * the loop underneath's WITH the trajectory view, and under TERMINATE constraints the first-violation view (0 for bad arguments); with
 * params NULL that of cadm_uncertain_plan. */
size_t cadm_valued_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate, int actuator, int uncertainty);
int cadm_valued_plan(cadm_ctx* ctx, const cadm_value_params* params, const cadm_uncertainty_params* uncertainty,
                     const cadm_actuator_params* actuator, float* prev_io, float* prefix_io, int advance, const cadm_track_params* track,
                     const float* targets, int T, const int32_t* offset, const cadm_knot_params* knots, const int32_t* phase,
                     const cadm_constraint_params* constraints, const cadm_score_params* score, int update,
                     const cadm_mppi_params* mppi_params, const float* obs, const float* cp_obs, const float* cp_act,
                     const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m, int n, uint32_t seed,
                     uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream);

/* Learned reward (no reference twin, OPT-IN): a caller-supplied reward net R on EVERY step of every particle's trajectory, so that a
 * plan is scored by  return + weight * sum_t R_t  (+ the terminal value) and a reward that is no sum of one-dim terms -- a product of two
 * dims, a distance in a plane, a contact or success signal, a reward known only from logged (s, a, s', r) -- can be planned against
 * (MBPO, PlaNet, Dreamer, TD-MPC).  The term is ADDED to the env's own return; an env whose reward is entirely learned is declared with
 * no reward terms.
 * R is an MLP  K -> h_1 -> .. -> h_L -> 1  under the value net's conventions: L = n_hidden in 0 .. CADM_MAX_VALUE_LAYERS, every width in
 * 1 .. CADM_MAX_VALUE_WIDTH, one hidden activation CADM_VALUE_RELU | _TANH | _SWISH, a linear output.  Its input for step t of particle
 * row q = (env mi, candidate ni, particle j) is the concatenation that `inputs` selects:
 *   CADM_REWARD_NEXT_OBS          s_{t+1}                 K = D
 *   CADM_REWARD_OBS_ACT           s_t, a_t                K = D + A
 *   CADM_REWARD_OBS_ACT_NEXT_OBS  s_t, a_t, s_{t+1}       K = 2 D + A
 * with  s_0 = obs[mi],  s_t = traj[t-1,q] (t >= 1),  s_{t+1} = traj[t,q],  a_t = actions[mi,ni,t,:] -- the candidate buffer exactly as
 * the rollout reads it (behind the injections, the knot shaping and the actuator pass), raw, not normalised.  K <= CADM_MAX_REWARD_DIMS.
 * For one (t, q), all in float32 (csrc/reward.hip, csrc/mlp_chain.h):
 *   x_k = (in_k - mean_k) * std_inv_k   over the K concatenated dims              one subtract, one multiply
 *   layer with K inputs, unit u:  acc = b[u];  for k = 0 .. K4-1 ascending:  acc = fmaf(W[k][u], x_k, acc)
 *       (K4: K rounded up to 4; W and x are exact zeros for K <= k < K4; the bias seeds the accumulator) -- the chain of the value net
 *   hidden: the activation;   output: the sum itself.
 * The step sum:  S[q] = ((0 + R_0) + R_1) + ..,  plain float32 adds in ascending t over the COUNTED steps: every step without `first`;
 * with first [m,n,p] (cadm_constrain_returns' first_violation, TERMINATE mode) the steps t <= first[q] -- the step that violates still
 * pays, later steps are not counted and their states are not read.   rows_out[q] = rows_in[q] + weight * S[q]:  one multiply, then one
 * add, no fma.  A counted step whose input holds a non-finite value has R = NaN, set explicitly, so S and the row are NaN (a diverged
 * rollout's row already is).
 * Determinism: R(t, q) is one chain in ascending k, the step sum is sequential in t, no floating-point atomics: the same bits run to run,
 * in any batch, at any row position, for any m, n or p, from cadm_reward_eval as from the planner.
 * cadm_set_reward_net: W[l] [in,out] row-major and b[l] [out] (l = 0 .. n_hidden), mean [K] and std_inv [K] are DEVICE pointers; they are
 * copied and packed into memory the ctx owns, on `stream`.  A second call replaces the net (one of the same shape allocates nothing);
 * params NULL clears it.  params->weight is not kept: every call below brings its own.
 * cadm_reward_eval: r_out[r] = R(x[r]) for ALREADY CONCATENATED inputs x [R,K], through the same per-row chain.
 * cadm_reward_returns: traj [H,m,n,p,D] (a rollout's traj_out, n its packed candidate count), obs [m,D], actions [m,n,H,A], first
 * [m,n,p] or NULL.  step_out [H,m,n,p] or NULL: R of every (step, row), NaN for the steps that are not counted; sum_out [m,n,p] or NULL:
 * S.  rows_out may alias rows_in.  workspace: cadm_reward_workspace_bytes(ctx, m, n) bytes (H m n p floats, where the step rewards go
 * when step_out is NULL; may be NULL with step_out).  params must describe the registered net (inputs, layer count, widths, activation),
 * else CADM_EINVAL; no registered net: CADM_ESTATE.
 * Refusals, before any HIP call: CADM_EINVAL for null pointers, n_hidden outside 0 .. 4, a width outside 1 .. 512, an unknown
 * activation, unknown inputs, a weight that is not finite, K > CADM_MAX_REWARD_DIMS, a discrete ctx (cartpole), a candidate-sharded ctx,
 * activation tiles (two regions of 16 rows x the widest layers, each width rounded up to 4) beyond the 160 KiB of LDS. */
#define CADM_MAX_REWARD_DIMS 256
#define CADM_REWARD_NEXT_OBS 0
#define CADM_REWARD_OBS_ACT 1
#define CADM_REWARD_OBS_ACT_NEXT_OBS 2
typedef struct cadm_reward_params {
    int32_t n_hidden;                          /* L: 0 .. CADM_MAX_VALUE_LAYERS */
    int32_t hidden[CADM_MAX_VALUE_LAYERS];     /* h_1 .. h_L, each 1 .. CADM_MAX_VALUE_WIDTH */
    int32_t activation;                        /* CADM_VALUE_RELU | CADM_VALUE_TANH | CADM_VALUE_SWISH */
    int32_t inputs;                            /* CADM_REWARD_NEXT_OBS | CADM_REWARD_OBS_ACT | CADM_REWARD_OBS_ACT_NEXT_OBS */
    float weight;                              /* finite */
} cadm_reward_params;
int cadm_set_reward_net(cadm_ctx* ctx, const cadm_reward_params* params, const float* const* W, const float* const* b, const float* mean,
                        const float* std_inv, void* stream);
int cadm_reward_eval(cadm_ctx* ctx, const float* x, int R, float* r_out, void* stream);
size_t cadm_reward_workspace_bytes(cadm_ctx* ctx, int m, int n);
int cadm_reward_returns(cadm_ctx* ctx, const cadm_reward_params* params, const float* traj, const float* obs, const float* actions,
                        const int32_t* first, int m, int n, const float* rows_in, float* rows_out, float* step_out, float* sum_out,
                        void* workspace, void* stream);
/* The loop of cadm_valued_plan with that term in the particle returns: the next level of the nest.  Every iteration's rollout
 * records its trajectories; TERMINATE constraints write their first violations into the workspace.  Per iteration: rollout ->
 * constraints -> tracking -> rows[q] += weight * S[q] on the particle rows [m,n_it,p] -> the terminal value -> cadm_particle_score (a
 * risk-aware score sees return + learned reward (+ value) per particle) -> the actuator's and the uncertainty term's costs off the
 * candidate score, unchanged -> the refit.  PENALTY constraints do not gate the reward.  params NULL: exactly the launches of
 * cadm_valued_plan.  Refusals: those of cadm_valued_plan and of cadm_reward_returns.  workspace:
 * cadm_rewarded_workspace_bytes(ctx, m, n, K, mppi, terminate, actuator, uncertainty) with params set -- the loop underneath's WITH the
 * trajectory view, under TERMINATE constraints the first-violation view, and behind everything the step rewards [H,m,n,p] (0 for bad
 * arguments); with params NULL that of cadm_valued_plan. */
size_t cadm_rewarded_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate, int actuator, int uncertainty);
int cadm_rewarded_plan(cadm_ctx* ctx, const cadm_reward_params* params, const cadm_value_params* value,
                       const cadm_uncertainty_params* uncertainty, const cadm_actuator_params* actuator, float* prev_io, float* prefix_io,
                       int advance, const cadm_track_params* track, const float* targets, int T, const int32_t* offset,
                       const cadm_knot_params* knots, const int32_t* phase, const cadm_constraint_params* constraints,
                       const cadm_score_params* score, int update, const cadm_mppi_params* mppi_params, const float* obs,
                       const float* cp_obs, const float* cp_act, const float* init_mean, const float* init_var, float* carry_io,
                       int32_t* carry_valid_io, int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out,
                       float* best_return_out, void* stream);

/* Policy prior (no reference twin, OPT-IN): a caller-supplied actor pi rolled through the ensemble, its trajectories placed among the
 * candidates of every iteration of the opt-in loop (LOOP, TD-MPC): with few candidates and a short horizon the planner then starts from
 * what the learner already knows instead of from draws around a mean.
 * pi is an MLP  D -> h_1 -> .. -> h_L -> A  under the value net's conventions: L = n_hidden in 0 .. CADM_MAX_VALUE_LAYERS, every width in
 * 1 .. CADM_MAX_VALUE_WIDTH, one hidden activation CADM_VALUE_RELU | _TANH | _SWISH, a linear output of A <= CADM_MAX_POLICY_ACTIONS
 * units, D <= CADM_MAX_VALUE_DIMS.  For a state s [D], all in float32 (csrc/policy.hip, csrc/mlp_chain.h):
 *   x_k = (s_k - mean_k) * std_inv_k                                        one subtract, one multiply
 *   layer with K inputs, unit u:  acc = b[u];  for k = 0 .. K4-1 ascending:  acc = fmaf(W[k][u], x_k, acc)     (the value net's chain)
 *   hidden: the activation;   output z_d: the sum itself
 *   CADM_POLICY_TANH: a_d = mid + half * tanhf(z_d),  mid = 0.5f * (ub + lb), half = 0.5f * (ub - lb)  (one multiply, then one add, no
 *   fma; lb / ub: the ctx's lower_bound / upper_bound);   CADM_POLICY_NONE: a_d = z_d
 *   with noise:  a_d = a_d + noise_std * xi_d  (one multiply, one add);   always last:  a_d = fminf(fmaxf(a_d, lb), ub).
 * cadm_set_policy_net: as cadm_set_value_net (device pointers, a packed copy the ctx owns, a second call replaces the net, params NULL
 * clears it).  n_samples and noise_std of the registered params are not kept: every call below brings its own.
 * cadm_policy_eval: act_out[r,:] = the action of states[r,:] for states [R,D]: squash and clip, no noise -- the chain of the roll below.
 * cadm_policy_propose: P = n_samples proposal sequences per env, seqs_out [m,P,H,A].  Sequence (mi, j) acts at step t on its STATE
 * ESTIMATE, the mean over its p particles: obs[mi] at t = 0; at t >= 1 sequential float32 adds over the particles in ascending order,
 * starting from particle 0's value, then one IEEE division by (float)p.  A sequence with a non-finite value in any particle takes the
 * fallback clip(0, lb, ub) in every dim.  Its action then moves its particles one step through the model (a one-step rollout under the
 * iteration word CADM_POLICY_IT + 2 t = 0xFA0000 + 2 t; particles keep their member; a deterministic ctx rolls the mean head): H policy
 * steps and H - 1 one-step rollouts, nothing behind the last action.  Sequence 0 never gets noise; for j >= 1 xi is drawn with
 * Philox4x32-10 keyed (seed, call), counter (mi * P + j, t, g, 5): one call serves dims 4 g .. 4 g + 3, words (0, 1) through Box-Muller to
 * dims 4 g and 4 g + 1, words (2, 3) to 4 g + 2 and 4 g + 3; noise_std == 0 draws nothing.  ctx_vec: the context encoder's output
 * (cadm_context_forward), NULL for a model without one.  states_out [H,m,P,p,D] or NULL: the particle states every step read (step 0:
 * obs[mi] in every particle).  workspace: cadm_policy_workspace_bytes(ctx, m, P) bytes.  The roll follows its own actions: an actuator
 * model's delay is not honoured inside it.
 * Determinism: an action is one chain in ascending k behind a sequential particle sum, no floating-point atomics: the same bits run to
 * run, at any row position, for any m or P, from cadm_policy_eval as from the roll.
 * Refusals, before any HIP call: CADM_EINVAL for null pointers, n_hidden outside 0 .. 4, a width outside 1 .. 512, an unknown activation
 * or squash, n_samples < 1, a noise_std negative or not finite, D > CADM_MAX_VALUE_DIMS, A > CADM_MAX_POLICY_ACTIONS, a discrete ctx
 * (cartpole), a candidate-sharded ctx, activation tiles beyond the 160 KiB of LDS, a ctx whose num_cem_iters or horizon reaches the
 * roll's iteration words; params that do not describe the registered net (layers, widths, activation, squash): CADM_EINVAL; no
 * registered net: CADM_ESTATE. */
#define CADM_MAX_POLICY_ACTIONS 64
#define CADM_POLICY_NONE 0
#define CADM_POLICY_TANH 1
typedef struct cadm_policy_params {
    int32_t n_hidden;                          /* L: 0 .. CADM_MAX_VALUE_LAYERS */
    int32_t hidden[CADM_MAX_VALUE_LAYERS];     /* h_1 .. h_L, each 1 .. CADM_MAX_VALUE_WIDTH */
    int32_t activation;                        /* CADM_VALUE_RELU | CADM_VALUE_TANH | CADM_VALUE_SWISH */
    int32_t squash;                            /* CADM_POLICY_NONE | CADM_POLICY_TANH */
    int32_t n_samples;                         /* P >= 1: proposal sequences per env */
    float noise_std;                           /* finite, >= 0: exploration noise of sequences 1 .. P - 1 */
} cadm_policy_params;
int cadm_set_policy_net(cadm_ctx* ctx, const cadm_policy_params* params, const float* const* W, const float* const* b, const float* mean,
                        const float* std_inv, void* stream);
int cadm_policy_eval(cadm_ctx* ctx, const float* states, int R, float* act_out, void* stream);
size_t cadm_policy_workspace_bytes(cadm_ctx* ctx, int m, int P);
int cadm_policy_propose(cadm_ctx* ctx, const cadm_policy_params* params, const float* obs, const float* ctx_vec, int m, uint32_t seed,
                        uint32_t call, float* seqs_out, float* states_out, void* workspace, void* stream);
/* The loop of cadm_rewarded_plan with the policy's proposals among its candidates: the next level of the nest.  Behind the context
 * encoder ONE cadm_policy_propose; every iteration then writes the P sequences into the candidate slots [K + (last iteration &&
 * add_mean_last ? 1 : 0), .. + P) -- behind the kept elites and the mean candidate, in front of the knot shaping and the actuator pass,
 * so proposals are shaped and pinned like any other candidate.  policy NULL: exactly the launches of cadm_rewarded_plan.  Refusals: those
 * of cadm_rewarded_plan and of cadm_policy_propose, and keep_elites + 1 + n_samples beyond the smallest per-iteration candidate count
 * max(floor(n / decay^it), 2 num_elites, keep_elites + 1) capped at n.  workspace: cadm_guided_workspace_bytes(ctx, m, n, K, mppi,
 * terminate, actuator, uncertainty, P), enough for every combination of terms: cadm_rewarded_workspace_bytes' with a reward set, and
 * with P = n_samples > 0 behind it the proposals [m,P,H,A] and the roll's workspace (0 for bad arguments) -- a loop with fewer terms
 * takes fewer views in front of the policy's and fits; with policy NULL the workspace of cadm_rewarded_plan will do. */
size_t cadm_guided_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate, int actuator, int uncertainty, int P);
int cadm_guided_plan(cadm_ctx* ctx, const cadm_policy_params* policy, const cadm_reward_params* params, const cadm_value_params* value,
                     const cadm_uncertainty_params* uncertainty, const cadm_actuator_params* actuator, float* prev_io, float* prefix_io,
                     int advance, const cadm_track_params* track, const float* targets, int T, const int32_t* offset,
                     const cadm_knot_params* knots, const int32_t* phase, const cadm_constraint_params* constraints,
                     const cadm_score_params* score, int update, const cadm_mppi_params* mppi_params, const float* obs,
                     const float* cp_obs, const float* cp_act, const float* init_mean, const float* init_var, float* carry_io,
                     int32_t* carry_valid_io, int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out,
                     float* best_return_out, void* stream);

/* Terminal value from Q critics (no reference twin, OPT-IN): for a learner that has an actor pi and critics Q_c(s, a) but no state-value
 * net (LOOP on SAC / TD3: twin critics; TD-MPC: Q(z_H, pi(z_H)) behind every imagined trajectory), the terminal term
 *   rows_out[q] = rows_in[q] + weight * reduce_c Q_c(s, pi(s)),   s = traj[H-1,q]
 * on the LAST state of every particle, in ONE launch: actor, then critics, then the reduction.  It stands where cadm_value_returns'
 * term stands and excludes it.  pi is the net of cadm_set_policy_net.  Each of the C = n_critics critics is an MLP
 * D + A -> h_1 -> .. -> h_L -> 1 under the value net's conventions; all share one layer count, one set of widths, one activation and
 * the input statistics, weights are per critic.  For one row, all in float32 (csrc/critic.hip, csrc/mlp_chain.h):
 *   actor: exactly cadm_policy_eval of s -- x_k = (s_k - pmean_k) * pistd_k, the chain, the squash, no noise, the clip to [lb, ub]
 *   critic input u = [s ; a], K = D + A:  x_k = (u_k - mean_k) * std_inv_k                      one subtract, one multiply
 *   critic c, unit u of a layer:  acc = b[u];  for k = 0 .. K4-1 ascending:  acc = fmaf(W_c[k][u], x_k, acc)   (the value net's chain)
 *   hidden: the activation;   output q_c: the sum itself
 *   CADM_CRITIC_MIN:   r = q_0;  r = fminf(r, q_c) in ascending c
 *   CADM_CRITIC_MEAN:  r = q_0;  r = r + q_c in ascending c;  for C > 1 then r = r / (float)C  (IEEE division)
 *   rows_out = rows_in + weight * r:  one multiply, then one add, no fma.   weight carries a discount gamma^H, unless the
 *   ctx has a discount over the horizon (cadm_set_discount): the library then multiplies disc[H] in.
 * A row whose terminal state holds a non-finite value has r = NaN, set explicitly, and so a NaN return: the actor's fallback action is
 * not what a Q is computed from.  With first [m,n,p] (cadm_constrain_returns' first_violation, TERMINATE mode) a row with first[q] < H
 * keeps the bits of rows_in, its q_out is NaN, and its terminal state is not read.
 * Determinism: a row's result is one column's chains in ascending k, behind one another in a fixed order, no floating-point atomics:
 * the same bits run to run, in any batch, at any row position, for any m or n, from cadm_critic_eval as from the planner.
 * cadm_set_critic_nets: W and b hold C * (L + 1) DEVICE pointers, critic-major (W[c * (L + 1) + l] [in,out] row-major, b[..] [out]);
 * mean [D + A] and std_inv [D + A] are device pointers; everything is copied and packed into memory the ctx owns, on `stream`.  A second
 * call replaces the critics (the same shapes allocate nothing); params NULL clears them; cadm_ctx_destroy frees them.  params->weight is
 * not kept: every planner call brings its own weight and reduce; params->reduce is what cadm_critic_eval reduces with.
 * cadm_critic_eval: states [R,D].  actions NULL: the registered policy net acts (required: CADM_ESTATE without one); actions [R,A]: the
 * actor is skipped and the critics are evaluated at these (a non-finite action: NaN).  q_out [R]; q_each_out [C,R] or NULL: every
 * critic's q_c; act_out [R,A] or NULL: the action that was used.
 * cadm_critic_returns: traj [H,m,n,p,D] (a rollout's traj_out, n its packed candidate count), first [m,n,p] or NULL; q_out [m,n,p] or
 * NULL: r of every row, NaN where cut or non-finite.  rows_out may alias rows_in.
 * Refusals, before any HIP call: CADM_EINVAL for null pointers, n_hidden outside 0 .. 4, a width outside 1 .. 512, an unknown
 * activation, n_critics outside 1 .. CADM_MAX_CRITICS, an unknown reduce, a weight that is not finite, D > CADM_MAX_VALUE_DIMS,
 * A > CADM_MAX_POLICY_ACTIONS, a discrete ctx (cartpole), a candidate-sharded ctx, LDS at one row tile (the critics' input tile of 16
 * rows x (D + A rounded up to 4), two regions of 16 rows x the widest layers of actor and critics, the output sums and the flags) beyond
 * 160 KiB; no registered critics, or on the actor path no registered policy net: CADM_ESTATE; params that do not describe the
 * registered critics (count, layers, widths, activation): CADM_EINVAL. */
#define CADM_MAX_CRITICS 5
#define CADM_CRITIC_MIN 0
#define CADM_CRITIC_MEAN 1
typedef struct cadm_critic_params {
    int32_t n_hidden;                          /* L: 0 .. CADM_MAX_VALUE_LAYERS */
    int32_t hidden[CADM_MAX_VALUE_LAYERS];     /* h_1 .. h_L, each 1 .. CADM_MAX_VALUE_WIDTH */
    int32_t activation;                        /* CADM_VALUE_RELU | CADM_VALUE_TANH | CADM_VALUE_SWISH */
    int32_t n_critics;                         /* C: 1 .. CADM_MAX_CRITICS */
    int32_t reduce;                            /* CADM_CRITIC_MIN | CADM_CRITIC_MEAN */
    float weight;                              /* finite */
} cadm_critic_params;
int cadm_set_critic_nets(cadm_ctx* ctx, const cadm_critic_params* params, const float* const* W, const float* const* b, const float* mean,
                         const float* std_inv, void* stream);
int cadm_critic_eval(cadm_ctx* ctx, const float* states, const float* actions, int R, float* q_out, float* q_each_out, float* act_out,
                     void* stream);
int cadm_critic_returns(cadm_ctx* ctx, const cadm_critic_params* params, const float* traj, const int32_t* first, int m, int n,
                        const float* rows_in, float* rows_out, float* q_out, void* stream);
/* The loop of cadm_guided_plan with that term in the particle returns (cadm_anchored_plan is the level above).  Per iteration the stage runs
 * where the terminal value's runs: rollout -> constraints -> tracking -> the learned reward -> rows[q] += weight * r[q] on the particle
 * rows [m,n_it,p] -> cadm_particle_score -> the costs off the candidate score -> the refit.  critic NULL: exactly the launches of
 * cadm_guided_plan.  policy may be NULL while a policy net is registered: the term needs the registered net, not the proposals.
 * Refusals: those of cadm_guided_plan and of cadm_critic_returns, and critic and value both non-NULL (CADM_EINVAL: a plan has one
 * terminal term).  workspace: cadm_critic_workspace_bytes(ctx, m, n, K, mppi, terminate, actuator, uncertainty, P) -- that of
 * cadm_guided_workspace_bytes: the term reads the trajectory view and takes none of its own. */
size_t cadm_critic_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate, int actuator, int uncertainty, int P);
int cadm_critic_plan(cadm_ctx* ctx, const cadm_critic_params* critic, const cadm_policy_params* policy, const cadm_reward_params* params,
                     const cadm_value_params* value, const cadm_uncertainty_params* uncertainty, const cadm_actuator_params* actuator,
                     float* prev_io, float* prefix_io, int advance, const cadm_track_params* track, const float* targets, int T,
                     const int32_t* offset, const cadm_knot_params* knots, const int32_t* phase, const cadm_constraint_params* constraints,
                     const cadm_score_params* score, int update, const cadm_mppi_params* mppi_params, const float* obs,
                     const float* cp_obs, const float* cp_act, const float* init_mean, const float* init_var, float* carry_io,
                     int32_t* carry_valid_io, int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out,
                     float* best_return_out, void* stream);

/* A discount over the horizon of the opt-in planner (csrc/discount.hip; no reference twin, OPT-IN).  It is state of the ctx, as the
 * horizon is, not an argument of the plan entry points: every quantity that enters a candidate's score is weighted per step by ONE
 * table, so that a learner's critic behind the plan and the step rewards in front of it obey one Bellman equation.
 * cadm_set_discount: gamma in (0, 1]; NaN, gamma <= 0 and gamma > 1 are CADM_EINVAL before any HIP call.  gamma == 1 clears the
 * discount: the table is then null and every launch of the library is the undiscounted one.  Otherwise the ctx owns a device table
 *   disc[t] = (float)pow((double)gamma, (double)t),  t = 0 .. H,  disc[0] = 1 exactly,
 * built on the host and copied on `stream`.  Set the discount BEFORE a workspace is sized: with a discount the loop always records
 * trajectories, and every cadm_*_workspace_bytes(ctx, ..) of the nest from cadm_icem_workspace_bytes to cadm_anchored_workspace_bytes
 * returns the size with the trajectory view.  Refusals of a gamma < 1: a discrete ctx (cartpole), a candidate-sharded ctx, a D whose two
 * tiles of 64 x D floats and the table exceed 48 KiB of LDS (CADM_EINVAL); a CADM_ENV_SPEC ctx whose spec is not set (CADM_ESTATE).
 * cadm_discount_weights: *set_out = 1 and host_out[0 .. H] = the same floats the kernels read (host_out may be NULL), or *set_out = 0.
 * What a table does, with disc[t] the weight of step t (every product and every add one fp32 rounding, nothing fused):
 *   the env's own return      the loop launches cadm_discount_returns directly behind the rollout:  sum = disc[0] * r_0;  for t = 1 ..
 *                             H - 1: sum = sum + disc[t] * r_t;  rows_out[q] = isnan(rows_in[q]) ? rows_in[q] : sum.  r_t is the step
 *                             reward from the recorded states (pre-step state obs at t = 0, else traj[t - 1]; post-step state traj[t];
 *                             the raw action), as cadm_constrain_returns' TERMINATE mode takes it
 *   cadm_constrain_returns    PENALTY: pen = pen + disc[t] on the violating steps, ascending t from 0.0f;  rows - w * pen (a row without
 *                             a violation keeps its bits; the counters are unchanged).  TERMINATE: sum as above up to tau, then
 *                             sum - w * disc[tau]: the penalty is paid at the step that leaves
 *   cadm_tracking_returns     cost = cost + disc[t] * (w_k * c), the order (t, k) ascending and the NaN-target skip unchanged
 *   cadm_reward_returns       S = S + disc[t] * R_t; step_out stays undiscounted
 *   cadm_uncertainty_cost     cost = cost + disc[t] * u_t, u_t behind form and cap; step [m,n,H] stays undiscounted
 *   cadm_actuate_actions      c_a = c_a + disc[t] * (w_a * (y - last)^2); pins, limits and the sequences are untouched
 *   cadm_value_returns,       rows + weight_eff * V with weight_eff = weight * disc[H], one fp32 product on the host: with a discount
 *   cadm_critic_returns       set, `weight` no longer carries gamma^H, the library multiplies it in
 * The `first` cuts of these calls are unchanged.  The stand-alone calls read the table as the loop's stages do: a diagnostic reports what
 * the planner scored.  cadm_cem_plan, cadm_cem_plan_staged and cadm_rs_plan sum the step rewards inside the rollout kernel: on a ctx with
 * a discount they return CADM_ESTATE and launch nothing.  cadm_plan_forecast, cadm_policy_propose, cadm_eval_horizon and
 * cadm_eval_calibration do not score a plan and ignore the table: a forecast's returns stay the undiscounted sums.
 * cadm_discount_returns: traj [H,m,n,p,D] (a rollout's traj_out, n its packed candidate count), obs [m,D], actions [m,n,H,A] (raw, as the
 * rollout read them), rows_in / rows_out [m,n,p] (rows_out may alias rows_in), step_out [H,m,n,p] or NULL: the undiscounted r_t.  With no
 * discount set: CADM_ESTATE.  Determinism: a row's sum is one thread's chain in ascending t, no floating-point atomics, nothing depends
 * on the grid, on m or n, or on the row's position: the same bits run to run and inside any batch. */
int cadm_set_discount(cadm_ctx* ctx, float gamma, void* stream);
int cadm_discount_weights(cadm_ctx* ctx, float* host_out, int* set_out);
int cadm_discount_returns(cadm_ctx* ctx, const float* traj, const float* obs, const float* actions, int m, int n, const float* rows_in,
                          float* rows_out, float* step_out, void* stream);

/* Imagined rollouts for a learner (csrc/imagine.hip; no reference twin): n = branches independent model rollouts of k steps from each of
 * m start states, recorded as transitions -- what MBPO / Dyna train an actor and critics on, with the per-transition ensemble
 * disagreement MOPO / M2AC penalise or mask by.  Every step is ONE one-step rollout of the unchanged rollout kernels over [m,n,p] particle
 * rows (k is independent of the ctx's horizon) under the even iteration word CADM_IMAGINE_IT + 2 t = 0xF00000 + 2 t -- above every planner
 * iteration, below the proposal roll's 0xFA0000 --, so the head noise never repeats that of a plan, a roll or a forecast of the same
 * (seed, call).  A row is (start state mi, branch j), row = mi * n + j; all of its p particles start step t from states[t,row] (step 0:
 * obs[mi]), so every member predicts p / E times and one particle is kept (MBPO's scheme).  Per row and step t, in this order:
 *   a_t   actions NULL: the registered policy net (cadm_set_policy_net) on states[t,row], exactly cadm_policy_eval's chain, then with
 *         noise_std > 0  a_d = a_d + noise_std * xi_d  (one multiply, one add) on EVERY row, xi drawn as cadm_policy_propose draws it but
 *         under counter (row, t, g, 7), then the clip;  actions [m,n,k,A]: a_t = fminf(fmaxf(actions[mi,j,t,:], lb), ub), no net is evaluated
 *   sel   = (uint64(w0) * p) >> 32,  w0 = word 0 of Philox4x32-10 keyed (seed, call), counter (row, t, 0, 6);  member = sel / (p / E)
 *   s'    = next[row,sel,:], the kept particle's post-step state;   r = rows1[row,sel], the rollout's own one-step return of that particle
 *   u     = sum_d w_d v_d in ascending d from the first term, v_d the epistemic variance over the row's p particles exactly as
 *         cadm_uncertainty_cost computes it (kind epistemic, form var, no cap; dims with w_d == 0 are not read); a non-finite u is +inf
 *   alive, s' finite, healthy:      valid 1, done 0, states[t+1] = s'
 *   alive, s' finite, not healthy:  valid 1, done 1, states[t+1] = s', the row is dead afterwards
 *   alive, a value of s' NaN / inf: valid 0, done 0, rew 0, states[t+1] = states[t], the row is dead afterwards (member and u are recorded)
 *   dead:                           valid 0, done 0, rew 0, member -1, u 0, states[t+1] = states[t]
 *   healthy: s'[dim] > lo && s'[dim] < hi in float32 for every constraint (cadm_constrain_returns' test; only n, dim, lo, hi are read:
 *   either mode defines termination here);  length[row] = the number of valid transitions.  A dead row's rollout still runs (static
 *   shapes) from its frozen, finite state and is ignored.  A deterministic ctx draws no head noise and still draws sel.
 * cadm_imagine_workspace_bytes: the bytes of `buffer`; offsets_out [CADM_IMAGINE_VIEWS] or NULL takes the byte offsets of the outputs in
 * it, in this order: states [k+1,m,n,D] float, act [k,m,n,A] float, rew [k,m,n] float, done [k,m,n] uint8, valid [k,m,n] uint8, member
 * [k,m,n] int32, disagreement [k,m,n] float, length [m,n] int32, alive [m,n] uint8 (the state machine's flag behind the last step); the
 * chain's own views lie behind them.  Nothing is compacted: shapes are static.  0 for bad arguments.
 * cadm_imagine: obs [m,D]; ctx_vec the context encoder's output for the m start states, NULL without one; disagreement NULL: w = 1 (only
 * n_dims and w are read).  cadm_imagine_select: the stage between two rollouts alone, on the caller's next [rows,p,D], rows1 [rows,p],
 * state [rows,D] (states[t]) and alive_io [rows]; sel_in [rows] or NULL replaces the draw (clamped to 0 .. p - 1); length_io [rows] or
 * NULL is incremented by valid; bcast_out [rows,p,D] or NULL takes states[t+1] in every particle slot (it must not alias next).
 * Determinism: every output is one thread's chain in the order above, no floating-point atomics, nothing depends on the grid or the
 * group size: the same bits run to run, and at any row position for the same sel.
 * Refusals, before any HIP call: CADM_EINVAL for null pointers, m, n or k < 1, a noise_std negative or not finite, a discrete ctx
 * (cartpole), a candidate-sharded ctx, D > CADM_MAX_UNC_DIMS, a p * D tile beyond the stage's 48 KiB LDS budget, m * n * p rows beyond
 * one rollout launch's 32-bit indexing, a num_cem_iters or a k whose last word leaves 0xF00000 .. 0xF9FFFE, what cadm_constrain_returns
 * / cadm_uncertainty_cost refuse of their parameters; neither actions nor a registered policy net: CADM_ESTATE. */
#define CADM_IMAGINE_VIEWS 9
size_t cadm_imagine_workspace_bytes(cadm_ctx* ctx, int m, int n, int k, uint64_t* offsets_out);
int cadm_imagine(cadm_ctx* ctx, const float* obs, const float* ctx_vec, const float* actions, int m, int n, int k, float noise_std,
                 const cadm_constraint_params* constraints, const cadm_uncertainty_params* disagreement, uint32_t seed, uint32_t call,
                 void* buffer, void* stream);
int cadm_imagine_select(cadm_ctx* ctx, const float* next, const float* rows1, const float* state, const int32_t* sel_in, int rows, int t,
                        const cadm_constraint_params* constraints, const cadm_uncertainty_params* disagreement, uint32_t seed,
                        uint32_t call, uint8_t* alive_io, float* state_out, float* rew_out, uint8_t* done_out, uint8_t* valid_out,
                        int32_t* member_out, float* disagreement_out, int32_t* length_io, float* bcast_out, void* stream);

/* Stochastic actor head (csrc/policy_gauss.hip; no reference twin): the registered policy net read as a SAC actor -- a diagonal Gaussian
 * whose mean mu [A] is the net's own output layer (so cadm_policy_eval, cadm_policy_propose and the critics' actor are the MODE actor,
 * unchanged) and whose log standard deviation l [A] is a second linear layer on the same last hidden tile: W_ls [h_L, A] (L = 0: [D, A]),
 * b_ls [A], device pointers, a packed copy the ctx owns.  The head hangs on the registered net: cadm_set_policy_head without one is
 * CADM_ESTATE; every cadm_set_policy_net (a new net or a clear) drops it; params NULL clears it; a second call replaces it.
 * Per row q = row0 + r and action dim d, all float32, every operation rounded on its own, no fma outside the matrix pipe:
 *   ls_d   CADM_LOGSTD_CLAMP: fminf(fmaxf(l_d, lo), hi)      CADM_LOGSTD_TANH: lo + (0.5f * (hi - lo)) * (tanhf(l_d) + 1.0f)
 *   sig_d  = expf(ls_d)
 *   xi_d   Philox4x32-10 keyed (seed, call), counter (q, t, d >> 2, 8), words to dims through Box-Muller exactly as cadm_policy_propose's
 *          noise (words 0, 1 -> dims 4 g, 4 g + 1; words 2, 3 -> 4 g + 2, 4 g + 3)
 *   u_d    = mu_d + sig_d * xi_d                              (one multiply, one add)
 *   CADM_POLICY_TANH:  a_d = mid + half * tanhf(u_d);   J_d = logf(half) + 2 * ((LN2 - u_d) - softplus(-2 * u_d)),
 *                      softplus(x) = fmaxf(x, 0) + log1pf(expf(-fabsf(x))),  LN2 = 0.6931472f      (no epsilon inside a log)
 *   CADM_POLICY_NONE:  a_d = u_d;   J_d = 0      (logp is the UNCLIPPED Gaussian's density: the clip below is not part of it)
 *   a_d    = fminf(fmaxf(a_d, lb), ub)
 *   term_d = (((-0.5f * xi_d) * xi_d - ls_d) - 0.9189385f) - J_d
 *   logp   = term_0 + term_1 + ..  in ascending d from term_0, one thread per row
 *   mode_d = exactly cadm_policy_eval's action of the row (the squash of mu_d, the clip)
 * A row with a non-finite value in its state: act = mode = clip(0, lb, ub) in every dim, logp = NaN.  half > 0 (lb < ub) is required.
 * cadm_policy_sample: states [R,D] -> act_out [R,A], logp_out [R], mode_out [R,A] or NULL; row r draws as row row0 + r, so a batch cut
 * into calls draws what one call draws.  cadm_imagine_sampled: cadm_imagine with actions NULL whose per-step action launch is this draw
 * under counter (row, t, g, 8) on states[t] -- act[t] the sampled action, logp[t,row] its log-density at states[t,row], computed on every
 * row (static shapes) and meaningful where valid; every other launch and output is cadm_imagine's.
 * cadm_imagine_sampled_workspace_bytes: cadm_imagine's nine views first, in their order, then logp [k,m,n] float, then the chain's own.
 * Determinism: every output is one thread's chain in the stated order, no floating-point atomics; nothing depends on the row tiles, the
 * grid, R or the row's position for the same q: the same bits run to run.
 * Refusals, before any HIP call: CADM_EINVAL for null pointers, an unknown kind or bound, log-std bounds that are not finite, lo >= hi,
 * hi > 10 (expf stays finite with a margin), R < 1, t < 0, row0 + R beyond 2^32, what cadm_set_policy_net refuses of the registered net's
 * description, lb >= ub, activation tiles beyond the 160 KiB of LDS at one row tile, and for cadm_imagine_sampled what cadm_imagine
 * refuses; no registered net (call cadm_set_policy_net) or no head (call cadm_set_policy_head): CADM_ESTATE. */
#define CADM_HEAD_GAUSSIAN 1
#define CADM_LOGSTD_CLAMP 0
#define CADM_LOGSTD_TANH 1
typedef struct cadm_policy_head_params { int32_t kind, bound; float log_std_min, log_std_max; } cadm_policy_head_params;
int cadm_set_policy_head(cadm_ctx* ctx, const cadm_policy_head_params* params /* NULL: clear */, const float* W_ls /* [h_L, A]; L = 0: [D, A] */,
                         const float* b_ls /* [A] */, void* stream);
int cadm_policy_sample(cadm_ctx* ctx, const float* states /* [R,D] */, int R, uint32_t row0, int t, uint32_t seed, uint32_t call,
                       float* act_out /* [R,A] */, float* logp_out /* [R] */, float* mode_out /* [R,A] or NULL */, void* stream);
#define CADM_IMAGINE_SAMPLED_VIEWS 10   /* cadm_imagine's nine, then logp [k,m,n] float */
size_t cadm_imagine_sampled_workspace_bytes(cadm_ctx* ctx, int m, int n, int k, uint64_t* offsets_out);
int cadm_imagine_sampled(cadm_ctx* ctx, const float* obs, const float* ctx_vec, int m, int n, int k, const cadm_constraint_params* constraints,
                         const cadm_uncertainty_params* disagreement, uint32_t seed, uint32_t call, void* buffer, void* stream);
/* Proposals of the policy prior drawn from the head (csrc/policy_gauss.hip; no reference twin, OPT-IN): cadm_set_policy_proposals chooses
 * where sequences 1 .. P - 1 of cadm_policy_propose (and so of cadm_guided_plan and cadm_critic_plan) come from.  CADM_PROPOSE_NOISE, the
 * default: the mode action plus the call's noise_std behind the squash, as described at "Policy prior".  CADM_PROPOSE_HEAD: trajectories
 * of pi itself (TD-MPC's policy trajectories, LOOP on SAC), the standard deviation the head predicts at every state times std_scale.
 * Sequence 0 stays the mode trajectory.  The setting is state of the ctx, a planner option and not part of a net: no plan entry point
 * gains an argument, the default is NOISE with scale 1, and it survives cadm_set_policy_net and cadm_set_policy_head.  Under HEAD every
 * policy step of the roll is one launch of the kernel below; the one-step rollouts between the steps, their iteration words
 * CADM_POLICY_IT + 2 t, the workspace and the injection into the candidates are the noise route's.
 * A row is (env mi, sequence j), q = mi * P + j, at step t; all float32, every operation rounded on its own, no fma outside the matrix pipe:
 *   state   exactly cadm_policy_propose's estimate: obs[mi] at t = 0; at t >= 1 the sequential particle sum in ascending order, then one
 *           IEEE division by (float)p; the non-finite flag, the normalisation and the states_out copies are the same
 *   mu_d, l_d   the hidden layers on the registered net's packed copy, then the two output layers on the last hidden tile, as
 *           cadm_policy_sample reads them
 *   ls_d    by the registered head's bound:  CADM_LOGSTD_CLAMP: fminf(fmaxf(l_d, lo), hi);  CADM_LOGSTD_TANH: lo + (0.5f * (hi - lo)) *
 *           (tanhf(l_d) + 1.0f)
 *   sig_d   = expf(ls_d);   s_d = std_scale * sig_d                      (one multiply)
 *   xi_d    Philox4x32-10 keyed (seed, call), counter (q, t, d >> 2, 5): the counter, the stream word and the word-to-dim mapping of the
 *           noise route.  A call has one source of proposals, so nothing is drawn twice; xi is bit for bit the noise route's
 *   j == 0, or std_scale == 0:  no draw, u_d = mu_d;   else  u_d = mu_d + s_d * xi_d      (one multiply, one add)
 *   CADM_POLICY_TANH: a_d = mid + half * tanhf(u_d);   CADM_POLICY_NONE: a_d = u_d;   always last: a_d = fminf(fmaxf(a_d, lb), ub)
 *           (the noise sits BEFORE the squash, as in cadm_policy_sample, not behind it as on the noise route)
 * A row with a non-finite value in any particle of its state takes clip(0, lb, ub) in every dim.  No log-density is computed: proposals
 * are candidates, nothing reads their density.
 * Determinism: the reduction contract of the two kernels it is made of -- one thread's chain per output in the stated order, no
 * floating-point atomics, nothing depends on the row tiles, the grid, m, P or the row's position: the same bits run to run.  Sequence 0 has
 * cadm_policy_eval's bits on its state estimate.
 * Refusals, before any HIP call.  cadm_set_policy_proposals: CADM_EINVAL for a null ctx, an unknown source, a std_scale negative or not
 * finite.  cadm_policy_propose, cadm_guided_plan (with a policy) and cadm_critic_plan (with a policy) under HEAD, behind their own
 * refusals: CADM_EINVAL for a noise_std > 0 in the call's params (one source per call), lb >= ub, activation tiles beyond the 160 KiB of
 * LDS at one row tile; no head on the registered net: CADM_ESTATE (every cadm_set_policy_net drops the head, so HEAD is refused from
 * then until cadm_set_policy_head is called again). */
#define CADM_PROPOSE_NOISE 0
#define CADM_PROPOSE_HEAD 1
int cadm_set_policy_proposals(cadm_ctx* ctx, int32_t source, float std_scale);

/* Log-density of given actions (csrc/policy_logp.hip; no reference twin, OPT-IN): log pi(a | s) of the stochastic actor above at an action
 * the CALLER brings -- cadm_policy_sample returns the density of an action it drew itself.  Two uses of one kernel.  cadm_policy_logp: x
 * [R,D], act [R,A] -> logp_out [R], for a learner that re-weights stored transitions under its current actor.  cadm_policy_logp_returns
 * and the cadm_anchored_plan level of the nest: the actor-regularised score of LOOP / MBOP / KL-regularised MPC,
 *   rows' = rows + weight * S,   S = ((0 + logp_0) + logp_1) + ..  over the counted steps of a particle's trajectory,
 * with logp_t = log pi(a_t | s_t), s_t = obs[mi] at t = 0 and traj[t-1, q] after it, a_t = actions[mi, ni, t, :] raw, as the rollout
 * read them (behind knot shaping and the actuator pass).  Every (step, particle) pair is a row: e = t * (m n p) + q, cadm_reward_returns'
 * row space.  With `first` (cadm_constrain_returns' first_violation) the counted steps are t <= first[q]; the others are not loaded and
 * read NaN in step_out.
 * Per counted row and action dim d, all float32, every operation rounded on its own, no fma outside the matrix pipe:
 *   x, the hidden layers, mu_d, l_d   exactly cadm_policy_sample's walk, on the registered net's packed copy and the head's layer
 *   ls_d   the registered head's bound, as cadm_policy_sample:  CADM_LOGSTD_CLAMP: fminf(fmaxf(l_d, lo), hi);  CADM_LOGSTD_TANH: lo +
 *          (0.5f * (hi - lo)) * (tanhf(l_d) + 1.0f)
 *   CADM_POLICY_TANH:  y = (a_d - mid) / half       one subtraction, one correctly rounded division; mid = 0.5f * (ub + lb), half =
 *                                                    0.5f * (ub - lb), as the policy kernels define them
 *                      y = fminf(fmaxf(y, -CADM_LOGP_YMAX), CADM_LOGP_YMAX)
 *                      lp = log1pf(y);  lm = log1pf(-y);  u = 0.5f * (lp - lm);  J = logf(half) + (lp + lm)      (= log(half (1 - y^2)))
 *   CADM_POLICY_NONE:  u = a_d;  J = 0
 *   xi     = (u - mu_d) * expf(-ls_d)
 *   g_d    = ((-0.5f * xi) * xi - ls_d) - 0.9189385f
 *   term_d = space == CADM_LOGP_ACTION ? g_d - J : g_d      (CADM_LOGP_PRE_SQUASH: the Gaussian's density of u, with no Jacobian)
 *   logp   = term_0 + term_1 + ..  in ascending d from term_0, one thread per row
 * A counted row with a non-finite value in its state or in its action gets logp = NaN explicitly (the clamp would hide an infinite
 * action).  Nothing is drawn and no counter moves.  An action on or beyond a bound sits at |y| = CADM_LOGP_YMAX, |u| = atanh(YMAX) ~ 7.25:
 * in action space that is the tanh-Gaussian's own spike at the bounds, which a narrow policy prices at thousands of nats;
 * CADM_LOGP_PRE_SQUASH is the quadratic form without the Jacobian.
 * Step sum and row update, cadm_reward_returns' arithmetic: S as above in ascending t; on a ctx with a discount over the horizon S = S +
 * disc[t] * logp_t (step_out stays undiscounted); rows_out = rows_in + weight * S, one multiply and then one add.  step_out [H,m,n,p]
 * or NULL (then workspace: cadm_policy_logp_workspace_bytes(ctx, m, n) bytes), sum_out [m,n,p] or NULL; rows_out may be rows_in.
 * Determinism: every output is one thread's chain in the stated order, no floating-point atomics; nothing depends on the row tiles, the
 * grid, m, n, p or the row's position: the same bits run to run, in any batch, and from cadm_policy_logp as from the planner stage.
 * cadm_anchored_plan: the loop of cadm_critic_plan with that term in the particle returns, the outermost level of the nest today.  Per
 * iteration: rollout -> constraints -> tracking -> the learned reward -> rows[q] += weight * S[q] -> the terminal value / Q ->
 * cadm_particle_score (a risk-aware score sees the term per particle) -> the costs off the candidate score -> the refit.  logp NULL:
 * exactly the launches of cadm_critic_plan.  policy may be NULL while a policy net is registered: the term needs the registered net and
 * its head, not the proposals.  workspace: cadm_anchored_workspace_bytes(..) -- that of cadm_critic_workspace_bytes, and behind it the
 * step log-densities [H,m,n,p] (rounded up to 256 bytes); the views in front keep their places.
 * Refusals, before any HIP call: CADM_EINVAL for null pointers, R, m or n < 1, an unknown space, a weight that is not finite, lb >= ub, a
 * head whose log_std_min < -10 (the mirror of log_std_max > 10: expf(-ls) stays finite with a margin), a discrete or candidate-sharded
 * ctx, what cadm_set_policy_net refuses of the registered net's description, activation tiles beyond the 160 KiB of LDS at one row tile;
 * no registered net (call cadm_set_policy_net) or no head on it (call cadm_set_policy_head; every cadm_set_policy_net drops the head):
 * CADM_ESTATE; for cadm_anchored_plan also what cadm_critic_plan refuses. */
#define CADM_LOGP_ACTION 0
#define CADM_LOGP_PRE_SQUASH 1
#define CADM_LOGP_YMAX 0.999999f   /* where |y| is clamped before atanh: the value SAC implementations clamp at */
typedef struct cadm_policy_logp_params { float weight; /* finite */ int32_t space; /* CADM_LOGP_ACTION | CADM_LOGP_PRE_SQUASH */ } cadm_policy_logp_params;
int cadm_policy_logp(cadm_ctx* ctx, const float* x /* [R,D] */, const float* act /* [R,A] */, int R, int space, float* logp_out /* [R] */,
                     void* stream);
size_t cadm_policy_logp_workspace_bytes(cadm_ctx* ctx, int m, int n);
int cadm_policy_logp_returns(cadm_ctx* ctx, const cadm_policy_logp_params* params, const float* traj, const float* obs, const float* actions,
                             const int32_t* first, int m, int n, const float* rows_in, float* rows_out, float* step_out, float* sum_out,
                             void* workspace, void* stream);
size_t cadm_anchored_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate, int actuator, int uncertainty, int P);
int cadm_anchored_plan(cadm_ctx* ctx, const cadm_policy_logp_params* logp, const cadm_critic_params* critic, const cadm_policy_params* policy,
                       const cadm_reward_params* params, const cadm_value_params* value, const cadm_uncertainty_params* uncertainty,
                       const cadm_actuator_params* actuator, float* prev_io, float* prefix_io, int advance, const cadm_track_params* track,
                       const float* targets, int T, const int32_t* offset, const cadm_knot_params* knots, const int32_t* phase,
                       const cadm_constraint_params* constraints, const cadm_score_params* score, int update,
                       const cadm_mppi_params* mppi_params, const float* obs, const float* cp_obs, const float* cp_act,
                       const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m, int n, uint32_t seed,
                       uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream);

/* Value-expansion targets (csrc/imagine_targets.hip; no reference twin): what a critic is trained on, out of cadm_imagine's transitions
 * and the caller's bootstrap values of their states, in ONE launch -- lambda-returns on every imagined state (Dreamer, TD-MPC), the n-step
 * targets of the start state (MVE), their inverse-variance combination over the branches (STEVE), the reward reduced by a multiple of the
 * disagreement and the rollout cut where it passes a bound (MOPO, M2AC).  rew, valid, done, disagreement are [k,m,n] as cadm_imagine lays
 * them out; boot [k+1,m,n] is the bootstrap value of states[t].  A row is (start state i, branch j); element t of the row is [t,i,j].
 * Everything is float32 and every operation is rounded on its own (no fused multiply-add); divisions are correctly rounded;
 * one_minus_lambda = 1.0f - lambda is computed once on the host.  Per row, in this order:
 *   L        the number of leading steps with valid[t] && !(disagreement[t] > max_disagreement);   used[t] = t < L
 *   term     L >= 1 && done[L-1]   (a done in front of the last used step is not read)
 *   r~_t     rew[t] where penalty == 0 (no multiply, so 0 * inf cannot arise), else rew[t] - penalty * disagreement[t]
 *   lambda   for t = L-1 down to 0:  t == L-1:  G = term ? r~_t : r~_t + gamma * boot[t+1]
 *                                    otherwise:  G = r~_t + gamma * (one_minus_lambda * boot[t+1] + lambda * G)
 *            lambda_return[t] = G for t < L and 0 behind; a non-finite bootstrap propagates
 *   n-step   acc = 0, disc = 1;  for h = 1 .. L:  acc = acc + disc * r~_{h-1};  disc = disc * gamma;
 *            x_h = (h == L && term) ? acc : acc + disc * boot[h].   For h > L: x_h = x_L with term (a terminated row is worth its terminal
 *            return at every longer horizon), no target without.  nstep[h-1] = x_h and nstep_ok[h-1] = 1 where a target exists and is
 *            finite, otherwise both are 0
 * So a diverged row (valid 0 without done) bootstraps from boot[L], the value of its last finite state, and a terminated row does not
 * bootstrap.  Per start state i and horizon h, with want_steve only:
 *   c = the number of branches with nstep_ok;  mean = c > 0 ? (sum x) / c : 0;  var = c > 0 ? (sum (x - mean) * (x - mean)) / c : 0, both
 *   sums from 0.0f over those branches in ascending j (two passes);   w_h = c >= 2 ? 1 / (var + var_floor) : 0
 *   W = sum_h w_h and S = sum_h w_h * mean_h, from 0.0f in ascending h;   steve[i] = W > 0 ? S / W : boot[0,i,0];
 *   steve_weight[h-1,i] = W > 0 ? w_h / W : 0;   steve_fallback[i] = !(W > 0)
 * cadm_imagine_targets_workspace_bytes: the bytes of `buffer`; offsets_out [CADM_TARGET_VIEWS] or NULL takes the byte offsets of the
 * outputs in it, in this order: lambda_return [k,m,n] float, nstep [k,m,n] float, nstep_ok [k,m,n] uint8, used [k,m,n] uint8, and with
 * want_steve steve [m] float, steve_weight [k,m] float, steve_mean [k,m] float, steve_var [k,m] float, steve_count [k,m] int32,
 * steve_fallback [m] uint8 (without: these six offsets are 0 and take no bytes).  Every view starts on a multiple of 256 bytes; the
 * bytes between two views are never written.  0 for a null ctx and for what cadm_imagine_targets refuses of the shape.
 * cadm_imagine_targets: the inputs are read only and must not overlap `buffer`; prm->want_steve switches the STEVE outputs on and must be
 * what the buffer was sized with.  The ctx supplies the device and the error channel: no weights are read, nothing of the ctx changes.
 * Determinism: every output is one thread's chain in the order above, no floating-point atomics, no cross-lane reduction; nothing depends
 * on the grid, the group size, m, or the position of a row or a start state: the same bits run to run.
 * Refusals, CADM_EINVAL before any HIP call: null pointers; m, n or k < 1; m * n beyond 2^31 - 1 rows; gamma outside (0, 1]; lambda outside
 * [0, 1]; a penalty negative or not finite; max_disagreement not > 0 (+inf: no bound); with want_steve a var_floor not finite and > 0,
 * n < 2, or an n * k whose tile for ONE start state (5 bytes per target and 8 k bytes) is beyond the reduction's 48 KiB LDS budget -- the
 * scan without the STEVE outputs has no such limit. */
typedef struct cadm_target_params {
    float gamma;              /* (0, 1]: the discount */
    float lambda;             /* [0, 1]: lambda of the lambda-return */
    float penalty;            /* finite, >= 0: the multiple of disagreement taken off the reward */
    float max_disagreement;   /* > 0, +inf = none: the bound beyond which a rollout is cut */
    float var_floor;          /* finite, > 0: added to the branch variance; read only with want_steve */
    int32_t want_steve;       /* != 0: the STEVE outputs are computed and `buffer` holds their views */
} cadm_target_params;
#define CADM_TARGET_VIEWS 10
size_t cadm_imagine_targets_workspace_bytes(cadm_ctx* ctx, int m, int n, int k, int want_steve, uint64_t* offsets_out);
int cadm_imagine_targets(cadm_ctx* ctx, const float* rew, const uint8_t* valid, const uint8_t* done, const float* disagreement,
                         const float* boot, int m, int n, int k, const cadm_target_params* prm, void* buffer, void* stream);

/* One training step =sess.run([mse_loss, back_mse_loss, recon_loss, train_op]) (dynamics.py:505-507):
 * forward of context / forward / backward nets on the [E,B,.] bootstrap batch, losses
 * (dynamics.py:269-314), gradients, TF1-semantics Adam (dynamics.py:316-317) applied IN PLACE to the
 * registered master weights.  train != 0 applies the update; train == 0 only evaluates the losses
 * (validation, dynamics.py:531-533).  losses_out: device float[3] = mse, back_mse, recon. */
typedef struct cadm_train_hparams {
    float learning_rate;          /* 1e-3 */
    float beta1, beta2, epsilon;  /* 0.9, 0.999, 1e-8 */
    float back_coeff;             /* dynamics.py:53 */
    float weight_decay_coeff;     /* dynamics.py:45 */
    float weight_decays[CADM_MAX_HIDDEN_LAYERS + 1];      /* hidden_i ..., last = both heads (core/utils.py:319,328,334) */
    float context_weight_decays[CADM_MAX_CP_LAYERS + 1];  /* cp_hidden_i ..., last = cp_output (core/utils.py:601,610) */
} cadm_train_hparams;
int cadm_train_configure(cadm_ctx* ctx, const cadm_train_hparams* hp, int max_batch);
int cadm_train_step(cadm_ctx* ctx, const float* obs, const float* act, const float* delta,
                    const float* obs_next, const float* back_delta, const float* cp_obs,
                    const float* cp_act, int B, int train, float* losses_out, void* stream);
/* The same step on rows of a windowed dataset that stays on the device -- what `fit` (dynamics.py:382-569) feeds after
 * `_preprocess_inputs` (:676-696) without materialising the exploded rows: per-step tensors are [N, F, .] (obs, act,
 * delta, obs_next, back_delta), history tensors [N, .] (cp_obs, cp_act); training row rid is window row_w[rid] at future
 * offset row_f[rid]; the batch is idx[e * idx_ld + b], b < B (row ids, int64): a column slice of the [E, n_train] bootstrap
 * matrix needs no copy. */
int cadm_train_step_rows(cadm_ctx* ctx, const float* ds_obs, const float* ds_act, const float* ds_delta,
                         const float* ds_obs_next, const float* ds_back_delta, const float* ds_cp_obs,
                         const float* ds_cp_act, int F, const long long* row_w, const long long* row_f,
                         const long long* idx, long long idx_ld, int B, int train, float* losses_out, void* stream);
/* One-step prediction heads of every member on an [E,B,.] batch: normalised mean mu [E,B,D] and (optional,
 * probabilistic models) soft-clamped log-variance [E,B,D] -- the vanilla reference's `_get_pred`
 * (mlp_ensemble_cem_dynamics.py:185-189 -> [mlp.mu, mlp.logvar]); backs the public predict(). */
int cadm_predict(cadm_ctx* ctx, const float* obs, const float* act, const float* cp_obs, const float* cp_act,
                 int B, float* mu_out, float* logvar_out, void* stream);
/* Reset Adam moments / step count (a fresh tf.global_variables_initializer()). */
int cadm_train_reset(cadm_ctx* ctx, void* stream);

/* Caller-side planner state on the device (no host round trips between env steps):
 * cadm_warm_start_shift: the samplers' CEM warm start (cadm/samplers/sampler.py:118-120):
 *   prev_sol[:, :-1] = plan[:, 1:]; prev_sol[:, -1] = 0; action = plan[:, 0]     (plan/prev_sol [m,H,A], action [m,A])
 * cadm_history_update: the history ring buffer behind cp_obs / cp_act (sampler.py:165-178,193-202):
 *   per env: entry = (state_diff ? next_obs - obs : obs, action) written at slot count (< Hh) or, once full,
 *   after shifting the window left by one entry; count += 1; done[mi] != 0 instead zeroes the window, the count
 *   and (if given) that env's prev_sol (reset_cem).  done may be NULL.  action is the [m,A] vector fed to the
 *   model (one-hot for discrete envs, sampler.py:148-149). */
int cadm_warm_start_shift(cadm_ctx* ctx, const float* plan, int m, float* prev_sol_io, float* action_out, void* stream);
int cadm_history_update(cadm_ctx* ctx, const float* obs, const float* next_obs, const float* action,
                        const int32_t* done, int m, int state_diff, int32_t* counts_io, float* hist_obs_io,
                        float* hist_act_io, float* prev_sol_io, void* stream);

/* Training-set builder of the context model: device twin of the `context` branch of
 * ModelSampleProcessor.process_samples (cadm/samplers/model_sample_processor.py:58-100).  All paths' steps are concatenated:
 * obs [T,D], act [T,A], cp_obs [T,Dh], cp_act [T,Ah] of 4- or 8-byte elements (elem_bytes; float32 or the reference's
 * float64 -- the kernel only moves words, results are bit-exact); path_off [P+1] = first step of every path (int32);
 * a path of len steps yields n = max(len, F+1) - 1 rows (short paths are zero-padded, :62-68); row_path / row_step [N] name
 * the path and step of every output row (N = sum of n).  Writes concat_obs / concat_next_obs [N,F*D], concat_act [N,F*A],
 * concat_bool [N,F] (1.0 / 0.0 of the element type, including the reference's "row 0 of every path is masked" quirk,
 * :85-86) and the rows' history windows cp_obs_out [N,Dh], cp_act_out [N,Ah].  Needs no ctx; asynchronous on `stream`. */
int cadm_build_windows(const void* obs, const void* act, const void* cp_obs, const void* cp_act, int elem_bytes, int D, int A,
                       int Dh, int Ah, const int32_t* path_off, const int32_t* row_path, const int32_t* row_step, int N, int F,
                       void* concat_obs, void* concat_act, void* concat_next_obs, void* concat_bool, void* cp_obs_out,
                       void* cp_act_out, void* stream);

/* Open-loop prediction error along the horizon: how far along the planner's rollouts the ensemble's trajectories still resemble
 * held-out data (the planner scores candidates on n_forwards-step rollouts; training and validation see one step).
 *
 * cadm_horizon_error: the statistics of trajectories against truth, on the device.  Needs no ctx; asynchronous on `stream`.
 *   traj   [F,m,1,p,D]  the layout of cadm_rollout_returns' traj_out (m windows, one candidate each)
 *   truth  [m,F,D] read in place, `truth_row_stride` floats between windows (a slice of the dataset's obs_next: F * D)
 *   mask   [m,F]   future_bool as float32 (non-zero = recorded step)
 *   E              p % E == 0; particle j belongs to member j / (p / E), as in the rollout
 * Step h of window i is VALID iff mask[i, 0..h] are all non-zero (a hole invalidates everything behind it).  A valid (window, step)
 * with a non-finite value among its p * D trajectory values is left out of every sum and counted in diverged[h] instead.  Over the
 * rest, fp32 SUMS (the caller divides by count):
 *   se_out [F,D]           sum of (mean over the p particles - truth)^2
 *   spread_out [F,D]       sum of the biased variance over the p particles
 *   se_member_out [E,F,D]  sum of (mean over member e's p / E particles - truth)^2
 *   count_out, diverged_out [F] int32
 * Reduction contract: no floating-point atomics.  Stage 1 (every call) writes one partial per block of 64 consecutive windows and
 * step into `partials` -- block b = windows [64 b, 64 b + 64) of the GLOBAL index window0 + i, window0 % 64 == 0 -- with a summation
 * order inside the block that depends on (p, E, D) only.  Stage 2 (`finalize` != 0) adds the partials of blocks 0 .. (window0 + m
 * + 63) / 64 - 1, i.e. all blocks written so far, in block order into the outputs.  Results are bit-identical run to run and do not
 * depend on how the windows were cut into calls.  `partials`: partials_blocks * F * ((2 + E) * D + 2) 4-byte words.
 * All argument checks run before any HIP call: null pointers, F, m, p, D >= 1, p % E == 0, window0 % 64 == 0, D <= 64,
 * D * (p + E + 2) * 4 bytes within one LDS tile (48 KiB), the blocks within partials_blocks. */
int cadm_horizon_error(const float* traj, const float* truth, long long truth_row_stride, const float* mask, int m, int F, int p,
                       int E, int D, long long window0, float* partials, long long partials_blocks, float* se_out,
                       float* spread_out, float* se_member_out, int32_t* count_out, int32_t* diverged_out, int finalize,
                       void* stream);
/* The same statistics for the ctx's model on a windowed dataset that is resident on the device (what `fit` uploads): ds_obs /
 * ds_obs_next [N,F,D], ds_act [N,F,A], ds_cp_obs [N,D*Hh], ds_cp_act [N,A*Hh] (NULL when C == 0), future_bool [N,F] float32.
 * Per chunk of `chunk` windows (a multiple of 64): the start states ds_obs[:,0,:] are gathered, the context encoder runs on the
 * chunk's histories, ONE rollout of F steps replays the recorded actions (every window is an env with one candidate; F <=
 * cfg.horizon, else CADM_EINVAL; the rollout runs F steps, not cfg.horizon), and stage 1 of cadm_horizon_error reduces its
 * trajectories; stage 2 runs after the last chunk.  Everything is enqueued on `stream`; nothing is copied to the host.
 * The rows are the rows the PLANNER scores: actions normalised as in planning and training, context laid out per the ctx's
 * reference_quirks as at CEM iteration 0 (particle j of member j / (p / E) reads encoder j % E with quirks on), noise per the
 * ctx's `deterministic` flag.  eps: injected N(0,1) [F,N,1,p,D], or NULL to draw from Philox keyed (seed, call); drawn noise is
 * keyed by a row's position inside its chunk and the chunk's index, so with drawn noise the result depends on `chunk` (and on
 * nothing else); with injected noise or a deterministic model it does not.  CADM_ENV_SPEC ctxs need their rollout module registered.
 * workspace: device scratch of cadm_eval_workspace_bytes(ctx, N, F, chunk) bytes (0 for bad arguments). */
size_t cadm_eval_workspace_bytes(cadm_ctx* ctx, int N, int F, int chunk);
int cadm_eval_horizon(cadm_ctx* ctx, const float* ds_obs, const float* ds_act, const float* ds_obs_next, const float* ds_cp_obs,
                      const float* ds_cp_act, const float* future_bool, int N, int F, int chunk, uint32_t seed, uint32_t call,
                      const float* eps, void* workspace, float* se_out, float* spread_out, float* se_member_out,
                      int32_t* count_out, int32_t* diverged_out, void* stream);

/* Calibration of the predictive distribution (no reference twin): are the particles the planner scores a calibrated sample of where
 * the system went?  The inputs of cadm_horizon_error -- traj [F,m,1,p,D], truth with a row stride, mask [m,F], p % E == 0 -- and its
 * rule for which (window, step) pairs count; count_out / diverged_out equal cadm_horizon_error's on the same inputs.  Per counted
 * pair and dim d, with particles x_0 .. x_{p-1}, truth y, every comparison in float32 (cadm_calibration_out, device pointers):
 *   rank_hist [F,D,p+1] int32           += 1 at r = #{j : x_j < y}
 *   rank_hist_member [E,F,D,p/E+1] int32   the same over each member's own p / E particles
 *   ties [F,D] int32                    += 1 where some x_j == y
 *   degenerate [F,D] int32              += 1 where the biased particle variance v is exactly 0; left out of z2 and nll
 *   crps [F,D] fp32 sum                 (1/p) sum_j |x_j - y| - (1/(2 p^2)) sum_j sum_k |x_j - x_k|, formed per window, then summed
 *   z2 [F,D] fp32 sum                   (xbar - y)^2 / v
 *   nll [F,D] fp32 sum                  0.5 (log 2 pi + log v + (xbar - y)^2 / v)
 *   count, diverged [F] int32           as cadm_horizon_error
 * xbar and v are formed as cadm_horizon_error forms them: v is the per-window term of its spread_out.  Sums and counts; the caller divides.
 * Reduction contract: the float sums follow cadm_horizon_error's (stage 1 per block of 64 windows of the GLOBAL index window0 + i,
 * window0 % 64 == 0; stage 2 when `finalize` != 0 over all blocks written so far; no floating-point atomics; the same bits run to
 * run and however the windows are cut into calls).  `partials`: partials_blocks * F * 3 * D floats.  The integers are exact in any
 * order: every call ADDS to them (integer atomics), and the call with window0 == 0 clears them first -- so every pointer of `out` is
 * required in every call, and the calls of one evaluation share one `out`.
 * All argument checks run before any HIP call: null pointers, F, m, p, D >= 1, p % E == 0, window0 % 64 == 0, D <= 64, F <= 65535,
 * one window's tile, float slots and the histograms (4 D (p + 3) + D (2 p + E + 9) + 40 bytes) within 48 KiB, the blocks within
 * partials_blocks. */
typedef struct cadm_calibration_out {
    int32_t *rank_hist, *rank_hist_member, *ties, *degenerate;
    float *crps, *z2, *nll;
    int32_t *count, *diverged;
} cadm_calibration_out;
int cadm_calibration_stats(const float* traj, const float* truth, long long truth_row_stride, const float* mask, int m, int F, int p,
                           int E, int D, long long window0, float* partials, long long partials_blocks,
                           const cadm_calibration_out* out, int finalize, void* stream);
/* The same statistics for the ctx's model on a device-resident windowed dataset: cadm_eval_horizon's arguments, chunk loop, rollout
 * rows and noise keys (with the same (seed, call) the two see the same trajectories), with cadm_calibration_stats as the reduction.
 * workspace: cadm_eval_calibration_workspace_bytes(ctx, N, F, chunk) bytes (0 for bad arguments). */
size_t cadm_eval_calibration_workspace_bytes(cadm_ctx* ctx, int N, int F, int chunk);
int cadm_eval_calibration(cadm_ctx* ctx, const float* ds_obs, const float* ds_act, const float* ds_obs_next, const float* ds_cp_obs,
                          const float* ds_cp_act, const float* future_bool, int N, int F, int chunk, uint32_t seed, uint32_t call,
                          const float* eps, void* workspace, const cadm_calibration_out* out, void* stream);

/* Forecast of a plan (no reference twin, OPT-IN): what the ensemble predicts under given action sequences, step by step, and how
 * sure it is -- the trajectories of one rollout reduced on the device.  The rollout kernels and the planner loops are untouched.
 *
 * cadm_forecast_stats: the statistics of recorded trajectories.  The ctx supplies D, A and the reward closure; nothing of its model.
 *   traj     [H,m,n,p,D]  post-step states: the layout of cadm_rollout_returns' traj_out; H >= 1 may be below the ctx's horizon
 *   obs      [m,D]        start state
 *   actions  [m,n,H,A]    raw, as the rollout takes them (the same H)
 *   p, E                  p % E == 0; particle j belongs to member j / (p / E), as in the rollout
 *   band_k                1 .. p
 * Outputs (cadm_forecast_out; every pointer but rollout_returns is required), per sequence (mi, ni) and step t:
 *   mean [m,n,H,D]           over the p particles
 *   member_mean [E,m,n,H,D]  over a member's p / E particles
 *   var_total [m,n,H,D]      biased variance over the particles
 *   var_epistemic [m,n,H,D]  biased variance of the E member means: what the members disagree about
 *   var_aleatoric [m,n,H,D]  mean over the members of the biased variance inside a member; total = epistemic + aleatoric
 *   lo, hi [m,n,H,D]         the band_k-th smallest / band_k-th largest particle value (order statistics, no interpolation; 1: min, max)
 *   reward_mean, reward_var [m,n,H], reward_member [E,m,n,H]   the same mean / biased variance / member means of the step reward
 *   returns [m,n,p]          per particle, its step rewards added in step order
 *   diverged_step [m,n]      int32: the first t at which any of the sequence's p * D values is non-finite, H if there is none
 * VARIANCES, not standard deviations.  Means and variances are formed relative to particle 0: particles that agree give exactly their
 * value as every mean and exactly 0 as every variance.  The step reward of particle j at step t reads the pre-step state (obs at
 * t = 0, else traj[t-1]), the post-step state traj[t] and the raw action: for the built-in continuous kinds the pair parts the
 * rollout adds, summed in ascending dim-pair order; for CADM_ENV_SPEC the ctx's cadm_env_spec evaluated at run time as
 * ((pre-step terms of the first term's dim pair, in order) - ctrl_cost sum(a^2)) + bonus, then the other terms in declaration order.
 * Divergence: every statistic of a sequence at t >= its diverged_step is NaN, and so are its returns; other sequences are unaffected.
 * It is read off `traj` alone: a non-finite `obs` leaves diverged_step as it is and shows as non-finite step-0 rewards and returns.
 * A member of one particle (p == E) has that particle's value, bit for bit, as its member_mean / reward_member.
 * Every sum is one thread's chain in a fixed order (csrc/forecast.hip, "Reduction contract"); no floating-point atomics: the same
 * bits run to run, and per sequence whatever m and n.
 * Refusals, before any HIP call: CADM_EINVAL for a null pointer, a discrete ctx (cartpole; the RS planner returns no plan), m, n, H,
 * p < 1, p % E != 0, band_k outside 1 .. p, and a p * D whose two LDS tiles and accumulators (8 p D + 8 p + 40 bytes at most) exceed
 * 48 KiB; CADM_ESTATE for a CADM_ENV_SPEC ctx before cadm_set_env_spec. */
typedef struct cadm_forecast_out {
    float *mean, *member_mean, *var_total, *var_epistemic, *var_aleatoric, *lo, *hi;
    float *reward_mean, *reward_var, *reward_member, *returns;
    int32_t* diverged_step;
    float* rollout_returns;   /* cadm_plan_forecast only: [m,n,p], the rollout's own returns_rows */
} cadm_forecast_out;
int cadm_forecast_stats(cadm_ctx* ctx, const float* traj, const float* obs, const float* actions, int m, int n, int H, int p, int E,
                        int band_k, const cadm_forecast_out* out, void* stream);
/* The forecast of the ctx's model for n given action sequences per env: the context encoder as cadm_cem_plan runs it (C > 0), ONE
 * rollout of m envs x n sequences over the ctx's full horizon that records its trajectories (n_local = n_global = n, cand_offset 0),
 * and cadm_forecast_stats with the ctx's p and E.  obs [m,D], cp_obs / cp_act as cadm_cem_plan, actions [m,n,H,A] raw.
 * Noise: eps [H,m,n,p,D] injected N(0,1), or NULL to draw from Philox keyed (seed, call) (a deterministic ctx reads neither).  The
 * rollout's iteration word is the constant 0xFC0000 (16515072): even, so the context layout is iteration 0's, and beyond every
 * planner loop's iterations 0 .. num_cem_iters - 1 (a ctx whose num_cem_iters exceeds it is refused): a forecast never repeats the
 * noise the planner drew for the same (seed, call).  out->rollout_returns receives the rollout's own returns_rows: the forecast's
 * returns account for the return the planner scores, up to the order of the additions.
 * A sharded ctx runs it unsharded on every rank; there is no collective.  Refusals: those of cadm_forecast_stats and of
 * cadm_rollout_returns.  workspace: cadm_forecast_workspace_bytes(ctx, m, n) bytes (0 for bad arguments).  Everything is enqueued
 * on `stream`. */
size_t cadm_forecast_workspace_bytes(cadm_ctx* ctx, int m, int n);
int cadm_plan_forecast(cadm_ctx* ctx, const float* obs, const float* cp_obs, const float* cp_act, const float* actions, const float* eps,
                       int m, int n, int band_k, uint32_t seed, uint32_t call, void* workspace, const cadm_forecast_out* out,
                       void* stream);

/* Multi-GPU planning: candidates shard contiguously over the ranks of an RCCL communicator owned by the
 * ctx (one process per GPU).  The reference is single-device (cadm/trainers/mb_trainer.py:103-107); this
 * adds exactly one collective per CEM iteration -- ncclAllGather of the per-candidate returns
 * ([m, n/G] floats per rank) -- between core/utils.py:474 and :475.  RCCL is dlopen'ed on first use.
 *   cadm_dist_unique_id  rank 0: fill a 128-byte ncclUniqueId, to be broadcast by the host to every rank
 *   cadm_dist_init       every rank: ncclCommInitRank on the ctx's device
 * Once initialised, cadm_cem_plan / cadm_rs_plan take n = GLOBAL candidate count (divisible by nranks),
 * roll out candidates [rank*n/G, (rank+1)*n/G) and return the identical plan on every rank.
 * cadm_cem_plan: a rank draws only its own candidates (cadm_sample_actions_shard; the draws are keyed by the global
 * element index) and the refit regenerates the elite sequences (cadm_cem_refit_regen) instead of reading them.  Every
 * rank's payload carries one more float: a checksum word of its replicated inputs (obs, cp_obs, cp_act, mean, var).
 * The refit compares the ranks' words; on a mismatch -- the ranks were fed different inputs -- the plan is NaN on EVERY
 * rank and a flag is raised (cadm_dist_mismatch; a staged call also writes it into m words behind its completion flags).  The
 * call still returns CADM_OK; the Python class raises RuntimeError on the flag. */
int cadm_dist_unique_id(char out_id[128]);
int cadm_dist_init(cadm_ctx* ctx, const char id[128], int nranks, int rank);
int cadm_dist_destroy(cadm_ctx* ctx);
/* The same sharded planner over a collective the HOST supplies (any torch.distributed backend, MPI, ...): every rank registers an
 * all-gather `fn(user, send, recv, count, stream)` -- [count] floats at device pointer `send` of every rank -> [nranks * count] floats at
 * device pointer `recv`, rank-major, valid for work enqueued on `stream` after fn returns; 0 = success.  cadm_cem_plan / cadm_rs_plan
 * then run EXACTLY the loop of the RCCL path (same shard arithmetic, same payload with the trailing checksum word, same regenerating
 * refit) and call fn where they would call ncclAllGather: there is one sharded implementation, the collective is a plug.  fn is called
 * on the thread that called the planner, between kernel enqueues (it may synchronise `stream`; both pointers lie inside the `workspace`
 * argument of the planner call). */
typedef int (*cadm_allgather_fn)(void* user, const void* send, void* recv, size_t count, void* stream);
int cadm_dist_init_external(cadm_ctx* ctx, int nranks, int rank, cadm_allgather_fn fn, void* user);
/* Did the ranks of the last sharded cadm_cem_plan feed different replicated inputs (obs, history, warm start)?  *mismatch_out = 1 / 0;
 * reading resets the flag.  Synchronises `stream`.  On a mismatch the plan of that call is NaN on every rank; a NaN plan WITHOUT this
 * flag is what a single-rank call returns for the same inputs (a non-finite observation, a diverged model).  Inputs are compared by
 * value: -0.0 equals +0.0 and every NaN equals every NaN. */
int cadm_dist_mismatch(cadm_ctx* ctx, int* mismatch_out, void* stream);
/* (nranks, rank) as RCCL reports them for the ctx's communicator (ncclCommCount / ncclCommUserRank); (1, 0) without one. */
int cadm_dist_info(cadm_ctx* ctx, int* nranks_out, int* rank_out);

/* In-library timing of the dominant kernel (the rollout): when enabled, every
 * cadm_rollout_returns launch is bracketed by hipEvents on the launch stream.
 * cadm_profile_read synchronises, returns the summed elapsed milliseconds and launch count
 * since the last read, and resets both. */
int cadm_profile_enable(cadm_ctx* ctx, int enable);
int cadm_profile_read(cadm_ctx* ctx, float* total_ms_out, int* launches_out);
/* Same for the sharded planner's collective: every ncclAllGather issued by cadm_cem_plan / cadm_rs_plan while profiling is
 * enabled is bracketed too; returns the summed milliseconds and the number of all-gathers since the last read. */
int cadm_profile_read_collective(cadm_ctx* ctx, float* total_ms_out, int* calls_out);
/* (Developer hooks -- comparison kernel, forced launch flavours, phase timing -- are NOT part of this interface and not
 * in libcadm_hip.so: cadm_amd/csrc/dev/dev_api.h, libcadm_hip_dev.so.  The product reads no environment variable.) */

#ifdef __cplusplus
}
#endif
#endif /* CADM_HIP_H */
