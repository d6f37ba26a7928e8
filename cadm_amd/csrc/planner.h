// Internal header of the planner's host side (capi.hip, plan.hip, cem.hip, icem.hip, mppi.hip, score.hip, context.hip, horizon.hip, calibration.hip, forecast.hip, constrain.hip, knots.hip, tracking.hip, actuator.hip, uncertainty.hip, value.hip, reward.hip, policy.hip, policy_gauss.hip, policy_logp.hip, critic.hip, discount.hip, imagine.hip, imagine_targets.hip): the loops' types, ONE declaration
// of every launcher another file calls, and the helpers the loops share.  Not part of a JIT rollout module (rollout_jit.hip sees common.h only).
#pragma once
#include "common.h"

// Sharded planner (plan.hip: cem_plan_impl): what the refit needs to REGENERATE the elites' action sequences by global
// candidate id instead of reading them (a rank draws only its own shard), and to check the input checksums at the end of every rank's
// all-gather payload.
struct RefitRegen {
    int on;                    // 1: elite actions are drawn again from (seed, call, it); the actions pointer may be null
    uint32_t seed, call; int it;
    float lb, ub;
    int gstride;               // floats per rank in the gathered buffer (0: m * n_local); m * n_local + 1 with the trailing checksum
    int my_rank;               // >= 0: compare every rank's checksum with this rank's; mismatch -> NaN plan
    unsigned* mismatch;        // device word raised on a checksum mismatch (ctx->dist_flag), may be null
    unsigned* mismatch_host;   // pinned host words [m] behind the completion flags of a staged call, may be null
};
// completion flags of a staged planner call: [m] words in pinned host memory, set to `val` by the refit that writes the plan (null: none)
struct PlanDone { unsigned* flags = nullptr; unsigned val = 0; };
// Per-call inputs of a small planner call travel as KERNEL ARGUMENTS (cadm_cem_plan_staged, plan.hip): up to CADM_INGEST_MAX floats.
#define CADM_INGEST_MAX 960
struct IngestBlock { float v[CADM_INGEST_MAX]; };
// the fused head's copy of the block shares the 4 KB kernel-argument segment with the encoder's and the sampler's arguments: a smaller cap
// (blocks between the two caps take the plain ingest kernel + the unfused head)
#define CADM_HEAD_INGEST_MAX 896
struct HeadBlock { float v[CADM_HEAD_INGEST_MAX]; };
#define CADM_CONTEXT_BATCHED_MIN_ROWS 48    // histories per member from which the context encoder runs as a GEMM chain (context.hip)

// Views of a caller's workspace, taken in order, each start rounded up to 256 bytes.  base == null: only the running total is wanted.
struct Carver {
    char* base;
    size_t off = 0;
    template <class T> T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

// forecast.hip: the rollout of cadm_plan_forecast runs under this iteration word (include/cadm_hip.h).  Even: the context layout is
// iteration 0's.  The planner loops count 0 .. num_cem_iters - 1 (cadm_plan_forecast refuses a ctx whose loop could get here), so a
// forecast never repeats the noise a planner call drew for the same (seed, call).  (The word takes 24 bits of a Philox counter.)
#define CADM_FORECAST_IT 0xFC0000
// policy.hip: the one-step rollouts of cadm_policy_propose run under CADM_POLICY_IT + 2 t, t = 0 .. H - 2.  Even: the context layout is
// iteration 0's.  The range lies above every planner iteration and below the forecast's word (cadm_policy_propose refuses a ctx whose
// num_cem_iters or horizon could break that), so a roll never repeats the noise of a planner call or a forecast of the same (seed, call).
#define CADM_POLICY_IT 0xFA0000
// imagine.hip: the one-step rollouts of cadm_imagine run under CADM_IMAGINE_IT + 2 t, t = 0 .. k - 1.  Even: the context layout is
// iteration 0's.  The range lies above every planner iteration and below the proposal roll's words (cadm_imagine refuses a ctx whose
// num_cem_iters, or a k whose last word, would leave it), so imagined rollouts never repeat the noise of a plan, a roll or a forecast.
#define CADM_IMAGINE_IT 0xF00000

// cem.hip
int cadm_launch_clip(const float* in, float* out, int total, float lo, float hi, int do_clip, hipStream_t s);
int cadm_launch_refit(cadm_ctx* ctx, const float* cand_returns, const float* rows, int G, int n_local, const float* actions,
                      int m, const float* mean_in, const float* var_in, float* mean_out, float* var_out, int32_t* elites_out,
                      float* plan_out, hipStream_t stream, const RefitRegen* regen = nullptr, PlanDone done = {});
int cadm_launch_refit_sample(cadm_ctx* ctx, const float* cand_returns, const float* rows, int G, int n_local, float* actions, int m,
                             const float* mean_in, const float* var_in, float* mean_out, float* var_out, uint32_t seed, uint32_t call,
                             int next_it, hipStream_t stream);
bool cadm_refit_sample_ok(const cadm_ctx* ctx, int n);
int cadm_launch_particle_mean_tail(cadm_ctx* ctx, const float* returns_rows, int m, int n_local, float* cand_returns, const unsigned* tail,
                                   hipStream_t stream);
int cadm_launch_input_checksum(cadm_ctx* ctx, const float* obs, const float* cp_obs, const float* cp_act, const float* mean, const float* var,
                               int m, unsigned* out, hipStream_t s);
// The head of a staged planner call as ONE launch (context.hip: plan_head_kernel): unpack the ingest block into the device block, the
// context encoder on the block's history (C > 0), and the candidates of CEM iteration 0.  off[5] = float offsets of obs, cp_obs,
// cp_act, init_mean, init_var inside the block (-1: absent).
int cadm_launch_plan_head(cadm_ctx* ctx, const float* host_block, int nfloats, const int32_t off[5], float* dev_block, int m, int n,
                          uint32_t seed, uint32_t call, float* ctx_out, float* actions_out, hipStream_t s);
int cadm_rollout_builtin_env(cadm_ctx* ctx);     // rollout.hip
// mppi.hip: the softmax-weighted refit.  scratch: cadm_mppi_scratch_floats(ctx, m, n) floats, 16-byte aligned; mean_in / var_in may
// alias mean_out / var_out.  cadm_mppi_check: the refusals of the update (temperature, discrete, sharded), before any HIP call.
size_t cadm_mppi_scratch_floats(const cadm_ctx* ctx, int m, int n);
int cadm_mppi_check(const cadm_ctx* ctx, int m, float temperature, const char* who);
int cadm_launch_mppi_refit(cadm_ctx* ctx, const float* cand_returns, const float* actions, int m, int n, float temperature, int relative,
                           const float* mean_in, const float* var_in, float* mean_out, float* var_out, float* plan_out, float* scratch,
                           hipStream_t s);
// score.hip: the refusals of a candidate score (unknown mode, kappa not finite, cvar k outside [1, p]), before any HIP call; null = the mean
int cadm_score_check(const cadm_ctx* ctx, const cadm_score_params* score, const char* who);
// constrain.hip: the refusals of a constraint set (count, dims, bounds, mode, weight, a discrete / sharded ctx, a spec ctx without its spec in
// terminate mode, a D whose tiles exceed the kernel's LDS), before any HIP call
int cadm_constraint_check(const cadm_ctx* ctx, const cadm_constraint_params* c, const char* who);
// knots.hip: the refusals of a knot grid (spacing < 1, an unknown interp), before any HIP call; and the in-place shaping of seqs [m, n, H, A]
// onto the grid (phase [m] int32 on the device, or null = 0), n the PACKED candidate count of the buffer
int cadm_knot_check(const cadm_knot_params* knots, const char* who);
int cadm_launch_shape_actions(cadm_ctx* ctx, const cadm_knot_params* knots, const int32_t* phase, int m, int n, float* seqs, hipStream_t s);
// tracking.hip: the refusals of a set of tracking terms and its targets (count, dims, kinds, weights, Huber deltas, T < 1, null targets, a
// discrete / sharded ctx, a D whose tile exceeds the kernel's LDS), before any HIP call
int cadm_track_check(const cadm_ctx* ctx, const cadm_track_params* track, const float* targets, int T, const char* who);
// actuator.hip: the refusals of an actuator model (delay outside [0, H), a limit <= 0 or NaN, a cost negative or not finite, arrays built
// for another A, A beyond their capacity, a discrete / sharded ctx), before any HIP call; the in-place pass over seqs [m, n, H, A] (n the
// PACKED candidate count; prev [m, A] / prefix [m, delay, A] on the device or null = NaN; cost_out [m, n] or null); cand -= cost; and the
// step of episode time behind a plan [m, H, A]: prev <- plan[:, 0], prefix[:, j] <- plan[:, 1 + j]
int cadm_actuator_check(const cadm_ctx* ctx, const cadm_actuator_params* act, const char* who);
int cadm_launch_actuate(cadm_ctx* ctx, const cadm_actuator_params* act, const float* prev, const float* prefix, int m, int n, float* seqs,
                        float* cost_out, hipStream_t s);
int cadm_launch_actuator_sub(float* cand, const float* cost, size_t total, hipStream_t s);
int cadm_launch_actuator_advance(cadm_ctx* ctx, const cadm_actuator_params* act, const float* plan, float* prev, float* prefix, int m,
                                 hipStream_t s);
// uncertainty.hip: the refusals of an uncertainty term (an unknown kind or form, a lambda that is not finite, a cap <= 0 or NaN, a weight
// negative or not finite, every weight 0, weights built for another D, D beyond their capacity, a discrete / sharded ctx, a p * D tile beyond
// the kernel's LDS), before any HIP call; and the two launches behind a rollout's traj [H, m, n, p, D] (n the PACKED candidate count; first
// [m, n, p] or null): u into step [m, n, H], the cost of the counted steps into cost [m, n], and with cand [m, n]: cand -= lambda * cost
int cadm_uncertainty_check(const cadm_ctx* ctx, const cadm_uncertainty_params* unc, const char* who);
int cadm_launch_uncertainty(cadm_ctx* ctx, const cadm_uncertainty_params* unc, const float* traj, const int32_t* first, int m, int n,
                            float* step, float* cost, float* cand, hipStream_t s);
// value.hip: the refusals of a terminal value (null parameters, a layer count outside 0 .. 4, a width outside 1 .. 512, an unknown
// activation, a weight that is not finite, D beyond the net's input dims, a discrete / sharded ctx, activation tiles beyond the LDS; no
// registered net: CADM_ESTATE; parameters that do not describe the registered net), before any HIP call; and the launch behind a rollout's
// traj [H, m, n, p, D] (n the PACKED candidate count; first [m, n, p] or null): rows[q] += weight * V(traj[H - 1, q]) in place
int cadm_value_plan_check(const cadm_ctx* ctx, const cadm_value_params* value, const char* who);
int cadm_launch_value(cadm_ctx* ctx, const cadm_value_params* value, const float* traj, const int32_t* first, int m, int n, float* rows,
                      hipStream_t s);
// reward.hip: the refusals of a learned reward (null parameters, a layer count outside 0 .. 4, a width outside 1 .. 512, an unknown
// activation or inputs, a weight that is not finite, K beyond CADM_MAX_REWARD_DIMS, a discrete / sharded ctx, activation tiles beyond the
// LDS; no registered net: CADM_ESTATE; parameters that do not describe the registered net), before any HIP call; and the two launches
// behind a rollout's traj [H, m, n, p, D] (n the PACKED candidate count; first [m, n, p] or null): r_step [H, m, n, p] = R of every
// (step, row), NaN where not counted, then rows[q] += weight * (the sum of the counted steps in ascending t) in place
int cadm_reward_plan_check(const cadm_ctx* ctx, const cadm_reward_params* reward, const char* who);
int cadm_launch_reward(cadm_ctx* ctx, const cadm_reward_params* reward, const float* traj, const float* obs, const float* actions,
                       const int32_t* first, int m, int n, float* rows, float* r_step, hipStream_t s);
// policy.hip: the refusals of a policy prior (null parameters, a layer count outside 0 .. 4, a width outside 1 .. 512, an unknown
// activation or squash, n_samples < 1, a noise_std negative or not finite, D or A beyond the net's dims, a discrete / sharded ctx,
// activation tiles beyond the LDS, a num_cem_iters or horizon that reaches the roll's iteration words; no registered net: CADM_ESTATE;
// parameters that do not describe the registered net), before any HIP call; and the roll itself: seqs_out [m, P, H, A], states_out
// [H, m, P, p, D] or null, workspace of cadm_policy_workspace_bytes(ctx, m, P)
int cadm_policy_plan_check(const cadm_ctx* ctx, const cadm_policy_params* policy, const char* who);
int cadm_launch_policy_propose(cadm_ctx* ctx, const cadm_policy_params* policy, const float* obs, const float* ctx_vec, int m, uint32_t seed,
                               uint32_t call, float* seqs_out, float* states_out, void* workspace, hipStream_t s, const char* who);
// policy.hip, for imagine.hip: ONE policy step of the registered net (CADM_ESTATE without one) on states x [total, D], one state per row:
// a1 [total, A] = the squashed action, with noise_std > 0 perturbed on EVERY row by noise_std * xi under the given stream word
// (counter (row, t, g, stream)), clipped.  noise_std == 0: the launch of cadm_policy_eval.
int cadm_launch_policy_step(cadm_ctx* ctx, const float* x, size_t total, int t, float noise_std, uint32_t seed, uint32_t call,
                            uint32_t stream_word, float* a1, hipStream_t s, const char* who);
// policy.hip, for critic.hip and imagine.hip: false while no policy net is registered; else `d` (or null) receives the net's half of a
// kernel's arguments (mlp_chain.h) and `squash` (or null) its squash
struct MlpDev;
bool cadm_policy_dev(const cadm_ctx* ctx, MlpDev* d, int* squash);
// policy.hip, for policy_gauss.hip: the refusals of a policy net's description alone (cadm_policy_plan_check's first half)
int cadm_policy_check(const cadm_ctx* ctx, const cadm_policy_params* policy, const char* who);
// policy_gauss.hip: the stochastic actor head on the registered net (include/cadm_hip.h, "Stochastic actor head").  For policy.hip:
// cadm_set_policy_net drops the head (the last hidden width may have changed); the packed copy stays allocated.  For imagine.hip: the
// refusals of a sampled step before any HIP call (no registered net, or no head on it: CADM_ESTATE; what cadm_policy_check refuses, lb >=
// ub, the kernel's LDS), and ONE sampling step on states x [total, D], one state per row, under counter (row, t, g,
// CADM_STREAM_POLICY_SAMPLE): a1 [total, A] the sampled action, logp [total] its log-density
void cadm_policy_head_drop(cadm_ctx* ctx);
int cadm_policy_gauss_check(const cadm_ctx* ctx, const char* who);
int cadm_launch_policy_gauss_step(cadm_ctx* ctx, const float* x, size_t total, int t, uint32_t seed, uint32_t call, float* a1, float* logp,
                                  hipStream_t s, const char* who);
// policy_gauss.hip, for policy.hip: proposals drawn from the head (cadm_set_policy_proposals; include/cadm_hip.h).  The refusals a plan
// check adds under CADM_PROPOSE_HEAD (a noise_std > 0, lb >= ub, the kernel's LDS; no head: CADM_ESTATE; CADM_OK under
// CADM_PROPOSE_NOISE), and ONE policy step of the roll with the head's draws: the arguments of policy.hip's own step launch
int cadm_policy_proposals_check(const cadm_ctx* ctx, const cadm_policy_params* policy, const char* who);
int cadm_launch_policy_gauss_roll(cadm_ctx* ctx, const float* obs, const float* x, int P, int p, int t, uint32_t seed, uint32_t call, float* seqs,
                                  float* a1, float* states, size_t total, hipStream_t s, const char* who);
// policy_gauss.hip, for policy_logp.hip: false while the registered net has no head; else the head's packed layer h_L -> A (mlp_chain.h's
// layout) and its description, each where asked for (null: not wanted)
bool cadm_policy_head_dev(const cadm_ctx* ctx, const float** W_ls, const float** b_ls, cadm_policy_head_params* prm);
// policy_logp.hip: the refusals of the actor's log-density as a term of the score (an unknown space, a weight that is not finite, what
// cadm_policy_gauss_check refuses, a head whose log_std_min < -10, activation tiles beyond the LDS; no registered net or no head on it:
// CADM_ESTATE), before any HIP call; and the two launches behind a rollout's traj [H, m, n, p, D] (n the PACKED candidate count; first
// [m, n, p] or null): step [H, m, n, p] = log pi(a_t | s_t) of every (step, row), NaN where not counted, then rows[q] += weight * (the
// sum of the counted steps in ascending t) in place
int cadm_policy_logp_plan_check(const cadm_ctx* ctx, const cadm_policy_logp_params* logp, const char* who);
int cadm_launch_policy_logp(cadm_ctx* ctx, const cadm_policy_logp_params* logp, const float* traj, const float* obs, const float* actions,
                            const int32_t* first, int m, int n, float* rows, float* step, hipStream_t s);
// critic.hip: the refusals of a terminal Q (null parameters, a layer count outside 0 .. 4, a width outside 1 .. 512, an unknown
// activation or reduce, a critic count outside 1 .. 5, a weight that is not finite, D or A beyond the nets' dims, a discrete / sharded
// ctx, the input tile and the activation tiles beyond the LDS; no registered critics or no registered policy net: CADM_ESTATE;
// parameters that do not describe the registered critics), before any HIP call; and the launch behind a rollout's traj [H, m, n, p, D]
// (n the PACKED candidate count; first [m, n, p] or null): rows[q] += weight * reduce_c Q_c(s, pi(s)), s = traj[H - 1, q], in place
int cadm_critic_plan_check(const cadm_ctx* ctx, const cadm_critic_params* critic, const char* who);
int cadm_launch_critic(cadm_ctx* ctx, const cadm_critic_params* critic, const float* traj, const int32_t* first, int m, int n, float* rows,
                       hipStream_t s);
// discount.hip: the refusals of a discount over the horizon (a discrete / sharded ctx, a D whose two tiles exceed the kernel's LDS, a spec
// ctx without its spec: CADM_ESTATE), before any HIP call; and the launch behind a rollout's traj [H, m, n, p, D] (n the PACKED candidate
// count) on a ctx whose table is set: rows_out[q] = sum_t disc[t] * r_t in ascending t (a NaN rows_in[q] stays), step_out [H, m, n, p] or
// null takes the undiscounted r_t.  The other stages read ctx->disc themselves: null = their undiscounted launch.
int cadm_discount_check(const cadm_ctx* ctx, const char* who);
int cadm_launch_discount(cadm_ctx* ctx, const float* traj, const float* obs, const float* actions, int m, int n, const float* rows_in,
                         float* rows_out, float* step_out, hipStream_t s);
// imagine.hip: branched one-step rollouts recorded as transitions (include/cadm_hip.h, "Imagined rollouts").  The refusals of the chain
// (k or branches < 1, a discrete / sharded ctx, a p * D tile beyond the select kernel's LDS, m * n * p rows beyond one rollout launch, a
// num_cem_iters or k that leaves the chain's iteration words, constraints that constrain.hip or weights that uncertainty.hip refuses),
// before any HIP call; and the chain itself over the buffer of cadm_imagine_workspace_bytes(ctx, m, n, k)
int cadm_imagine_check(const cadm_ctx* ctx, int m, int n, int k, const cadm_constraint_params* constraints,
                       const cadm_uncertainty_params* disagreement, const char* who);
// sampled: the buffer is cadm_imagine_sampled_workspace_bytes', and every step's action is the Gaussian head's draw with its logp
int cadm_launch_imagine(cadm_ctx* ctx, const float* obs, const float* ctx_vec, const float* actions, int m, int n, int k, float noise_std,
                        const cadm_constraint_params* constraints, const cadm_uncertainty_params* disagreement, uint32_t seed, uint32_t call,
                        void* buffer, hipStream_t s, const char* who, bool sampled = false);
// what the reference-path loops (plan.hip) answer on a discounted ctx: they sum the step rewards inside the rollout kernel
inline int cadm_refuse_discounted(const cadm_ctx* ctx, const char* who) {
    if (!ctx->disc) return CADM_OK;
    cadm_set_error("%s: a discount over the horizon is set (cadm_set_discount): this loop plans the undiscounted sum of the rollout kernel; "
                   "use the opt-in loop, or clear the discount", who);
    return CADM_ESTATE;
}
// value.hip, critic.hip: the weight of a terminal term on this ctx: weight * disc[H], one fp32 product on the host; without a discount the weight
inline float cadm_discounted_weight(const cadm_ctx* ctx, float weight) { return ctx->disc ? weight * ctx->disc_host[(size_t)ctx->H] : weight; }

// next start/stop event pair of a profiling list (grown on demand)
inline int cadm_prof_pair(std::vector<hipEvent_t>& ev, size_t& used, hipEvent_t* e0, hipEvent_t* e1) {
    if (used + 2 > ev.size()) {
        hipEvent_t a, b;
        CADM_CHECK_HIP(hipEventCreate(&a));
        CADM_CHECK_HIP(hipEventCreate(&b));
        ev.push_back(a);
        ev.push_back(b);
    }
    *e0 = ev[used];
    *e1 = ev[used + 1];
    used += 2;
    return CADM_OK;
}

inline int cadm_require_ready(cadm_ctx* ctx, const char* who) {
    if (!ctx->st.set) { cadm_set_error("%s: normalisation stats not set (call cadm_set_norm_stats)", who); return CADM_ESTATE; }
    if (!ctx->ff_maxlv || !ctx->ff_minlv) { cadm_set_error("%s: logvar bounds not set", who); return CADM_ESTATE; }
    return CADM_OK;
}
