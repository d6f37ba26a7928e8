// Policy prior of the opt-in planner loop (icem.hip): a caller-supplied actor pi, an MLP D -> h_1 -> .. -> h_L -> A, rolled through the
// ensemble so that its trajectories sit among the candidates of every CEM / MPPI iteration (LOOP, TD-MPC).  No reference twin: the
// reference's planner draws every candidate around a mean.  Two pieces: policy_step_kernel, which acts for P proposal sequences per env
// on their state estimates, and cadm_policy_propose, the serial chain  policy step -> one-step rollout -> policy step -> ..  over the
// horizon.  The rollout kernels are not touched: the roll calls cadm_launch_rollout with horizon 1 and the previous step's trajectory
// as the per-row start state.
//
// A "row" is one proposal sequence (env mi, sequence j), j < P.  Its state estimate is the mean over the sequence's p particles:
//   t = 0: obs[mi] itself;   t >= 1: s = x_0; s = s + x_1; .. ; s = s + x_{p-1} (float32 adds, ascending); mean = s / (float)p (IEEE)
// and its action, all in float32 (nothing fused but the MFMA's own multiply-add):
//   x_k = (mean_k - net_mean_k) * inv_std_k                one subtract, one multiply
//   a layer with K inputs:  acc = b_u;  for k = 0 .. K4-1 ascending: acc = fma(W[k][u], x_k, acc)      (mlp_chain.h, the value net's chain)
//   hidden: relu, tanhf or swish;  output z_d: linear, A units
//   CADM_POLICY_TANH: a_d = mid + half * tanhf(z_d)  (one multiply, one add);  CADM_POLICY_NONE: a_d = z_d
//   j >= 1 and noise_std > 0: a_d = a_d + noise_std * xi_d  (one multiply, one add);   a_d = fminf(fmaxf(a_d, lb), ub)
//   (PolicyArgs::all_rows, imagine.hip's steps only: j == 0 is perturbed too, and xi's stream word is PolicyArgs::stream)
// xi: Philox4x32-10 keyed (seed, call), counter (mi * P + j, t, g, CADM_STREAM_POLICY); one call serves dims 4 g .. 4 g + 3, words
// (0, 1) through Box-Muller to dims 4 g and 4 g + 1, words (2, 3) to 4 g + 2 and 4 g + 3 (u01 / box_muller of common.h, the Gaussian
// head's).  Sequence 0 never gets noise: the policy's own trajectory is always among the proposals.
// A row with a non-finite value in any particle of its state takes the fallback clip(0, lb, ub) in every dim: the sequence stays finite
// and loses on its own score.
// Mapping: value_kernel's (value.hip): a workgroup of 4 waves owns 16 * RT consecutive rows, activations resident in LDS as [unit][row],
// weights from the ctx-owned packed copy through a register ring; the output layer is one more layer with the identity activation, its
// A <= 64 sums in LDS, from where the epilogue squashes, perturbs, clips and stores.
// Reduction contract: a row's action is one column's chain in ascending k behind a sequential particle sum; no floating-point atomics;
// nothing depends on the grid, on RT, on m or P: the same bits run to run, wherever the row sits, from cadm_policy_eval as from the roll.
// The host path around the kernel (description checks, registration, row tiles, launch) is mlp_chain.h's; what stands below is what
// this net has of its own.
#include "mlp_chain.h"

namespace {

struct PolicyArgs {
    MlpDev net;                    // D -> h_1 .. h_L -> A
    const float* obs;              // [m, D]: the state of every row of env mi (t == 0), or null
    const float* x;                // [total, p, D]: the particle states of the rows (t >= 1; cadm_policy_eval: p = 1), or null
    int squash, P, p, t, H;        // (squash behind the pointers: mean, istd, obs and x stay adjacent, one scalar load)
    float lb, ub, mid, half, noise_std;
    uint32_t seed, call;
    float* seqs;                   // [total, H, A] or null: a_t goes to [q, t, :]
    float* a1;                     // [total, A]: a_t
    float* states;                 // [total, p, D] or null: the particle states that were read
    size_t total;
    int region0, region1;          // LDS floats of the two activation regions
    int all_rows;                  // 1: row j == 0 is perturbed like the others (imagine.hip); 0: sequence 0 never gets noise
    uint32_t stream;               // the stream word of xi: CADM_STREAM_POLICY for the proposals
};

template <int RT>
__global__ __launch_bounds__(MLP_THREADS) void policy_step_kernel(const PolicyArgs a) {
    extern __shared__ __attribute__((aligned(16))) float pol_smem[];
    constexpr int R = 16 * RT;
    float* reg0 = pol_smem;
    float* reg1 = reg0 + a.region0;
    int* bad = reinterpret_cast<int*>(reg1 + a.region1);         // [R] 1: a non-finite value in the row's state
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t q0 = (size_t)blockIdx.x * R;                    // (q0 < total: the grid is ceil(total / R))
    const int rows = a.total - q0 < (size_t)R ? (int)(a.total - q0) : R;
    if (tid < R) bad[tid] = 0;
    __syncthreads();
    // the input tile [k][row]: the state estimate, normalised on the way in; rows behind the batch and the k behind D are zeros
    const int D = a.net.dims[0], D4 = (D + 3) & ~3;
    for (int idx = tid; idx < R * D4; idx += MLP_THREADS) {
        const int row = idx / D4, k = idx - row * D4;
        float x = 0.0f;
        if (k < D && row < rows) {
            const size_t q = q0 + row;
            float est;
            bool nf;
            if (a.obs) {
                est = a.obs[(q / a.P) * D + k];
                nf = mlp_nonfinite(est);
                if (a.states)
                    for (int j = 0; j < a.p; ++j) a.states[(q * a.p + j) * D + k] = est;
            } else {
                const float* xp = a.x + q * a.p * D + k;
                float s = xp[0];
                nf = mlp_nonfinite(s);
                if (a.states) a.states[q * a.p * D + k] = s;
                for (int j = 1; j < a.p; ++j) {
                    const float v = xp[(size_t)j * D];
                    nf = nf || mlp_nonfinite(v);
                    if (a.states) a.states[(q * a.p + j) * D + k] = v;
                    s = __fadd_rn(s, v);
                }
                est = a.p > 1 ? __fdiv_rn(s, (float)a.p) : s;
            }
            if (nf) bad[row] = 1;                                // (every writer stores the same 1)
            x = (est - a.net.mean[k]) * a.net.istd[k];
        }
        reg0[k * R + mlp_swz<RT>(row, k)] = x;
    }
    __syncthreads();
    const float* xin = mlp_forward<RT>(a.net, false, reg0, reg1, reg0, nullptr, wave, lane);
    const int A = a.net.dims[a.net.nlayers];
    for (int idx = tid; idx < rows * A; idx += MLP_THREADS) {
        const int row = idx / A, d = idx - row * A;
        const size_t q = q0 + row;
        float v;
        if (bad[row]) {
            v = 0.0f;
        } else {
            v = mlp_squash(xin[d * R + mlp_swz<RT>(row, d)], a.squash, a.mid, a.half);
            if (a.noise_std > 0.0f && (a.all_rows || q % a.P != 0)) {
                uint32_t r[4];
                philox4x32_10((uint32_t)q, (uint32_t)a.t, (uint32_t)(d >> 2), a.stream, a.seed, a.call, r);
                float z0, z1;
                const int w = d & 2;
                box_muller(u01(r[w]), u01(r[w + 1]), z0, z1);
                v = __fadd_rn(v, __fmul_rn(a.noise_std, (d & 1) ? z1 : z0));
            }
        }
        v = fminf(fmaxf(v, a.lb), a.ub);
        if (a.seqs) a.seqs[(q * a.H + a.t) * A + d] = v;
        a.a1[q * A + d] = v;
    }
}

// LDS of a workgroup with RT row tiles: the two activation regions, the output layer's A sums in one of them, and the flags
size_t policy_lds_bytes(const int* dims, int nlayers, int RT, int* region0, int* region1) {
    return (mlp_region_floats(dims, nlayers + 1, RT, region0, region1) + 16 * (size_t)RT) * sizeof(float);
}

void policy_dims(const cadm_ctx* ctx, const cadm_policy_params* p, int* dims) { mlp_dims(mlp_shape(p), ctx->D, ctx->A, dims); }

struct PolicyWs { float *a1, *rows1, *cur, *next; };

size_t policy_carve(const cadm_ctx* ctx, int m, int P, char* base, PolicyWs* w) {
    Carver c{base};
    PolicyWs t{};
    t.a1 = c.take<float>((size_t)m * P * ctx->A);
    t.rows1 = c.take<float>((size_t)m * P * ctx->p);
    t.cur = c.take<float>((size_t)m * P * ctx->p * ctx->D);
    t.next = c.take<float>((size_t)m * P * ctx->p * ctx->D);
    if (w) *w = t;
    return c.off;
}

}  // namespace

// the ctx-owned packed copy of the registered net (n_samples and noise_std of its prm are not used: every call brings its own)
struct PolicyNet : MlpOwned<cadm_policy_params> {};

void cadm_policy_free(cadm_ctx* ctx) { mlp_free(ctx->policy); }

// false while no net is registered; else the registered net D -> h_1 .. h_L -> A as its half of a kernel's arguments and its squash,
// where asked for (critic.hip's actor reads both)
bool cadm_policy_dev(const cadm_ctx* ctx, MlpDev* d, int* squash) {
    if (!mlp_registered(ctx->policy)) return false;
    if (d) mlp_dev(*d, ctx->policy->net[0], mlp_shape(&ctx->policy->prm), ctx->D, ctx->A);
    if (squash) *squash = ctx->policy->prm.squash;
    return true;
}

// the refusals of a policy net's description, before any HIP call
int cadm_policy_check(const cadm_ctx* ctx, const cadm_policy_params* p, const char* who) {
    int rc;
    if ((rc = mlp_shape_check(mlp_shape(p), "policy", who))) return rc;
    CADM_REQUIRE(p->squash == CADM_POLICY_NONE || p->squash == CADM_POLICY_TANH, "%s: unknown policy squash %d", who, p->squash);
    CADM_REQUIRE(p->n_samples >= 1, "%s: n_samples must be >= 1 (got %d)", who, p->n_samples);
    CADM_REQUIRE(isfinite(p->noise_std) && p->noise_std >= 0.0f, "%s: the policy noise_std %g is negative or not finite", who,
                 (double)p->noise_std);
    CADM_REQUIRE(ctx->D <= CADM_MAX_VALUE_DIMS, "%s: D (%d) is beyond the policy net's %d input dims", who, ctx->D, CADM_MAX_VALUE_DIMS);
    CADM_REQUIRE(ctx->A <= CADM_MAX_POLICY_ACTIONS, "%s: A (%d) is beyond the policy net's %d action dims", who, ctx->A,
                 CADM_MAX_POLICY_ACTIONS);
    if ((rc = mlp_ctx_check(ctx, "a policy prior", who))) return rc;
    int dims[MLP_NL + 1];
    policy_dims(ctx, p, dims);
    const size_t lds = policy_lds_bytes(dims, p->n_hidden + 1, 1, nullptr, nullptr);
    CADM_REQUIRE(lds <= (size_t)MLP_LDS_MAX, "%s: the policy net's activation tiles need %zu bytes of LDS at one row tile, the bound is %d", who,
                 lds, MLP_LDS_MAX);
    return CADM_OK;
}

// `p` must describe the registered net
static int policy_match(const cadm_ctx* ctx, const cadm_policy_params* p, const char* who) {
    if (!mlp_registered(ctx->policy)) { cadm_set_error("%s: no policy net is registered (call cadm_set_policy_net)", who); return CADM_ESTATE; }
    const cadm_policy_params& r = ctx->policy->prm;
    CADM_REQUIRE(p->squash == r.squash && mlp_shape_same(mlp_shape(p), mlp_shape(&r)), "%s: the policy parameters do not describe the registered net (layers, widths, activation or squash differ)", who);
    return CADM_OK;
}

int cadm_policy_plan_check(const cadm_ctx* ctx, const cadm_policy_params* p, const char* who) {
    int rc;
    if ((rc = cadm_policy_check(ctx, p, who))) return rc;
    CADM_REQUIRE(ctx->cfg.num_cem_iters <= CADM_POLICY_IT && CADM_POLICY_IT + 2 * (long long)ctx->H < CADM_FORECAST_IT,
                 "%s: num_cem_iters (%d) or the horizon (%d) reaches the iteration words %d .. of the proposal roll", who,
                 ctx->cfg.num_cem_iters, ctx->H, CADM_POLICY_IT);
    if ((rc = policy_match(ctx, p, who))) return rc;
    return cadm_policy_proposals_check(ctx, p, who);      // (proposals drawn from the head: what that source asks on top)
}

// one policy step over `total` rows: obs [m, D] (t == 0) or x [total, p, D]; seqs [total, H, A] or null; a1 [total, A]; states or null
static int policy_launch(cadm_ctx* ctx, const float* obs, const float* x, int P, int p, int t, float noise_std, uint32_t seed, uint32_t call,
                         float* seqs, float* a1, float* states, size_t total, hipStream_t s, const char* who, int all_rows = 0,
                         uint32_t stream_word = CADM_STREAM_POLICY) {
    PolicyArgs a{};
    cadm_policy_dev(ctx, &a.net, &a.squash);
    a.obs = obs; a.x = x; a.P = P; a.p = p; a.t = t; a.H = ctx->H;
    a.lb = ctx->cfg.lower_bound; a.ub = ctx->cfg.upper_bound;
    a.mid = 0.5f * (a.ub + a.lb); a.half = 0.5f * (a.ub - a.lb);
    a.noise_std = noise_std; a.seed = seed; a.call = call;
    a.all_rows = all_rows; a.stream = stream_word;
    a.seqs = seqs; a.a1 = a1; a.states = states; a.total = total;
    // two row tiles where the rows are many (mlp_many_tiles) and their LDS fits; else one
    int RT = mlp_many_tiles(ctx, total) ? 2 : 1;
    size_t lds = policy_lds_bytes(a.net.dims, a.net.nlayers, RT, &a.region0, &a.region1);
    if (lds > (size_t)MLP_LDS_MAX) { RT = 1; lds = policy_lds_bytes(a.net.dims, a.net.nlayers, RT, &a.region0, &a.region1); }
    CADM_REQUIRE(total <= 0xffffffffull, "%s: %zu rows are too many for one launch", who, total);      // (xi's Philox counter takes the row)
    return mlp_launch(ctx, policy_step_kernel<1>, policy_step_kernel<2>, RT, lds, total, a, s, who);
}

// the roll: H policy steps and H - 1 one-step rollouts; nothing is evaluated behind the last action.  Every one-step rollout runs under
// its own even iteration word CADM_POLICY_IT + 2 t (the context layout of iteration 0; the head noise of step t is drawn at the
// rollout's own t = 0, so the word is what tells the steps apart).
int cadm_launch_policy_propose(cadm_ctx* ctx, const cadm_policy_params* prm, const float* obs, const float* ctx_vec, int m, uint32_t seed,
                               uint32_t call, float* seqs_out, float* states_out, void* workspace, hipStream_t s, const char* who) {
    const int P = prm->n_samples, H = ctx->H;
    PolicyWs w;
    policy_carve(ctx, m, P, (char*)workspace, &w);
    const size_t total = (size_t)m * P, srows = total * ctx->p * ctx->D;
    int rc;
    if (!ctx->packed && (rc = cadm_pack_streams(ctx, s))) return rc;
    float *cur = w.cur, *next = w.next;
    const bool head = ctx->propose_source == CADM_PROPOSE_HEAD;      // (cadm_set_policy_proposals: every step is policy_gauss.hip's launch)
    for (int t = 0; t < H; ++t) {
        float* st = states_out ? states_out + (size_t)t * srows : nullptr;
        rc = head ? cadm_launch_policy_gauss_roll(ctx, t ? nullptr : obs, t ? cur : nullptr, P, ctx->p, t, seed, call, seqs_out, w.a1, st, total, s, who)
                  : policy_launch(ctx, t ? nullptr : obs, t ? cur : nullptr, P, ctx->p, t, prm->noise_std, seed, call, seqs_out, w.a1, st, total, s, who);
        if (rc) return rc;
        if (t + 1 < H) {
            if ((rc = cadm_launch_rollout(ctx, obs, t ? cur : nullptr, ctx_vec, w.a1, nullptr, 1, seed, call, CADM_POLICY_IT + 2 * t, 0, P, m, P,
                                          w.rows1, next, s, 0, -1, /*horizon=*/1))) return rc;
            float* sw = cur; cur = next; next = sw;
        }
    }
    return CADM_OK;
}

// imagine.hip's step: the registered net on one state per row (cadm_policy_eval's launch), every row perturbed under `stream_word`
int cadm_launch_policy_step(cadm_ctx* ctx, const float* x, size_t total, int t, float noise_std, uint32_t seed, uint32_t call,
                            uint32_t stream_word, float* a1, hipStream_t s, const char* who) {
    if (!mlp_registered(ctx->policy)) { cadm_set_error("%s: no policy net is registered (call cadm_set_policy_net)", who); return CADM_ESTATE; }
    return policy_launch(ctx, nullptr, x, 1, 1, t, noise_std, seed, call, nullptr, a1, nullptr, total, s, who, 1, stream_word);
}

extern "C" int cadm_set_policy_net(cadm_ctx* ctx, const cadm_policy_params* params, const float* const* W, const float* const* b,
                                   const float* mean, const float* std_inv, void* stream) {
    const char* who = "cadm_set_policy_net";
    CADM_REQUIRE(ctx, "%s: ctx is null", who);
    if (!params) { mlp_clear(ctx->policy); cadm_policy_head_drop(ctx); return CADM_OK; }
    int rc;
    if ((rc = cadm_policy_check(ctx, params, who))) return rc;
    int dims[MLP_NL + 1];
    policy_dims(ctx, params, dims);
    rc = mlp_register(ctx, ctx->policy, 1, nullptr, dims, params->n_hidden + 1, W, b, mean, std_inv, stream, who);
    if (rc != CADM_EINVAL) cadm_policy_head_drop(ctx);      // (a refusal touched nothing; anything else touched the net the head hangs on)
    if (rc) return rc;
    ctx->policy->prm = *params;
    return CADM_OK;
}

extern "C" int cadm_policy_eval(cadm_ctx* ctx, const float* states, int R, float* act_out, void* stream) {
    CADM_REQUIRE(ctx && states && act_out, "cadm_policy_eval: ctx / states / act_out is null");
    CADM_REQUIRE(R >= 1, "cadm_policy_eval: R must be >= 1 (got %d)", R);
    if (!mlp_registered(ctx->policy)) { cadm_set_error("cadm_policy_eval: no policy net is registered (call cadm_set_policy_net)"); return CADM_ESTATE; }
    CADM_ON_DEVICE(ctx);
    return policy_launch(ctx, nullptr, states, 1, 1, 0, 0.0f, 0, 0, nullptr, act_out, nullptr, (size_t)R, (hipStream_t)stream, "cadm_policy_eval");
}

extern "C" size_t cadm_policy_workspace_bytes(cadm_ctx* ctx, int m, int P) {
    if (!ctx || m <= 0 || P <= 0) return 0;
    return policy_carve(ctx, m, P, nullptr, nullptr);
}

extern "C" int cadm_policy_propose(cadm_ctx* ctx, const cadm_policy_params* params, const float* obs, const float* ctx_vec, int m,
                                   uint32_t seed, uint32_t call, float* seqs_out, float* states_out, void* workspace, void* stream) {
    const char* who = "cadm_policy_propose";
    CADM_REQUIRE(ctx && params && obs && seqs_out && workspace, "%s: ctx / params / obs / seqs_out / workspace is null", who);
    int rc;
    if ((rc = cadm_policy_plan_check(ctx, params, who))) return rc;
    CADM_REQUIRE(m >= 1, "%s: m must be >= 1 (got %d)", who, m);
    CADM_REQUIRE(ctx->C == 0 || ctx_vec, "%s: ctx_vec required for a context model", who);
    if ((rc = cadm_require_ready(ctx, who))) return rc;
    CADM_ON_DEVICE(ctx);
    return cadm_launch_policy_propose(ctx, params, obs, ctx_vec, m, seed, call, seqs_out, states_out, workspace, (hipStream_t)stream, who);
}
