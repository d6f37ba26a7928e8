// Terminal value from Q critics in the opt-in planner loop (icem.hip): a caller-supplied actor pi (the net of cadm_set_policy_net, policy.hip)
// and C critics Q_c, MLPs D + A -> h_1 -> .. -> h_L -> 1, evaluated on the LAST state of every particle's trajectory and added to the
// particle's return: rows' = rows + weight * reduce_c Q_c(s_H, pi(s_H)).  What LOOP (on SAC / TD3: an actor and twin critics) and TD-MPC
// (Q(z_H, pi(z_H)) behind every imagined trajectory) close their horizon with; neither has a state-value net.  No reference twin.  One
// kernel BEHIND the rollout, in the place of the terminal value (value.hip), which it excludes; the rollout kernels are not touched.
//
// Arithmetic of one row with terminal state s (all fp32, nothing fused but the MFMA's own multiply-add):
//   actor, exactly cadm_policy_eval of s:  x_k = (s_k - pmean_k) * pistd_k;  the chain of mlp_chain.h;  the output layer as an identity
//     layer into LDS;  CADM_POLICY_TANH: a_d = mid + half * tanhf(z_d) (one multiply, one add);  no noise;  a_d = fminf(fmaxf(a_d, lb), ub)
//   critic input u = [s ; a], K = D + A:  x_k = (u_k - cmean_k) * cistd_k                 one subtract, one multiply
//   critic c = 0 .. C-1, the value net's chain:  acc = b_u;  for k = 0 .. K4-1 ascending: acc = fma(W_c[k][u], x_k, acc);  relu, tanhf or
//     swish;  a linear output q_c
//   CADM_CRITIC_MIN:  r = q_0;  r = fminf(r, q_c) in ascending c
//   CADM_CRITIC_MEAN: r = q_0;  r = r + q_c in ascending c;  for C > 1 then r = r / (float)C (IEEE)
//   rows' = rows + weight * r: one multiply, then one add.  On a ctx with a discount over the horizon (cadm_set_discount, discount.hip)
//   the launcher passes weight * disc[H], one fp32 product on the host; the kernel is the same.
// A row whose terminal state (or, with given actions, whose action) holds a non-finite value gets r = NaN explicitly and so a NaN return:
// the actor's fallback action clip(0, lb, ub) is what act_out reads for it, never what a Q is computed from.  With `first` (the
// constraint kernel's first_violation) a row with first < H keeps its input bits, reads NaN in the outputs, and its state is not loaded.
//
// Mapping: value_kernel's (value.hip): a workgroup of 4 waves owns 16 * RT consecutive rows, activations resident in LDS as [unit][row]
// with mlp_swz, weights from ctx-owned packed copies through the register ring, every layer through mlp_layer<RT>.  New here: the critics'
// input tile [K4][16 RT] has a region of its own beside the two ping-pong regions, because C critics read it one after the other and the
// actor's output is written into its action lines.  The raw state is read from HBM once per row: the same load fills the actor's input
// tile (its statistics) and the state lines of the critics' (theirs).  Between the two chains one thread per (row, action dim) squashes,
// clips, normalises.  Every critic's output sum has its own line of 16 RT floats; the reduction runs over them in a register.
// Reduction contract: a row's result is one column's chains in ascending k, behind one another in a fixed order: the same instruction
// sequence wherever the row sits; no floating-point atomics; nothing depends on the grid, on RT, on m or n: the same bits run to run,
// inside any batch, and from cadm_critic_eval as from the planner stage.
// The host path around the kernel (description checks, registration, row tiles, launch) is mlp_chain.h's; what stands below is what
// this net has of its own.
#include "mlp_chain.h"

namespace {

// (Not built from MlpDev: with the actor's and the critics' halves embedded the fields move, and the launch of few rows, whose time is one
// workgroup's latency, measured slower than with this order: profiles/mlp_host_refactor.md.)
struct CriticArgs {
    const float* pW[MLP_NL];                       // the actor: packed, per layer
    const float* pb[MLP_NL];
    int pdims[MLP_NL + 1];                         // D, h_1 .. h_L, A
    int pnl;                                       // dense layers including the output
    int pact, squash;
    const float *pmean, *pistd;                    // [D]
    float lb, ub, mid, half;
    const float* cW[CADM_MAX_CRITICS][MLP_NL];     // the critics: packed, per critic and layer
    const float* cb[CADM_MAX_CRITICS][MLP_NL];
    int cdims[MLP_NL + 1];                         // D + A, h_1 .. h_L, 1
    int cnl, cact, C, reduce;
    const float *cmean, *cistd;                    // [D + A]
    const float* x;                                // [total, D] row-major states
    const float* actions;                          // [total, A], or null: the actor acts
    const int32_t* first;                          // [total] or null
    int H;
    const float* rows_in;                          // [total] or null (cadm_critic_eval)
    float *rows_out, *q_out;                       // [total] or null each
    float* q_each;                                 // [C, total] or null
    float* act_out;                                // [total, A] or null
    float weight;
    size_t total;
    int inp, region0, region1;                     // LDS floats of the critics' input tile and of the two activation regions
};

template <int RT>
__global__ __launch_bounds__(MLP_THREADS) void critic_kernel(const CriticArgs a) {
    extern __shared__ __attribute__((aligned(16))) float crt_smem[];
    constexpr int R = 16 * RT;
    float* inp = crt_smem;                                       // [K4][R] the critics' input: outlives both chains
    float* reg0 = inp + a.inp;
    float* reg1 = reg0 + a.region0;
    float* vres = reg1 + a.region1;                              // [C][R] the critics' output sums
    int* flag = reinterpret_cast<int*>(vres + a.C * R);          // [R] 0: a row to evaluate, 1: cut by `first`, 2: behind the batch
    int* bad = flag + R;                                         // [R] 1: a non-finite value in the terminal state (or the given action)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t q0 = (size_t)blockIdx.x * R;                    // (q0 < total: the grid is ceil(total / R))
    const int rows = a.total - q0 < (size_t)R ? (int)(a.total - q0) : R;
    const bool actor = a.actions == nullptr;
    if (tid < R) {
        flag[tid] = tid >= rows ? 2 : (a.first && a.first[q0 + tid] < a.H) ? 1 : 0;
        bad[tid] = 0;
    }
    __syncthreads();
    // one load of the raw state, two tiles [k][row]: the actor's under its statistics (region 0, zeros behind D), the state lines of the
    // critics' under theirs; rows that are not evaluated are zeros
    const int D = a.cdims[0] - a.pdims[a.pnl], D4 = (D + 3) & ~3;
    for (int idx = tid; idx < R * D4; idx += MLP_THREADS) {
        const int row = idx / D4, k = idx - row * D4;
        float xa = 0.0f, xc = 0.0f;
        if (k < D && flag[row] == 0) {
            const float v = a.x[(q0 + row) * D + k];
            if (mlp_nonfinite(v)) bad[row] = 1;               // (every writer stores the same 1)
            xc = (v - a.cmean[k]) * a.cistd[k];
            if (actor) xa = (v - a.pmean[k]) * a.pistd[k];
        }
        if (k < D) inp[k * R + mlp_swz<RT>(row, k)] = xc;
        if (actor) reg0[k * R + mlp_swz<RT>(row, k)] = xa;
    }
    __syncthreads();
    const float* xin = reg0;
    // (both chains stand here and do not go through mlp_forward: this kernel's registers and branches came out differently with it)
    if (actor)
        for (int l = 0; l < a.pnl; ++l) {
            float* xout = (l & 1) ? reg0 : reg1;
            mlp_layer<RT>(a.pW[l], a.pb[l], a.pdims[l], a.pdims[l + 1], l + 1 == a.pnl ? MLP_ACT_NONE : a.pact, false, xin, xout, nullptr, wave, lane);
            __syncthreads();
            xin = xout;
        }
    // the action lines of the critics' tile, and its zeros behind K: the policy kernel's epilogue without noise, or the given action
    const int K = a.cdims[0], K4 = (K + 3) & ~3, A = K - D, W = K4 - D;
    for (int idx = tid; idx < R * W; idx += MLP_THREADS) {
        const int row = idx / W, d = idx - row * W, k = D + d;
        float x = 0.0f;
        if (d < A && row < rows) {
            const size_t q = q0 + row;
            float v = 0.0f;
            if (actor) {
                if (!bad[row]) v = mlp_squash(xin[d * R + mlp_swz<RT>(row, d)], a.squash, a.mid, a.half);
                v = fminf(fmaxf(v, a.lb), a.ub);
            } else if (flag[row] == 0) {
                v = a.actions[q * A + d];
                if (mlp_nonfinite(v)) bad[row] = 1;
            }
            if (a.act_out) a.act_out[q * A + d] = v;
            if (flag[row] == 0) x = (v - a.cmean[k]) * a.cistd[k];
        }
        inp[k * R + mlp_swz<RT>(row, k)] = x;
    }
    __syncthreads();
    for (int c = 0; c < a.C; ++c) {
        xin = inp;
        for (int l = 0; l < a.cnl; ++l) {
            float* xout = (l & 1) ? reg0 : reg1;
            mlp_layer<RT>(a.cW[c][l], a.cb[c][l], a.cdims[l], a.cdims[l + 1], a.cact, l + 1 == a.cnl, xin, xout, vres + c * R, wave, lane);
            __syncthreads();
            xin = xout;
        }
    }
    if (tid >= rows) return;
    const size_t q = q0 + tid;
    const float nan = __uint_as_float(0x7fc00000u);
    const bool cut = flag[tid] == 1, none = cut || bad[tid];
    float r = vres[tid];
    if (a.q_each) a.q_each[q] = none ? nan : r;
    for (int c = 1; c < a.C; ++c) {
        const float qc = vres[c * R + tid];
        if (a.q_each) a.q_each[(size_t)c * a.total + q] = none ? nan : qc;
        r = a.reduce == CADM_CRITIC_MIN ? fminf(r, qc) : __fadd_rn(r, qc);
    }
    if (a.reduce == CADM_CRITIC_MEAN && a.C > 1) r = __fdiv_rn(r, (float)a.C);
    if (none) r = nan;
    if (a.q_out) a.q_out[q] = r;
    if (a.rows_out) {
        const float r_in = a.rows_in[q];
        const float wr = __fmul_rn(a.weight, r);                 // (one multiply, then one add: never an fma)
        a.rows_out[q] = cut ? r_in : __fadd_rn(r_in, wr);
    }
}

void critic_dims(const cadm_ctx* ctx, const cadm_critic_params* p, int* dims) { mlp_dims(mlp_shape(p), ctx->D + ctx->A, 1, dims); }

// LDS of a workgroup with RT row tiles: the critics' input tile, two regions sized for the wider of the actor (pdims: its input tile and
// every layer's outputs, the A sums of the output layer among them; null: no actor in the launch) and a critic (its hidden layers'
// outputs), the C lines of output sums and the two flag arrays
size_t critic_lds_bytes(const int* pdims, int pnl, const int* cdims, int cnl, int C, int RT, int* inp, int* region0, int* region1) {
    const size_t R = 16 * (size_t)RT;
    size_t r0 = 0, r1 = 0;
    if (pdims) {
        int a0, a1;
        mlp_region_floats(pdims, pnl + 1, RT, &a0, &a1);
        r0 = (size_t)a0; r1 = (size_t)a1;
    }
    for (int l = 0; l + 1 < cnl; ++l) {
        const size_t need = R * (size_t)((cdims[l + 1] + 3) & ~3);
        if (l & 1) r0 = need > r0 ? need : r0; else r1 = need > r1 ? need : r1;
    }
    const size_t in = R * (size_t)((cdims[0] + 3) & ~3);
    if (inp) *inp = (int)in;
    if (region0) *region0 = (int)r0;
    if (region1) *region1 = (int)r1;
    return (in + r0 + r1 + ((size_t)C + 2) * R) * sizeof(float);
}

}  // namespace

// the ctx-owned packed copies of the registered critics (every one carries the shared input statistics; critic 0's are read).  The
// weight of its prm is not used; its reduce is cadm_critic_eval's: a planner call brings both
struct CriticNets : MlpOwned<cadm_critic_params, CADM_MAX_CRITICS> {};

void cadm_critic_free(cadm_ctx* ctx) { mlp_free(ctx->critic); }

// the refusals of a description of critics, before any HIP call
int cadm_critic_check(const cadm_ctx* ctx, const cadm_critic_params* p, const char* who) {
    int rc;
    if ((rc = mlp_shape_check(mlp_shape(p), "critic", who))) return rc;
    CADM_REQUIRE(p->n_critics >= 1 && p->n_critics <= CADM_MAX_CRITICS, "%s: %d critics, outside 1 .. %d", who, p->n_critics, CADM_MAX_CRITICS);
    CADM_REQUIRE(p->reduce == CADM_CRITIC_MIN || p->reduce == CADM_CRITIC_MEAN, "%s: unknown critic reduce %d", who, p->reduce);
    CADM_REQUIRE(isfinite(p->weight), "%s: the critic weight %g is not finite", who, (double)p->weight);
    CADM_REQUIRE(ctx->D <= CADM_MAX_VALUE_DIMS, "%s: D (%d) is beyond the critics' %d state dims", who, ctx->D, CADM_MAX_VALUE_DIMS);
    CADM_REQUIRE(ctx->A <= CADM_MAX_POLICY_ACTIONS, "%s: A (%d) is beyond the critics' %d action dims", who, ctx->A, CADM_MAX_POLICY_ACTIONS);
    if ((rc = mlp_ctx_check(ctx, "a terminal Q", who))) return rc;
    int cdims[MLP_NL + 1];
    critic_dims(ctx, p, cdims);
    MlpDev pd{};
    const bool actor = cadm_policy_dev(ctx, &pd, nullptr);
    const size_t lds = critic_lds_bytes(actor ? pd.dims : nullptr, pd.nlayers, cdims, p->n_hidden + 1, p->n_critics, 1, nullptr, nullptr, nullptr);
    CADM_REQUIRE(lds <= (size_t)MLP_LDS_MAX, "%s: the critics' input tile and the activation tiles of actor and critics need %zu bytes of LDS "
                 "at one row tile, the bound is %d", who, lds, MLP_LDS_MAX);
    return CADM_OK;
}

// `p` must describe the registered critics; need_actor: and a policy net must be registered
static int critic_match(const cadm_ctx* ctx, const cadm_critic_params* p, bool need_actor, const char* who) {
    if (!mlp_registered(ctx->critic)) { cadm_set_error("%s: no critics are registered (call cadm_set_critic_nets)", who); return CADM_ESTATE; }
    if (need_actor && !cadm_policy_dev(ctx, nullptr, nullptr)) {
        cadm_set_error("%s: no policy net is registered (call cadm_set_policy_net): the critics are evaluated at its action", who);
        return CADM_ESTATE;
    }
    if (!p) return CADM_OK;
    const cadm_critic_params& r = ctx->critic->prm;
    CADM_REQUIRE(p->n_critics == r.n_critics && mlp_shape_same(mlp_shape(p), mlp_shape(&r)), "%s: the critic parameters do not describe the registered critics (count, layers, widths or activation differ)", who);
    return CADM_OK;
}

int cadm_critic_plan_check(const cadm_ctx* ctx, const cadm_critic_params* p, const char* who) {
    int rc;
    if ((rc = cadm_critic_check(ctx, p, who))) return rc;
    return critic_match(ctx, p, true, who);
}

// x [total, D]; actions [total, A] or null (the actor acts); first [total] or null; rows_in / rows_out [total] or both null; q_out [total],
// q_each [C, total], act_out [total, A] or null each
static int critic_launch(cadm_ctx* ctx, int reduce, float weight, const float* x, const float* actions, const int32_t* first, size_t total,
                         const float* rows_in, float* rows_out, float* q_out, float* q_each, float* act_out, hipStream_t s, const char* who) {
    const CriticNets& nets = *ctx->critic;
    CriticArgs a{};
    critic_dims(ctx, &nets.prm, a.cdims);
    a.cnl = nets.prm.n_hidden + 1;
    a.cact = nets.prm.activation;
    a.cmean = nets.net[0].mean; a.cistd = nets.net[0].istd;
    a.C = nets.prm.n_critics;
    a.reduce = reduce;
    for (int c = 0; c < a.C; ++c)
        for (int l = 0; l < a.cnl; ++l) { a.cW[c][l] = nets.net[c].W[l]; a.cb[c][l] = nets.net[c].b[l]; }
    const bool actor = actions == nullptr;
    a.pdims[0] = ctx->D; a.pdims[1] = ctx->A; a.pnl = 1; // (the kernel reads D and A from the two sets of dims)
    if (actor) {
        MlpDev pd{};
        cadm_policy_dev(ctx, &pd, &a.squash);                    // (registered: critic_match has asked)
        for (int l = 0; l < pd.nlayers; ++l) { a.pW[l] = pd.W[l]; a.pb[l] = pd.b[l]; a.pdims[l + 1] = pd.dims[l + 1]; }
        a.pnl = pd.nlayers; a.pact = pd.act; a.pmean = pd.mean; a.pistd = pd.istd;
    }
    a.lb = ctx->cfg.lower_bound; a.ub = ctx->cfg.upper_bound;
    a.mid = 0.5f * (a.ub + a.lb); a.half = 0.5f * (a.ub - a.lb);
    a.x = x; a.actions = actions; a.first = first; a.H = ctx->H; a.rows_in = rows_in; a.rows_out = rows_out; a.q_out = q_out; a.q_each = q_each;
    a.act_out = act_out; a.weight = weight; a.total = total;
    // two row tiles where the rows are many (mlp_many_tiles) and their LDS fits; else one
    int RT = mlp_many_tiles(ctx, total) ? 2 : 1;
    size_t lds = critic_lds_bytes(actor ? a.pdims : nullptr, a.pnl, a.cdims, a.cnl, a.C, RT, &a.inp, &a.region0, &a.region1);
    if (lds > (size_t)MLP_LDS_MAX) {
        RT = 1;
        lds = critic_lds_bytes(actor ? a.pdims : nullptr, a.pnl, a.cdims, a.cnl, a.C, RT, &a.inp, &a.region0, &a.region1);
    }
    CADM_REQUIRE(lds <= (size_t)MLP_LDS_MAX, "%s: the critics' input tile and the activation tiles of actor and critics need %zu bytes of LDS "
                 "at one row tile, the bound is %d", who, lds, MLP_LDS_MAX);
    return mlp_launch(ctx, critic_kernel<1>, critic_kernel<2>, RT, lds, total, a, s, who);
}

// the planner's stage: rows [m, n, p] in place, behind a rollout's traj [H, m, n, p, D] (n the PACKED candidate count)
int cadm_launch_critic(cadm_ctx* ctx, const cadm_critic_params* p, const float* traj, const int32_t* first, int m, int n, float* rows,
                       hipStream_t s) {
    const size_t total = (size_t)m * n * ctx->p;
    return critic_launch(ctx, p->reduce, cadm_discounted_weight(ctx, p->weight), traj + (size_t)(ctx->H - 1) * total * ctx->D, nullptr, first, total, rows, rows, nullptr,
                         nullptr, nullptr, s, "cadm_critic_plan");
}

extern "C" int cadm_set_critic_nets(cadm_ctx* ctx, const cadm_critic_params* params, const float* const* W, const float* const* b,
                                    const float* mean, const float* std_inv, void* stream) {
    const char* who = "cadm_set_critic_nets";
    CADM_REQUIRE(ctx, "%s: ctx is null", who);
    if (!params) { mlp_clear(ctx->critic); return CADM_OK; }
    int rc;
    if ((rc = cadm_critic_check(ctx, params, who))) return rc;
    int dims[MLP_NL + 1];
    critic_dims(ctx, params, dims);
    if ((rc = mlp_register(ctx, ctx->critic, params->n_critics, "critic", dims, params->n_hidden + 1, W, b, mean, std_inv, stream, who))) return rc;
    ctx->critic->prm = *params;
    return CADM_OK;
}

extern "C" int cadm_critic_eval(cadm_ctx* ctx, const float* states, const float* actions, int R, float* q_out, float* q_each_out, float* act_out,
                                void* stream) {
    CADM_REQUIRE(ctx && states && q_out, "cadm_critic_eval: ctx / states / q_out is null");
    CADM_REQUIRE(R >= 1, "cadm_critic_eval: R must be >= 1 (got %d)", R);
    int rc;
    if ((rc = critic_match(ctx, nullptr, actions == nullptr, "cadm_critic_eval"))) return rc;
    CADM_ON_DEVICE(ctx);
    return critic_launch(ctx, ctx->critic->prm.reduce, 0.0f, states, actions, nullptr, (size_t)R, nullptr, nullptr, q_out, q_each_out, act_out,
                         (hipStream_t)stream, "cadm_critic_eval");
}

extern "C" int cadm_critic_returns(cadm_ctx* ctx, const cadm_critic_params* params, const float* traj, const int32_t* first, int m, int n,
                                   const float* rows_in, float* rows_out, float* q_out, void* stream) {
    CADM_REQUIRE(ctx && params && traj && rows_in && rows_out, "cadm_critic_returns: ctx / params / traj / rows_in / rows_out is null");
    int rc;
    if ((rc = cadm_critic_plan_check(ctx, params, "cadm_critic_returns"))) return rc;
    CADM_REQUIRE(m >= 1 && n >= 1, "cadm_critic_returns: m, n must be >= 1 (got m=%d n=%d)", m, n);
    CADM_ON_DEVICE(ctx);
    const size_t total = (size_t)m * n * ctx->p;
    return critic_launch(ctx, params->reduce, cadm_discounted_weight(ctx, params->weight), traj + (size_t)(ctx->H - 1) * total * ctx->D, nullptr, first, total, rows_in,
                         rows_out, q_out, nullptr, nullptr, (hipStream_t)stream, "cadm_critic_returns");
}
