// Learned step reward of the opt-in planner loop (icem.hip): a caller-supplied reward net R, an MLP K -> h_1 -> .. -> h_L -> 1, evaluated
// on EVERY step of every particle's trajectory; the sum over the counted steps, times a weight, is added to the particle's return:
// rows' = rows + weight * S,  S = ((0 + R_0) + R_1) + ..  No reference twin: the reference's planner knows analytic rewards only.  Two
// launches BEHIND the rollout, behind the constraints (constrain.hip) and the tracking terms (tracking.hip) and in front of the terminal
// value (value.hip); the rollout kernels are not touched.
//
// Input of step t of row q = (env mi, candidate ni, particle j), by `inputs`: s_{t+1} | s_t, a_t | s_t, a_t, s_{t+1}  with s_0 = obs[mi],
// s_t = traj[t - 1, q], s_{t+1} = traj[t, q], a_t = actions[mi, ni, t, :] (raw, as the rollout read them).
// Arithmetic of one (t, q) (all fp32): x_k = (in_k - mean_k) * inv_std_k over the K concatenated dims, then the chain of mlp_chain.h --
// the one value.hip runs.  A counted step whose input holds a non-finite value gets R = NaN explicitly.  With `first` (the constraint
// kernel's first_violation) the counted steps are t <= first[q]; the others read NaN in r_step, are not summed, and their inputs are not
// loaded.  On a ctx with a discount over the horizon (cadm_set_discount, discount.hip): S = S + disc[t] * R_t; r_step stays undiscounted.
//
// Mapping.  reward_kernel: the (t, q) pairs are one flat row space e = t * (m n p) + q, the order of traj itself, and of r_step
// [H, m, n, p].  A workgroup of 4 waves owns 16 * RT consecutive e (RT = 1 or 2), gathers their input tile [k][row] from the three
// sources -- a tile may straddle a step, an env and a candidate: every row carries its own two source pointers, worked out once per row
// -- and takes it through every layer as mlp_chain.h describes.  reward_sum_kernel: one thread per q walks t ascending over r_step with
// plain adds (its loads 32 at a time, so the walk is a chain of adds and not of memory latencies) and writes S and the row.  The
// one-kernel form, a workgroup that owns particle rows and walks t, was not built: the GEMM wants the rows of all steps side by side, and
// the uncertainty stage measured two launches 10 x faster than an H-step walk.
// Row tiles, by measurement (one MI355X, 120 000 rows, us per stage; value.hip's launch on as many rows beside it, which takes RT = 2):
//   net (relu, K = 18)    RT = 1    RT = 2    RT = 4    value.hip
//   (64, 64)                55.0      50.4      51.7       44.5
//   (128, 128)              92.1      78.9      96.1       72.6
//   (200, 200)             155.7     170.2     260.9      163.5
//   (256, 256)             205.5     234.0     297.4      226.0
//   (512, 512)             776.5     912.1   no fit       906.5
// The rows are plentiful, but amortising the weight stream over more of them does not pay: the chain is bound by latency, not by the L2,
// and what decides is how many waves a CU holds.  A 64-row variant (RT = 4, pairs of row tiles per wave) lost everywhere and was taken
// out again.  The launcher's rule: RT = 2 when there are more than 2 sixteen-row tiles per CU (value.hip's rule) AND four workgroups of
// it, 16 waves, still fit a CU's LDS (<= 40 KiB each); else RT = 1.  That is RT = 2 up to (128, 128) and RT = 1 from (200, 200) on,
// the faster one in every row above.
// LDS per workgroup: 16 RT * (4 * (region 0 + region 1) + 28) bytes, region 0 = max(K4, widths of the even hidden layers h_2, h_4),
// region 1 = max(h_1, h_3), each rounded up to 4; 28 = the output sum, two flags and two source pointers per row.
//   net (K = 44)         RT = 1      RT = 2
//   (128, 128)          16.4 KiB    32.9 KiB   (RT = 2: four workgroups per CU)
//   (256, 256)          32.4 KiB    64.9 KiB   (RT = 1: four workgroups per CU)
//   (512, 512)          64.4 KiB   128.9 KiB   (RT = 1, above 64 KiB: the kernel's dynamic-LDS attribute is raised, once per ctx)
// Reduction contract: R(t, q) is one column's chain in ascending k, the same instruction sequence wherever the row sits; the step sum is
// sequential in t per row; no floating-point atomics; nothing depends on the grid, on RT, on m, n or p: the same bits run to run, inside
// any batch, and from cadm_reward_eval as from the planner stage.
// The host path around the kernel (description checks, registration, row tiles, launch) is mlp_chain.h's; what stands below is what
// this net has of its own.
#include "mlp_chain.h"

namespace {

struct RewardArgs {
    MlpDev net;                    // K -> h_1 .. h_L -> 1
    const float* x;                // cadm_reward_eval: [rows, K] concatenated inputs; else null
    const float *traj, *obs, *actions;      // [H, m, n, p, D], [m, D], [m, n, H, A]
    const int32_t* first;          // [m, n, p] or null
    int inputs, D, A, H, n, p;
    size_t total;                  // m n p: the rows of one step
    size_t rows;                   // H * total, or the R of cadm_reward_eval
    float* r_out;                  // [rows]
    int region0, region1;          // LDS floats of the two activation regions
};

template <int RT>
__global__ __launch_bounds__(MLP_THREADS) void reward_kernel(const RewardArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rew_smem[];
    constexpr int R = 16 * RT;
    float* reg0 = rew_smem;
    float* reg1 = reg0 + a.region0;
    float* vres = reg1 + a.region1;                              // [R] the output layer's sums
    int* flag = reinterpret_cast<int*>(vres + R);                // [R] 0: a row to evaluate, 1: not counted (`first`), 2: behind the batch
    int* bad = flag + R;                                         // [R] 1: a non-finite value in the row's input
    const float** sp = reinterpret_cast<const float**>(bad + R); // [R] s_t of the row: obs[mi] or traj[t - 1, q]   (8-byte aligned: the
    const float** ap = sp + R;                                   // [R] a_t of the row                               regions are even)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t e0 = (size_t)blockIdx.x * R;                    // (e0 < rows: the grid is ceil(rows / R))
    const int rows = a.rows - e0 < (size_t)R ? (int)(a.rows - e0) : R;
    if (tid < R) {
        int f = tid >= rows ? 2 : 0;
        const float *s = nullptr, *ac = nullptr;
        if (f == 0 && !a.x) {
            const size_t e = e0 + tid;
            size_t t, q, cand, mi;
            if ((a.rows >> 32) == 0) {                           // (the usual case: 32-bit divisions)
                const unsigned e32 = (unsigned)e, tot = (unsigned)a.total, t32 = e32 / tot, q32 = e32 - t32 * tot, c32 = q32 / (unsigned)a.p;
                t = t32; q = q32; cand = c32; mi = c32 / (unsigned)a.n;
            } else {
                t = e / a.total; q = e - t * a.total; cand = q / a.p; mi = cand / a.n;
            }
            if (a.first && (int)t > a.first[q]) f = 1;
            else {
                s = t == 0 ? a.obs + mi * a.D : a.traj + (e - a.total) * a.D;
                ac = a.actions + (cand * a.H + t) * a.A;
            }
        }
        flag[tid] = f; bad[tid] = 0; sp[tid] = s; ap[tid] = ac;
    }
    __syncthreads();
    // the input tile [k][row], gathered and normalised on the way in; rows that are not evaluated and the k behind K are zeros
    const int K = a.net.dims[0], K4 = (K + 3) & ~3, D = a.D, DA = a.D + a.A;
    for (int idx = tid; idx < R * K4; idx += MLP_THREADS) {
        const int row = idx / K4, k = idx - row * K4;
        float x = 0.0f;
        if (k < K && flag[row] == 0) {
            float v;
            if (a.x) v = a.x[(e0 + row) * K + k];
            else if (a.inputs == CADM_REWARD_NEXT_OBS) v = a.traj[(e0 + row) * D + k];
            else if (k < D) v = sp[row][k];
            else if (k < DA) v = ap[row][k - D];
            else v = a.traj[(e0 + row) * D + (k - DA)];
            if (mlp_nonfinite(v)) bad[row] = 1;                  // (every writer stores the same 1)
            x = (v - a.net.mean[k]) * a.net.istd[k];
        }
        reg0[k * R + mlp_swz<RT>(row, k)] = x;
    }
    __syncthreads();
    mlp_forward<RT>(a.net, true, reg0, reg1, reg0, vres, wave, lane);
    if (tid >= rows) return;
    a.r_out[e0 + tid] = (flag[tid] == 1 || bad[tid]) ? __uint_as_float(0x7fc00000u) : vres[tid];
}

// S[q] = ((0 + r[0, q]) + r[1, q]) + .. over the counted steps t <= first[q] (all H without `first`), rows_out = rows_in + weight * S
// DISC: the ctx's discount over the horizon (discount.hip): S = S + disc[t] * r[t, q].  false: the undiscounted kernel as it was
template <bool DISC>
__global__ void reward_sum_kernel(const float* __restrict__ r_step, const int32_t* __restrict__ first, int H, size_t total, float weight,
                                  const float* rows_in, float* rows_out, float* __restrict__ sum_out, const float* __restrict__ disc) {
    const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (q >= total) return;
    int last = H - 1;
    if (first) { const int f = first[q]; last = f < last ? f : last; }
    float S = 0.0f;
    for (int t0 = 0; t0 <= last; t0 += 32) {                     // 32 loads in flight, then their adds in order
        float r[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) r[u] = t0 + u <= last ? r_step[(size_t)(t0 + u) * total + q] : 0.0f;
#pragma unroll
        for (int u = 0; u < 32; ++u)
            if (t0 + u <= last) S = DISC ? __fadd_rn(S, __fmul_rn(disc[t0 + u], r[u])) : __fadd_rn(S, r[u]);
    }
    if (sum_out) sum_out[q] = S;
    rows_out[q] = __fadd_rn(rows_in[q], __fmul_rn(weight, S));   // (one multiply, then one add: never an fma)
}

// LDS of a workgroup with RT row tiles: the two activation regions, and per row the output sum, two flags and two source pointers
size_t reward_lds_bytes(const int* dims, int nlayers, int RT, int* region0, int* region1) {
    return mlp_region_floats(dims, nlayers, RT, region0, region1) * sizeof(float) + 16 * (size_t)RT * 28;
}

int reward_K(const cadm_ctx* ctx, int inputs) {
    return inputs == CADM_REWARD_NEXT_OBS ? ctx->D : inputs == CADM_REWARD_OBS_ACT ? ctx->D + ctx->A : 2 * ctx->D + ctx->A;
}

}  // namespace

// the ctx-owned packed copy of the registered net (the weight of its prm is not used: every call brings its own)
struct RewardNet : MlpOwned<cadm_reward_params> {};

void cadm_reward_free(cadm_ctx* ctx) { mlp_free(ctx->reward); }

// the refusals of a reward net's description, before any HIP call
static int reward_check(const cadm_ctx* ctx, const cadm_reward_params* p, const char* who) {
    int rc;
    if ((rc = mlp_shape_check(mlp_shape(p), "reward", who))) return rc;
    CADM_REQUIRE(p->inputs == CADM_REWARD_NEXT_OBS || p->inputs == CADM_REWARD_OBS_ACT || p->inputs == CADM_REWARD_OBS_ACT_NEXT_OBS,
                 "%s: unknown reward inputs %d", who, p->inputs);
    CADM_REQUIRE(isfinite(p->weight), "%s: the reward weight %g is not finite", who, (double)p->weight);
    if ((rc = mlp_ctx_check(ctx, "a learned reward", who))) return rc;
    const int K = reward_K(ctx, p->inputs);
    CADM_REQUIRE(K <= CADM_MAX_REWARD_DIMS, "%s: the reward net's input has %d dims, beyond %d", who, K, CADM_MAX_REWARD_DIMS);
    int dims[MLP_NL + 1];
    mlp_dims(mlp_shape(p), K, 1, dims);
    const size_t lds = reward_lds_bytes(dims, p->n_hidden + 1, 1, nullptr, nullptr);
    CADM_REQUIRE(lds <= (size_t)MLP_LDS_MAX, "%s: the reward net's activation tiles need %zu bytes of LDS at one row tile, the bound is %d", who,
                 lds, MLP_LDS_MAX);
    return CADM_OK;
}

// `p` must describe the registered net
static int reward_match(const cadm_ctx* ctx, const cadm_reward_params* p, const char* who) {
    if (!mlp_registered(ctx->reward)) { cadm_set_error("%s: no reward net is registered (call cadm_set_reward_net)", who); return CADM_ESTATE; }
    const cadm_reward_params& r = ctx->reward->prm;
    CADM_REQUIRE(p->inputs == r.inputs && mlp_shape_same(mlp_shape(p), mlp_shape(&r)), "%s: the reward parameters do not describe the registered net (inputs, layers, widths or activation differ)", who);
    return CADM_OK;
}

int cadm_reward_plan_check(const cadm_ctx* ctx, const cadm_reward_params* p, const char* who) {
    int rc;
    if ((rc = reward_check(ctx, p, who))) return rc;
    return reward_match(ctx, p, who);
}

// the GEMM launch over a.rows rows: the net's half of `a` is filled here
static int reward_launch(cadm_ctx* ctx, RewardArgs& a, hipStream_t s, const char* who) {
    const RewardNet& net = *ctx->reward;
    mlp_dev(a.net, net.net[0], mlp_shape(&net.prm), reward_K(ctx, net.prm.inputs), 1);
    a.inputs = net.prm.inputs;
    a.D = ctx->D; a.A = ctx->A; a.H = ctx->H; a.p = ctx->p;
    // two row tiles where four workgroups of them still fit a CU and the rows fill the CUs twice over; else one (see the header)
    const int RT = mlp_many_tiles(ctx, a.rows) && reward_lds_bytes(a.net.dims, a.net.nlayers, 2, nullptr, nullptr) <= (size_t)MLP_LDS_MAX / 4 ? 2 : 1;
    const size_t lds = reward_lds_bytes(a.net.dims, a.net.nlayers, RT, &a.region0, &a.region1);
    return mlp_launch(ctx, reward_kernel<1>, reward_kernel<2>, RT, lds, a.rows, a, s, who);
}

// both launches behind a rollout's traj [H, m, n, p, D] (n the PACKED candidate count): r_step [H, m, n, p], then the step sum
static int reward_stage(cadm_ctx* ctx, float weight, const float* traj, const float* obs, const float* actions, const int32_t* first, int m,
                        int n, const float* rows_in, float* rows_out, float* r_step, float* sum_out, hipStream_t s, const char* who) {
    RewardArgs a{};
    a.traj = traj; a.obs = obs; a.actions = actions; a.first = first; a.n = n;
    a.total = (size_t)m * n * ctx->p;
    a.rows = (size_t)ctx->H * a.total;
    a.r_out = r_step;
    int rc;
    if ((rc = reward_launch(ctx, a, s, who))) return rc;
    if (ctx->disc) hipLaunchKernelGGL(reward_sum_kernel<true>, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, s, r_step, first, ctx->H,
                                      a.total, weight, rows_in, rows_out, sum_out, ctx->disc);
    else hipLaunchKernelGGL(reward_sum_kernel<false>, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, s, r_step, first, ctx->H, a.total,
                            weight, rows_in, rows_out, sum_out, nullptr);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

// the planner's stage: rows [m, n, p] in place
int cadm_launch_reward(cadm_ctx* ctx, const cadm_reward_params* p, const float* traj, const float* obs, const float* actions,
                       const int32_t* first, int m, int n, float* rows, float* r_step, hipStream_t s) {
    return reward_stage(ctx, p->weight, traj, obs, actions, first, m, n, rows, rows, r_step, nullptr, s, "cadm_rewarded_plan");
}

extern "C" int cadm_set_reward_net(cadm_ctx* ctx, const cadm_reward_params* params, const float* const* W, const float* const* b,
                                   const float* mean, const float* std_inv, void* stream) {
    const char* who = "cadm_set_reward_net";
    CADM_REQUIRE(ctx, "%s: ctx is null", who);
    if (!params) { mlp_clear(ctx->reward); return CADM_OK; }
    int rc;
    if ((rc = reward_check(ctx, params, who))) return rc;
    int dims[MLP_NL + 1];
    mlp_dims(mlp_shape(params), reward_K(ctx, params->inputs), 1, dims);
    if ((rc = mlp_register(ctx, ctx->reward, 1, nullptr, dims, params->n_hidden + 1, W, b, mean, std_inv, stream, who))) return rc;
    ctx->reward->prm = *params;
    return CADM_OK;
}

extern "C" int cadm_reward_eval(cadm_ctx* ctx, const float* x, int R, float* r_out, void* stream) {
    CADM_REQUIRE(ctx && x && r_out, "cadm_reward_eval: ctx / x / r_out is null");
    CADM_REQUIRE(R >= 1, "cadm_reward_eval: R must be >= 1 (got %d)", R);
    if (!mlp_registered(ctx->reward)) { cadm_set_error("cadm_reward_eval: no reward net is registered (call cadm_set_reward_net)"); return CADM_ESTATE; }
    CADM_ON_DEVICE(ctx);
    RewardArgs a{};
    a.x = x; a.n = 1; a.total = (size_t)R; a.rows = (size_t)R; a.r_out = r_out;
    return reward_launch(ctx, a, (hipStream_t)stream, "cadm_reward_eval");
}

extern "C" size_t cadm_reward_workspace_bytes(cadm_ctx* ctx, int m, int n) {
    if (!ctx || m <= 0 || n <= 0) return 0;
    return (size_t)ctx->H * m * n * ctx->p * sizeof(float);
}

extern "C" int cadm_reward_returns(cadm_ctx* ctx, const cadm_reward_params* params, const float* traj, const float* obs, const float* actions,
                                   const int32_t* first, int m, int n, const float* rows_in, float* rows_out, float* step_out, float* sum_out,
                                   void* workspace, void* stream) {
    CADM_REQUIRE(ctx && params && traj && obs && actions && rows_in && rows_out,
                 "cadm_reward_returns: ctx / params / traj / obs / actions / rows_in / rows_out is null");
    CADM_REQUIRE(step_out || workspace, "cadm_reward_returns: without step_out the step rewards need a workspace");
    int rc;
    if ((rc = cadm_reward_plan_check(ctx, params, "cadm_reward_returns"))) return rc;
    CADM_REQUIRE(m >= 1 && n >= 1, "cadm_reward_returns: m, n must be >= 1 (got m=%d n=%d)", m, n);
    CADM_ON_DEVICE(ctx);
    return reward_stage(ctx, params->weight, traj, obs, actions, first, m, n, rows_in, rows_out, step_out ? step_out : (float*)workspace, sum_out,
                        (hipStream_t)stream, "cadm_reward_returns");
}
