// Log-density of GIVEN actions under the stochastic actor (no reference twin): log pi(a | s) of the registered policy net read as a SAC
// actor (policy_gauss.hip: the net's output layer the mean, cadm_set_policy_head's layer the log standard deviation).  policy_gauss.hip
// returns the density of an action it drew itself; this file evaluates it at an action the caller brings.  One kernel, policy_logp_kernel:
// cadm_policy_logp is its launch on the caller's states and actions, and the planner's stage (cadm_policy_logp_returns, the
// cadm_anchored_plan level of icem.hip) its launch on EVERY step of every particle's trajectory -- the actor-regularised score of LOOP /
// MBOP / KL-regularised MPC: rows' = rows + weight * S, S = ((0 + logp_0) + logp_1) + ..  Two launches BEHIND the rollout, behind
// the learned reward (reward.hip) and in front of the terminal value / Q; the rollout kernels and the other MLP kernels are not touched.
//
// Rows.  The flat space of reward_kernel: e = t * (m n p) + q over traj [H, m, n, p, D], the order of traj and of the step output
// [H, m, n, p].  A workgroup of 4 waves owns 16 * RT consecutive e; every row carries its own two source pointers, worked out once:
// s_t = obs[mi] at t = 0, else traj[t - 1, q];  a_t = actions[mi, ni, t, :], raw, as the rollout read them.  A tile may straddle a step,
// an env and a candidate.  With `first` (the constraint kernel's first_violation) the counted steps are t <= first[q]; the others are not
// loaded and read NaN in the step output.  cadm_policy_logp: the same kernel with plain row pointers x + e D, act + e A.
//
// Arithmetic per counted row and action dim d, all float32, every operation rounded on its own, nothing fused but the MFMA's own
// multiply-add (include/cadm_hip.h, "Log-density of given actions", restates it):
//   x, the hidden layers, mu_d, l_d: policy_gauss_kernel's walk, on the registered net's packed copy and the head's layer
//   ls_d   the registered head's bound (policy_gauss.hip's gauss_log_std: the statement is repeated below, that file is not touched)
//   CADM_POLICY_TANH:  y = (a_d - mid) / half;  y = fminf(fmaxf(y, -YMAX), YMAX), YMAX = CADM_LOGP_YMAX = 0.999999f
//                      lp = log1pf(y);  lm = log1pf(-y);  u = 0.5f * (lp - lm);  J = logf(half) + (lp + lm)       (= log(half (1 - y^2)))
//   CADM_POLICY_NONE:  u = a_d;  J = 0
//   xi     = (u - mu_d) * expf(-ls_d)
//   g_d    = ((-0.5f * xi) * xi - ls_d) - 0.9189385f
//   term_d = space == CADM_LOGP_ACTION ? g_d - J : g_d
//   logp   = term_0 + term_1 + ..   one thread per row, ascending d from term_0, out of LDS behind a barrier
// A counted row with a non-finite value in its state or in its action gets logp = NaN explicitly.  Nothing is drawn, no counter moves.
// Step sum and row update: reward_sum_kernel's arithmetic, in a copy of this file's own (reward.hip stays as it is): S over the counted
// steps in ascending t, on a discounted ctx S = S + disc[t] * logp_t; rows = rows + weight * S, one multiply and then one add.
//
// Mapping (policy_gauss_kernel's): activations resident in LDS as [unit][row]; the last hidden tile is read twice through mlp_layer, the
// head's layer by the waves that would idle (wave ^ 2, as the roll flavour does); one thread per (row, dim) forms term_d in the log-std's
// place; behind a barrier one thread per row sums.
// LDS per workgroup: 16 RT * (4 * (region 0 + region 1 + A4) + 24) bytes: reward.hip's two regions (the mean's A sums in one of them),
// the log-std's A4 sums, and per row two flags and two source pointers.
// Row tiles: reward.hip's rule -- RT = 2 when there are more than 2 sixteen-row tiles per CU AND four workgroups of it still fit a
// CU's LDS (<= 40 KiB each), else RT = 1.  The rule is INHERITED from reward.hip's table; RT = 1 against RT = 2 has not been measured
// for this kernel.  Measured under that rule (one MI355X, 120 000 rows, a (256, 256) relu actor, A = 6, RT = 1): 286.8 us per stage, next
// to 218.2 us for reward.hip's stage with a (256, 256) net in the same run (profiles/policy_logp.md).
// Reduction contract: every output is ONE thread's chain in the order above; no floating-point atomics; nothing depends on RT, the grid,
// m, n, p or the row's position: the same bits run to run, in any batch, and from cadm_policy_logp as from the planner stage.
#include "mlp_chain.h"

namespace {

constexpr float LOGP_HALF_LOG_2PI = 0.9189385f;

struct LogpArgs {
    MlpDev net;                    // D -> h_1 .. h_L -> A: the registered net, its output layer the mean
    const float *Wls, *bls;        // the head's packed layer h_L -> A
    const float *x, *act;          // cadm_policy_logp: [rows, D], [rows, A]; else null
    const float *traj, *obs, *actions;      // [H, m, n, p, D], [m, D], [m, n, H, A]
    const int32_t* first;          // [m, n, p] or null
    int squash, bound, space, D, A, H, n, p;
    float lb, ub, mid, half, lo, hi;
    size_t total;                  // m n p: the rows of one step
    size_t rows;                   // H * total, or the R of cadm_policy_logp
    float* out;                    // [rows]
    int region0, region1;          // LDS floats of the two activation regions; the log-std's A sums follow them
};

// policy_gauss.hip's gauss_log_std, statement for statement (hw = 0.5f * (hi - lo))
__device__ __forceinline__ float logp_log_std(float l, int bound, float lo, float hi, float hw) {
    return bound == CADM_LOGSTD_TANH ? __fadd_rn(lo, __fmul_rn(hw, __fadd_rn(tanhf(l), 1.0f))) : fminf(fmaxf(l, lo), hi);
}

template <int RT>
__global__ __launch_bounds__(MLP_THREADS) void policy_logp_kernel(const LogpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float logp_smem[];
    constexpr int R = 16 * RT;
    float* reg0 = logp_smem;
    float* reg1 = reg0 + a.region0;
    const int A = a.A, A4 = (A + 3) & ~3;
    float* lsr = reg1 + a.region1;                               // [A4][R] the log-std's sums, later term_d
    int* flag = reinterpret_cast<int*>(lsr + A4 * R);            // [R] 0: a row to evaluate, 1: not counted (`first`), 2: behind the batch
    int* bad = flag + R;                                         // [R] 1: a non-finite value in the row's state or action
    const float** sp = reinterpret_cast<const float**>(bad + R); // [R] s_t of the row   (8-byte aligned: every region in front is an even
    const float** ap = sp + R;                                   // [R] a_t of the row    number of floats)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t e0 = (size_t)blockIdx.x * R;                    // (e0 < rows: the grid is ceil(rows / R))
    const int rows = a.rows - e0 < (size_t)R ? (int)(a.rows - e0) : R;
    if (tid < R) {
        int f = tid >= rows ? 2 : 0;
        const float *s = nullptr, *ac = nullptr;
        if (f == 0) {
            const size_t e = e0 + tid;
            if (a.x) {
                s = a.x + e * a.D;
                ac = a.act + e * a.A;
            } else {
                size_t t, q, cand, mi;                           // reward_kernel's split of e
                if ((a.rows >> 32) == 0) {                       // (the usual case: 32-bit divisions)
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
        }
        flag[tid] = f; bad[tid] = 0; sp[tid] = s; ap[tid] = ac;
    }
    __syncthreads();
    // the input tile [k][row], gathered and normalised on the way in; rows that are not evaluated and the k behind D are zeros
    const int D = a.D, D4 = (D + 3) & ~3;
    for (int idx = tid; idx < R * D4; idx += MLP_THREADS) {
        const int row = idx / D4, k = idx - row * D4;
        float x = 0.0f;
        if (k < D && flag[row] == 0) {
            const float est = sp[row][k];
            if (mlp_nonfinite(est)) bad[row] = 1;                // (every writer stores the same 1)
            x = (est - a.net.mean[k]) * a.net.istd[k];
        }
        reg0[k * R + mlp_swz<RT>(row, k)] = x;
    }
    __syncthreads();
    // the hidden layers as policy_gauss_kernel walks them, then the last hidden tile twice, the head's layer from wave 2 on
    const int L = a.net.nlayers - 1;
    const float* xin = reg0;
    for (int l = 0; l < L; ++l) {
        float* xout = (l & 1) ? reg0 : reg1;
        mlp_layer<RT>(a.net.W[l], a.net.b[l], a.net.dims[l], a.net.dims[l + 1], a.net.act, false, xin, xout, nullptr, wave, lane);
        __syncthreads();
        xin = xout;
    }
    float* mur = (L & 1) ? reg0 : reg1;
    mlp_layer<RT>(a.net.W[L], a.net.b[L], a.net.dims[L], A, MLP_ACT_NONE, false, xin, mur, nullptr, wave, lane);
    mlp_layer<RT>(a.Wls, a.bls, a.net.dims[L], A, MLP_ACT_NONE, false, xin, lsr, nullptr, wave ^ 2, lane);
    __syncthreads();
    const float hw = __fmul_rn(0.5f, __fsub_rn(a.hi, a.lo));
    for (int idx = tid; idx < rows * A; idx += MLP_THREADS) {
        const int row = idx / A, d = idx - row * A;
        if (flag[row] != 0) continue;                            // (not counted: its action is not loaded)
        const int at = d * R + mlp_swz<RT>(row, d);
        const float av = ap[row][d];
        if (mlp_nonfinite(av)) bad[row] = 1;                     // (read behind the barrier below only; every writer stores the same 1)
        const float mu = mur[at];
        const float ls = logp_log_std(lsr[at], a.bound, a.lo, a.hi, hw);
        float u = av, J = 0.0f;
        if (a.squash == CADM_POLICY_TANH) {
            float y = __fdiv_rn(__fsub_rn(av, a.mid), a.half);
            y = fminf(fmaxf(y, -CADM_LOGP_YMAX), CADM_LOGP_YMAX);
            const float lp = log1pf(y), lm = log1pf(-y);
            u = __fmul_rn(0.5f, __fsub_rn(lp, lm));
            J = __fadd_rn(logf(a.half), __fadd_rn(lp, lm));
        }
        const float xi = __fmul_rn(__fsub_rn(u, mu), expf(-ls));
        const float g = __fsub_rn(__fsub_rn(__fmul_rn(__fmul_rn(-0.5f, xi), xi), ls), LOGP_HALF_LOG_2PI);
        lsr[at] = a.space == CADM_LOGP_ACTION ? __fsub_rn(g, J) : g;      // (this thread's own slot: read above, summed behind the barrier)
    }
    __syncthreads();
    if (tid < rows) {
        float s = __uint_as_float(0x7fc00000u);
        if (flag[tid] == 0 && !bad[tid]) {
            s = lsr[mlp_swz<RT>(tid, 0)];
            for (int d = 1; d < A; ++d) s = __fadd_rn(s, lsr[d * R + mlp_swz<RT>(tid, d)]);
        }
        a.out[e0 + tid] = s;
    }
}

// reward_sum_kernel's arithmetic on the step log-densities: S[q] = ((0 + lp[0, q]) + lp[1, q]) + .. over the counted steps t <= first[q]
// (all H without `first`), rows_out = rows_in + weight * S.  DISC: the ctx's discount over the horizon: S = S + disc[t] * lp[t, q]
template <bool DISC>
__global__ void logp_sum_kernel(const float* __restrict__ step, const int32_t* __restrict__ first, int H, size_t total, float weight,
                                const float* rows_in, float* rows_out, float* __restrict__ sum_out, const float* __restrict__ disc) {
    const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (q >= total) return;
    int last = H - 1;
    if (first) { const int f = first[q]; last = f < last ? f : last; }
    float S = 0.0f;
    for (int t0 = 0; t0 <= last; t0 += 32) {                     // 32 loads in flight, then their adds in order
        float r[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) r[u] = t0 + u <= last ? step[(size_t)(t0 + u) * total + q] : 0.0f;
#pragma unroll
        for (int u = 0; u < 32; ++u)
            if (t0 + u <= last) S = DISC ? __fadd_rn(S, __fmul_rn(disc[t0 + u], r[u])) : __fadd_rn(S, r[u]);
    }
    if (sum_out) sum_out[q] = S;
    rows_out[q] = __fadd_rn(rows_in[q], __fmul_rn(weight, S));   // (one multiply, then one add: never an fma)
}

// LDS of a workgroup with RT row tiles: the two activation regions (the mean's A sums in one of them), the log-std's A4 sums, and per
// row two flags and two source pointers
size_t logp_lds_bytes(const int* dims, int nlayers, int RT, int* region0, int* region1) {
    const size_t A4 = (size_t)((dims[nlayers] + 3) & ~3);
    return (mlp_region_floats(dims, nlayers + 1, RT, region0, region1) + 16 * (size_t)RT * A4) * sizeof(float) + 16 * (size_t)RT * 24;
}

// what every entry point asks of the ctx's state, before any HIP call: policy_gauss.hip's refusals of a sampled step (no registered net or
// no head on it: CADM_ESTATE; the net's description, a discrete / sharded ctx, lb >= ub), a head whose lo < -10, this kernel's LDS
int logp_ready(const cadm_ctx* ctx, const char* who) {
    int rc;
    if ((rc = cadm_policy_gauss_check(ctx, who))) return rc;
    cadm_policy_head_params h;
    cadm_policy_head_dev(ctx, nullptr, nullptr, &h);
    CADM_REQUIRE(h.log_std_min >= -10.0f, "%s: the head's log_std_min %g is below -10 (expf(-log_std) must stay finite with a margin)", who,
                 (double)h.log_std_min);
    MlpDev d;
    cadm_policy_dev(ctx, &d, nullptr);
    const size_t lds = logp_lds_bytes(d.dims, d.nlayers, 1, nullptr, nullptr);
    CADM_REQUIRE(lds <= (size_t)MLP_LDS_MAX, "%s: the log-density kernel's activation tiles need %zu bytes of LDS at one row tile, the bound is %d",
                 who, lds, MLP_LDS_MAX);
    return CADM_OK;
}

int logp_space_check(int space, const char* who) {
    CADM_REQUIRE(space == CADM_LOGP_ACTION || space == CADM_LOGP_PRE_SQUASH, "%s: unknown log-density space %d", who, space);
    return CADM_OK;
}

// the launch over a.rows rows: the net's, the head's and the bounds' half of `a` is filled here
int logp_launch(cadm_ctx* ctx, LogpArgs& a, int space, hipStream_t s, const char* who) {
    cadm_policy_head_params h;
    cadm_policy_dev(ctx, &a.net, &a.squash);
    cadm_policy_head_dev(ctx, &a.Wls, &a.bls, &h);
    a.bound = h.bound; a.lo = h.log_std_min; a.hi = h.log_std_max;
    a.space = space;
    a.D = ctx->D; a.A = ctx->A; a.H = ctx->H; a.p = ctx->p;
    a.lb = ctx->cfg.lower_bound; a.ub = ctx->cfg.upper_bound;
    a.mid = 0.5f * (a.ub + a.lb); a.half = 0.5f * (a.ub - a.lb);
    // reward.hip's rule (see the header): two row tiles where four workgroups of them still fit a CU and the rows fill the CUs twice over
    const int RT = mlp_many_tiles(ctx, a.rows) && logp_lds_bytes(a.net.dims, a.net.nlayers, 2, nullptr, nullptr) <= (size_t)MLP_LDS_MAX / 4 ? 2 : 1;
    const size_t lds = logp_lds_bytes(a.net.dims, a.net.nlayers, RT, &a.region0, &a.region1);
    return mlp_launch(ctx, policy_logp_kernel<1>, policy_logp_kernel<2>, RT, lds, a.rows, a, s, who);
}

// both launches behind a rollout's traj [H, m, n, p, D] (n the PACKED candidate count): step [H, m, n, p], then the step sum
int logp_stage(cadm_ctx* ctx, const cadm_policy_logp_params* p, const float* traj, const float* obs, const float* actions, const int32_t* first,
               int m, int n, const float* rows_in, float* rows_out, float* step, float* sum_out, hipStream_t s, const char* who) {
    LogpArgs a{};
    a.traj = traj; a.obs = obs; a.actions = actions; a.first = first; a.n = n;
    a.total = (size_t)m * n * ctx->p;
    a.rows = (size_t)ctx->H * a.total;
    a.out = step;
    int rc;
    if ((rc = logp_launch(ctx, a, p->space, s, who))) return rc;
    if (ctx->disc) hipLaunchKernelGGL(logp_sum_kernel<true>, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, s, step, first, ctx->H,
                                      a.total, p->weight, rows_in, rows_out, sum_out, ctx->disc);
    else hipLaunchKernelGGL(logp_sum_kernel<false>, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, s, step, first, ctx->H, a.total,
                            p->weight, rows_in, rows_out, sum_out, nullptr);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

}  // namespace

// the refusals of the planner's term, before any HIP call: an unknown space, a weight that is not finite, then what the ctx must hold
int cadm_policy_logp_plan_check(const cadm_ctx* ctx, const cadm_policy_logp_params* p, const char* who) {
    int rc;
    if ((rc = logp_space_check(p->space, who))) return rc;
    CADM_REQUIRE(isfinite(p->weight), "%s: the log-density weight %g is not finite", who, (double)p->weight);
    return logp_ready(ctx, who);
}

// the planner's stage: rows [m, n, p] in place
int cadm_launch_policy_logp(cadm_ctx* ctx, const cadm_policy_logp_params* p, const float* traj, const float* obs, const float* actions,
                            const int32_t* first, int m, int n, float* rows, float* step, hipStream_t s) {
    return logp_stage(ctx, p, traj, obs, actions, first, m, n, rows, rows, step, nullptr, s, "cadm_anchored_plan");
}

extern "C" int cadm_policy_logp(cadm_ctx* ctx, const float* x, const float* act, int R, int space, float* logp_out, void* stream) {
    const char* who = "cadm_policy_logp";
    CADM_REQUIRE(ctx && x && act && logp_out, "%s: ctx / x / act / logp_out is null", who);
    CADM_REQUIRE(R >= 1, "%s: R must be >= 1 (got %d)", who, R);
    int rc;
    if ((rc = logp_space_check(space, who))) return rc;
    if ((rc = logp_ready(ctx, who))) return rc;
    CADM_ON_DEVICE(ctx);
    LogpArgs a{};
    a.x = x; a.act = act; a.n = 1; a.total = (size_t)R; a.rows = (size_t)R; a.out = logp_out;
    return logp_launch(ctx, a, space, (hipStream_t)stream, who);
}

extern "C" size_t cadm_policy_logp_workspace_bytes(cadm_ctx* ctx, int m, int n) {
    if (!ctx || m <= 0 || n <= 0) return 0;
    return (size_t)ctx->H * m * n * ctx->p * sizeof(float);
}

extern "C" int cadm_policy_logp_returns(cadm_ctx* ctx, const cadm_policy_logp_params* params, const float* traj, const float* obs,
                                        const float* actions, const int32_t* first, int m, int n, const float* rows_in, float* rows_out,
                                        float* step_out, float* sum_out, void* workspace, void* stream) {
    const char* who = "cadm_policy_logp_returns";
    CADM_REQUIRE(ctx && params && traj && obs && actions && rows_in && rows_out, "%s: ctx / params / traj / obs / actions / rows_in / rows_out is null",
                 who);
    CADM_REQUIRE(step_out || workspace, "%s: without step_out the step log-densities need a workspace", who);
    int rc;
    if ((rc = cadm_policy_logp_plan_check(ctx, params, who))) return rc;
    CADM_REQUIRE(m >= 1 && n >= 1, "%s: m, n must be >= 1 (got m=%d n=%d)", who, m, n);
    CADM_ON_DEVICE(ctx);
    return logp_stage(ctx, params, traj, obs, actions, first, m, n, rows_in, rows_out, step_out ? step_out : (float*)workspace, sum_out,
                      (hipStream_t)stream, who);
}
