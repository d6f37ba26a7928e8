// State constraints and early termination of the opt-in planner loop (icem.hip): what a candidate's particle returns become when the
// predicted trajectory leaves a region the caller declared healthy.  No reference twin: the reference scores the sum of the step
// rewards over all H steps, whatever the states.  One kernel BEHIND the rollout, like the score (score.hip) and the forecast
// (forecast.hip): it reads the trajectories the rollout recorded (`traj_out`, [H, m, n, p, D]) and rewrites the rollout's returns
// (rows [m, n, p]); the rollout kernels are not touched.
//
// A constraint reads one observation dim d: healthy iff x[d] > lo && x[d] < hi in float32, for every constraint.  A value equal to a
// bound violates; so does NaN or +-inf in a constrained dim (the comparisons are false); other dims are not looked at.  What is
// checked is the POST-step state traj[t] of every step t = 0 .. H - 1, never the observation the call starts from.  Per row (one
// particle of one candidate):
//     violations       the number of steps whose post-step state violates
//     first_violation  the first such step, H if there is none
//     PENALTY          rows' = rows - w * (float)violations                       (one fp32 multiply, one subtract)
//     TERMINATE        rows' = (r_0 + r_1 + ... + r_tau) - w,  tau = first_violation < H -- r_t the step reward of step_reward.h
//                      (pre-step state, post-step state, raw action), added in step order from r_0; the step that leaves still pays;
//                      nothing the trajectory holds after tau reaches the return
// A row without a violation keeps its input bits in both modes.
// On a ctx with a discount over the horizon (cadm_set_discount, discount.hip; disc[t] its table):
//     PENALTY          pen = pen + disc[t] on the violating steps, ascending t from 0.0f;  rows' = rows - w * pen; the counters are unchanged
//     TERMINATE        sum = disc[0] r_0, sum = sum + disc[t] r_t up to tau;  rows' = sum - w * disc[tau]: the penalty is paid at the step that leaves
//
// Mapping and traffic: a workgroup owns CN_ROWS consecutive rows, one thread per row; its CN_THREADS threads (four waves) all load.
// For a fixed step those rows' D values are ONE contiguous span of `traj`, loaded lane-linear into an LDS tile (16-byte loads where the
// span is 16-byte aligned, scalar loads otherwise); every value of `traj` is read at most once.  A step is a chain of load, barrier,
// test: with one wave the span's loads go out one after the other and their latency is the kernel's time, so three more waves share
// them.  TERMINATE keeps two tiles -- the other one still holds the previous step, the pre-step state of the reward (step 0: the
// observation) -- PENALTY one.  A workgroup of TERMINATE whose rows have all terminated stops loading, unless the caller asked for the
// violation counts.
// Reduction contract: a row's counters and partial sum are one thread's chain in step order; no floating-point atomics, nothing
// depends on the grid, on m or n, or on the row's position: the same bits run to run and inside any batch.
#include <math.h>

#include "step_reward.h"

namespace {

constexpr int CN_ROWS = 64;                  // rows per workgroup: the first wave's threads, one row each
constexpr int CN_THREADS = 256;              // threads per workgroup: all of them load
constexpr int CN_LDS_BUDGET = 48 * 1024;     // two tiles of CN_ROWS * D floats, below the 64 KiB a kernel gets without an attribute

struct ConstrainArgs {
    const float *traj, *obs, *actions, *rows_in;
    const float* disc;         // [H + 1] the ctx's discount table (DISC kernels only)
    float* rows_out;
    int32_t *first, *viol;
    size_t total;              // m * n * p rows
    int np;                    // n * p: rows per env
    int H, p, D, A, term;
    cadm_constraint_params c;
    ForecastSpec spec;
};

// DISC: the ctx's discount over the horizon (discount.hip).  false: the undiscounted kernel, instruction for instruction what it was
template <int ENV, bool DISC>
__global__ __launch_bounds__(CN_THREADS) void constrain_returns_kernel(const ConstrainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cn_smem[];
    const int D = a.D, H = a.H, ts = (CN_ROWS * D + 3) & ~3, tid = threadIdx.x;
    const size_t q0 = (size_t)blockIdx.x * CN_ROWS;      // first row of this workgroup (q0 < total: the grid is ceil(total / CN_ROWS))
    const int nr = a.total - q0 < (size_t)CN_ROWS ? (int)(a.total - q0) : CN_ROWS;
    const int span = nr * D;
    const bool mine = tid < nr;
    const size_t q = q0 + tid;
    if (a.term) {
        // step 0's pre-step state: obs[mi] for every row, in the tile step 0 does not load into
        for (int i = tid; i < span; i += CN_THREADS) {
            const int r = i / D;
            cn_smem[ts + i] = a.obs[((q0 + r) / (size_t)a.np) * D + (i - r * D)];
        }
    }
    const float* act = a.term && mine ? a.actions + (q / (size_t)a.p) * H * a.A : nullptr;      // the row's sequence: [H, A]
    int count = 0, first = H;
    float sum = 0.0f, pen = 0.0f, dfirst = 0.0f;      // (DISC: the discounted count; disc[first])
    for (int t = 0; t < H; ++t) {
        float* cur = cn_smem + (a.term ? (t & 1) * ts : 0);
        const float* pre = cn_smem + ((t & 1) ^ 1) * ts;
        const float* src = a.traj + ((size_t)t * a.total + q0) * D;
        const int nvec = (reinterpret_cast<uintptr_t>(src) & 15) == 0 ? span >> 2 : 0;
        for (int i = tid; i < nvec; i += CN_THREADS) reinterpret_cast<floatx4*>(cur)[i] = reinterpret_cast<const floatx4*>(src)[i];
        for (int i = 4 * nvec + tid; i < span; i += CN_THREADS) cur[i] = src[i];
        __syncthreads();
        if (mine) {
            const float* x = cur + tid * D;
            bool bad = false;
            for (int k = 0; k < a.c.n; ++k) {
                const float v = x[a.c.dim[k]];
                bad = bad || !(v > a.c.lo[k] && v < a.c.hi[k]);
            }
            if (a.term && first == H) {          // still alive before this step: it pays, also when it leaves
                const float r = step_reward<ENV>(a.spec, D, a.A, pre + tid * D, x, act + (size_t)t * a.A);
                if constexpr (DISC) {
                    const float dr = __fmul_rn(a.disc[t], r);    // (one product, then one add: never an fma)
                    sum = t == 0 ? dr : __fadd_rn(sum, dr);
                } else {
                    sum = t == 0 ? r : sum + r;
                }
            }
            if (bad) {
                ++count;
                if constexpr (DISC) {
                    pen = __fadd_rn(pen, a.disc[t]);
                    if (first == H) dfirst = a.disc[t];
                }
                if (first == H) first = t;
            }
        }
        // every read of the tile the next step loads over is done; TERMINATE without counts: leave when no row is alive
        if (a.term && !a.viol) {
            if (__syncthreads_count(mine && first == H) == 0) break;
        } else {
            __syncthreads();
        }
    }
    if (!mine) return;
    const float r_in = a.rows_in[q];
    float r_out = r_in;
    if (a.term) {
        if constexpr (DISC) {
            if (first < H) r_out = __fsub_rn(sum, __fmul_rn(a.c.weight, dfirst));      // the penalty is paid at the step that leaves
        } else {
            if (first < H) r_out = sum - a.c.weight;
        }
    } else if (count > 0) {
        if constexpr (DISC) r_out = __fsub_rn(r_in, __fmul_rn(a.c.weight, pen));
        else r_out = r_in - a.c.weight * (float)count;
    }
    a.rows_out[q] = r_out;
    if (a.first) a.first[q] = first;
    if (a.viol) a.viol[q] = count;
}

size_t constrain_lds_bytes(int D, int term) { return (size_t)(term ? 2 : 1) * (((size_t)CN_ROWS * D + 3) & ~(size_t)3) * sizeof(float); }

template <int ENV>
int constrain_launch(const ConstrainArgs& a, size_t blocks, size_t lds, hipStream_t s) {
    if (a.disc) hipLaunchKernelGGL((constrain_returns_kernel<ENV, true>), dim3((unsigned)blocks), dim3(CN_THREADS), lds, s, a);
    else hipLaunchKernelGGL((constrain_returns_kernel<ENV, false>), dim3((unsigned)blocks), dim3(CN_THREADS), lds, s, a);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

}  // namespace

// the refusals of a constraint set, before any HIP call
int cadm_constraint_check(const cadm_ctx* ctx, const cadm_constraint_params* c, const char* who) {
    CADM_REQUIRE(c, "%s: the constraint parameters are null", who);
    CADM_REQUIRE(c->n >= 1 && c->n <= CADM_MAX_CONSTRAINTS, "%s: %d constraints, outside 1 .. %d", who, c->n, CADM_MAX_CONSTRAINTS);
    CADM_REQUIRE(c->mode == CADM_CONSTRAIN_PENALTY || c->mode == CADM_CONSTRAIN_TERMINATE, "%s: unknown constraint mode %d", who, c->mode);
    CADM_REQUIRE(isfinite(c->weight) && c->weight >= 0.0f, "%s: constraint weight %g is not finite and >= 0", who, (double)c->weight);
    for (int k = 0; k < c->n; ++k) {
        CADM_REQUIRE(c->dim[k] >= 0 && c->dim[k] < ctx->D, "%s: constraint %d reads dim %d, outside 0 .. %d", who, k, c->dim[k], ctx->D - 1);
        CADM_REQUIRE(!isnan(c->lo[k]) && !isnan(c->hi[k]), "%s: constraint %d has a NaN bound", who, k);
        CADM_REQUIRE(c->lo[k] < c->hi[k], "%s: constraint %d: lo %g >= hi %g", who, k, (double)c->lo[k], (double)c->hi[k]);
        CADM_REQUIRE(!(isinf(c->lo[k]) && isinf(c->hi[k])), "%s: constraint %d has no finite bound (both sides infinite)", who, k);
    }
    CADM_REQUIRE(!ctx->cfg.discrete && ctx->cfg.env_kind != CADM_ENV_CARTPOLE, "%s: state constraints need a continuous-action ctx (discrete "
                 "actions are planned by random shooting)", who);
    CADM_REQUIRE(!cadm_sharded(ctx), "%s: state constraints are not supported on a candidate-sharded ctx", who);
    CADM_REQUIRE(constrain_lds_bytes(ctx->D, c->mode == CADM_CONSTRAIN_TERMINATE) <= (size_t)CN_LDS_BUDGET,
                 "%s: D (%d) does not fit the kernel's LDS: its tiles of %d x D floats need %zu bytes, the bound is %d", who, ctx->D, CN_ROWS,
                 constrain_lds_bytes(ctx->D, c->mode == CADM_CONSTRAIN_TERMINATE), CN_LDS_BUDGET);
    if (c->mode == CADM_CONSTRAIN_TERMINATE && ctx->cfg.env_kind == CADM_ENV_SPEC && !ctx->spec_set) {
        cadm_set_error("%s: the env spec is not set (call cadm_set_env_spec): a terminated return is summed from its reward terms", who);
        return CADM_ESTATE;
    }
    return CADM_OK;
}

extern "C" int cadm_constrain_returns(cadm_ctx* ctx, const cadm_constraint_params* prm, const float* traj, const float* obs,
                                      const float* actions, const float* rows_in, int m, int n, float* rows_out,
                                      int32_t* first_violation_out, int32_t* violations_out, void* stream) {
    CADM_REQUIRE(ctx && prm && traj && rows_in && rows_out, "cadm_constrain_returns: ctx / params / traj / rows_in / rows_out is null");
    int rc;
    if ((rc = cadm_constraint_check(ctx, prm, "cadm_constrain_returns"))) return rc;
    const int term = prm->mode == CADM_CONSTRAIN_TERMINATE;
    CADM_REQUIRE(!term || (obs && actions), "cadm_constrain_returns: obs / actions required in terminate mode");
    CADM_REQUIRE(m >= 1 && n >= 1, "cadm_constrain_returns: m, n must be >= 1 (got m=%d n=%d)", m, n);
    CADM_REQUIRE((long long)n * ctx->p <= 0x7fffffffLL, "cadm_constrain_returns: n * p = %lld rows per env are too many", (long long)n * ctx->p);
    const size_t total = (size_t)m * n * ctx->p, blocks = (total + CN_ROWS - 1) / CN_ROWS;
    CADM_REQUIRE(blocks <= 0x7fffffffull, "cadm_constrain_returns: %zu rows are too many for one launch", total);
    CADM_ON_DEVICE(ctx);
    ConstrainArgs a{};
    a.traj = traj; a.obs = obs; a.actions = actions; a.rows_in = rows_in; a.rows_out = rows_out;
    a.first = first_violation_out; a.viol = violations_out; a.disc = ctx->disc;
    a.total = total; a.np = n * ctx->p; a.H = ctx->H; a.p = ctx->p; a.D = ctx->D; a.A = ctx->A; a.term = term;
    a.c = *prm;
    if (term) forecast_spec_fill(ctx, &a.spec);
    const size_t lds = constrain_lds_bytes(ctx->D, term);
    hipStream_t s = (hipStream_t)stream;
    switch (ctx->cfg.env_kind) {
        case CADM_ENV_HALFCHEETAH: return constrain_launch<CADM_ENV_HALFCHEETAH>(a, blocks, lds, s);
        case CADM_ENV_ANT: return constrain_launch<CADM_ENV_ANT>(a, blocks, lds, s);
        case CADM_ENV_SLIM_HUMANOID: return constrain_launch<CADM_ENV_SLIM_HUMANOID>(a, blocks, lds, s);
        case CADM_ENV_PENDULUM: return constrain_launch<CADM_ENV_PENDULUM>(a, blocks, lds, s);
        default: return constrain_launch<CADM_ENV_SPEC>(a, blocks, lds, s);
    }
}
