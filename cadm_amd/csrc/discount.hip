// A discount over the horizon of the opt-in planner loop (icem.hip): every quantity that enters a candidate's score is weighted per
// step by ONE table disc[0 .. H], disc[t] = (float)pow((double)gamma, (double)t), disc[0] = 1 exactly, which the ctx owns
// (cadm_set_discount).  No reference twin: the reference's planner sums the step rewards undiscounted.  The table is state of the ctx,
// as H is: the stages behind the rollout (constrain.hip, tracking.hip, reward.hip, uncertainty.hip, actuator.hip, value.hip, critic.hip)
// read it from there, in the loop and in their stand-alone calls; with no table (gamma == 1) every launch is the undiscounted one.
//
// The kernel here is the env's own return.  The rollout kernels add the step rewards in registers, undiscounted, and are not touched:
// on a discounted ctx the loop launches this stage directly BEHIND the rollout and in front of the constraints, and it rewrites rows
// [m, n, p] from the recorded trajectories traj [H, m, n, p, D]:
//     sum = disc[0] * r_0;  for t = 1 .. H - 1:  sum = sum + disc[t] * r_t          (one fp32 product, one fp32 add per step)
//     rows_out[q] = isnan(rows_in[q]) ? rows_in[q] : sum
// r_t the step reward of step_reward.h (pre-step state: obs at t = 0, else traj[t - 1]; post-step state traj[t]; the raw action of the
// candidate buffer), as constrain.hip's TERMINATE form takes it.  step_out [H, m, n, p] (optional) takes the undiscounted r_t.
//
// Mapping and traffic: constrain.hip's TERMINATE mapping without its tests.  A workgroup owns DC_ROWS consecutive rows, one thread per
// row; its DC_THREADS threads (four waves) all load.  For a fixed step those rows' D values are ONE contiguous span of `traj`, loaded
// lane-linear into one of two LDS tiles (16-byte loads where the span is 16-byte aligned, scalar loads otherwise); the other tile still
// holds the pre-step state; every value of `traj` is read from memory once.  The table goes through LDS once per workgroup.
// Reduction contract: a row's sum is one thread's chain in ascending t; no floating-point atomics, nothing depends on the grid, on m or
// n, or on the row's position: the same bits run to run and inside any batch.
#include <math.h>

#include "step_reward.h"

namespace {

constexpr int DC_ROWS = 64;                  // rows per workgroup: the first wave's threads, one row each
constexpr int DC_THREADS = 256;              // threads per workgroup: all of them load
constexpr int DC_LDS_BUDGET = 48 * 1024;     // two tiles of DC_ROWS * D floats and the table, below the 64 KiB a kernel gets without an attribute

struct DiscountArgs {
    const float *traj, *obs, *actions, *rows_in, *disc;
    float *rows_out, *step_out;
    size_t total;              // m * n * p rows
    int np;                    // n * p: rows per env
    int H, p, D, A;
    ForecastSpec spec;
};

template <int ENV>
__global__ __launch_bounds__(DC_THREADS) void discount_returns_kernel(const DiscountArgs a) {
    extern __shared__ __attribute__((aligned(16))) float dc_smem[];
    const int D = a.D, H = a.H, ts = (DC_ROWS * D + 3) & ~3, tid = threadIdx.x;
    float* sdisc = dc_smem + 2 * ts;                     // [H] the weights of the steps
    const size_t q0 = (size_t)blockIdx.x * DC_ROWS;      // first row of this workgroup (q0 < total: the grid is ceil(total / DC_ROWS))
    const int nr = a.total - q0 < (size_t)DC_ROWS ? (int)(a.total - q0) : DC_ROWS;
    const int span = nr * D;
    const bool mine = tid < nr;
    const size_t q = q0 + tid;
    // step 0's pre-step state: obs[mi] for every row, in the tile step 0 does not load into
    for (int i = tid; i < span; i += DC_THREADS) {
        const int r = i / D;
        dc_smem[ts + i] = a.obs[((q0 + r) / (size_t)a.np) * D + (i - r * D)];
    }
    for (int t = tid; t < H; t += DC_THREADS) sdisc[t] = a.disc[t];
    const float* act = mine ? a.actions + (q / (size_t)a.p) * H * a.A : nullptr;      // the row's sequence: [H, A]
    float sum = 0.0f;
    for (int t = 0; t < H; ++t) {
        float* cur = dc_smem + (t & 1) * ts;
        const float* pre = dc_smem + ((t & 1) ^ 1) * ts;
        const float* src = a.traj + ((size_t)t * a.total + q0) * D;
        const int nvec = (reinterpret_cast<uintptr_t>(src) & 15) == 0 ? span >> 2 : 0;
        for (int i = tid; i < nvec; i += DC_THREADS) reinterpret_cast<floatx4*>(cur)[i] = reinterpret_cast<const floatx4*>(src)[i];
        for (int i = 4 * nvec + tid; i < span; i += DC_THREADS) cur[i] = src[i];
        __syncthreads();
        if (mine) {
            const float r = step_reward<ENV>(a.spec, D, a.A, pre + tid * D, cur + tid * D, act + (size_t)t * a.A);
            const float dr = __fmul_rn(sdisc[t], r);             // (one product, then one add: never an fma)
            sum = t == 0 ? dr : __fadd_rn(sum, dr);
            if (a.step_out) a.step_out[(size_t)t * a.total + q] = r;
        }
        __syncthreads();      // every read of the tile the next step loads over is done
    }
    if (!mine) return;
    const float r_in = a.rows_in[q];
    a.rows_out[q] = r_in != r_in ? r_in : sum;
}

size_t discount_lds_bytes(int D, int H) { return (2 * (((size_t)DC_ROWS * D + 3) & ~(size_t)3) + (size_t)H) * sizeof(float); }

template <int ENV>
int discount_launch(const DiscountArgs& a, size_t blocks, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(discount_returns_kernel<ENV>, dim3((unsigned)blocks), dim3(DC_THREADS), lds, s, a);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

}  // namespace

void cadm_discount_free(cadm_ctx* ctx) {
    if (ctx->disc_buf) (void)hipFree(ctx->disc_buf);
    ctx->disc_buf = nullptr;
    ctx->disc = nullptr;
    ctx->disc_host.clear();
}

// the refusals of a discount, before any HIP call
int cadm_discount_check(const cadm_ctx* ctx, const char* who) {
    CADM_REQUIRE(!ctx->cfg.discrete && ctx->cfg.env_kind != CADM_ENV_CARTPOLE, "%s: a discount over the horizon needs a continuous-action ctx "
                 "(discrete actions are planned by random shooting)", who);
    CADM_REQUIRE(!cadm_sharded(ctx), "%s: a discount over the horizon is not supported on a candidate-sharded ctx", who);
    CADM_REQUIRE(discount_lds_bytes(ctx->D, ctx->H) <= (size_t)DC_LDS_BUDGET,
                 "%s: D (%d) does not fit the discount kernel's LDS: its two tiles of %d x D floats and the %d weights need %zu bytes, the "
                 "bound is %d", who, ctx->D, DC_ROWS, ctx->H, discount_lds_bytes(ctx->D, ctx->H), DC_LDS_BUDGET);
    if (ctx->cfg.env_kind == CADM_ENV_SPEC && !ctx->spec_set) {
        cadm_set_error("%s: the env spec is not set (call cadm_set_env_spec): a discounted return is summed from its reward terms", who);
        return CADM_ESTATE;
    }
    return CADM_OK;
}

extern "C" int cadm_set_discount(cadm_ctx* ctx, float gamma, void* stream) {
    CADM_REQUIRE(ctx, "cadm_set_discount: ctx is null");
    CADM_REQUIRE(gamma > 0.0f && gamma <= 1.0f, "cadm_set_discount: the discount %g is not in (0, 1]", (double)gamma);      // (NaN: false)
    if (gamma == 1.0f) {      // none: every launch is the undiscounted one
        ctx->disc = nullptr;
        ctx->disc_host.clear();
        return CADM_OK;
    }
    int rc;
    if ((rc = cadm_discount_check(ctx, "cadm_set_discount"))) return rc;
    const int H = ctx->H;
    std::vector<float> tab((size_t)H + 1);
    tab[0] = 1.0f;
    for (int t = 1; t <= H; ++t) tab[t] = (float)pow((double)gamma, (double)t);
    CADM_ON_DEVICE(ctx);
    if (!ctx->disc_buf) {
        hipError_t e = hipMalloc(&ctx->disc_buf, ((size_t)H + 1) * sizeof(float));
        if (e != hipSuccess) {
            ctx->disc_buf = nullptr;
            cadm_set_error("cadm_set_discount: hipMalloc failed (%s)", hipGetErrorString(e));
            return CADM_ENOMEM;
        }
    }
    // the copy is ordered on `stream` behind whatever still reads the table there; the host vector is a local: wait for the copy
    CADM_CHECK_HIP(hipMemcpyAsync(ctx->disc_buf, tab.data(), ((size_t)H + 1) * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)stream));
    CADM_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    ctx->disc_host.swap(tab);
    ctx->disc = ctx->disc_buf;
    return CADM_OK;
}

extern "C" int cadm_discount_weights(cadm_ctx* ctx, float* host_out, int* set_out) {
    CADM_REQUIRE(ctx && set_out, "cadm_discount_weights: ctx / set_out is null");
    *set_out = ctx->disc != nullptr;
    if (ctx->disc && host_out)
        for (int t = 0; t <= ctx->H; ++t) host_out[t] = ctx->disc_host[t];
    return CADM_OK;
}

// the stage of the loop: rows [m, n, p] from traj [H, m, n, p, D] (n the PACKED candidate count); the ctx's table is set
int cadm_launch_discount(cadm_ctx* ctx, const float* traj, const float* obs, const float* actions, int m, int n, const float* rows_in,
                         float* rows_out, float* step_out, hipStream_t s) {
    const size_t total = (size_t)m * n * ctx->p, blocks = (total + DC_ROWS - 1) / DC_ROWS;
    CADM_REQUIRE((long long)n * ctx->p <= 0x7fffffffLL, "discounted return: n * p = %lld rows per env are too many", (long long)n * ctx->p);
    CADM_REQUIRE(blocks <= 0x7fffffffull, "discounted return: %zu rows are too many for one launch", total);
    DiscountArgs a{};
    a.traj = traj; a.obs = obs; a.actions = actions; a.rows_in = rows_in; a.disc = ctx->disc; a.rows_out = rows_out; a.step_out = step_out;
    a.total = total; a.np = n * ctx->p; a.H = ctx->H; a.p = ctx->p; a.D = ctx->D; a.A = ctx->A;
    forecast_spec_fill(ctx, &a.spec);
    const size_t lds = discount_lds_bytes(ctx->D, ctx->H);
    switch (ctx->cfg.env_kind) {
        case CADM_ENV_HALFCHEETAH: return discount_launch<CADM_ENV_HALFCHEETAH>(a, blocks, lds, s);
        case CADM_ENV_ANT: return discount_launch<CADM_ENV_ANT>(a, blocks, lds, s);
        case CADM_ENV_SLIM_HUMANOID: return discount_launch<CADM_ENV_SLIM_HUMANOID>(a, blocks, lds, s);
        case CADM_ENV_PENDULUM: return discount_launch<CADM_ENV_PENDULUM>(a, blocks, lds, s);
        default: return discount_launch<CADM_ENV_SPEC>(a, blocks, lds, s);
    }
}

extern "C" int cadm_discount_returns(cadm_ctx* ctx, const float* traj, const float* obs, const float* actions, int m, int n,
                                     const float* rows_in, float* rows_out, float* step_out, void* stream) {
    CADM_REQUIRE(ctx && traj && obs && actions && rows_in && rows_out, "cadm_discount_returns: ctx / traj / obs / actions / rows_in / rows_out is null");
    CADM_REQUIRE(m >= 1 && n >= 1, "cadm_discount_returns: m, n must be >= 1 (got m=%d n=%d)", m, n);
    if (!ctx->disc) {
        cadm_set_error("cadm_discount_returns: no discount is set (call cadm_set_discount with gamma < 1)");
        return CADM_ESTATE;
    }
    int rc;
    if ((rc = cadm_discount_check(ctx, "cadm_discount_returns"))) return rc;      // (a spec taken away since the discount was set)
    CADM_ON_DEVICE(ctx);
    return cadm_launch_discount(ctx, traj, obs, actions, m, n, rows_in, rows_out, step_out, (hipStream_t)stream);
}
