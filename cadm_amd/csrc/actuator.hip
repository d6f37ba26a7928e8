// Actuator model of the opt-in planner loop (icem.hip; no reference twin, OPT-IN): what the device that executes a plan can do with it.
//   * action delay: the plan's steps 0 .. d-1 were decided by earlier calls (a committed prefix, per env) and are facts;
//   * rate limits: a step moves an action dim by at most delta_a from the step before, step 0 from the action applied last (prev, per env);
//   * rate cost: sum_t w_a (u_t - u_{t-1})^2 comes off a candidate's score; on a ctx with a discount over the horizon (cadm_set_discount,
//     discount.hip) sum_t disc[t] (w_a (u_t - u_{t-1})^2).
// All three act on the candidate action sequences [m, n, H, A], not on trajectories: ONE kernel between the sampler (and the injections
// and the knot shaping) and the rollout, and one subtraction behind the score.  The rollout kernels are not touched.  The semantics are
// restated in include/cadm_hip.h (cadm_actuate_actions).
//
// Mapping: one thread per (env, candidate, action dim) chain, steps in ascending order -- a step reads what the step before wrote, so a
// chain is serial.  A workgroup owns floor(ACT_THREADS / A) whole candidates: the A threads of a candidate are neighbours, their A floats of
// a step are contiguous, and a candidate's dims meet in LDS, where the thread of dim 0 adds them in ascending order.
// Reduction contract (tracking.hip's): a chain is one thread's; a candidate's cost is ((c_0 + c_1) + c_2) + ... by one thread; no
// floating-point atomics; nothing depends on the grid, on m or n, or on the row's position.
#include <math.h>

#include "planner.h"

namespace {

constexpr int ACT_THREADS = 256;

struct ActArgs {
    float* seqs;               // [m, n, H, A], in place
    const float* prev;         // [m, A], or null: unknown (NaN) everywhere
    const float* prefix;       // [m, d, A], or null: nothing committed
    float* cost;               // [m, n], or null
    const float* disc;         // [H + 1] the ctx's discount table (DISC kernel only)
    size_t cands;              // m * n
    int n, H, A, cpb;          // cpb: candidates per workgroup
    float lb, ub;
    cadm_actuator_params c;
};

// clip by comparisons, not fminf / fmaxf (which drop a NaN operand): a NaN x stays NaN, and a zero keeps its sign unless a bound replaces it
__device__ __forceinline__ float act_clip(float x, float lo, float hi) {
    const float v = x < lo ? lo : x;
    return v > hi ? hi : v;
}

// DISC: the ctx's discount over the horizon (discount.hip): c_a = c_a + disc[t] * (w_a (y - last)^2).  false: the kernel as it was
template <bool DISC>
__global__ __launch_bounds__(ACT_THREADS) void actuate_kernel(const ActArgs a) {
    __shared__ float sc[ACT_THREADS];
    const int tid = threadIdx.x, A = a.A;
    const int lc = tid / A, dim = tid - lc * A;
    const size_t mc = (size_t)blockIdx.x * a.cpb + lc;           // mi * n + c
    const bool live = lc < a.cpb && mc < a.cands;
    float cost = 0.0f;
    if (live) {
        const size_t mi = mc / (size_t)a.n;
        const int d = a.c.delay;
        const float dl = a.c.rate_limit[dim], w = a.c.rate_w[dim];
        const bool limited = dl < INFINITY;
        const float nan = __uint_as_float(0x7fc00000u);
        float last = a.prev ? a.prev[mi * A + dim] : nan;
        const float* pin = a.prefix ? a.prefix + mi * (size_t)d * A + dim : nullptr;
        float* u = a.seqs + mc * (size_t)a.H * A + dim;
        for (int t = 0; t < a.H; ++t) {
            const float x = u[(size_t)t * A];
            const float f = (pin && t < d) ? pin[(size_t)t * A] : nan;
            const bool known = last == last;
            float y = x;
            if (f == f) {
                y = f;                                           // a fact: neither limited nor clipped
            } else if (limited && known) {
                const float lo = last - dl, hi = last + dl;      // one rounding each
                y = act_clip(act_clip(x, lo, hi), a.lb, a.ub);
            }
            if (known) {
                const float e = y - last;
                const float sq = e * e;
                cost = DISC ? __fadd_rn(cost, __fmul_rn(a.disc[t], __fmul_rn(w, sq))) : cost + w * sq;
            }
            u[(size_t)t * A] = y;
            last = y;
        }
    }
    if (!a.cost) return;                                         // (uniform over the grid)
    sc[tid] = cost;
    __syncthreads();
    if (live && dim == 0) {
        float s = sc[tid];
        for (int k = 1; k < A; ++k) s = s + sc[tid + k];
        a.cost[mc] = s;
    }
}

__global__ void actuator_sub_kernel(float* __restrict__ cand, const float* __restrict__ cost, size_t total) {
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) cand[q] = cand[q] - cost[q];
}

// prev <- plan[:, 0], prefix[:, j] <- plan[:, 1 + j] for j < d (d < H: step 1 + j exists)
__global__ void actuator_advance_kernel(const float* __restrict__ plan, float* __restrict__ prev, float* __restrict__ prefix, int m, int d,
                                        int H, int A) {
    const size_t per = (size_t)(d + 1) * A, total = (size_t)m * per;
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
        const size_t mi = q / per;
        const int e = (int)(q - mi * per);                       // step * A + dim, steps 0 .. d
        const float v = plan[mi * (size_t)H * A + e];
        if (e < A) prev[mi * A + e] = v;
        else prefix[mi * (size_t)d * A + (e - A)] = v;
    }
}

}  // namespace

// the refusals of an actuator model, before any HIP call
int cadm_actuator_check(const cadm_ctx* ctx, const cadm_actuator_params* c, const char* who) {
    CADM_REQUIRE(c, "%s: the actuator parameters are null", who);
    CADM_REQUIRE(!ctx->cfg.discrete && ctx->cfg.env_kind != CADM_ENV_CARTPOLE, "%s: the actuator model needs a continuous-action ctx (discrete "
                 "actions are planned by random shooting)", who);
    CADM_REQUIRE(!cadm_sharded(ctx), "%s: the actuator model is not supported on a candidate-sharded ctx", who);
    CADM_REQUIRE(ctx->A <= CADM_MAX_ACT_DIMS, "%s: %d action dims, the actuator parameters hold %d", who, ctx->A, CADM_MAX_ACT_DIMS);
    CADM_REQUIRE(c->n_dims == 0 || c->n_dims == ctx->A, "%s: the actuator parameters were built for %d action dims, this ctx has %d", who,
                 c->n_dims, ctx->A);
    CADM_REQUIRE(c->delay >= 0 && c->delay < ctx->H, "%s: action delay %d outside 0 .. %d (the horizon less one)", who, c->delay, ctx->H - 1);
    for (int k = 0; k < ctx->A; ++k) {
        CADM_REQUIRE(c->rate_limit[k] > 0.0f, "%s: action dim %d: rate limit %g is not > 0 (+inf: none)", who, k, (double)c->rate_limit[k]);
        CADM_REQUIRE(isfinite(c->rate_w[k]) && c->rate_w[k] >= 0.0f, "%s: action dim %d: rate cost %g is not finite and >= 0", who, k,
                     (double)c->rate_w[k]);
    }
    return CADM_OK;
}

int cadm_launch_actuate(cadm_ctx* ctx, const cadm_actuator_params* prm, const float* prev, const float* prefix, int m, int n, float* seqs,
                        float* cost_out, hipStream_t s) {
    ActArgs a{};
    a.seqs = seqs; a.prev = prev; a.prefix = prm->delay > 0 ? prefix : nullptr; a.cost = cost_out;
    a.cands = (size_t)m * n; a.n = n; a.H = ctx->H; a.A = ctx->A; a.cpb = ACT_THREADS / ctx->A;
    a.lb = ctx->cfg.lower_bound; a.ub = ctx->cfg.upper_bound;
    a.c = *prm;
    const size_t blocks = (a.cands + a.cpb - 1) / a.cpb;
    CADM_REQUIRE(blocks <= 0x7fffffffull, "actuate: %zu candidates are too many for one launch", a.cands);
    a.disc = cost_out ? ctx->disc : nullptr;      // (without a cost the discount has nothing to weigh: pins, limits and sequences are untouched)
    if (a.disc) hipLaunchKernelGGL(actuate_kernel<true>, dim3((unsigned)blocks), dim3(ACT_THREADS), 0, s, a);
    else hipLaunchKernelGGL(actuate_kernel<false>, dim3((unsigned)blocks), dim3(ACT_THREADS), 0, s, a);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

int cadm_launch_actuator_sub(float* cand, const float* cost, size_t total, hipStream_t s) {
    const size_t g = (total + 255) / 256;
    hipLaunchKernelGGL(actuator_sub_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, s, cand, cost, total);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

int cadm_launch_actuator_advance(cadm_ctx* ctx, const cadm_actuator_params* prm, const float* plan, float* prev, float* prefix, int m,
                                 hipStream_t s) {
    const size_t total = (size_t)m * (prm->delay + 1) * ctx->A, g = (total + 255) / 256;
    hipLaunchKernelGGL(actuator_advance_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, s, plan, prev, prefix, m, prm->delay,
                       ctx->H, ctx->A);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

extern "C" int cadm_actuate_actions(cadm_ctx* ctx, const cadm_actuator_params* params, const float* prev, const float* prefix, int m, int n,
                                    float* seqs_io, float* cost_out, void* stream) {
    CADM_REQUIRE(ctx && params && seqs_io && m > 0 && n > 0, "cadm_actuate_actions: bad arguments");
    int rc = cadm_actuator_check(ctx, params, "cadm_actuate_actions");
    if (rc) return rc;
    CADM_ON_DEVICE(ctx);
    return cadm_launch_actuate(ctx, params, prev, prefix, m, n, seqs_io, cost_out, (hipStream_t)stream);
}
