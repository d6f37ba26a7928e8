// Ensemble disagreement as a cost of the opt-in planner loop (icem.hip; no reference twin, OPT-IN): the spread of the particles over the
// STATES a candidate's plan visits, per step -- the forecast's var_epistemic / var_total (forecast.hip), turned from a diagnostic of a
// handful of plans into a term of every candidate's score.  Pessimistic (lambda > 0: stay where the members agree, the MOPO / MOReL
// penalty) or curious (lambda < 0: go where they do not).  Kernels BEHIND the rollout, like the constraints (constrain.hip) and the
// tracking targets (tracking.hip): they read the trajectories the rollout recorded (`traj_out`, [H, m, n, p, D]); the rollout kernels
// are not touched.  The arithmetic is restated in include/cadm_hip.h (cadm_uncertainty_cost).
//
// Per candidate (mi, c), step t and dim d with w_d > 0, over x_j = traj[t, mi, c, j, d] (particle j belongs to member j / (p / E)):
// the variance v by forecast_stats_kernel's chain, relative to particle 0;  u_t = sum_d w_d v[t, d] (ascending d, from the first
// term), sqrtf of it (STD), the cap by a comparison;  cost = sum of u_t over the counted steps (all, or t <= min_j first[mi, c, j]) in
// step order from 0;  in the loop cand' = cand - lambda cost.  On a ctx with a discount over the horizon (cadm_set_discount, discount.hip)
// cost = cost + disc[t] u_t, u_t taken behind the form and the cap, in both kernels that add; u [m, n, H] stays undiscounted.
//
// Mapping: the forecast kernel's (one workgroup per sequence, D busy threads, an H-long chain of loads) is the wrong one for every
// candidate of an iteration.  Here a work item is (a group of G consecutive candidates, ONE step): the grid is ceil(m n / G) x H, and no
// workgroup waits for H loads in turn.  For a fixed step the group's G p D floats are ONE contiguous span of `traj`, loaded lane-linear
// into an LDS tile (16-byte loads where the span is 16-byte aligned, scalar loads otherwise: odd D or p); every value of `traj` is read
// from memory once.  Behind a barrier one thread per (candidate, dim) runs the variance chain out of LDS (stride D: neighbouring dims
// are neighbouring banks) and leaves v in LDS; behind another, one thread per candidate adds the weighted variances in ascending d and
// writes u[mi, c, t].  Groups may span envs; the last one is partial.  G is chosen by the host (the LDS budget), the weights go through
// LDS.  A second kernel, one thread per candidate, takes the cut from `first` (a min over p ints), adds the counted steps in order and
// writes the cost, and in the loop takes lambda cost off the candidate score.  Without a step_out the exported call has nowhere to
// keep u: one kernel then walks the steps itself (the same body, the same chains, cost added by the candidate's thread).
// Reduction contract: every v, every u_t and every cost is ONE thread's chain in the order above; no floating-point atomics; nothing
// depends on G, on the grid, on m or n, or on the candidate's position: the same bits run to run and inside any batch.
#include <math.h>

#include "planner.h"

namespace {

constexpr int UNC_THREADS = 256;
constexpr int UNC_GROUP = 8;                  // candidates per workgroup at most (fewer where the tile would not fit)
constexpr int UNC_LDS_BUDGET = 48 * 1024;     // the tile of G * p * D floats, G * D variances and D weights; below the 64 KiB a kernel gets without an attribute

struct UncArgs {
    const float* traj;         // [H, m, n, p, D]
    const int32_t* first;      // [m, n, p], or null
    float* step;               // [m, n, H], or null (the walking kernel only)
    float* cost;               // [m, n] (the walking kernel only)
    size_t cands;              // m * n
    int H, p, E, PE, D, G;
    int kind, form;
    float cap;
    const float* disc;         // [H + 1] the ctx's discount table, or null (the walking kernel only)
    float w[CADM_MAX_UNC_DIMS];      // [D], broadcast already
};

__device__ __forceinline__ int unc_pad4(int v) { return (v + 3) & ~3; }

// steps t > cut are not counted: the smallest first violation of the candidate's particles (the step at which the first particle leaves
// still counts); without `first` every step
__device__ __forceinline__ int unc_cut(const int32_t* first, size_t q, int p, int H) {
    if (!first) return H;
    int cut = first[q * p];
    for (int j = 1; j < p; ++j) {
        const int f = first[q * p + j];
        cut = f < cut ? f : cut;
    }
    return cut;
}

// WALK = false: blockIdx.y is the step, u goes to a.step.  WALK = true: the workgroup walks the steps, the candidate's thread adds the
// counted ones and writes a.cost (a.step may be null).
// DISC (with WALK only): the ctx's discount over the horizon (discount.hip): cost = cost + disc[t] * u_t.  false: the kernel as it was
template <bool WALK, bool DISC = false>
__global__ __launch_bounds__(UNC_THREADS) void uncertainty_steps_kernel(const UncArgs a) {
    extern __shared__ __attribute__((aligned(16))) float unc_smem[];
    const int D = a.D, p = a.p, E = a.E, PE = a.PE, H = a.H, pD = p * D, tid = threadIdx.x;
    float* tile = unc_smem;                              // [ng, p, D] this step's values
    float* sv = tile + unc_pad4(a.G * pD);               // [ng, D] the variances of the weighted dims
    float* sw = sv + unc_pad4(a.G * D);                  // [D] the weights, copied out of the kernel arguments once
    const size_t c0 = (size_t)blockIdx.x * a.G;          // first candidate of this workgroup (c0 < cands: the grid is ceil(cands / G))
    const int ng = a.cands - c0 < (size_t)a.G ? (int)(a.cands - c0) : a.G;
    const int span = ng * pD;
    const bool mine = tid < ng;                          // (G <= UNC_GROUP <= UNC_THREADS)
    for (int d = tid; d < D; d += UNC_THREADS) sw[d] = a.w[d];
    const int cut = (WALK && mine) ? unc_cut(a.first, c0 + tid, p, H) : H;
    float cost = 0.0f;
    const int t0 = WALK ? 0 : (int)blockIdx.y, t1 = WALK ? H : t0 + 1;
    for (int t = t0; t < t1; ++t) {
        const float* src = a.traj + ((size_t)t * a.cands + c0) * pD;
        const int nvec = (reinterpret_cast<uintptr_t>(src) & 15) == 0 ? span >> 2 : 0;
        for (int i = tid; i < nvec; i += UNC_THREADS) reinterpret_cast<floatx4*>(tile)[i] = reinterpret_cast<const floatx4*>(src)[i];
        for (int i = 4 * nvec + tid; i < span; i += UNC_THREADS) tile[i] = src[i];
        __syncthreads();      // (behind it every read of sv of the step before is done as well: its reader is past this barrier)
        // the variance of a (candidate, dim): one thread's chain in particle order, members in member order, relative to particle 0 --
        // forecast_stats_kernel's, operation for operation.  Dims with w == 0 are not read.
        for (int i = tid; i < ng * D; i += UNC_THREADS) {
            const int c = i / D, d = i - c * D;
            if (!(sw[d] > 0.0f)) continue;
            const float* x = tile + c * pD + d;
            const float x0 = x[0];
            float tot = 0.0f;
            for (int e = 0; e < E; ++e) {
                float s = 0.0f;
                for (int j = 0; j < PE; ++j) s += x[(e * PE + j) * D] - x0;
                tot += s;
            }
            const float md = tot / (float)p;
            float v;
            if (a.kind == CADM_UNC_TOTAL) {
                float var = 0.0f;
                for (int j = 0; j < p; ++j) {
                    const float dv = (x[j * D] - x0) - md;
                    var += dv * dv;
                }
                v = var / (float)p;
            } else {
                float epi = 0.0f;
                for (int e = 0; e < E; ++e) {
                    float s = 0.0f;
                    for (int j = 0; j < PE; ++j) s += x[(e * PE + j) * D] - x0;
                    const float de = s / (float)PE - md;
                    epi += de * de;
                }
                v = epi / (float)E;
            }
            sv[i] = v;
        }
        __syncthreads();      // (behind it every read of the tile is done: the next step loads over it)
        if (mine) {
            float u = 0.0f;
            bool any = false;
            for (int d = 0; d < D; ++d) {
                const float w = sw[d];
                if (!(w > 0.0f)) continue;
                const float term = w * sv[tid * D + d];
                u = any ? u + term : term;
                any = true;
            }
            if (a.form == CADM_UNC_STD) u = sqrtf(u);
            u = u > a.cap ? a.cap : u;      // (a comparison, not fminf: a NaN stays NaN)
            if (a.step) a.step[(c0 + tid) * H + t] = u;
            if (WALK && t <= cut) cost = DISC ? __fadd_rn(cost, __fmul_rn(a.disc[t], u)) : cost + u;
        }
    }
    if (WALK && mine) a.cost[c0 + tid] = cost;
}

// cost[q] = the counted steps of step[q, :] added in order from 0; cand (or null): cand[q] = cand[q] - lambda * cost[q]
template <bool DISC>
__global__ void uncertainty_apply_kernel(const float* __restrict__ step, const int32_t* __restrict__ first, size_t cands, int H, int p,
                                         float lambda, float* __restrict__ cost_out, float* __restrict__ cand, const float* __restrict__ disc) {
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < cands; q += (size_t)gridDim.x * blockDim.x) {
        const int cut = unc_cut(first, q, p, H);
        float cost = 0.0f;
        for (int t = 0; t < H && t <= cut; ++t) cost = DISC ? __fadd_rn(cost, __fmul_rn(disc[t], step[q * H + t])) : cost + step[q * H + t];
        cost_out[q] = cost;
        if (cand) {
            const float pen = lambda * cost;
            cand[q] = cand[q] - pen;
        }
    }
}

size_t unc_lds_bytes(int G, int p, int D) {
    return (((size_t)G * p * D + 3) & ~(size_t)3) * sizeof(float) + (size_t)(((G * D + 3) & ~3) + ((D + 3) & ~3)) * sizeof(float);
}

// the largest group whose tile fits (0: not even one candidate's)
int unc_group(int p, int D) {
    int G = UNC_GROUP;
    while (G > 0 && unc_lds_bytes(G, p, D) > (size_t)UNC_LDS_BUDGET) --G;
    return G;
}

void unc_fill(const cadm_ctx* ctx, const cadm_uncertainty_params* prm, const float* traj, const int32_t* first, int m, int n, float* step,
              float* cost, UncArgs* a) {
    a->traj = traj; a->first = first; a->step = step; a->cost = cost;
    a->cands = (size_t)m * n;
    a->H = ctx->H; a->p = ctx->p; a->E = ctx->E; a->PE = ctx->p / ctx->E; a->D = ctx->D; a->G = unc_group(ctx->p, ctx->D);
    a->kind = prm->kind; a->form = prm->form; a->cap = prm->cap;
    for (int d = 0; d < ctx->D; ++d) a->w[d] = prm->n_dims == 0 ? prm->w[0] : prm->w[d];
}

}  // namespace

// the refusals of an uncertainty term, before any HIP call
int cadm_uncertainty_check(const cadm_ctx* ctx, const cadm_uncertainty_params* c, const char* who) {
    CADM_REQUIRE(c, "%s: the uncertainty parameters are null", who);
    CADM_REQUIRE(c->kind == CADM_UNC_EPISTEMIC || c->kind == CADM_UNC_TOTAL, "%s: unknown uncertainty kind %d", who, c->kind);
    CADM_REQUIRE(c->form == CADM_UNC_VAR || c->form == CADM_UNC_STD, "%s: unknown uncertainty form %d", who, c->form);
    CADM_REQUIRE(isfinite(c->weight), "%s: the uncertainty weight (lambda) %g is not finite", who, (double)c->weight);
    CADM_REQUIRE(c->cap > 0.0f, "%s: the uncertainty cap %g is not > 0 (+inf: none)", who, (double)c->cap);
    CADM_REQUIRE(!ctx->cfg.discrete && ctx->cfg.env_kind != CADM_ENV_CARTPOLE, "%s: the uncertainty cost needs a continuous-action ctx (discrete "
                 "actions are planned by random shooting)", who);
    CADM_REQUIRE(!cadm_sharded(ctx), "%s: the uncertainty cost is not supported on a candidate-sharded ctx", who);
    CADM_REQUIRE(ctx->D <= CADM_MAX_UNC_DIMS, "%s: %d observation dims, the uncertainty parameters hold %d", who, ctx->D, CADM_MAX_UNC_DIMS);
    CADM_REQUIRE(c->n_dims == 0 || c->n_dims == ctx->D, "%s: the uncertainty weights were built for %d observation dims, this ctx has %d", who,
                 c->n_dims, ctx->D);
    bool any = false;
    for (int k = 0; k < (c->n_dims == 0 ? 1 : ctx->D); ++k) {
        CADM_REQUIRE(isfinite(c->w[k]) && c->w[k] >= 0.0f, "%s: uncertainty weight w[%d] = %g is not finite and >= 0", who, k, (double)c->w[k]);
        any = any || c->w[k] > 0.0f;
    }
    CADM_REQUIRE(any, "%s: every uncertainty weight w is 0", who);
    CADM_REQUIRE(unc_group(ctx->p, ctx->D) >= 1,
                 "%s: p (%d) x D (%d) does not fit the kernel's LDS: one candidate's tile of p * D floats, D variances and D weights need %zu "
                 "bytes, the bound is %d", who, ctx->p, ctx->D, unc_lds_bytes(1, ctx->p, ctx->D), UNC_LDS_BUDGET);
    return CADM_OK;
}

// u into step [m, n, H], the cost into cost [m, n], and with cand [m, n]: cand -= lambda * cost.  n: the PACKED candidate count of traj.
int cadm_launch_uncertainty(cadm_ctx* ctx, const cadm_uncertainty_params* prm, const float* traj, const int32_t* first, int m, int n,
                            float* step, float* cost, float* cand, hipStream_t s) {
    UncArgs a{};
    unc_fill(ctx, prm, traj, first, m, n, step, cost, &a);
    const size_t blocks = (a.cands + a.G - 1) / a.G;
    CADM_REQUIRE(blocks <= 0x7fffffffull && ctx->H <= 65535, "uncertainty cost: %zu candidates x %d steps are too many for one launch", a.cands, ctx->H);
    hipLaunchKernelGGL(uncertainty_steps_kernel<false>, dim3((unsigned)blocks, (unsigned)ctx->H), dim3(UNC_THREADS),
                       unc_lds_bytes(a.G, ctx->p, ctx->D), s, a);
    CADM_CHECK_HIP(hipGetLastError());
    const size_t g = (a.cands + 255) / 256;
    if (ctx->disc) hipLaunchKernelGGL(uncertainty_apply_kernel<true>, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, s, step, first, a.cands,
                                      ctx->H, ctx->p, prm->weight, cost, cand, ctx->disc);
    else hipLaunchKernelGGL(uncertainty_apply_kernel<false>, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, s, step, first, a.cands, ctx->H,
                            ctx->p, prm->weight, cost, cand, nullptr);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

extern "C" int cadm_uncertainty_cost(cadm_ctx* ctx, const cadm_uncertainty_params* params, const float* traj, const int32_t* first, int m, int n,
                                     float* step_out, float* cost_out, void* stream) {
    CADM_REQUIRE(ctx && params && traj && cost_out, "cadm_uncertainty_cost: ctx / params / traj / cost_out is null");
    int rc = cadm_uncertainty_check(ctx, params, "cadm_uncertainty_cost");
    if (rc) return rc;
    CADM_REQUIRE(m >= 1 && n >= 1, "cadm_uncertainty_cost: m, n must be >= 1 (got m=%d n=%d)", m, n);
    CADM_ON_DEVICE(ctx);
    if (step_out) return cadm_launch_uncertainty(ctx, params, traj, first, m, n, step_out, cost_out, nullptr, (hipStream_t)stream);
    UncArgs a{};
    unc_fill(ctx, params, traj, first, m, n, nullptr, cost_out, &a);
    const size_t blocks = (a.cands + a.G - 1) / a.G;
    CADM_REQUIRE(blocks <= 0x7fffffffull, "cadm_uncertainty_cost: %zu candidates are too many for one launch", a.cands);
    a.disc = ctx->disc;
    if (a.disc) hipLaunchKernelGGL((uncertainty_steps_kernel<true, true>), dim3((unsigned)blocks), dim3(UNC_THREADS), unc_lds_bytes(a.G, ctx->p, ctx->D),
                                   (hipStream_t)stream, a);
    else hipLaunchKernelGGL((uncertainty_steps_kernel<true, false>), dim3((unsigned)blocks), dim3(UNC_THREADS), unc_lds_bytes(a.G, ctx->p, ctx->D),
                            (hipStream_t)stream, a);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}
