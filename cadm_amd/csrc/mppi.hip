// MPPI (information-theoretic) update of the sampling planner: an OPT-IN alternative to the hard top-k elite refit of cem.hip.  No
// reference twin.  EVERY candidate contributes to the new mean and variance, with weight exp(return / lambda) (Williams et al. 2017,
// "Information Theoretic MPC for Model-Based Reinforcement Learning").
//
// Per env i, over its n candidates with returns R_c and action sequences a_c [H, A]:
//     F       = the candidates whose return is finite (NaN, +inf, -inf: weight 0); F empty: mean / var untouched, plan = clip(mean)
//     R*      = max_F R,   lambda_eff = temperature   or (relative)   temperature (R* - min_F R);   relative and lambda_eff == 0: w_c = 1
//     w_c     = exp((R_c - R*) / lambda_eff),   W = sum_c w_c      (the best candidate has weight 1: W >= 1)
//     mu[t,a] = sum_c w_c a_c[t,a] / W
//     v[t,a]  = sum_c w_c (a_c[t,a] - mu[t,a])^2 / W               (mean first, then the variance around it: a one-pass sum of
//                                                                   squares cancels, as horizon.hip notes)
//     mean <- alpha mean + (1 - alpha) mu,   var <- alpha var + (1 - alpha) v      (the blend of cem_refit_kernel),   plan = clip(mean)
// The action sequences must be finite (the samplers clip them): a weight of 0 does not hide a NaN action.
//
// Reduction contract (no floating-point atomics anywhere):
//   Candidates are cut in RUNS of 8 and GROUPS of 64 (8 runs) by their index alone: run c / 8, group c / 64, whatever n, m, H, A.
//   Inside a run the terms are added in index order; a group adds its 8 run sums in run order; the groups' partials are added in
//   group order.  Every sum of the update -- W, the numerators of mu and of v -- has this shape, and every workgroup that needs mu
//   forms it from the same partials in the same order.  The result is therefore bit-identical run to run, and an env's result does
//   not depend on the other envs of the call.
//   Rounding chain of one element of mu or v:  8 + 8 + (ceil(n / 64) - 1) additions, + 4 (the product w a, resp. d, d^2 and w d^2;
//   the division by W), and W's own 8 + 8 + ceil(n / 64) - 1:  at most  2 (15 + ceil(n / 64)) + 4  fp32 roundings, each of at
//   most 2^-24 of the running sum (|a| <= 1, the sums are convex combinations scaled by W).  n = 1030: 68;  n = 8000: 284.
//   The weights carry the relative error of expf's argument (<= arg x 2^-23 for the subtraction and the division) on top.
//
// Launches (all on the caller's stream):
//   mppi_weights_kernel   one workgroup per env: R*, min_F R (max / min are exact in any order), w_c -> scratch, W, the F-empty flag
//   mppi_sum_kernel<0>    grid (group, element tile, env): the group's partial of sum_c w_c a_c            -> part1 [m][groups][HA]
//   mppi_sum_kernel<1>    the same grid: mu from part1 (groups in order), the group's partial of sum_c w_c (a_c - mu)^2 -> part2
//   mppi_final_kernel     one thread per element: mu and v from the partials, the blend, the clipped plan
// Traffic: `actions` is read twice (the second time from L2 / MALL at planner sizes), a group's [64, HA] span row by row: consecutive
// lanes read consecutive words of a row, as 16-byte loads where HA % 4 == 0 and the buffer is 16-byte aligned, scalar loads otherwise
// (same arithmetic, same bits).  LDS: 8 run sums + mu of one element tile, 36.3 KiB static: no attribute needed.
#include <math.h>

#include "planner.h"

namespace {

constexpr int MP_RUN = 8;                    // candidates per run
constexpr int MP_RUNS = 8;                   // runs per group
constexpr int MP_GROUP = MP_RUN * MP_RUNS;   // candidates per partial
constexpr int MP_THREADS = 256;
constexpr int MP_TILE = 1024;                // elements of [H, A] per workgroup (a multiple of 4)

__device__ __forceinline__ bool mp_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// sum of cnt words at p, p + stride, ... in that order: the loads are issued 8 at a time, the additions stay one chain in index order
// (a rolled loop waited out one memory round trip per term)
__device__ __forceinline__ float mp_ordered_sum(const float* __restrict__ p, size_t stride, int cnt) {
    float s = 0.0f;
    int b = 0;
    for (; b + 8 <= cnt; b += 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = p[(size_t)(b + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; b < cnt; ++b) s += p[(size_t)b * stride];
    return s;
}

// hdr [m][2]: W, 1.0f / 0.0f = some / no finite return
__global__ __launch_bounds__(MP_THREADS) void mppi_weights_kernel(const float* __restrict__ cand, int n, float temperature, int relative,
                                                                  float* __restrict__ w, float* __restrict__ hdr) {
    __shared__ float smax[MP_THREADS], smin[MP_THREADS], sw[MP_THREADS];
    const int mi = blockIdx.x, tid = threadIdx.x;
    const float* r = cand + (size_t)mi * n;
    float* wm = w + (size_t)mi * n;
    float hi = -INFINITY, lo = INFINITY;
    for (int c = tid; c < n; c += MP_THREADS) {
        const float v = r[c];
        if (mp_finite(v)) { hi = fmaxf(hi, v); lo = fminf(lo, v); }
    }
    smax[tid] = hi;
    smin[tid] = lo;
    __syncthreads();
    for (int d = MP_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) { smax[tid] = fmaxf(smax[tid], smax[tid + d]); smin[tid] = fminf(smin[tid], smin[tid + d]); }
        __syncthreads();
    }
    const float rmax = smax[0], rmin = smin[0];
    const bool any = rmax >= rmin;                       // (no finite return: -inf < +inf)
    const float lam = relative ? temperature * (rmax - rmin) : temperature;
    const bool flat = relative && lam == 0.0f;
    for (int c = tid; c < n; c += MP_THREADS) {
        const float v = r[c];
        wm[c] = !mp_finite(v) ? 0.0f : flat ? 1.0f : expf((v - rmax) / lam);
    }
    __syncthreads();                                     // (this workgroup's weights, read back below)
    // W: runs in index order, a group's runs in run order, the groups in group order
    const int groups = (n + MP_GROUP - 1) / MP_GROUP;
    float W = 0.0f;
    for (int g0 = 0; g0 < groups; g0 += MP_THREADS) {
        const int g = g0 + tid;
        float wg = 0.0f;
        if (g < groups)
            for (int q = 0; q < MP_RUNS; ++q) {
                float t[MP_RUN];
#pragma unroll
                for (int k = 0; k < MP_RUN; ++k) {
                    const int c = g * MP_GROUP + q * MP_RUN + k;
                    t[k] = c < n ? wm[c] : 0.0f;
                }
                float s = 0.0f;
#pragma unroll
                for (int k = 0; k < MP_RUN; ++k) s += t[k];
                wg += s;
            }
        sw[tid] = wg;
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < MP_THREADS && g0 + j < groups; ++j) W += sw[j];
        __syncthreads();
    }
    if (tid == 0) { hdr[2 * mi] = W; hdr[2 * mi + 1] = any ? 1.0f : 0.0f; }
}

template <int V> struct MpVec;
template <> struct MpVec<1> { using T = float; };
template <> struct MpVec<4> { using T = float4; };

// PASS 0: part_out[mi][group][e] = sum over the group's candidates of w_c a_c[e]
// PASS 1: mu[e] = (sum over groups of part_in[mi][.][e]) / W, then part_out[mi][group][e] = sum of w_c (a_c[e] - mu[e])^2
// V: floats per load (4: HA % 4 == 0 and a 16-byte aligned buffer)
template <int PASS, int V>
__global__ __launch_bounds__(MP_THREADS) void mppi_sum_kernel(const float* __restrict__ actions, const float* __restrict__ w,
                                                              const float* __restrict__ hdr, const float* __restrict__ part_in,
                                                              float* __restrict__ part_out, int n, int HA, int groups) {
    __shared__ __attribute__((aligned(16))) float run_s[MP_RUNS][MP_TILE];
    __shared__ __attribute__((aligned(16))) float mu_s[MP_TILE];
    __shared__ float w_s[MP_GROUP];
    const int g = blockIdx.x, mi = blockIdx.z, tid = threadIdx.x;
    const int e0 = blockIdx.y * MP_TILE;
    const int ne = HA - e0 < MP_TILE ? HA - e0 : MP_TILE;
    const int c0 = g * MP_GROUP;
    const int nc = n - c0 < MP_GROUP ? n - c0 : MP_GROUP;
    if (tid < MP_GROUP) w_s[tid] = tid < nc ? w[(size_t)mi * n + c0 + tid] : 0.0f;
    if (PASS == 1) {
        const float W = hdr[2 * mi], any = hdr[2 * mi + 1];
        for (int e = tid; e < ne; e += MP_THREADS) {
            const float s = mp_ordered_sum(part_in + (size_t)mi * groups * HA + e0 + e, (size_t)HA, groups);
            mu_s[e] = any != 0.0f ? s / W : 0.0f;
        }
    }
    __syncthreads();
    using T = typename MpVec<V>::T;
    const int nq = ne / V;                               // (V == 4: HA and MP_TILE are multiples of 4, so is ne)
    const float* base = actions + ((size_t)mi * n + c0) * HA + e0;
    for (int item = tid; item < MP_RUNS * nq; item += MP_THREADS) {
        const int q = item / nq, col = item - q * nq;    // run q of the group, V elements at col * V: consecutive lanes, consecutive words of a row
        float acc[V], mu[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { acc[j] = 0.0f; mu[j] = PASS == 1 ? mu_s[col * V + j] : 0.0f; }
        T av[MP_RUN];
#pragma unroll
        for (int k = 0; k < MP_RUN; ++k) {               // (independent loads first, the dependent adds behind them)
            const int c = q * MP_RUN + k;
            if (c < nc) av[k] = *reinterpret_cast<const T*>(base + (size_t)c * HA + col * V);
        }
#pragma unroll
        for (int k = 0; k < MP_RUN; ++k) {
            const int c = q * MP_RUN + k;
            if (c < nc) {
                const float wc = w_s[c];
                const float* a = reinterpret_cast<const float*>(&av[k]);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    if (PASS == 0) {
                        acc[j] += wc * a[j];
                    } else {
                        const float d = a[j] - mu[j];
                        acc[j] += wc * (d * d);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) run_s[q][col * V + j] = acc[j];
    }
    __syncthreads();
    for (int e = tid; e < ne; e += MP_THREADS) {
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < MP_RUNS; ++q) s += run_s[q][e];
        part_out[((size_t)mi * groups + g) * HA + e0 + e] = s;
    }
}

// mean_in / var_in may alias mean_out / var_out (an element is read and written by its own thread only)
__global__ __launch_bounds__(MP_THREADS) void mppi_final_kernel(const float* __restrict__ hdr, const float* __restrict__ part1,
                                                                const float* __restrict__ part2, int HA, int groups, float alpha,
                                                                const float* mean_in, const float* var_in, float* mean_out, float* var_out,
                                                                float* __restrict__ plan_out, float lo, float hi) {
    const int mi = blockIdx.y, e = blockIdx.x * MP_THREADS + threadIdx.x;
    if (e >= HA) return;
    const size_t o = (size_t)mi * HA + e;
    const float W = hdr[2 * mi];
    if (hdr[2 * mi + 1] == 0.0f) {                       // no finite return: the distribution stays as it is, bit for bit
        const float mo = mean_in[o], vo = var_in[o];
        if (mean_out != mean_in) mean_out[o] = mo;
        if (var_out != var_in) var_out[o] = vo;
        if (plan_out) plan_out[o] = fminf(fmaxf(mo, lo), hi);
        return;
    }
    const float s1 = mp_ordered_sum(part1 + (size_t)mi * groups * HA + e, (size_t)HA, groups);
    const float s2 = mp_ordered_sum(part2 + (size_t)mi * groups * HA + e, (size_t)HA, groups);
    const float mu = s1 / W, v = s2 / W;
    const float mo = mean_in[o] * alpha + (1.0f - alpha) * mu;      // the blend of cem_refit_kernel (core/utils.py:485-486)
    const float vo = var_in[o] * alpha + (1.0f - alpha) * v;
    mean_out[o] = mo;
    var_out[o] = vo;
    if (plan_out) plan_out[o] = fminf(fmaxf(mo, lo), hi);
}

}  // namespace

size_t cadm_mppi_scratch_floats(const cadm_ctx* ctx, int m, int n) {
    const size_t HA = (size_t)ctx->H * ctx->A, groups = ((size_t)n + MP_GROUP - 1) / MP_GROUP;
    const size_t wn = ((size_t)m * n + 2 * (size_t)m + 3) & ~(size_t)3;       // w [m][n], hdr [m][2]; the partials start 16-byte aligned
    return wn + 2 * (size_t)m * groups * HA;
}

int cadm_mppi_check(const cadm_ctx* ctx, int m, float temperature, const char* who) {
    CADM_REQUIRE(isfinite(temperature) && temperature > 0.0f, "%s: temperature %g must be finite and > 0", who, (double)temperature);
    CADM_REQUIRE(!ctx->cfg.discrete, "%s: continuous actions only", who);
    CADM_REQUIRE(!cadm_sharded(ctx), "%s: candidate-sharded planning is not supported (the update reads every candidate's action sequence)", who);
    CADM_REQUIRE(m <= 65535, "%s: %d envs are too many for one launch (65535)", who, m);
    return CADM_OK;
}

int cadm_launch_mppi_refit(cadm_ctx* ctx, const float* cand_returns, const float* actions, int m, int n, float temperature, int relative,
                           const float* mean_in, const float* var_in, float* mean_out, float* var_out, float* plan_out, float* scratch,
                           hipStream_t s) {
    const int HA = ctx->H * ctx->A, groups = (n + MP_GROUP - 1) / MP_GROUP, tiles = (HA + MP_TILE - 1) / MP_TILE;
    float* w = scratch;
    float* hdr = w + (size_t)m * n;
    float* part1 = scratch + (((size_t)m * n + 2 * (size_t)m + 3) & ~(size_t)3);
    float* part2 = part1 + (size_t)m * groups * HA;
    hipLaunchKernelGGL(mppi_weights_kernel, dim3(m), dim3(MP_THREADS), 0, s, cand_returns, n, temperature, relative ? 1 : 0, w, hdr);
    CADM_CHECK_HIP(hipGetLastError());
    const dim3 grid(groups, tiles, m);
    if (HA % 4 == 0 && (reinterpret_cast<uintptr_t>(actions) & 15) == 0) {
        hipLaunchKernelGGL((mppi_sum_kernel<0, 4>), grid, dim3(MP_THREADS), 0, s, actions, w, hdr, nullptr, part1, n, HA, groups);
        hipLaunchKernelGGL((mppi_sum_kernel<1, 4>), grid, dim3(MP_THREADS), 0, s, actions, w, hdr, part1, part2, n, HA, groups);
    } else {
        hipLaunchKernelGGL((mppi_sum_kernel<0, 1>), grid, dim3(MP_THREADS), 0, s, actions, w, hdr, nullptr, part1, n, HA, groups);
        hipLaunchKernelGGL((mppi_sum_kernel<1, 1>), grid, dim3(MP_THREADS), 0, s, actions, w, hdr, part1, part2, n, HA, groups);
    }
    CADM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(mppi_final_kernel, dim3((HA + MP_THREADS - 1) / MP_THREADS, m), dim3(MP_THREADS), 0, s, hdr, part1, part2, HA, groups,
                       ctx->cfg.alpha, mean_in, var_in, mean_out, var_out, plan_out, ctx->cfg.lower_bound, ctx->cfg.upper_bound);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

extern "C" int cadm_mppi_refit(cadm_ctx* ctx, const float* cand_returns, const float* actions, int m, int n, float temperature, int relative,
                               float* mean_io, float* var_io, float* plan_out, void* stream) {
    CADM_REQUIRE(ctx && cand_returns && actions && mean_io && var_io && m > 0 && n > 0, "cadm_mppi_refit: bad arguments");
    int rc;
    if ((rc = cadm_mppi_check(ctx, m, temperature, "cadm_mppi_refit"))) return rc;
    CADM_ON_DEVICE(ctx);
    // the partials live in a buffer the ctx owns and grows on demand (hipFree waits for the launches that still read the old one)
    const size_t need = cadm_mppi_scratch_floats(ctx, m, n);
    if (need > ctx->mppi_scratch_floats) {
        if (ctx->mppi_scratch) CADM_CHECK_HIP(hipFree(ctx->mppi_scratch));
        ctx->mppi_scratch = nullptr;
        ctx->mppi_scratch_floats = 0;
        CADM_CHECK_HIP(hipMalloc(&ctx->mppi_scratch, need * sizeof(float)));
        ctx->mppi_scratch_floats = need;
    }
    return cadm_launch_mppi_refit(ctx, cand_returns, actions, m, n, temperature, relative, mean_io, var_io, mean_io, var_io, plan_out,
                                  ctx->mppi_scratch, (hipStream_t)stream);
}
