// Forecast of a plan: what the ensemble predicts under given action sequences, per step -- the rollout kernel's trajectories
// (`traj_out`, [H, m, n, p, D]) reduced on the device to per-step state statistics, step rewards and their spread, per-particle
// returns and the step at which a sequence diverged (cadm_forecast_stats; cadm_plan_forecast, at the end of this file, strings
// encoder, rollout and this kernel together).  The rollout kernels are not touched: this kernel runs behind them.
//
// Per sequence (mi, ni) and step t, over the p particles x_j = traj[t, mi, ni, j, d] (particle j belongs to member j / (p / E)):
//     mean, member_mean[e]      over all particles / over member e's p / E particles
//     var_total                 biased variance over the particles
//     var_epistemic             biased variance of the E member means
//     var_aleatoric             mean over the members of the biased variance inside a member     (total = epistemic + aleatoric)
//     lo, hi                    the band_k-th smallest / largest particle value (no interpolation)
//     reward_mean / var / member  the same for the step reward r_j, evaluated from the pre-step state (obs at t = 0, else
//                               traj[t - 1]), the post-step state traj[t] and the raw action
//     returns[j]                r_j added in step order
// Everything is formed relative to particle 0, as horizon.hip does: differences of nearby values are exact, and particles that agree
// give exactly their value as every mean and exactly 0 as every variance.
//
// Reduction contract: one workgroup per sequence walks the steps in order; every statistic of a (step, dim) is ONE thread's chain in
// particle order (members in member order), the reward statistics of a step one thread's chain, returns[j] one thread's chain in
// step order.  No atomics on floating-point values, no dependence on the grid: the same bits run to run, and per sequence whatever
// m and n.  A mean is a chain of at most p + 2 fp32 roundings, a variance of at most p + 3 on top of its deviations'.
//
// Divergence: the first step at which any of the sequence's p * D values is non-finite is its diverged_step (H: none); every
// statistic of that sequence from that step on, and its returns, are NaN.  Other sequences are not affected.  Divergence is read off
// `traj` alone: a non-finite value in `obs` (step 0's pre-step state) leaves diverged_step as it is and shows as non-finite step-0
// rewards and returns.
//
// Parallelism: the state statistics keep D of the workgroup's 256 threads busy (one chain per dim), the reward statistics one; only
// the loads, the order statistics and the rewards spread over the workgroup.  That is what the fixed summation order costs: the
// kernel is bound by the latency of those chains, O(p) LDS reads each, not by bandwidth, and grows with p.
//
// Traffic: `traj` is read exactly once -- a (sequence, step)'s p * D values are one contiguous span, loaded lane-linear with 16-byte
// loads into one of two LDS tiles (scalar loads where the span is not 16-byte aligned); the other tile still holds the previous
// step: the pre-step state of the rewards.
#include "step_reward.h"

namespace {

constexpr int FC_THREADS = 256;
constexpr int FC_LDS_BUDGET = 48 * 1024;     // two tiles + per-particle rewards and returns, below the 64 KiB a kernel gets without an attribute

struct ForecastArgs {
    const float *traj, *obs, *actions;
    int m, n, H, p, E, D, A, PE, band_k;
    cadm_forecast_out out;
    ForecastSpec spec;
};

__device__ __forceinline__ bool fc_non_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

template <int ENV>
__global__ __launch_bounds__(FC_THREADS) void forecast_stats_kernel(const ForecastArgs a) {
    extern __shared__ __attribute__((aligned(16))) float fc_smem[];
    const int D = a.D, p = a.p, E = a.E, PE = a.PE, H = a.H, pD = p * D, ts = (pD + 3) & ~3;
    float* tiles = fc_smem;                              // [2][ts]: this step's values and the previous step's
    float* ret = tiles + 2 * ts;                         // [p] returns so far
    float* rew = ret + p;                                // [p] this step's rewards
    int* bad = reinterpret_cast<int*>(rew + p);          // a non-finite value was loaded
    const int tid = threadIdx.x;
    const size_t seq = blockIdx.x;                       // mi * n + ni
    const int mi = (int)(seq / (size_t)a.n);
    const float nan = __uint_as_float(0x7fc00000u);
    const cadm_forecast_out& o = a.out;
    // step 0's pre-step state: obs[mi] for every particle, in the tile step 0 does not load into
    for (int i = tid; i < pD; i += FC_THREADS) tiles[ts + i] = a.obs[(size_t)mi * D + i % D];
    for (int j = tid; j < p; j += FC_THREADS) ret[j] = 0.0f;
    if (tid == 0) bad[0] = 0;
    __syncthreads();
    int div = H;
    for (int t = 0; t < H; ++t) {
        float* cur = tiles + (t & 1) * ts;
        const float* pre = tiles + ((t & 1) ^ 1) * ts;
        const float* src = a.traj + ((size_t)t * a.m * a.n + seq) * pD;
        const int nvec = (reinterpret_cast<uintptr_t>(src) & 15) == 0 ? pD >> 2 : 0;
        for (int i = tid; i < nvec; i += FC_THREADS) {
            const floatx4 v = reinterpret_cast<const floatx4*>(src)[i];
            reinterpret_cast<floatx4*>(cur)[i] = v;
            if (fc_non_finite(v[0]) || fc_non_finite(v[1]) || fc_non_finite(v[2]) || fc_non_finite(v[3])) atomicOr(bad, 1);
        }
        for (int i = 4 * nvec + tid; i < pD; i += FC_THREADS) {
            const float v = src[i];
            cur[i] = v;
            if (fc_non_finite(v)) atomicOr(bad, 1);
        }
        __syncthreads();
        if (bad[0]) { div = t; break; }                  // (the same word for every thread: the whole workgroup leaves)
        const size_t row = seq * H + t;                  // (mi, ni, t)
        // state statistics: one thread per dim, every chain in particle order
        for (int d = tid; d < D; d += FC_THREADS) {
            const float* x = cur + d;
            const float x0 = x[0];
            float tot = 0.0f, alea = 0.0f;
            for (int e = 0; e < E; ++e) {
                float s = 0.0f;
                for (int j = 0; j < PE; ++j) s += x[(e * PE + j) * D] - x0;
                tot += s;
                const float me = s / (float)PE;
                o.member_mean[((size_t)e * a.m * a.n * H + row) * D + d] = PE == 1 ? x[e * D] : me == 0.0f ? x0 : x0 + me;      // (the mean of one value is that value)
                float v = 0.0f;
                for (int j = 0; j < PE; ++j) {
                    const float dv = (x[(e * PE + j) * D] - x0) - me;
                    v += dv * dv;
                }
                alea += v / (float)PE;
            }
            const float md = tot / (float)p;
            float var = 0.0f;
            for (int j = 0; j < p; ++j) {
                const float dv = (x[j * D] - x0) - md;
                var += dv * dv;
            }
            float epi = 0.0f;
            for (int e = 0; e < E; ++e) {
                float s = 0.0f;
                for (int j = 0; j < PE; ++j) s += x[(e * PE + j) * D] - x0;
                const float de = s / (float)PE - md;
                epi += de * de;
            }
            o.mean[row * D + d] = md == 0.0f ? x0 : x0 + md;
            o.var_total[row * D + d] = var / (float)p;
            o.var_epistemic[row * D + d] = epi / (float)E;
            o.var_aleatoric[row * D + d] = alea / (float)E;
        }
        // order statistics: one thread per (particle, dim) counts the values that sort before its own (ties: the lower index)
        for (int it = tid; it < pD; it += FC_THREADS) {
            const int j = it / D, d = it - j * D;
            const float xj = cur[it];
            int rank = 0;
            for (int i = 0; i < p; ++i) {
                const float xi = cur[i * D + d];
                rank += (xi < xj || (xi == xj && i < j)) ? 1 : 0;
            }
            if (rank == a.band_k - 1) o.lo[row * D + d] = xj;
            if (rank == p - a.band_k) o.hi[row * D + d] = xj;
        }
        // step rewards: one thread per particle
        const float* act = a.actions + row * a.A;
        for (int j = tid; j < p; j += FC_THREADS) {
            const float r = step_reward<ENV>(a.spec, D, a.A, pre + j * D, cur + j * D, act);
            rew[j] = r;
            ret[j] = ret[j] + r;
        }
        __syncthreads();      // every read of `pre` is done: the next step loads over it; the rewards are in place
        if (tid == 0) {
            const float r0 = rew[0];
            float tot = 0.0f;
            for (int e = 0; e < E; ++e) {
                float s = 0.0f;
                for (int j = 0; j < PE; ++j) s += rew[e * PE + j] - r0;
                tot += s;
                const float me = s / (float)PE;
                o.reward_member[(size_t)e * a.m * a.n * H + row] = PE == 1 ? rew[e] : me == 0.0f ? r0 : r0 + me;
            }
            const float md = tot / (float)p;
            float var = 0.0f;
            for (int j = 0; j < p; ++j) {
                const float dv = (rew[j] - r0) - md;
                var += dv * dv;
            }
            o.reward_mean[row] = md == 0.0f ? r0 : r0 + md;
            o.reward_var[row] = var / (float)p;
        }
    }
    // a diverged sequence: NaN from that step on, and as its returns
    for (int i = tid; i < (H - div) * D; i += FC_THREADS) {
        const size_t at = (seq * H + div) * D + i;
        o.mean[at] = nan; o.var_total[at] = nan; o.var_epistemic[at] = nan; o.var_aleatoric[at] = nan; o.lo[at] = nan; o.hi[at] = nan;
        for (int e = 0; e < E; ++e) o.member_mean[(size_t)e * a.m * a.n * H * D + at] = nan;
    }
    for (int i = tid; i < H - div; i += FC_THREADS) {
        const size_t at = seq * H + div + i;
        o.reward_mean[at] = nan; o.reward_var[at] = nan;
        for (int e = 0; e < E; ++e) o.reward_member[(size_t)e * a.m * a.n * H + at] = nan;
    }
    for (int j = tid; j < p; j += FC_THREADS) o.returns[seq * p + j] = div < H ? nan : ret[j];
    if (tid == 0) o.diverged_step[seq] = div;
}

size_t forecast_lds_bytes(int p, int D) {
    return ((size_t)2 * (((size_t)p * D + 3) & ~(size_t)3) + 2 * (size_t)p) * sizeof(float) + 16;
}

template <int ENV>
int forecast_launch(const ForecastArgs& a, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(forecast_stats_kernel<ENV>, dim3((unsigned)((size_t)a.m * a.n)), dim3(FC_THREADS), lds, s, a);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

// what a forecast refuses of the ctx, before any HIP call
int forecast_refuse_ctx(const cadm_ctx* ctx, const char* who) {
    CADM_REQUIRE(!ctx->cfg.discrete && ctx->cfg.env_kind != CADM_ENV_CARTPOLE,
                 "%s: discrete actions are not forecast (the random-shooting planner returns no plan)", who);
    if (ctx->cfg.env_kind == CADM_ENV_SPEC && !ctx->spec_set) {
        cadm_set_error("%s: the env spec is not set (call cadm_set_env_spec): its reward terms are evaluated from it", who);
        return CADM_ESTATE;
    }
    return CADM_OK;
}

int forecast_refuse_shape(const cadm_ctx* ctx, int m, int n, int H, int p, int E, int band_k, const char* who) {
    CADM_REQUIRE(m >= 1 && n >= 1 && H >= 1 && p >= 1, "%s: m, n, H, p must be >= 1 (got m=%d n=%d H=%d p=%d)", who, m, n, H, p);
    CADM_REQUIRE((long long)m * n <= 0x7fffffffLL, "%s: m * n = %lld sequences exceed one grid", who, (long long)m * n);
    CADM_REQUIRE(E >= 1 && p % E == 0, "%s: p (%d) must be a multiple of E (%d)", who, p, E);
    CADM_REQUIRE(band_k >= 1 && band_k <= p, "%s: band_k (%d) outside 1 .. p = %d", who, band_k, p);
    CADM_REQUIRE(forecast_lds_bytes(p, ctx->D) <= (size_t)FC_LDS_BUDGET,
                 "%s: p (%d) x D (%d) does not fit the kernel's LDS: two tiles of p * D floats and 2 * p accumulators need %zu bytes, the bound "
                 "is %d", who, p, ctx->D, forecast_lds_bytes(p, ctx->D), FC_LDS_BUDGET);
    return CADM_OK;
}

bool forecast_out_complete(const cadm_forecast_out* o) {
    return o && o->mean && o->member_mean && o->var_total && o->var_epistemic && o->var_aleatoric && o->lo && o->hi && o->reward_mean &&
           o->reward_var && o->reward_member && o->returns && o->diverged_step;
}

}  // namespace

extern "C" int cadm_forecast_stats(cadm_ctx* ctx, const float* traj, const float* obs, const float* actions, int m, int n, int H, int p, int E,
                                   int band_k, const cadm_forecast_out* out, void* stream) {
    CADM_REQUIRE(ctx && traj && obs && actions, "cadm_forecast_stats: ctx / traj / obs / actions is null");
    CADM_REQUIRE(forecast_out_complete(out), "cadm_forecast_stats: an output pointer is null");
    int rc = forecast_refuse_ctx(ctx, "cadm_forecast_stats");
    if (rc) return rc;
    if ((rc = forecast_refuse_shape(ctx, m, n, H, p, E, band_k, "cadm_forecast_stats"))) return rc;
    CADM_ON_DEVICE(ctx);
    ForecastArgs a{};
    a.traj = traj; a.obs = obs; a.actions = actions;
    a.m = m; a.n = n; a.H = H; a.p = p; a.E = E; a.D = ctx->D; a.A = ctx->A; a.PE = p / E; a.band_k = band_k;
    a.out = *out;
    forecast_spec_fill(ctx, &a.spec);
    const size_t lds = forecast_lds_bytes(p, ctx->D);
    hipStream_t s = (hipStream_t)stream;
    switch (ctx->cfg.env_kind) {
        case CADM_ENV_HALFCHEETAH: return forecast_launch<CADM_ENV_HALFCHEETAH>(a, lds, s);
        case CADM_ENV_ANT: return forecast_launch<CADM_ENV_ANT>(a, lds, s);
        case CADM_ENV_SLIM_HUMANOID: return forecast_launch<CADM_ENV_SLIM_HUMANOID>(a, lds, s);
        case CADM_ENV_PENDULUM: return forecast_launch<CADM_ENV_PENDULUM>(a, lds, s);
        default: return forecast_launch<CADM_ENV_SPEC>(a, lds, s);
    }
}

// cadm_plan_forecast: the context encoder, ONE rollout that records its trajectories, the statistics kernel above
struct ForecastWs {
    float *ctxv, *traj;
};

static size_t forecast_carve(cadm_ctx* ctx, int m, int n, char* base, ForecastWs* w) {
    Carver c{base};
    ForecastWs t;
    t.ctxv = c.take<float>((size_t)ctx->E * m * (ctx->C > 0 ? ctx->C : 1));
    t.traj = c.take<float>((size_t)ctx->H * m * n * ctx->p * ctx->D);
    if (w) *w = t;
    return c.off;
}

extern "C" size_t cadm_forecast_workspace_bytes(cadm_ctx* ctx, int m, int n) {
    if (!ctx || m <= 0 || n <= 0) return 0;
    return forecast_carve(ctx, m, n, nullptr, nullptr);
}

extern "C" int cadm_plan_forecast(cadm_ctx* ctx, const float* obs, const float* cp_obs, const float* cp_act, const float* actions,
                                  const float* eps, int m, int n, int band_k, uint32_t seed, uint32_t call, void* workspace,
                                  const cadm_forecast_out* out, void* stream) {
    CADM_REQUIRE(ctx && obs && actions && workspace, "cadm_plan_forecast: ctx / obs / actions / workspace is null");
    CADM_REQUIRE(forecast_out_complete(out) && out->rollout_returns, "cadm_plan_forecast: an output pointer is null");
    int rc = forecast_refuse_ctx(ctx, "cadm_plan_forecast");
    if (rc) return rc;
    if ((rc = forecast_refuse_shape(ctx, m, n, ctx->H, ctx->p, ctx->E, band_k, "cadm_plan_forecast"))) return rc;
    CADM_REQUIRE(ctx->C == 0 || (cp_obs && cp_act), "cadm_plan_forecast: cp_obs / cp_act required for a context model");
    CADM_REQUIRE(ctx->cfg.num_cem_iters <= CADM_FORECAST_IT, "cadm_plan_forecast: num_cem_iters (%d) reaches the forecast's iteration word %d",
                 ctx->cfg.num_cem_iters, CADM_FORECAST_IT);
    CADM_ON_DEVICE(ctx);
    ForecastWs w;
    forecast_carve(ctx, m, n, (char*)workspace, &w);
    if (ctx->C > 0 && (rc = cadm_context_forward(ctx, cp_obs, cp_act, m, 0, w.ctxv, stream))) return rc;
    // every rank of a sharded ctx rolls out all n sequences: no collective
    if ((rc = cadm_rollout_returns(ctx, obs, nullptr, ctx->C > 0 ? w.ctxv : nullptr, actions, ctx->cfg.deterministic ? nullptr : eps, 1, seed,
                                   call, CADM_FORECAST_IT, 0, n, m, n, out->rollout_returns, w.traj, stream))) return rc;
    return cadm_forecast_stats(ctx, w.traj, obs, actions, m, n, ctx->H, ctx->p, ctx->E, band_k, out, stream);
}
