// Risk-aware candidate scores of the opt-in planner loop (icem.hip): what a candidate's p particle returns become before the update
// ranks or weighs it.  No reference twin: the reference's score is the plain particle mean (core/utils.py:474), which stays the default
// and the only score of cadm_cem_plan / cadm_rs_plan.  rows [m, n_local, p] -> cand [m, n_local] under a mode:
//   MEAN        mu                                  -- cadm_particle_mean itself is enqueued: the same kernel, grid and bits
//   MEAN_STD    mu - kappa sigma,    sigma   = sqrt(sum_j (r_j - mu)^2 / p)
//   MEMBER_STD  mu - kappa sigma_E,  sigma_E = sqrt(sum_e (mu_e - mu)^2 / E),  mu_e = the mean of member e's q = p / E particles
//                                              (particle j belongs to member j / q: horizon.hip, the rollout)
//   CVAR        (sum of the k lowest r_j) / k;  r_j counts iff rank_j < k,  rank_j = #{i : r_i < r_j or (r_i == r_j and i < j)}
// mu is particle_mean_kernel's (cem.hip): one fp32 chain over j = 0 .. p - 1, then / (float)p; every other sum is one chain in index
// order as well (deviations after the mean: a one-pass sum of squares cancels), so a candidate's score is the same bits run to run
// and does not depend on m, n_local or the candidate's position.  kappa = 0 gives mu's bits (mu - 0 * sigma).
// Non-finite input: a candidate with a NaN or +-inf particle return (or finite returns whose sum overflows) scores mu, bit for bit what
// cadm_particle_mean gives it, in every mode: a diverged row meets the elite ranking, the best-plan tracking and MPPI's zero weight
// exactly as under MEAN.
//
// Mapping: one thread per candidate, one wave (64 candidates) per workgroup -- at planner sizes (m n of a few hundred to a few
// thousand) that is the most workgroups, and the kernel is latency-bound.  A thread walking its own row reads words p apart from
// its neighbour's: with short rows (p = 20: 80 bytes) every load instruction of the wave would touch 64 different cache lines.  So
// the workgroup first copies its 64 rows -- one contiguous span of 64 p floats -- into LDS with consecutive lanes reading consecutive
// words, and the threads then walk LDS.  Rows sit p | 1 floats apart there: an odd stride puts the 32 lanes of a ds_read_b32 group
// on 32 different banks.  The rank count reads r_i and r_j by index from LDS: no per-thread array, no scratch.
// From p = 128 on (64 rows of p | 1 floats no longer fit 32 KiB) the threads read global memory directly, through the same
// arithmetic (same bits): a row is then >= 512 bytes, whole cache lines of its own, so a thread's walk uses every byte it fetches
// and the L1 / L2 absorb the re-reads of the rank count.  p has no upper bound on that path.
#include <math.h>

#include "planner.h"

namespace {

constexpr int SC_BLOCK = 64;                 // candidates (threads) per workgroup: one wave
constexpr int SC_LDS_MAX_P = 127;            // 64 * (127 | 1 = 127) * 4 = 32512 bytes

__device__ __forceinline__ bool sc_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// r: the candidate's p returns (LDS or global); returns the score
__device__ __forceinline__ float sc_score(const float* __restrict__ r, int p, int mode, float kappa, int k, int E) {
    float s = 0.0f;
    bool finite = true;
    for (int j = 0; j < p; ++j) {
        const float v = r[j];
        s += v;
        finite = finite && sc_finite(v);
    }
    const float mu = s / (float)p;                       // particle_mean_kernel's chain
    if (!finite || !sc_finite(mu)) return mu;
    if (mode == CADM_SCORE_MEAN_STD) {
        float ss = 0.0f;
        for (int j = 0; j < p; ++j) {
            const float d = r[j] - mu;
            ss += d * d;
        }
        return mu - kappa * sqrtf(ss / (float)p);
    }
    if (mode == CADM_SCORE_MEMBER_STD) {
        const int q = p / E;
        float ss = 0.0f;
        for (int e = 0; e < E; ++e) {
            float se = 0.0f;
            for (int j = 0; j < q; ++j) se += r[e * q + j];
            const float d = se / (float)q - mu;
            ss += d * d;
        }
        return mu - kappa * sqrtf(ss / (float)E);
    }
    // CVAR: the k lowest by (value, index), added in particle order
    float t = 0.0f;
    for (int j = 0; j < p; ++j) {
        const float rj = r[j];
        int rank = 0;
        for (int i = 0; i < p; ++i) {
            const float ri = r[i];
            rank += (ri < rj || (ri == rj && i < j)) ? 1 : 0;
        }
        if (rank < k) t += rj;
    }
    return t / (float)k;
}

template <bool LDS>
__global__ __launch_bounds__(SC_BLOCK) void particle_score_kernel(const float* __restrict__ rows, int total, int p, int mode, float kappa,
                                                                  int k, int E, float* __restrict__ out) {
    extern __shared__ float sc_sm[];
    const int tid = threadIdx.x;
    const size_t c0 = (size_t)blockIdx.x * SC_BLOCK;     // first candidate of this workgroup (c0 < total: the grid is ceil(total / 64))
    const int nc = (size_t)total - c0 < (size_t)SC_BLOCK ? (int)((size_t)total - c0) : SC_BLOCK;
    const float* r;
    if (LDS) {
        const int ps = p | 1;
        const float* span = rows + c0 * p;               // nc rows, contiguous: lanes read consecutive words
        for (int e = tid; e < nc * p; e += SC_BLOCK) {
            const int c = e / p;
            sc_sm[c * ps + (e - c * p)] = span[e];
        }
        __syncthreads();
        r = sc_sm + tid * ps;
    } else {
        r = rows + (c0 + tid) * p;
    }
    if (tid >= nc) return;
    out[c0 + tid] = sc_score(r, p, mode, kappa, k, E);
}

}  // namespace

// the refusals of a score, before any HIP call (score == null: the mean)
int cadm_score_check(const cadm_ctx* ctx, const cadm_score_params* score, const char* who) {
    if (!score || score->mode == CADM_SCORE_MEAN) return CADM_OK;
    CADM_REQUIRE(score->mode == CADM_SCORE_MEAN_STD || score->mode == CADM_SCORE_MEMBER_STD || score->mode == CADM_SCORE_CVAR,
                 "%s: unknown score mode %d", who, score->mode);
    if (score->mode == CADM_SCORE_CVAR)
        CADM_REQUIRE(score->k >= 1 && score->k <= ctx->p, "%s: cvar k %d outside [1, n_particles %d]", who, score->k, ctx->p);
    else
        CADM_REQUIRE(isfinite(score->kappa), "%s: score kappa %g is not finite", who, (double)score->kappa);
    return CADM_OK;
}

extern "C" int cadm_particle_score(cadm_ctx* ctx, const float* returns_rows, int m, int n_local, const cadm_score_params* score,
                                   float* cand_returns, void* stream) {
    CADM_REQUIRE(ctx && returns_rows && cand_returns && m > 0 && n_local > 0, "cadm_particle_score: bad arguments");
    int rc;
    if ((rc = cadm_score_check(ctx, score, "cadm_particle_score"))) return rc;
    if (!score || score->mode == CADM_SCORE_MEAN) return cadm_particle_mean(ctx, returns_rows, m, n_local, cand_returns, stream);
    const size_t total = (size_t)m * n_local, blocks = (total + SC_BLOCK - 1) / SC_BLOCK;
    CADM_REQUIRE(total <= 0x7FFFFFFFull, "cadm_particle_score: %zu candidates are too many for one launch", total);
    CADM_ON_DEVICE(ctx);
    const int p = ctx->p;
    if (p <= SC_LDS_MAX_P) {
        hipLaunchKernelGGL(particle_score_kernel<true>, dim3((unsigned)blocks), dim3(SC_BLOCK), (size_t)SC_BLOCK * (p | 1) * sizeof(float),
                           (hipStream_t)stream, returns_rows, (int)total, p, score->mode, score->kappa, score->k, ctx->E, cand_returns);
    } else {
        hipLaunchKernelGGL(particle_score_kernel<false>, dim3((unsigned)blocks), dim3(SC_BLOCK), 0, (hipStream_t)stream, returns_rows,
                           (int)total, p, score->mode, score->kappa, score->k, ctx->E, cand_returns);
    }
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}
