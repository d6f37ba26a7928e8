// iCEM planner (Pinneri et al. 2020, "Sample-efficient Cross-Entropy Method for Real-time Planning"): an OPT-IN second planner loop
// beside cem_plan_impl (plan.hip).  No reference twin: the reference's CEM block (core/utils.py:398-488) draws white truncated-normal
// noise and keeps nothing between iterations or calls.  New here:
//   * temporally correlated ("coloured") candidate noise, synthesised per sequence from H spectral draws (icem_colored_kernel);
//   * elite carry-over inside a call and, shifted by one step, between calls (icem_keep_kernel / icem_inject_kernel);
//   * the best sequence seen in a call as the plan (icem_track_best_kernel);
//   * a decaying candidate count.
// The rollout, the context encoder, the truncated-normal sampler and the elite refit are the reference path's, called unchanged.
// The loop takes its update and its candidate score as parameters: cadm_icem_plan runs it with the elite refit, cadm_mppi_plan with the
// MPPI refit (mppi.hip), both on the particle mean; cadm_scored_plan chooses the update and the score (score.hip); cadm_constrained_plan
// also rewrites the particle returns under state constraints (constrain.hip) before the score sees them; cadm_knot_plan also shapes every
// iteration's candidates onto a grid of knot steps (knots.hip) before the rollout sees them; cadm_tracking_plan also takes the cost of
// run-time tracking targets (tracking.hip) off the particle returns, behind the constraints and before the score; cadm_actuated_plan also
// passes every iteration's candidates, and the plan, through an actuator model (actuator.hip: action delay, rate limits, rate cost);
// cadm_uncertain_plan also prices the ensemble's disagreement about the states a candidate visits (uncertainty.hip), off the candidate score;
// cadm_valued_plan also adds a caller-supplied value net's V of every particle's last state (value.hip) to the particle returns;
// cadm_rewarded_plan also adds a caller-supplied reward net's R of every step of every particle (reward.hip) to the particle returns;
// cadm_guided_plan also rolls a caller-supplied policy net through the model once per call (policy.hip) and places its proposal
// sequences among every iteration's candidates;
// cadm_critic_plan also adds weight * reduce_c Q_c(s_H, pi(s_H)) of caller-supplied critics at the registered actor's action (critic.hip) to
// the particle returns, in the place of the terminal value;
// cadm_anchored_plan also adds weight * sum_t log pi(a_t | s_t) of the registered actor's Gaussian head (policy_logp.hip) to the particle
// returns, behind the learned reward.
#include <math.h>

#include "planner.h"

// ---------------------------------------------------------------------------------------------
// coloured-noise candidates
// ---------------------------------------------------------------------------------------------
// One noise sequence z_0 .. z_{H-1} per (env mi, candidate c, action dim a), from spectral draws x_k, y_k ~ N(0,1):
//   z_t = c_b [ x_0 / sqrt2 + sum_{1 <= k < H/2} k^(-b/2) (x_k cos th_kt - y_k sin th_kt) + [H even] (H/2)^(-b/2) x_{H/2} (-1)^t / sqrt2 ]
//   th_kt = 2 pi ((k t) mod H) / H,    c_b = (1/2 + sum_{1 <= k < H/2} k^(-b) + [H even] (H/2)^(-b) / 2)^(-1/2)
// Var z_t = 1 for every t and b; b = 0 is an orthonormal transform of H iid normals (white); b > 0 weights the low frequencies.
// action = clip(mean + sd z_t, lb, ub), sd as in sample_action (common.h); no rejection (it would break the correlation).
//
// One thread owns one sequence: its H spectral numbers sit in LDS (slot-major: lanes read consecutive words), the H outputs are
// formed by direct synthesis (~H^2 / 2 multiply-adds).  The angle is reduced in integers, (k t) mod H, and looked up in a table of
// the H-th roots of unity built once per workgroup in double precision: accuracy does not depend on H.
// Spectral slots: 0 = x_0, then (x_k, y_k) at (2k - 1, 2k) for 1 <= k < H/2, and x_{H/2} at H - 1 when H is even: H numbers.
constexpr int ICEM_BLOCK = 64;

static size_t icem_colored_lds(int H) { return ((size_t)2 * H + (size_t)(H / 2 + 1) + (size_t)H * ICEM_BLOCK) * sizeof(float); }

__global__ __launch_bounds__(ICEM_BLOCK) void icem_colored_kernel(const float* __restrict__ mean, const float* __restrict__ var,
                                                                  const float* __restrict__ xi, float beta, double cbeta, uint32_t seed,
                                                                  uint32_t call, int it, int m, int n, int H, int A, float lb, float ub,
                                                                  float* __restrict__ out) {
    extern __shared__ float icem_sm[];
    float* ct = icem_sm;                    // [H] cos(2 pi j / H)
    float* st = ct + H;                     // [H] sin(2 pi j / H)
    float* wt = st + H;                     // [H/2 + 1] c_b k^(-b/2); [0] = c_b / sqrt2; [H/2] (H even) = c_b (H/2)^(-b/2) / sqrt2
    float* sp = wt + (H / 2 + 1);           // [H][ICEM_BLOCK] spectral numbers of this workgroup's sequences
    const int tid = threadIdx.x;
    const int nyq = (H & 1) ? -1 : H / 2;   // the Nyquist term exists for even H only
    for (int j = tid; j < H; j += ICEM_BLOCK) {
        double s, c;
        sincospi(2.0 * (double)j / (double)H, &s, &c);
        ct[j] = (float)c;
        st[j] = (float)s;
    }
    for (int k = tid; k <= H / 2; k += ICEM_BLOCK) {
        double w = k == 0 ? 0.70710678118654752440 : pow((double)k, -0.5 * (double)beta);
        if (k > 0 && k == nyq) w *= 0.70710678118654752440;
        wt[k] = (float)(cbeta * w);
    }
    const size_t total = (size_t)m * n * A;
    const size_t q = (size_t)blockIdx.x * ICEM_BLOCK + tid;      // global sequence index (mi * n + c) * A + a
    const bool live = q < total;
    if (live) {
        if (xi) {
            for (int s = 0; s < H; ++s) sp[s * ICEM_BLOCK + tid] = xi[q * H + s];
        } else {
            for (int k = 0; 2 * k <= H; ++k) {
                uint32_t r[4];
                philox4x32_10((uint32_t)(q & 0xFFFFFFFFull), (uint32_t)k, (uint32_t)(q >> 32), CADM_STREAM_ICEM | ((uint32_t)it << 8), seed, call, r);
                // Box-Muller with the library's accurate logf / sincosf: the spectral draws are summed, so their errors add up
                const float rad = sqrtf(-2.0f * logf(u01(r[0])));
                float sn, cs;
                sincosf(6.28318530717958647692f * u01(r[1]), &sn, &cs);
                if (k == 0) sp[tid] = rad * cs;
                else if (2 * k < H) { sp[(2 * k - 1) * ICEM_BLOCK + tid] = rad * cs; sp[(2 * k) * ICEM_BLOCK + tid] = rad * sn; }
                else sp[(H - 1) * ICEM_BLOCK + tid] = rad * cs;
            }
        }
    }
    __syncthreads();
    if (!live) return;
    const int a = (int)(q % A);
    const size_t mc = q / A;                                     // mi * n + c
    const int mi = (int)(mc / n);
    const float* mu_m = mean + (size_t)mi * H * A + a;
    const float* var_m = var + (size_t)mi * H * A + a;
    float* o = out + mc * H * A + a;
    const float x0 = sp[tid];
    const float xn = nyq > 0 ? sp[(H - 1) * ICEM_BLOCK + tid] : 0.0f;
    for (int t = 0; t < H; ++t) {
        float z = wt[0] * x0;
        for (int k = 1; 2 * k < H; ++k) {
            const int j = (k * t) % H;
            const float xk = sp[(2 * k - 1) * ICEM_BLOCK + tid], yk = sp[(2 * k) * ICEM_BLOCK + tid];
            z += wt[k] * (xk * ct[j] - yk * st[j]);
        }
        if (nyq > 0) z += (t & 1) ? -(wt[nyq] * xn) : wt[nyq] * xn;
        const float mu = mu_m[(size_t)t * A];
        const float a1 = (mu - lb) / 2.0f, a2 = (ub - mu) / 2.0f;
        const float cv = fminf(fminf(a1 * a1, a2 * a2), var_m[(size_t)t * A]);
        o[(size_t)t * A] = fminf(fmaxf(mu + sqrtf(cv) * z, lb), ub);
    }
}

static double icem_cbeta(int H, double beta) {
    double s = 0.5;
    for (int k = 1; 2 * k < H; ++k) s += pow((double)k, -beta);
    if (H % 2 == 0) s += 0.5 * pow((double)(H / 2), -beta);
    return 1.0 / sqrt(s);
}

extern "C" int cadm_sample_actions_colored(cadm_ctx* ctx, const float* mean, const float* var, const float* xi, float beta,
                                           uint32_t seed, uint32_t call, int it, int m, int n, float* actions_out, void* stream) {
    CADM_REQUIRE(ctx && mean && var && actions_out && m > 0 && n > 0, "cadm_sample_actions_colored: bad arguments");
    CADM_REQUIRE(beta >= 0.0f && beta <= 16.0f, "cadm_sample_actions_colored: noise_beta %g outside [0, 16]", (double)beta);
    CADM_REQUIRE(it >= 0 && it < (1 << 24), "cadm_sample_actions_colored: iteration %d outside [0, 2^24)", it);
    CADM_REQUIRE(!ctx->cfg.discrete, "cadm_sample_actions_colored: continuous actions only");
    const size_t lds = icem_colored_lds(ctx->H);
    CADM_REQUIRE(lds <= 64 * 1024, "cadm_sample_actions_colored: horizon %d needs %zu bytes of LDS (limit 65536)", ctx->H, lds);
    const size_t total = (size_t)m * n * ctx->A, blocks = (total + ICEM_BLOCK - 1) / ICEM_BLOCK;
    CADM_REQUIRE(blocks <= 0x7FFFFFFFull, "cadm_sample_actions_colored: %zu sequences are too many for one launch", total);
    CADM_ON_DEVICE(ctx);
    hipLaunchKernelGGL(icem_colored_kernel, dim3((unsigned)blocks), dim3(ICEM_BLOCK), lds, (hipStream_t)stream, mean, var, xi, beta,
                       icem_cbeta(ctx->H, (double)beta), seed, call, it, m, n, ctx->H, ctx->A, ctx->cfg.lower_bound, ctx->cfg.upper_bound,
                       actions_out);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

// ---------------------------------------------------------------------------------------------
// elite carry-over and the best plan of a call
// ---------------------------------------------------------------------------------------------
// kept[mi, j] = actions[mi, elites[mi, j]] for j < K (elites [m, KE]: the refit's order, return descending, ties to the lower index);
// valid_out (optional): valid_out[mi] = 1
__global__ void icem_keep_kernel(const float* __restrict__ actions, const int32_t* __restrict__ elites, int m, int n, int K, int KE, int HA,
                                 float* __restrict__ kept, int32_t* __restrict__ valid_out) {
    const size_t total = (size_t)m * K * HA;
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(q % HA);
        const size_t mj = q / HA;
        const int j = (int)(mj % K), mi = (int)(mj / K);
        const int32_t c = elites[(size_t)mi * KE + j];
        if ((uint32_t)c < (uint32_t)n) kept[q] = actions[((size_t)mi * n + c) * HA + e];
        if (valid_out && j == 0 && e == 0) valid_out[mi] = 1;
    }
}

// candidate slots [0, K) of every env (with valid[mi] != 0, when valid is given) take the kept sequences: whole (shift = 0), or moved one
// step towards the present (shift = 1: steps [0, H - 1) take kept steps [1, H); step H - 1 keeps what the sampler drew)
__global__ void icem_inject_kernel(const float* __restrict__ kept, const int32_t* __restrict__ valid, int m, int n, int K, int H, int A,
                                   int shift, float* __restrict__ actions) {
    const int HA = H * A;
    const size_t total = (size_t)m * K * HA;
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(q % HA);
        const size_t mj = q / HA;
        const int j = (int)(mj % K), mi = (int)(mj / K);
        if (valid && valid[mi] == 0) continue;
        if (shift && e >= HA - A) continue;
        actions[((size_t)mi * n + j) * HA + e] = kept[q + (shift ? A : 0)];
    }
}

// The iteration's best candidate against the best of this call so far.  Non-finite returns: the iteration's best is the candidate
// with the GREATEST NON-NaN return (+inf and -inf are returns like any other), ties -- -0.0 against +0.0 included -- to the lower
// index.  make_key (common.h) ranks a positive NaN above +inf, so an iteration's NaN returns come FIRST among its elites: the kernel
// walks elites[mi, 0 .. KE) (the refit's order) to the first whose return is not NaN, and when all KE are NaN takes the arg-max over
// the env's candidates itself.  An elite id outside [0, n) ends the walk: that env is left as it is.  The stored best is replaced
// where it holds nothing yet (best_ret NaN: icem_best_init_kernel) or the new return is STRICTLY greater (a tie keeps the earlier
// sequence): over a call the plan is the sequence with the greatest non-NaN return, ties to the earliest iteration, then to the
// lowest index, and NaN only if every return of the call is NaN.  One workgroup of TB_THREADS per env; every thread reads the
// stored return before any thread writes it.
constexpr int TB_THREADS = 256;

__global__ __launch_bounds__(TB_THREADS) void icem_track_best_kernel(const float* __restrict__ cand, const int32_t* __restrict__ elites,
                                                                     const float* __restrict__ actions, int n, int KE, int HA,
                                                                     float* __restrict__ best_ret, float* __restrict__ best_seq) {
    __shared__ float sv[TB_THREADS];
    __shared__ int si[TB_THREADS];
    const int mi = blockIdx.x, tid = threadIdx.x;
    const float* r_m = cand + (size_t)mi * n;
    const float old = best_ret[mi];
    int c = -1, j = 0;
    float r = 0.0f;
    for (; j < KE; ++j) {                                // (the same walk in every thread: what follows is uniform over the workgroup)
        const int32_t cj = elites[(size_t)mi * KE + j];
        if ((uint32_t)cj >= (uint32_t)n) break;
        const float rj = r_m[cj];
        if (rj == rj) { c = cj; r = rj; break; }
    }
    if (j == KE) {                                       // every elite's return is NaN
        int bi = -1;
        float bv = 0.0f;
        for (int i = tid; i < n; i += TB_THREADS) {      // (ascending i: a strict > keeps the lower index)
            const float v = r_m[i];
            if (v == v && (bi < 0 || v > bv)) { bv = v; bi = i; }
        }
        sv[tid] = bv;
        si[tid] = bi;
        __syncthreads();
        for (int d = TB_THREADS / 2; d > 0; d >>= 1) {
            if (tid < d) {
                const int oi = si[tid + d];
                const float ov = sv[tid + d];
                if (oi >= 0 && (si[tid] < 0 || ov > sv[tid] || (ov == sv[tid] && oi < si[tid]))) { sv[tid] = ov; si[tid] = oi; }
            }
            __syncthreads();
        }
        c = si[0];
        r = sv[0];
    }
    __syncthreads();
    if (c < 0 || r <= old) return;                       // (old NaN: nothing stored yet, r <= old is false)
    for (int e = tid; e < HA; e += TB_THREADS) best_seq[(size_t)mi * HA + e] = actions[((size_t)mi * n + c) * HA + e];
    if (tid == 0) best_ret[mi] = r;
}

__global__ void icem_best_init_kernel(int m, int HA, float* __restrict__ best_ret, float* __restrict__ best_seq) {
    const size_t total = (size_t)m * HA;
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
        best_seq[q] = __uint_as_float(0x7fc00000u);      // (a call whose returns are ALL NaN plans NaN, as the mean would,
        if (q < (size_t)m) best_ret[q] = __uint_as_float(0x7fc00000u);      //  and reports a NaN best return: nothing was scored)
    }
}

static int icem_grid(size_t total) {
    const size_t g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

static int launch_keep(cadm_ctx* ctx, const float* actions, const int32_t* elites, int m, int n, int K, float* kept, int32_t* valid_out,
                       hipStream_t s) {
    const int HA = ctx->H * ctx->A;
    hipLaunchKernelGGL(icem_keep_kernel, dim3(icem_grid((size_t)m * K * HA)), dim3(256), 0, s, actions, elites, m, n, K, ctx->cfg.num_elites,
                       HA, kept, valid_out);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

static int launch_inject(cadm_ctx* ctx, const float* kept, const int32_t* valid, int m, int n, int K, int shift, float* actions, hipStream_t s) {
    hipLaunchKernelGGL(icem_inject_kernel, dim3(icem_grid((size_t)m * K * ctx->H * ctx->A)), dim3(256), 0, s, kept, valid, m, n, K, ctx->H,
                       ctx->A, shift, actions);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

static int launch_track_best(cadm_ctx* ctx, const float* cand, const int32_t* elites, const float* actions, int m, int n, float* best_ret,
                             float* best_seq, hipStream_t s) {
    hipLaunchKernelGGL(icem_track_best_kernel, dim3(m), dim3(TB_THREADS), 0, s, cand, elites, actions, n, ctx->cfg.num_elites, ctx->H * ctx->A,
                       best_ret, best_seq);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

extern "C" int cadm_icem_keep(cadm_ctx* ctx, const float* actions, const int32_t* elites, int m, int n, int K, float* kept_out, void* stream) {
    CADM_REQUIRE(ctx && actions && elites && kept_out && m > 0 && n > 0, "cadm_icem_keep: bad arguments");
    CADM_REQUIRE(K >= 0 && K <= ctx->cfg.num_elites && K <= n, "cadm_icem_keep: keep_elites %d outside [0, min(num_elites %d, n %d)]", K,
                 ctx->cfg.num_elites, n);
    if (K == 0) return CADM_OK;
    CADM_ON_DEVICE(ctx);
    return launch_keep(ctx, actions, elites, m, n, K, kept_out, nullptr, (hipStream_t)stream);
}

extern "C" int cadm_icem_inject(cadm_ctx* ctx, const float* kept, const int32_t* valid, int m, int n, int K, int shift, float* actions_io,
                                void* stream) {
    CADM_REQUIRE(ctx && kept && actions_io && m > 0 && n > 0, "cadm_icem_inject: bad arguments");
    CADM_REQUIRE(K >= 0 && K <= n, "cadm_icem_inject: keep_elites %d outside [0, n %d]", K, n);
    CADM_REQUIRE(shift == 0 || shift == 1, "cadm_icem_inject: shift %d is not 0 or 1", shift);
    if (K == 0) return CADM_OK;
    CADM_ON_DEVICE(ctx);
    return launch_inject(ctx, kept, valid, m, n, K, shift, actions_io, (hipStream_t)stream);
}

extern "C" int cadm_icem_track_best(cadm_ctx* ctx, const float* cand_returns, const int32_t* elites, const float* actions, int m, int n,
                                    float* best_ret_io, float* best_seq_io, void* stream) {
    CADM_REQUIRE(ctx && cand_returns && elites && actions && best_ret_io && best_seq_io && m > 0 && n > 0, "cadm_icem_track_best: bad arguments");
    CADM_ON_DEVICE(ctx);
    return launch_track_best(ctx, cand_returns, elites, actions, m, n, best_ret_io, best_seq_io, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// the planner loop
// ---------------------------------------------------------------------------------------------
// the update that turns an iteration's scored candidates into the next distribution: the elite refit (cem.hip), or the softmax-weighted
// refit over all candidates (mppi.hip).  The rest of the loop is one body.
struct PlanUpdate {
    const char* who;           // the entry point's name, for its messages
    int mppi;                  // 0: cadm_launch_refit; 1: cadm_launch_mppi_refit
    float temperature;
    int relative;
};

struct IcemWs {
    float *ctxv, *actions, *rows, *cand, *mean, *var, *meanclip, *kept, *best_ret, *best_seq;
    int32_t* elites;
    float *emean, *evar, *mppi;      // MPPI only: where the elite selection's own refit goes (discarded), the update's weights and partials
    int32_t* first;                  // tracked under TERMINATE constraints only: the constraint kernel's first_violation [m, n, p], in front of traj
    float* traj;                     // constrained or tracked only: the rollout's trajectories [H, m, n, p, D], the last view of every loop before the
                                     // actuated one (the sums before it stay)
    float *acost, *aplan;            // actuated only, behind traj: the candidates' rate cost [m, n]; the plan [m, H, A] before its last actuate pass
    float *ustep, *ucost;            // uncertainty term only, behind everything before: the step costs u [m, n, H]; the candidates' cost [m, n]
    float* rstep;                    // learned reward only, behind everything before: the step rewards [H, m, n, p]
    float* pseqs; char* pws;         // policy prior only, behind everything before: the proposals [m, P, H, A]; the roll's workspace
    float* lstep;                    // actor's log-density only, behind everything else: the step log-densities [H, m, n, p]
};

static size_t icem_carve(const cadm_ctx* ctx, int m, int n, int K, int mppi, char* base, IcemWs* w, int traj = 0, int first = 0, int act = 0,
                         int unc = 0, int rew = 0, int pol = 0, int lgp = 0) {
    Carver c{base};
    const size_t HA = (size_t)ctx->H * ctx->A;
    IcemWs t{};
    t.ctxv = c.take<float>((size_t)ctx->E * m * (ctx->C > 0 ? ctx->C : 1));
    t.actions = c.take<float>((size_t)m * n * HA);
    t.rows = c.take<float>((size_t)m * n * ctx->p);
    t.cand = c.take<float>((size_t)m * n);
    t.mean = c.take<float>((size_t)m * HA);
    t.var = c.take<float>((size_t)m * HA);
    t.meanclip = c.take<float>((size_t)m * HA);
    t.kept = c.take<float>((size_t)m * (K > 0 ? K : 1) * HA);
    t.best_ret = c.take<float>((size_t)m);
    t.best_seq = c.take<float>((size_t)m * HA);
    t.elites = c.take<int32_t>((size_t)m * ctx->cfg.num_elites);
    if (mppi) {
        t.emean = c.take<float>((size_t)m * HA);
        t.evar = c.take<float>((size_t)m * HA);
        t.mppi = c.take<float>(cadm_mppi_scratch_floats(ctx, m, n));
    }
    if (first) t.first = c.take<int32_t>((size_t)m * n * ctx->p);
    if (traj) t.traj = c.take<float>((size_t)ctx->H * m * n * ctx->p * ctx->D);
    if (act) {
        t.acost = c.take<float>((size_t)m * n);
        t.aplan = c.take<float>((size_t)m * HA);
    }
    if (unc) {
        t.ustep = c.take<float>((size_t)m * n * ctx->H);
        t.ucost = c.take<float>((size_t)m * n);
    }
    if (rew) t.rstep = c.take<float>((size_t)ctx->H * m * n * ctx->p);
    if (pol > 0) {
        t.pseqs = c.take<float>((size_t)m * pol * HA);
        t.pws = c.take<char>(cadm_policy_workspace_bytes(const_cast<cadm_ctx*>(ctx), m, pol));
    }
    if (lgp) t.lstep = c.take<float>((size_t)ctx->H * m * n * ctx->p);
    if (w) *w = t;
    return c.off;
}

// On a ctx with a discount over the horizon (cadm_set_discount, discount.hip) the loop always records trajectories: every size below is
// then the one with the trajectory view.  The discount is set BEFORE the workspace is sized.  (A null ctx has none: icem_size refuses it.)
static int icem_discounted(const cadm_ctx* ctx) { return ctx && ctx->disc != nullptr; }

// every size export below: 0 for bad arguments (P, the proposals per env, at the levels that have them), else what icem_carve takes under
// the export's mapping of its flags to the carver's
static size_t icem_size(const cadm_ctx* ctx, int m, int n, int K, int mppi, int traj, int first = 0, int act = 0, int unc = 0, int rew = 0,
                        int P = 0, int lgp = 0) {
    if (!ctx || m <= 0 || n <= 0 || K < 0 || P < 0) return 0;
    return icem_carve(ctx, m, n, K, mppi != 0, nullptr, nullptr, traj, first, act, unc, rew, P, lgp);
}

extern "C" size_t cadm_icem_workspace_bytes(cadm_ctx* ctx, int m, int n, int K) { return icem_size(ctx, m, n, K, 0, icem_discounted(ctx)); }

extern "C" size_t cadm_mppi_workspace_bytes(cadm_ctx* ctx, int m, int n, int K) { return icem_size(ctx, m, n, K, 1, icem_discounted(ctx)); }

extern "C" size_t cadm_constrained_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi) { return icem_size(ctx, m, n, K, mppi, 1); }

extern "C" size_t cadm_tracking_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate) {
    return icem_size(ctx, m, n, K, mppi, 1, terminate != 0);
}

extern "C" size_t cadm_actuated_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int traj, int terminate) {
    return icem_size(ctx, m, n, K, mppi, traj != 0 || icem_discounted(ctx), traj != 0 && terminate != 0, 1);
}

extern "C" size_t cadm_uncertain_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate, int actuator) {
    return icem_size(ctx, m, n, K, mppi, 1, terminate != 0, actuator != 0, 1);
}

extern "C" size_t cadm_valued_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate, int actuator, int uncertainty) {
    return icem_size(ctx, m, n, K, mppi, 1, terminate != 0, actuator != 0, uncertainty != 0);
}

extern "C" size_t cadm_rewarded_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate, int actuator, int uncertainty) {
    return icem_size(ctx, m, n, K, mppi, 1, terminate != 0, actuator != 0, uncertainty != 0, 1);
}

// enough for every combination of terms: the rewarded loop's views, and with P > 0 behind them the proposals and the roll's workspace
// (a loop with fewer terms takes fewer views in front of the policy's: it fits)
extern "C" size_t cadm_guided_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate, int actuator, int uncertainty, int P) {
    return icem_size(ctx, m, n, K, mppi, 1, terminate != 0, actuator != 0, uncertainty != 0, 1, P);
}

// the guided loop's: a terminal Q reads the trajectory view and the first violations the other terms read, and takes no view of its own
extern "C" size_t cadm_critic_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate, int actuator, int uncertainty, int P) {
    return cadm_guided_workspace_bytes(ctx, m, n, K, mppi, terminate, actuator, uncertainty, P);
}

// the critic loop's, and behind everything the step log-densities [H, m, n, p] of the actor's log-density term (the views in front keep
// their places: a loop without the term carves what cadm_critic_plan carves)
extern "C" size_t cadm_anchored_workspace_bytes(cadm_ctx* ctx, int m, int n, int K, int mppi, int terminate, int actuator, int uncertainty, int P) {
    return icem_size(ctx, m, n, K, mppi, 1, terminate != 0, actuator != 0, uncertainty != 0, 1, P, 1);
}

// candidates of iteration `it`: max(floor(n / decay^it), 2 num_elites, K + 1), never more than the n the workspace holds
static int icem_n_it(int n, double decay, int it, int num_elites, int K) {
    double v = floor((double)n / pow(decay, (double)it));
    int ni = v >= (double)n ? n : (int)v;
    if (ni < 2 * num_elites) ni = 2 * num_elites;
    if (ni < K + 1) ni = K + 1;
    return ni < n ? ni : n;
}

// The terms a level of the nest may add to the loop; a value-initialised PlanTerms is "no term", and cadm_scored_plan's launches.  Each
// export fills the fields it has parameters for.  The ctx's discount over the horizon (cadm_set_discount, discount.hip) is not a term: with
// a table set every rollout records its trajectories, the env's own return is rewritten as sum_t disc[t] r_t directly behind the rollout
// (cadm_launch_discount), and every stage below weighs its steps by the same table; a terminal term's weight is multiplied by disc[H].
// No table: today's launches.
struct PlanTerms {
    // state constraints that rewrite the particle returns before the score (constrain.hip); null = none, and today's launches
    const cadm_constraint_params* constraints;
    // the grid every candidate is shaped onto before its rollout (knots.hip), phase [m] int32 on the device or null = 0; knots null or
    // spacing 1 = none, and today's launches.  With a grid, iteration 0's mean is the caller's shaped, in the workspace (init_mean is not written).
    const cadm_knot_params* knots;
    const int32_t* phase;
    // tracking terms whose cost against targets [m, T, K] (offset [m] int32 on the device or null = 0) comes off the particle returns behind
    // the constraints and before the score (tracking.hip); null = none, and today's launches.  With terms every rollout records its
    // trajectories, and TERMINATE constraints hand their first violations on: what a terminated trajectory holds behind them is not tracked.
    const cadm_track_params* terms;
    const float* targets;
    int T;
    const int32_t* offset;
    // an actuator model (actuator.hip) with the envs' last applied action prev [m, A] and committed steps prefix [m, delay, A] on the
    // device; null = none, and today's launches.  With it every iteration's candidates are actuated in place behind the knot shaping, their
    // rate cost comes off the candidate score behind cadm_particle_score, and the plan is actuated once more (n = 1) on a device copy before
    // it is written to plan_out; advance: then prev <- plan[:, 0], prefix[:, j] <- plan[:, 1 + j].
    const cadm_actuator_params* act;
    float* prev_io;
    float* prefix_io;
    int advance;
    // an uncertainty term (uncertainty.hip); null = none, and today's launches.  With it every rollout records its trajectories, TERMINATE
    // constraints hand their first violations on (with or without terms), and lambda times the cost of the counted steps comes off the
    // candidate score behind the actuator's: a statistic OVER the particles, so not off the particle rows.
    const cadm_uncertainty_params* unc;
    // a terminal value (value.hip) of the net registered with cadm_set_value_net; null = none, and today's launches.  With it every
    // rollout records its trajectories, TERMINATE constraints hand their first violations on, and weight * V(traj[H - 1]) is added to the
    // particle rows behind the constraints and the tracking terms and before the score: a risk-aware score sees return + value per particle.
    const cadm_value_params* value;
    // a learned step reward (reward.hip) of the net registered with cadm_set_reward_net; null = none, and today's launches.  With it
    // every rollout records its trajectories, TERMINATE constraints hand their first violations on, and weight * (the sum of R over the
    // counted steps) is added to the particle rows behind the constraints and the tracking terms and IN FRONT OF the terminal value.
    const cadm_reward_params* reward;
    // a policy prior (policy.hip) of the net registered with cadm_set_policy_net; null = none, and today's launches.  With it ONE
    // proposal roll behind the context encoder, and in every iteration its P sequences take the slots behind the kept elites and the mean
    // candidate, in front of the knot shaping and the actuator pass.
    const cadm_policy_params* policy;
    // a terminal Q (critic.hip) of the critics registered with cadm_set_critic_nets at the action of the registered policy net; null =
    // none, and today's launches.  It stands where the terminal value stands and excludes it: weight * reduce_c Q_c(s, pi(s)), s = traj[H - 1],
    // is added to the particle rows behind the constraints, the tracking terms and the learned reward, before the score.  `policy` may be
    // null with it: the critic needs the registered net, not the proposals.
    const cadm_critic_params* critic;
    // the actor's log-density (policy_logp.hip) of the registered policy net and its Gaussian head; null = none, and today's launches.
    // With it every rollout records its trajectories, TERMINATE constraints hand their first violations on, and weight * (the sum of
    // log pi(a_t | s_t) over the counted steps) is added to the particle rows behind the learned reward and IN FRONT OF the terminal value /
    // Q: a risk-aware score sees it per particle.  `policy` may be null with it, as for the critic.
    const cadm_policy_logp_params* logp;
};

// score: what a candidate's particle returns become before the update sees them (score.hip); null = the particle mean
static int icem_loop(cadm_ctx* ctx, const PlanUpdate& upd, const cadm_score_params* score, const cadm_icem_params* prm, const float* obs,
                     const float* cp_obs, const float* cp_act, const float* init_mean, const float* init_var, float* carry_io,
                     int32_t* carry_valid_io, int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out,
                     float* best_return_out, void* stream, const PlanTerms& t) {
    // (the fields by name, in their order: the body below reads them as it read its parameters)
    const auto& [constraints, knots, phase, terms, targets, T, offset, act, prev_io, prefix_io, advance, unc, value, reward, policy, critic, logp] = t;
    const char* who = upd.who;
    CADM_REQUIRE(ctx && prm && obs && init_mean && init_var && workspace && plan_out && m > 0 && n > 0, "%s: bad arguments", who);
    CADM_REQUIRE(!cadm_sharded(ctx), "%s: candidate-sharded planning is not supported (carried elites cannot be regenerated by id)", who);
    CADM_REQUIRE(!ctx->cfg.discrete, "%s: continuous actions only", who);
    const int K = prm->keep_elites, KE = ctx->cfg.num_elites, iters = ctx->cfg.num_cem_iters;
    CADM_REQUIRE(K >= 0 && K <= KE, "%s: keep_elites %d outside [0, num_elites %d]", who, K, KE);
    CADM_REQUIRE(prm->decay >= 1.0f && prm->decay <= 1e6f, "%s: decay %g must be >= 1", who, (double)prm->decay);
    CADM_REQUIRE(prm->noise_beta >= 0.0f && prm->noise_beta <= 16.0f, "%s: noise_beta %g outside [0, 16]", who, (double)prm->noise_beta);
    CADM_REQUIRE(n >= KE, "%s: n_candidates %d < num_elites %d", who, n, KE);
    CADM_REQUIRE(!prm->add_mean_last || n >= K + 1, "%s: n_candidates %d leaves no slot for the mean candidate behind %d kept elites", who, n, K);
    CADM_REQUIRE(K == 0 || (carry_io && carry_valid_io), "%s: carry / carry_valid required with keep_elites > 0", who);
    CADM_REQUIRE(ctx->C == 0 || (cp_obs && cp_act), "%s: cp_obs/cp_act required for a context model", who);
    CADM_REQUIRE(prm->noise_beta == 0.0f || icem_colored_lds(ctx->H) <= 64 * 1024, "%s: horizon %d is too long for the coloured sampler", who, ctx->H);
    int rc;
    if (upd.mppi && (rc = cadm_mppi_check(ctx, m, upd.temperature, who))) return rc;
    if ((rc = cadm_score_check(ctx, score, who))) return rc;
    if (constraints && (rc = cadm_constraint_check(ctx, constraints, who))) return rc;
    if (knots && (rc = cadm_knot_check(knots, who))) return rc;
    if (terms && (rc = cadm_track_check(ctx, terms, targets, T, who))) return rc;
    if (act) {
        if ((rc = cadm_actuator_check(ctx, act, who))) return rc;
        CADM_REQUIRE(prev_io && (act->delay == 0 || prefix_io), "%s: the actuator model needs prev [m, A], and prefix [m, delay, A] with a delay", who);
    }
    if (unc && (rc = cadm_uncertainty_check(ctx, unc, who))) return rc;
    if (value && (rc = cadm_value_plan_check(ctx, value, who))) return rc;
    if (reward && (rc = cadm_reward_plan_check(ctx, reward, who))) return rc;
    if (critic) {
        CADM_REQUIRE(!value, "%s: a terminal Q and a terminal value are both given: a plan has one terminal term", who);
        if ((rc = cadm_critic_plan_check(ctx, critic, who))) return rc;
    }
    if (logp && (rc = cadm_policy_logp_plan_check(ctx, logp, who))) return rc;
    const bool disc = ctx->disc != nullptr;
    if (disc && (rc = cadm_discount_check(ctx, who))) return rc;
    const int P = policy ? policy->n_samples : 0;
    if (policy) {
        if ((rc = cadm_policy_plan_check(ctx, policy, who))) return rc;
        const int n_min = icem_n_it(n, (double)prm->decay, iters - 1, KE, K);      // (the count never grows with the iteration)
        CADM_REQUIRE((long long)K + 1 + P <= n_min, "%s: %d kept elites, the mean candidate and %d policy proposals do not fit the %d "
                     "candidates of the smallest iteration", who, K, P, n_min);
        if ((rc = cadm_require_ready(ctx, who))) return rc;
    }
    const bool shape = knots && knots->spacing > 1;
    CADM_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    IcemWs w;
    // (w.traj: null without constraints, terms, an uncertainty term, a value, a reward, a critic, a log-density and a discount; w.first: null
    // unless terms, an uncertainty term, a value, a reward, a critic or a log-density follow TERMINATE constraints)
    const bool reads_traj = terms != nullptr || unc != nullptr || value != nullptr || reward != nullptr || critic != nullptr || logp != nullptr;
    icem_carve(ctx, m, n, K, upd.mppi, (char*)workspace, &w, constraints != nullptr || reads_traj || disc,
               reads_traj && constraints != nullptr && constraints->mode == CADM_CONSTRAIN_TERMINATE, act != nullptr, unc != nullptr,
               reward != nullptr, P, logp != nullptr);
    const int HA = ctx->H * ctx->A;
    const bool track = prm->return_best != 0 || best_return_out != nullptr;
    if (ctx->C > 0 && (rc = cadm_context_forward(ctx, cp_obs, cp_act, m, 0, w.ctxv, stream))) return rc;
    // the policy's proposals: one roll per call, injected into every iteration's candidates below
    if (policy && (rc = cadm_launch_policy_propose(ctx, policy, obs, ctx->C > 0 ? w.ctxv : nullptr, m, seed, call, w.pseqs, nullptr, w.pws, s,
                                                   who))) return rc;
    if (track) {
        hipLaunchKernelGGL(icem_best_init_kernel, dim3(icem_grid((size_t)m * HA)), dim3(256), 0, s, m, HA, w.best_ret, w.best_seq);
        CADM_CHECK_HIP(hipGetLastError());
    }
    if (shape) {      // iteration 0 samples around the caller's mean on the grid: a shaped copy (the refit runs with mean_in == mean_out anyway)
        if ((rc = cadm_launch_clip(init_mean, w.mean, m * HA, 0.0f, 0.0f, 0, s))) return rc;
        if ((rc = cadm_launch_shape_actions(ctx, knots, phase, m, 1, w.mean, s))) return rc;
    }
    for (int it = 0; it < iters; ++it) {
        const bool first = it == 0, last = it + 1 == iters;
        const int ni = icem_n_it(n, (double)prm->decay, it, KE, K);
        const float* mean_in = (first && !shape) ? init_mean : w.mean;
        const float* var_in = first ? init_var : w.var;
        // candidates [m, ni, H, A]: white truncated-normal noise (the reference path's sampler) or coloured noise
        if (prm->noise_beta > 0.0f) rc = cadm_sample_actions_colored(ctx, mean_in, var_in, nullptr, prm->noise_beta, seed, call, it, m, ni, w.actions, stream);
        else rc = cadm_sample_actions(ctx, mean_in, var_in, nullptr, seed, call, it, m, ni, w.actions, stream);
        if (rc) return rc;
        // slots [0, K): the previous call's elites moved one step on (iteration 0, envs that have some), or the previous iteration's
        if (K > 0 && (rc = first ? launch_inject(ctx, carry_io, carry_valid_io, m, ni, K, 1, w.actions, s)
                                 : launch_inject(ctx, w.kept, nullptr, m, ni, K, 0, w.actions, s))) return rc;
        // slot K of the last iteration: the current mean itself
        if (last && prm->add_mean_last) {
            if ((rc = cadm_launch_clip(mean_in, w.meanclip, m * HA, ctx->cfg.lower_bound, ctx->cfg.upper_bound, 1, s))) return rc;
            if ((rc = launch_inject(ctx, w.meanclip, nullptr, m, ni, 1, 0, w.actions + (size_t)K * HA, s))) return rc;
        }
        // behind them: the policy's proposals
        if (policy && (rc = launch_inject(ctx, w.pseqs, nullptr, m, ni, P, 0,
                                          w.actions + (size_t)(K + (last && prm->add_mean_last ? 1 : 0)) * HA, s))) return rc;
        // every candidate onto the grid, the injected slots included: ni, the packed count of this iteration, not the workspace's n
        if (shape && (rc = cadm_launch_shape_actions(ctx, knots, phase, m, ni, w.actions, s))) return rc;
        // and through the actuator: pins, rate limits, and what the moves cost
        if (act && (rc = cadm_launch_actuate(ctx, act, prev_io, prefix_io, m, ni, w.actions, w.acost, s))) return rc;
        if ((rc = cadm_rollout_returns(ctx, obs, nullptr, ctx->C > 0 ? w.ctxv : nullptr, w.actions, nullptr, 1, seed, call, it, 0, ni, m, ni,
                                       w.rows, w.traj, stream))) return rc;
        // a discount over the horizon: the rollout's undiscounted sums are replaced by sum_t disc[t] r_t from the trajectories, in front of
        // everything that rewrites the rows; the stages below read the ctx's table themselves
        if (disc && (rc = cadm_launch_discount(ctx, w.traj, obs, w.actions, m, ni, w.rows, w.rows, nullptr, s))) return rc;
        // the trajectories are [H, m, ni, p, D] of this iteration's ni candidates; the returns are rewritten in place
        if (constraints && (rc = cadm_constrain_returns(ctx, constraints, w.traj, obs, w.actions, w.rows, m, ni, w.rows, w.first, nullptr,
                                                        stream))) return rc;
        if (terms && (rc = cadm_tracking_returns(ctx, terms, w.traj, targets, T, offset, w.first, w.rows, m, ni, w.rows, nullptr, stream))) return rc;
        // what the env's own reward does not say: rows += weight * (the sum of R over the counted steps), of this iteration's ni packed candidates
        if (reward && (rc = cadm_launch_reward(ctx, reward, w.traj, obs, w.actions, w.first, m, ni, w.rows, w.rstep, s))) return rc;
        // what the actor would do: rows += weight * (the sum of log pi(a_t | s_t) over the counted steps), of this iteration's ni packed candidates
        if (logp && (rc = cadm_launch_policy_logp(ctx, logp, w.traj, obs, w.actions, w.first, m, ni, w.rows, w.lstep, s))) return rc;
        // what lies behind the horizon: rows += weight * V(last state), of this iteration's ni packed candidates
        if (value && (rc = cadm_launch_value(ctx, value, w.traj, w.first, m, ni, w.rows, s))) return rc;
        // or, from a learner without a V: rows += weight * reduce_c Q_c(last state, pi(last state)), one launch
        if (critic && (rc = cadm_launch_critic(ctx, critic, w.traj, w.first, m, ni, w.rows, s))) return rc;
        if ((rc = cadm_particle_score(ctx, w.rows, m, ni, score, w.cand, stream))) return rc;      // (the mean: cadm_particle_mean itself)
        // the cost is deterministic per candidate: it comes off the candidate score, not off the particle rows
        if (act && (rc = cadm_launch_actuator_sub(w.cand, w.acost, (size_t)m * ni, s))) return rc;
        // so is the ensemble's disagreement about the states: cand -= lambda * ucost, of this iteration's ni packed candidates
        if (unc && (rc = cadm_launch_uncertainty(ctx, unc, w.traj, w.first, m, ni, w.ustep, w.ucost, w.cand, s))) return rc;
        // the refitted mean, clipped (dynamics.py:365-366); actuated: into the workspace, for its last pass
        float* plan = (last && !prm->return_best) ? (act ? w.aplan : plan_out) : nullptr;
        if (!upd.mppi) {
            if ((rc = cadm_launch_refit(ctx, w.cand, nullptr, 1, ni, w.actions, m, mean_in, var_in, w.mean, w.var, w.elites, plan, s))) return rc;
        } else {
            // the elite ids that keep / track-best read are the elite selection's (top num_elites by return, descending, ties to the lower
            // index): its own refit goes to scratch.  Only when somebody reads them.
            if ((K > 0 || track) &&
                (rc = cadm_launch_refit(ctx, w.cand, nullptr, 1, ni, w.actions, m, mean_in, var_in, w.emean, w.evar, w.elites, nullptr, s))) return rc;
            if ((rc = cadm_launch_mppi_refit(ctx, w.cand, w.actions, m, ni, upd.temperature, upd.relative, mean_in, var_in, w.mean, w.var, plan,
                                             w.mppi, s))) return rc;
        }
        if (track && (rc = launch_track_best(ctx, w.cand, w.elites, w.actions, m, ni, w.best_ret, w.best_seq, s))) return rc;
        if (K > 0 && (rc = last ? launch_keep(ctx, w.actions, w.elites, m, ni, K, carry_io, carry_valid_io, s)
                                : launch_keep(ctx, w.actions, w.elites, m, ni, K, w.kept, nullptr, s))) return rc;
    }
    if (act) {
        // a mean of feasible sequences is feasible only up to rounding: one more pass with n = 1 on a device copy (plan_out may be pinned
        // host memory), for the best sequence a bitwise no-op; then the plan leaves, and episode time moves on by one step
        float* fin = prm->return_best ? w.best_seq : w.aplan;
        if ((rc = cadm_launch_actuate(ctx, act, prev_io, prefix_io, m, 1, fin, nullptr, s))) return rc;
        if ((rc = cadm_launch_clip(fin, plan_out, m * HA, 0.0f, 0.0f, 0, s))) return rc;
        if (advance && (rc = cadm_launch_actuator_advance(ctx, act, fin, prev_io, prefix_io, m, s))) return rc;
    } else if (prm->return_best && (rc = cadm_launch_clip(w.best_seq, plan_out, m * HA, 0.0f, 0.0f, 0, s))) return rc;
    if (best_return_out && (rc = cadm_launch_clip(w.best_ret, best_return_out, m, 0.0f, 0.0f, 0, s))) return rc;
    return CADM_OK;
}

extern "C" int cadm_icem_plan(cadm_ctx* ctx, const cadm_icem_params* prm, const float* obs, const float* cp_obs, const float* cp_act,
                              const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m, int n,
                              uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream) {
    const PlanUpdate upd{"cadm_icem_plan", 0, 0.0f, 0};
    return icem_loop(ctx, upd, nullptr, prm, obs, cp_obs, cp_act, init_mean, init_var, carry_io, carry_valid_io, m, n, seed, call, workspace,
                     plan_out, best_return_out, stream, PlanTerms{});
}

// the same loop with the MPPI update (mppi.hip) in place of the elite refit
extern "C" int cadm_mppi_plan(cadm_ctx* ctx, const cadm_mppi_params* prm, const float* obs, const float* cp_obs, const float* cp_act,
                              const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m, int n,
                              uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream) {
    CADM_REQUIRE(prm, "cadm_mppi_plan: bad arguments");
    const PlanUpdate upd{"cadm_mppi_plan", 1, prm->temperature, prm->relative};
    return icem_loop(ctx, upd, nullptr, &prm->icem, obs, cp_obs, cp_act, init_mean, init_var, carry_io, carry_valid_io, m, n, seed, call,
                     workspace, plan_out, best_return_out, stream, PlanTerms{});
}

// The nest: eleven exports, each the one before it with its own term's parameters in front; a level whose own struct is null enqueues the
// launches of the level below.  Each fills the leading fields of a PlanTerms -- its own parameters, in the struct's order -- and leaves the
// rest "no term".  What all eleven refuse first, in this order, the update they choose, and the loop:
static int nest_plan(const char* who, const PlanTerms& t, cadm_ctx* ctx, const cadm_score_params* score, int update, const cadm_mppi_params* prm,
                     const float* obs, const float* cp_obs, const float* cp_act, const float* init_mean, const float* init_var, float* carry_io,
                     int32_t* carry_valid_io, int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out,
                     float* best_return_out, void* stream) {
    CADM_REQUIRE(prm, "%s: bad arguments", who);
    CADM_REQUIRE(update == 0 || update == 1, "%s: update %d is not 0 (elite refit) or 1 (MPPI)", who, update);
    const PlanUpdate upd{who, update, update ? prm->temperature : 0.0f, update ? prm->relative : 0};
    return icem_loop(ctx, upd, score, &prm->icem, obs, cp_obs, cp_act, init_mean, init_var, carry_io, carry_valid_io, m, n, seed, call,
                     workspace, plan_out, best_return_out, stream, t);
}

// the innermost: the update and the candidate score chosen by the caller (score.hip); score null or MEAN: the launches of the two above
extern "C" int cadm_scored_plan(cadm_ctx* ctx, const cadm_score_params* score, int update, const cadm_mppi_params* prm, const float* obs,
                                const float* cp_obs, const float* cp_act, const float* init_mean, const float* init_var, float* carry_io,
                                int32_t* carry_valid_io, int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out,
                                float* best_return_out, void* stream) {
    return nest_plan("cadm_scored_plan", PlanTerms{}, ctx, score, update, prm, obs, cp_obs, cp_act, init_mean, init_var, carry_io,
                     carry_valid_io, m, n, seed, call, workspace, plan_out, best_return_out, stream);
}

// adds state constraints (constrain.hip) between the rollout and the score; constraints null: cadm_scored_plan's launches
extern "C" int cadm_constrained_plan(cadm_ctx* ctx, const cadm_constraint_params* constraints, const cadm_score_params* score, int update,
                                     const cadm_mppi_params* prm, const float* obs, const float* cp_obs, const float* cp_act,
                                     const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m, int n,
                                     uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream) {
    return nest_plan("cadm_constrained_plan", PlanTerms{constraints}, ctx, score, update, prm, obs, cp_obs, cp_act, init_mean, init_var,
                     carry_io, carry_valid_io, m, n, seed, call, workspace, plan_out, best_return_out, stream);
}

// adds the shaping of every candidate onto a grid of knot steps (knots.hip) between the injections and the rollout; knots null or
// spacing 1: cadm_constrained_plan's launches
extern "C" int cadm_knot_plan(cadm_ctx* ctx, const cadm_knot_params* knots, const int32_t* phase, const cadm_constraint_params* constraints,
                              const cadm_score_params* score, int update, const cadm_mppi_params* prm, const float* obs, const float* cp_obs,
                              const float* cp_act, const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io,
                              int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out,
                              void* stream) {
    return nest_plan("cadm_knot_plan", PlanTerms{constraints, knots, phase}, ctx, score, update, prm, obs, cp_obs, cp_act, init_mean,
                     init_var, carry_io, carry_valid_io, m, n, seed, call, workspace, plan_out, best_return_out, stream);
}

// adds the cost of run-time tracking targets (tracking.hip), taken off the particle returns between the constraints and the score;
// track null: cadm_knot_plan's launches
extern "C" int cadm_tracking_plan(cadm_ctx* ctx, const cadm_track_params* track, const float* targets, int T, const int32_t* offset,
                                  const cadm_knot_params* knots, const int32_t* phase, const cadm_constraint_params* constraints,
                                  const cadm_score_params* score, int update, const cadm_mppi_params* prm, const float* obs,
                                  const float* cp_obs, const float* cp_act, const float* init_mean, const float* init_var, float* carry_io,
                                  int32_t* carry_valid_io, int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out,
                                  float* best_return_out, void* stream) {
    return nest_plan("cadm_tracking_plan", PlanTerms{constraints, knots, phase, track, targets, T, offset}, ctx, score, update, prm, obs,
                     cp_obs, cp_act, init_mean, init_var, carry_io, carry_valid_io, m, n, seed, call, workspace, plan_out, best_return_out,
                     stream);
}

// adds an actuator model (actuator.hip) between the knot shaping and the rollout, its rate cost behind the score and its last pass over
// the plan; act null: cadm_tracking_plan's launches
extern "C" int cadm_actuated_plan(cadm_ctx* ctx, const cadm_actuator_params* act, float* prev_io, float* prefix_io, int advance,
                                  const cadm_track_params* track, const float* targets, int T, const int32_t* offset,
                                  const cadm_knot_params* knots, const int32_t* phase, const cadm_constraint_params* constraints,
                                  const cadm_score_params* score, int update, const cadm_mppi_params* prm, const float* obs,
                                  const float* cp_obs, const float* cp_act, const float* init_mean, const float* init_var, float* carry_io,
                                  int32_t* carry_valid_io, int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out,
                                  float* best_return_out, void* stream) {
    return nest_plan("cadm_actuated_plan", PlanTerms{constraints, knots, phase, track, targets, T, offset, act, prev_io, prefix_io,
                     advance}, ctx, score, update, prm, obs, cp_obs, cp_act, init_mean, init_var, carry_io, carry_valid_io, m, n, seed,
                     call, workspace, plan_out, best_return_out, stream);
}

// adds the price of the ensemble's disagreement about the states a candidate visits (uncertainty.hip), off the candidate score, behind
// the actuator's cost and before the refit; unc null: cadm_actuated_plan's launches
extern "C" int cadm_uncertain_plan(cadm_ctx* ctx, const cadm_uncertainty_params* unc, const cadm_actuator_params* act, float* prev_io,
                                   float* prefix_io, int advance, const cadm_track_params* track, const float* targets, int T,
                                   const int32_t* offset, const cadm_knot_params* knots, const int32_t* phase,
                                   const cadm_constraint_params* constraints, const cadm_score_params* score, int update,
                                   const cadm_mppi_params* prm, const float* obs, const float* cp_obs, const float* cp_act,
                                   const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m, int n,
                                   uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream) {
    return nest_plan("cadm_uncertain_plan", PlanTerms{constraints, knots, phase, track, targets, T, offset, act, prev_io, prefix_io,
                     advance, unc}, ctx, score, update, prm, obs, cp_obs, cp_act, init_mean, init_var, carry_io, carry_valid_io, m, n, seed,
                     call, workspace, plan_out, best_return_out, stream);
}

// adds weight * V of every particle's last state (value.hip, the net of cadm_set_value_net) to the particle returns, behind the
// constraints and the tracking terms and before the score; value null: cadm_uncertain_plan's launches
extern "C" int cadm_valued_plan(cadm_ctx* ctx, const cadm_value_params* value, const cadm_uncertainty_params* unc,
                                const cadm_actuator_params* act, float* prev_io, float* prefix_io, int advance,
                                const cadm_track_params* track, const float* targets, int T, const int32_t* offset,
                                const cadm_knot_params* knots, const int32_t* phase, const cadm_constraint_params* constraints,
                                const cadm_score_params* score, int update, const cadm_mppi_params* prm, const float* obs, const float* cp_obs,
                                const float* cp_act, const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io,
                                int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out,
                                void* stream) {
    return nest_plan("cadm_valued_plan", PlanTerms{constraints, knots, phase, track, targets, T, offset, act, prev_io, prefix_io, advance,
                     unc, value}, ctx, score, update, prm, obs, cp_obs, cp_act, init_mean, init_var, carry_io, carry_valid_io, m, n, seed,
                     call, workspace, plan_out, best_return_out, stream);
}

// adds weight * (the sum over the counted steps of R, reward.hip, the net of cadm_set_reward_net) to the particle returns, behind the
// constraints and the tracking terms and in front of the terminal value; reward null: cadm_valued_plan's launches
extern "C" int cadm_rewarded_plan(cadm_ctx* ctx, const cadm_reward_params* reward, const cadm_value_params* value,
                                  const cadm_uncertainty_params* unc, const cadm_actuator_params* act, float* prev_io, float* prefix_io,
                                  int advance, const cadm_track_params* track, const float* targets, int T, const int32_t* offset,
                                  const cadm_knot_params* knots, const int32_t* phase, const cadm_constraint_params* constraints,
                                  const cadm_score_params* score, int update, const cadm_mppi_params* prm, const float* obs,
                                  const float* cp_obs, const float* cp_act, const float* init_mean, const float* init_var, float* carry_io,
                                  int32_t* carry_valid_io, int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out,
                                  float* best_return_out, void* stream) {
    return nest_plan("cadm_rewarded_plan", PlanTerms{constraints, knots, phase, track, targets, T, offset, act, prev_io, prefix_io, advance,
                     unc, value, reward}, ctx, score, update, prm, obs, cp_obs, cp_act, init_mean, init_var, carry_io, carry_valid_io, m, n,
                     seed, call, workspace, plan_out, best_return_out, stream);
}

// adds the proposals of a caller-supplied policy net (policy.hip, the net of cadm_set_policy_net), rolled through the model once per
// call, among every iteration's candidates; policy null: cadm_rewarded_plan's launches
extern "C" int cadm_guided_plan(cadm_ctx* ctx, const cadm_policy_params* policy, const cadm_reward_params* reward,
                                const cadm_value_params* value, const cadm_uncertainty_params* unc, const cadm_actuator_params* act,
                                float* prev_io, float* prefix_io, int advance, const cadm_track_params* track, const float* targets, int T,
                                const int32_t* offset, const cadm_knot_params* knots, const int32_t* phase,
                                const cadm_constraint_params* constraints, const cadm_score_params* score, int update,
                                const cadm_mppi_params* prm, const float* obs, const float* cp_obs, const float* cp_act,
                                const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m, int n,
                                uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream) {
    return nest_plan("cadm_guided_plan", PlanTerms{constraints, knots, phase, track, targets, T, offset, act, prev_io, prefix_io, advance,
                     unc, value, reward, policy}, ctx, score, update, prm, obs, cp_obs, cp_act, init_mean, init_var, carry_io,
                     carry_valid_io, m, n, seed, call, workspace, plan_out, best_return_out, stream);
}

// adds weight * reduce_c Q_c(s_H, pi(s_H)) of every particle's last state (critic.hip, the critics of
// cadm_set_critic_nets at the action of the net of cadm_set_policy_net) to the particle returns where the terminal value would be;
// critic null: cadm_guided_plan's launches
extern "C" int cadm_critic_plan(cadm_ctx* ctx, const cadm_critic_params* critic, const cadm_policy_params* policy,
                                const cadm_reward_params* reward, const cadm_value_params* value, const cadm_uncertainty_params* unc,
                                const cadm_actuator_params* act, float* prev_io, float* prefix_io, int advance, const cadm_track_params* track,
                                const float* targets, int T, const int32_t* offset, const cadm_knot_params* knots, const int32_t* phase,
                                const cadm_constraint_params* constraints, const cadm_score_params* score, int update,
                                const cadm_mppi_params* prm, const float* obs, const float* cp_obs, const float* cp_act,
                                const float* init_mean, const float* init_var, float* carry_io, int32_t* carry_valid_io, int m, int n,
                                uint32_t seed, uint32_t call, void* workspace, float* plan_out, float* best_return_out, void* stream) {
    return nest_plan("cadm_critic_plan", PlanTerms{constraints, knots, phase, track, targets, T, offset, act, prev_io, prefix_io, advance,
                     unc, value, reward, policy, critic}, ctx, score, update, prm, obs, cp_obs, cp_act, init_mean, init_var, carry_io,
                     carry_valid_io, m, n, seed, call, workspace, plan_out, best_return_out, stream);
}

// the outermost level today: adds weight * (the sum over the counted steps of log pi(a_t | s_t), policy_logp.hip, the net of
// cadm_set_policy_net with the head of cadm_set_policy_head) to the particle returns, behind the learned reward and in front of the
// terminal value / Q; logp null: cadm_critic_plan's launches
extern "C" int cadm_anchored_plan(cadm_ctx* ctx, const cadm_policy_logp_params* logp, const cadm_critic_params* critic,
                                  const cadm_policy_params* policy, const cadm_reward_params* reward, const cadm_value_params* value,
                                  const cadm_uncertainty_params* unc, const cadm_actuator_params* act, float* prev_io, float* prefix_io,
                                  int advance, const cadm_track_params* track, const float* targets, int T, const int32_t* offset,
                                  const cadm_knot_params* knots, const int32_t* phase, const cadm_constraint_params* constraints,
                                  const cadm_score_params* score, int update, const cadm_mppi_params* prm, const float* obs,
                                  const float* cp_obs, const float* cp_act, const float* init_mean, const float* init_var, float* carry_io,
                                  int32_t* carry_valid_io, int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out,
                                  float* best_return_out, void* stream) {
    return nest_plan("cadm_anchored_plan", PlanTerms{constraints, knots, phase, track, targets, T, offset, act, prev_io, prefix_io, advance,
                     unc, value, reward, policy, critic, logp}, ctx, score, update, prm, obs, cp_obs, cp_act, init_mean, init_var, carry_io,
                     carry_valid_io, m, n, seed, call, workspace, plan_out, best_return_out, stream);
}
