// Open-loop prediction error of the ensemble along the horizon: trajectories of a rollout (`traj_out` of the rollout kernel,
// [F, m, 1, p, D]) against held-out next observations, reduced on the device to per-step sums (cadm_horizon_error;
// cadm_eval_horizon, at the end of this file, strings encoder, rollout and this kernel together chunk by chunk).
//
// Per (window i, step h) that is VALID -- future_bool[i, 0..h] all non-zero: a hole invalidates everything behind it -- and whose
// p * D trajectory values are all finite (else the pair only counts in diverged[h]):
//     se[h, d]           += (mean over the p particles - truth)^2
//     spread[h, d]       += biased variance over the p particles
//     se_member[e, h, d] += (mean over member e's p / E particles - truth)^2        (particle j belongs to member j / (p / E))
//     count[h]           += 1
// Sums and counts only; the caller divides.
//
// Reduction contract (no floating-point atomics anywhere):
//   stage 1  one workgroup per (block of 64 consecutive windows, step) writes ONE partial.  Block boundaries are multiples of 64 in
//            the GLOBAL window index (window0 % 64 == 0), and inside a block window w adds into slot w % WT in window order, the WT
//            slots are then added in slot order -- WT depends on (p, E, D) only.
//   stage 2  one thread per output entry adds the blocks' partials in block order.
// The result is therefore bit-identical run to run and does not depend on how the caller cuts the windows into launches.
// A statistic is a chain of at most p / E + E + 7 + 64 / WT + WT + (blocks - 1) fp32 roundings, its terms non-negative.
//
// Traffic: `traj` is read exactly once -- a (block, step)'s windows are one contiguous span of 64 * p * D floats, loaded lane-linear
// with 16-byte loads into LDS (scalar loads where the span is not 16-byte aligned), 16 windows at a time; means and variances are
// formed from LDS in two passes (mean first: a one-pass sum of squares cancels).  Truth (1 / p of the traffic) and mask are read in place.
#include "planner.h"

namespace {

constexpr int HE_BLOCK = 64;                 // windows per partial
constexpr int HE_THREADS = 256;
constexpr int HE_MAX_WT = 16;                // windows per LDS tile (keeps the rounding chain of a block short, see above)
constexpr int HE_LDS_BUDGET = 48 * 1024;     // tile + accumulators, below the 64 KiB a kernel gets without an attribute

struct HorizonArgs {
    const float *traj, *truth, *mask;
    long long truth_ld;                      // floats between the truth rows of consecutive windows
    int m, F, p, E, D, PE, WT;
    long long block0;                        // window0 / 64: global index of this launch's first block
    float* partials;                         // [blocks][F][stride] words
    int stride;                              // (2 + E) * D floats (se, spread, se_member[E]) + 2 int32 (count, diverged)
};

__device__ __forceinline__ bool non_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(HE_THREADS) void horizon_error_kernel(const HorizonArgs a) {
    extern __shared__ __attribute__((aligned(16))) float he_smem[];
    const int D = a.D, p = a.p, E = a.E, PE = a.PE, WT = a.WT, pD = p * D, K = 2 + E, KD = K * D;
    float* tile = he_smem;                                   // [WT][p][D]: the trajectory values of WT windows at this step
    float* acc = tile + ((WT * pD + 3) & ~3);                // [WT][K][D]: slot w % WT of every statistic
    int* ok = reinterpret_cast<int*>(acc + WT * KD);         // [WT] the window exists and the step is valid
    int* bad = ok + WT;                                      // [WT] a non-finite value was loaded
    int* cnt = bad + WT;                                     // count, diverged
    const int blk = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    const int wb0 = blk * HE_BLOCK;
    for (int i = tid; i < WT * KD; i += HE_THREADS) acc[i] = 0.0f;
    if (tid < 2) cnt[tid] = 0;
    for (int t0 = 0; t0 < HE_BLOCK && wb0 + t0 < a.m; t0 += WT) {
        const int w0 = wb0 + t0;
        const int nw = a.m - w0 < WT ? a.m - w0 : WT;
        __syncthreads();                                     // the previous tile is consumed (first round: the accumulators are zero)
        if (tid < WT) {
            int v = 0;
            if (tid < nw) {                                  // prefix rule
                const float* mk = a.mask + (size_t)(w0 + tid) * a.F;
                v = 1;
                for (int f = 0; f <= h; ++f) v &= mk[f] != 0.0f ? 1 : 0;
            }
            ok[tid] = v;
            bad[tid] = 0;
        }
        __syncthreads();
        const float* src = a.traj + ((size_t)h * a.m + w0) * pD;
        const int len = nw * pD;
        const int nvec = (reinterpret_cast<uintptr_t>(src) & 15) == 0 ? len >> 2 : 0;
        for (int i = tid; i < nvec; i += HE_THREADS) {
            const floatx4 v = reinterpret_cast<const floatx4*>(src)[i];
            reinterpret_cast<floatx4*>(tile)[i] = v;
            if (non_finite(v[0]) || non_finite(v[1]) || non_finite(v[2]) || non_finite(v[3])) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (non_finite(v[c])) atomicOr(&bad[(4 * i + c) / pD], 1);
            }
        }
        for (int i = 4 * nvec + tid; i < len; i += HE_THREADS) {
            const float v = src[i];
            tile[i] = v;
            if (non_finite(v)) atomicOr(&bad[i / pD], 1);
        }
        __syncthreads();
        if (tid < nw && ok[tid]) atomicAdd(&cnt[bad[tid] ? 1 : 0], 1);
        for (int it = tid; it < nw * D; it += HE_THREADS) {
            const int w = it / D, d = it - w * D;
            if (!ok[w] || bad[w]) continue;
            const float* x = tile + w * pD + d;
            const float y = a.truth[(size_t)(w0 + w) * a.truth_ld + (size_t)h * D + d];
            float* ac = acc + w * KD + d;
            // everything relative to particle 0: differences of nearby values are exact, and particles that agree (a deterministic
            // model of identical members) give exactly their value as every mean and exactly 0 as the variance
            const float x0 = x[0];
            float tot = 0.0f;
            for (int e = 0; e < E; ++e) {
                float s = 0.0f;
                for (int j = 0; j < PE; ++j) s += x[(e * PE + j) * D] - x0;
                tot += s;
                const float dm = (x0 + s / (float)PE) - y;
                ac[(2 + e) * D] += dm * dm;
            }
            const float md = tot / (float)p;
            float var = 0.0f;
            for (int j = 0; j < p; ++j) {
                const float dv = (x[j * D] - x0) - md;
                var += dv * dv;
            }
            const float dt = (x0 + md) - y;
            ac[0] += dt * dt;
            ac[D] += var / (float)p;
        }
    }
    __syncthreads();
    float* out = a.partials + ((size_t)(a.block0 + blk) * a.F + h) * a.stride;
    for (int i = tid; i < KD; i += HE_THREADS) {
        float s = 0.0f;
        for (int w = 0; w < WT; ++w) s += acc[w * KD + i];
        out[i] = s;
    }
    if (tid < 2) reinterpret_cast<int*>(out)[KD + tid] = cnt[tid];
}

// stage 2: one thread per output entry, blocks added in index order
__global__ __launch_bounds__(HE_THREADS) void horizon_finalize_kernel(const float* __restrict__ partials, long long nblocks, int F, int E, int D,
                                                                      float* se, float* spread, float* se_member, int32_t* count,
                                                                      int32_t* diverged) {
    const int KD = (2 + E) * D, stride = KD + 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= F * stride) return;
    const int h = idx / stride, i = idx - h * stride;
    const float* src = partials + (size_t)h * stride + i;
    const size_t step = (size_t)F * stride;
    if (i < KD) {
        float s = 0.0f;
        for (long long b = 0; b < nblocks; ++b) s += src[b * step];
        const int k = i / D, d = i - k * D;
        if (k == 0) se[h * D + d] = s;
        else if (k == 1) spread[h * D + d] = s;
        else se_member[((size_t)(k - 2) * F + h) * D + d] = s;
    } else {
        int s = 0;
        for (long long b = 0; b < nblocks; ++b) s += reinterpret_cast<const int*>(src)[b * step];
        (i == KD ? count : diverged)[h] = s;
    }
}

// windows per LDS tile: the largest power of two <= HE_MAX_WT whose tile + accumulators fit the budget (0: not even one window)
int tile_windows(int p, int E, int D) {
    const long long per_window = (long long)D * (p + 2 + E) * 4 + 16;
    int wt = HE_MAX_WT;
    while (wt >= 1 && wt * per_window + 32 > HE_LDS_BUDGET) wt >>= 1;
    return wt;
}

}  // namespace

extern "C" int cadm_horizon_error(const float* traj, const float* truth, long long truth_row_stride, const float* mask, int m, int F, int p,
                                  int E, int D, long long window0, float* partials, long long partials_blocks, float* se_out,
                                  float* spread_out, float* se_member_out, int32_t* count_out, int32_t* diverged_out, int finalize,
                                  void* stream) {
    CADM_REQUIRE(traj, "cadm_horizon_error: traj is null");
    CADM_REQUIRE(truth && mask && partials, "cadm_horizon_error: truth / mask / partials is null");
    CADM_REQUIRE(F >= 1 && m >= 1 && p >= 1 && D >= 1, "cadm_horizon_error: F, m, p, D must be >= 1 (got F=%d m=%d p=%d D=%d)", F, m, p, D);
    CADM_REQUIRE(E >= 1 && p % E == 0, "cadm_horizon_error: p (%d) must be a multiple of E (%d)", p, E);
    CADM_REQUIRE(window0 >= 0 && window0 % HE_BLOCK == 0, "cadm_horizon_error: window0 (%lld) must be a non-negative multiple of %d", window0,
                 HE_BLOCK);
    CADM_REQUIRE(D <= 64, "cadm_horizon_error: D (%d) must be <= 64", D);
    CADM_REQUIRE(F <= 65535, "cadm_horizon_error: F (%d) must be <= 65535", F);
    CADM_REQUIRE(truth_row_stride >= (long long)F * D, "cadm_horizon_error: truth_row_stride (%lld) is below F * D = %d", truth_row_stride, F * D);
    const int wt = tile_windows(p, E, D);
    CADM_REQUIRE(wt >= 1, "cadm_horizon_error: p (%d) x D (%d) does not fit an LDS tile (D * (p + E + 2) * 4 <= %d bytes)", p, D, HE_LDS_BUDGET - 48);
    const long long nblk = ((long long)m + HE_BLOCK - 1) / HE_BLOCK, block0 = window0 / HE_BLOCK;
    CADM_REQUIRE(block0 + nblk <= partials_blocks, "cadm_horizon_error: partials_blocks (%lld) is below the %lld blocks of windows [0, %lld)",
                 partials_blocks, block0 + nblk, window0 + m);
    CADM_REQUIRE(!finalize || (se_out && spread_out && se_member_out && count_out && diverged_out),
                 "cadm_horizon_error: finalize needs se_out, spread_out, se_member_out, count_out and diverged_out");
    hipStream_t s = (hipStream_t)stream;
    HorizonArgs a{};
    a.traj = traj; a.truth = truth; a.mask = mask; a.truth_ld = truth_row_stride;
    a.m = m; a.F = F; a.p = p; a.E = E; a.D = D; a.PE = p / E; a.WT = wt;
    a.block0 = block0; a.partials = partials; a.stride = (2 + E) * D + 2;
    const size_t lds = ((size_t)((wt * p * D + 3) & ~3) + (size_t)wt * (2 + E) * D) * sizeof(float) + (2 * (size_t)wt + 2) * sizeof(int);
    hipLaunchKernelGGL(horizon_error_kernel, dim3((unsigned)nblk, (unsigned)F), dim3(HE_THREADS), lds, s, a);
    CADM_CHECK_HIP(hipGetLastError());
    if (finalize) {
        const int total = F * a.stride;
        hipLaunchKernelGGL(horizon_finalize_kernel, dim3((total + HE_THREADS - 1) / HE_THREADS), dim3(HE_THREADS), 0, s, partials, block0 + nblk, F,
                           E, D, se_out, spread_out, se_member_out, count_out, diverged_out);
        CADM_CHECK_HIP(hipGetLastError());
    }
    return CADM_OK;
}

// cadm_eval_horizon and cadm_eval_calibration: encoder, rollout and a statistics kernel (the one above; calibration.hip's), strung
// together chunk by chunk of held-out windows by ONE loop, eval_chunks
// rows of `width` floats, `src_ld` floats apart -> contiguous rows
__global__ void strided_rows_kernel(const float* __restrict__ src, size_t src_ld, float* __restrict__ dst, size_t width, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / width, c = i - r * width;
        dst[i] = src[r * src_ld + c];
    }
}

static int launch_strided_rows(const float* src, size_t src_ld, float* dst, size_t width, size_t rows, hipStream_t s) {
    const size_t total = width * rows, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(strided_rows_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, src, src_ld, dst, width, total);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

struct EvalWs {
    float *obs0, *ctxv, *rows, *traj, *eps, *partials;
    long long blocks;
};

// windows per launch: the caller's chunk, no larger than the dataset rounded up to whole blocks of 64
static int eval_chunk(int N, int chunk) {
    const long long n64 = ((long long)N + 63) / 64 * 64;
    return (int)(chunk < n64 ? chunk : n64);
}

// partial_words: 4-byte words of one (block, step) partial of the statistics kernel that reduces the trajectories
static size_t eval_carve(cadm_ctx* ctx, int N, int F, int chunk, size_t partial_words, char* base, EvalWs* w) {
    Carver c{base};
    const size_t mc = (size_t)eval_chunk(N, chunk), blocks = ((size_t)N + 63) / 64;
    EvalWs t;
    t.obs0 = c.take<float>(mc * ctx->D);
    t.ctxv = c.take<float>((size_t)ctx->E * mc * (ctx->C > 0 ? ctx->C : 1));
    t.rows = c.take<float>(mc * ctx->p);
    t.traj = c.take<float>((size_t)F * mc * ctx->p * ctx->D);
    t.eps = c.take<float>((size_t)F * mc * ctx->p * ctx->D);      // a chunk of injected noise, made contiguous
    t.partials = c.take<float>(blocks * F * partial_words);
    t.blocks = (long long)blocks;
    if (w) *w = t;
    return c.off;
}

static size_t horizon_partial_words(const cadm_ctx* ctx) { return (size_t)(2 + ctx->E) * ctx->D + 2; }
static size_t calibration_partial_words(const cadm_ctx* ctx) { return 3 * (size_t)ctx->D; }

extern "C" size_t cadm_eval_workspace_bytes(cadm_ctx* ctx, int N, int F, int chunk) {
    if (!ctx || N <= 0 || F <= 0 || chunk <= 0 || chunk % 64) return 0;
    return eval_carve(ctx, N, F, chunk, horizon_partial_words(ctx), nullptr, nullptr);
}

extern "C" size_t cadm_eval_calibration_workspace_bytes(cadm_ctx* ctx, int N, int F, int chunk) {
    if (!ctx || N <= 0 || F <= 0 || chunk <= 0 || chunk % 64) return 0;
    return eval_carve(ctx, N, F, chunk, calibration_partial_words(ctx), nullptr, nullptr);
}

// The chunk loop of cadm_eval_horizon and cadm_eval_calibration (`who`): per chunk of windows the start states, the context encoder and
// ONE rollout of F steps, then stats(w, w0, mc, last) on the chunk's trajectories w.traj [F, mc, 1, p, D] -- windows [w0, w0 + mc) of the
// dataset; `last`: no chunk follows.  The callers have checked their own pointers.
template <class Stats>
static int eval_chunks(cadm_ctx* ctx, const char* who, const float* ds_obs, const float* ds_act, const float* ds_cp_obs, const float* ds_cp_act,
                       int N, int F, int chunk, uint32_t seed, uint32_t call, const float* eps, void* workspace, size_t partial_words,
                       hipStream_t s, Stats stats) {
    CADM_REQUIRE(N >= 1 && F >= 1, "%s: N (%d) and F (%d) must be >= 1", who, N, F);
    CADM_REQUIRE(chunk >= 64 && chunk % 64 == 0, "%s: chunk (%d) must be a positive multiple of 64", who, chunk);
    CADM_REQUIRE(F <= ctx->H, "%s: F (%d) exceeds the model's planning horizon n_forwards (%d)", who, F, ctx->H);
    CADM_REQUIRE(ctx->C == 0 || (ds_cp_obs && ds_cp_act), "%s: ds_cp_obs / ds_cp_act required for a context model", who);
    CADM_ON_DEVICE(ctx);
    int rc = cadm_require_ready(ctx, who);
    if (rc) return rc;
    if (!ctx->packed && (rc = cadm_pack_streams(ctx, s))) return rc;
    EvalWs w;
    eval_carve(ctx, N, F, chunk, partial_words, (char*)workspace, &w);
    const int D = ctx->D, A = ctx->A, p = ctx->p, Hh = ctx->cfg.history_length, mc_max = eval_chunk(N, chunk);
    const bool inject = eps && !ctx->cfg.deterministic;
    CADM_REQUIRE(((long long)N + mc_max - 1) / mc_max < (1 << 23), "%s: N (%d) needs too many chunks of %d windows", who, N, mc_max);
    for (int w0 = 0; w0 < N; w0 += mc_max) {
        const int mc = N - w0 < mc_max ? N - w0 : mc_max;
        // start state of every window: ds_obs[w, 0, :]
        if ((rc = launch_strided_rows(ds_obs + (size_t)w0 * F * D, (size_t)F * D, w.obs0, D, mc, s))) return rc;
        if (ctx->C > 0 && (rc = cadm_launch_context(ctx, ds_cp_obs + (size_t)w0 * D * Hh, ds_cp_act + (size_t)w0 * A * Hh, mc, 0, w.ctxv, s,
                                                    /*force_batched=*/1))) return rc;
        // eps [F, N, 1, p, D] -> this chunk's [F, mc, 1, p, D]
        if (inject && (rc = launch_strided_rows(eps + (size_t)w0 * p * D, (size_t)N * p * D, w.eps, (size_t)mc * p * D, F, s))) return rc;
        // one rollout of F steps: every window is an env with ONE candidate, its recorded actions ([N, F * A] is [m, 1, F, A]).  The
        // iteration word is 2 * (chunk index): even, so the context layout is iteration 0's, and device-drawn noise (keyed by the row
        // INSIDE the launch and the iteration word) is not repeated from chunk to chunk
        if ((rc = cadm_launch_rollout(ctx, w.obs0, nullptr, ctx->C > 0 ? w.ctxv : nullptr, ds_act + (size_t)w0 * F * A, inject ? w.eps : nullptr,
                                      /*norm_actions=*/1, seed, call, /*it=*/2 * (w0 / mc_max), 0, 1, mc, 1, w.rows, w.traj, s, 0, -1, /*horizon=*/F))) return rc;
        if ((rc = stats(w, w0, mc, w0 + mc >= N))) return rc;
    }
    return CADM_OK;
}

extern "C" int cadm_eval_horizon(cadm_ctx* ctx, const float* ds_obs, const float* ds_act, const float* ds_obs_next, const float* ds_cp_obs,
                                 const float* ds_cp_act, const float* future_bool, int N, int F, int chunk, uint32_t seed, uint32_t call,
                                 const float* eps, void* workspace, float* se_out, float* spread_out, float* se_member_out,
                                 int32_t* count_out, int32_t* diverged_out, void* stream) {
    CADM_REQUIRE(ctx && ds_obs && ds_act && ds_obs_next && future_bool && workspace && se_out && spread_out && se_member_out && count_out &&
                     diverged_out, "cadm_eval_horizon: null argument");
    return eval_chunks(ctx, "cadm_eval_horizon", ds_obs, ds_act, ds_cp_obs, ds_cp_act, N, F, chunk, seed, call, eps, workspace,
                       horizon_partial_words(ctx), (hipStream_t)stream, [&](const EvalWs& w, int w0, int mc, bool last) {
                           return cadm_horizon_error(w.traj, ds_obs_next + (size_t)w0 * F * ctx->D, (long long)F * ctx->D,
                                                     future_bool + (size_t)w0 * F, mc, F, ctx->p, ctx->E, ctx->D, w0, w.partials, w.blocks, se_out,
                                                     spread_out, se_member_out, count_out, diverged_out, last ? 1 : 0, stream);
                       });
}

// (the statistics kernel: calibration.hip)
extern "C" int cadm_eval_calibration(cadm_ctx* ctx, const float* ds_obs, const float* ds_act, const float* ds_obs_next, const float* ds_cp_obs,
                                     const float* ds_cp_act, const float* future_bool, int N, int F, int chunk, uint32_t seed, uint32_t call,
                                     const float* eps, void* workspace, const cadm_calibration_out* out, void* stream) {
    CADM_REQUIRE(ctx && ds_obs && ds_act && ds_obs_next && future_bool && workspace && out, "cadm_eval_calibration: null argument");
    CADM_REQUIRE(out->rank_hist && out->rank_hist_member && out->ties && out->degenerate && out->crps && out->z2 && out->nll && out->count &&
                     out->diverged, "cadm_eval_calibration: a pointer of out is null");
    return eval_chunks(ctx, "cadm_eval_calibration", ds_obs, ds_act, ds_cp_obs, ds_cp_act, N, F, chunk, seed, call, eps, workspace,
                       calibration_partial_words(ctx), (hipStream_t)stream, [&](const EvalWs& w, int w0, int mc, bool last) {
                           return cadm_calibration_stats(w.traj, ds_obs_next + (size_t)w0 * F * ctx->D, (long long)F * ctx->D,
                                                         future_bool + (size_t)w0 * F, mc, F, ctx->p, ctx->E, ctx->D, w0, w.partials, w.blocks, out,
                                                         last ? 1 : 0, stream);
                       });
}
