// Value-expansion targets for a learner (no reference twin): what a critic is trained on, out of the transitions cadm_imagine returned
// and the caller's bootstrap values of their states -- lambda-returns on every imagined state (Dreamer, TD-MPC), the n-step targets of the
// start state (MVE) and their inverse-variance combination over the branches (STEVE), with the reward reduced by a multiple of the
// disagreement and the rollout cut where it passes a bound (MOPO, M2AC).  ONE launch; the arithmetic is restated in include/cadm_hip.h
// ("Value-expansion targets") and, operation for operation, in tests/targets_ref.py.
//
// A "row" is one trajectory (start state i, branch j), q = i * n + j; element t of a [k,m,n] array of the row is t * m * n + q.  Per row,
// float32, every operation rounded on its own (no fmaf; the build has -ffp-contract=off), divisions __fdiv_rn:
//   L       the number of leading steps with valid[t] && !(disagreement[t] > max_disagreement);  used[t] = t < L
//   term    L >= 1 && done[L - 1]
//   r~_t    rew[t] with penalty == 0 (no multiply), else rew[t] - penalty * disagreement[t]
//   lambda  t = L - 1 .. 0:  G = t == L - 1 ? (term ? r~_t : r~_t + gamma * boot[t + 1])
//                                           : r~_t + gamma * (one_minus_lambda * boot[t + 1] + lambda * G);  lambda_return[t] = G, 0 behind L
//   n-step  acc = 0, disc = 1;  h = 1 .. L:  acc = acc + disc * r~_{h-1};  disc = disc * gamma;
//           x_h = (h == L && term) ? acc : acc + disc * boot[h];  h > L: x_h = x_L with term, no target without;
//           nstep[h - 1] = x_h, nstep_ok[h - 1] = 1 where a target exists and is finite, else both 0
// and per start state and h, with want_steve:
//   c = the branches with nstep_ok;  mean = c > 0 ? (sum x) / c : 0;  var = c > 0 ? (sum (x - mean)^2) / c : 0, each sum from 0.0f in
//   ascending j over those branches;  w_h = c >= 2 ? 1 / (var + var_floor) : 0;  W = sum_h w_h, S = sum_h w_h * mean_h from 0.0f in ascending
//   h;  steve = W > 0 ? S / W : boot[0,i,0];  steve_weight[h] = W > 0 ? w_h / W : 0;  steve_fallback = !(W > 0)
// Mapping: a workgroup of 256 threads owns G consecutive start states, G n consecutive rows (without want_steve: 256 consecutive rows and
// no LDS).  One thread per row runs the scan -- lanes read consecutive addresses of every [k,m,n] array -- and, with want_steve, leaves
// the row's targets in an LDS tile [k, G n] floats + [k, G n] flags; behind a barrier one thread per (h, start state) reduces its n
// branches out of the tile; behind another one thread per start state forms the weights.  The host takes the largest G <= 256 / n (at
// least 1) whose tile fits a 48 KiB budget; where one start state's n k targets do not fit, want_steve is refused.
// Reduction contract (imagine.hip's): every output is ONE thread's chain in the order above; no floating-point atomics, no cross-lane
// reduction; nothing depends on G, on the grid, on m or on the position of a row or a start state: the same bits run to run.
#include <math.h>

#include "planner.h"

namespace {

constexpr int TGT_THREADS = 256;
constexpr int TGT_LDS_BUDGET = 48 * 1024;     // the tile of G n k floats and flags and 2 G k floats; below the 64 KiB a kernel gets without an attribute

struct TargetArgs {
    const float *rew, *disag, *boot;          // [k,m,n], [k,m,n], [k+1,m,n]
    const uint8_t *valid, *done;              // [k,m,n]
    float *lam, *nstep;                       // [k,m,n]
    uint8_t *ok, *used;                       // [k,m,n]
    float *steve, *sweight, *smean, *svar;    // [m], [k,m], [k,m], [k,m]   (null without want_steve, as the two below)
    int32_t* scount;                          // [k,m]
    uint8_t* sfall;                           // [m]
    size_t rows;                              // m * n
    int m, n, k, G;                           // G == 0: no STEVE outputs, a workgroup owns TGT_THREADS rows
    float gamma, lambda, one_minus_lambda, penalty, max_disag, var_floor;
};

__device__ __host__ __forceinline__ size_t tgt_pad4(size_t v) { return (v + 3) & ~(size_t)3; }
__device__ __forceinline__ bool tgt_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(TGT_THREADS) void imagine_targets_kernel(const TargetArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tgt_smem[];
    const int k = a.k, n = a.n, G = a.G, tid = threadIdx.x;
    const size_t rows = a.rows;
    const bool steve = G > 0;
    const size_t i0 = (size_t)blockIdx.x * G;                       // first start state of this workgroup (i0 < m: the grid is ceil(m / G))
    const int ng = steve ? ((size_t)a.m - i0 < (size_t)G ? (int)(a.m - i0) : G) : 0;
    const size_t r0 = steve ? i0 * n : (size_t)blockIdx.x * TGT_THREADS;      // first row (r0 < rows)
    const int nr = steve ? ng * n : (rows - r0 < (size_t)TGT_THREADS ? (int)(rows - r0) : TGT_THREADS);
    const int cap = G * n;                                          // rows of a full group: the tile's stride
    float* xs = tgt_smem;                                           // [k, cap] the rows' n-step targets
    uint8_t* oks = reinterpret_cast<uint8_t*>(xs + tgt_pad4((size_t)k * cap));      // [k, cap] their flags
    float* sm = reinterpret_cast<float*>(oks + tgt_pad4((size_t)k * cap));          // [k, G] the means
    float* sw = sm + (size_t)k * G;                                 // [k, G] the weights
    const float gamma = a.gamma, lambda = a.lambda, oml = a.one_minus_lambda, beta = a.penalty;
    for (int r = tid; r < nr; r += TGT_THREADS) {                   // (more than one pass only where one start state has n > 256 branches)
        const size_t q = r0 + r;
        int L = 0;
        while (L < k && a.valid[(size_t)L * rows + q] != 0 && !(a.disag[(size_t)L * rows + q] > a.max_disag)) ++L;
        const bool term = L >= 1 && a.done[(size_t)(L - 1) * rows + q] != 0;
        float acc = 0.0f, disc = 1.0f, x = 0.0f;
        for (int h = 1; h <= k; ++h) {
            const size_t e = (size_t)(h - 1) * rows + q;
            if (h <= L) {
                float rt = a.rew[e];
                if (beta != 0.0f) rt = rt - beta * a.disag[e];
                acc = acc + disc * rt;
                disc = disc * gamma;
                x = (h == L && term) ? acc : acc + disc * a.boot[e + rows];
            }
            const bool good = (h <= L || term) && !tgt_nonfinite(x);      // (behind L a terminated row keeps x_L)
            a.nstep[e] = good ? x : 0.0f;
            a.ok[e] = good ? 1 : 0;
            a.used[e] = h <= L ? 1 : 0;
            if (steve) {
                xs[(h - 1) * cap + r] = good ? x : 0.0f;
                oks[(h - 1) * cap + r] = good ? 1 : 0;
            }
        }
        float g = 0.0f;
        for (int t = k - 1; t >= 0; --t) {
            const size_t e = (size_t)t * rows + q;
            if (t >= L) { a.lam[e] = 0.0f; continue; }
            float rt = a.rew[e];
            if (beta != 0.0f) rt = rt - beta * a.disag[e];
            if (t == L - 1) g = term ? rt : rt + gamma * a.boot[e + rows];
            else g = rt + gamma * (oml * a.boot[e + rows] + lambda * g);
            a.lam[e] = g;
        }
    }
    if (!steve) return;                                             // (uniform)
    __syncthreads();
    // one thread per (h, start state): count, mean and variance over the branches in ascending j, two passes
    for (int idx = tid; idx < k * ng; idx += TGT_THREADS) {
        const int h = idx / ng, gi = idx - h * ng;
        const float* x = xs + h * cap + gi * n;
        const uint8_t* o = oks + h * cap + gi * n;
        int c = 0;
        float s = 0.0f;
        for (int j = 0; j < n; ++j)
            if (o[j]) { ++c; s = s + x[j]; }
        const float mean = c > 0 ? __fdiv_rn(s, (float)c) : 0.0f;
        float ss = 0.0f;
        for (int j = 0; j < n; ++j)
            if (o[j]) { const float d = x[j] - mean; ss = ss + d * d; }
        const float var = c > 0 ? __fdiv_rn(ss, (float)c) : 0.0f;
        const size_t e = (size_t)h * a.m + i0 + gi;
        a.smean[e] = mean;
        a.svar[e] = var;
        a.scount[e] = c;
        sm[h * G + gi] = mean;
        sw[h * G + gi] = c >= 2 ? __fdiv_rn(1.0f, var + a.var_floor) : 0.0f;
    }
    __syncthreads();
    // one thread per start state: the weights over the horizons in ascending h
    for (int gi = tid; gi < ng; gi += TGT_THREADS) {
        float W = 0.0f, S = 0.0f;
        for (int h = 0; h < k; ++h) {
            const float w = sw[h * G + gi];
            W = W + w;
            S = S + w * sm[h * G + gi];
        }
        const bool any = W > 0.0f;
        const size_t i = i0 + gi;
        a.steve[i] = any ? __fdiv_rn(S, W) : a.boot[i * n];
        a.sfall[i] = any ? 0 : 1;
        for (int h = 0; h < k; ++h) a.sweight[(size_t)h * a.m + i] = any ? __fdiv_rn(sw[h * G + gi], W) : 0.0f;
    }
}

size_t tgt_lds_bytes(int G, int n, int k) {
    const size_t tile = tgt_pad4((size_t)G * n * k);
    return tile * sizeof(float) + tile + 2 * (size_t)G * k * sizeof(float);
}

// the start states a workgroup owns: as many as give it TGT_THREADS rows, at least one, fewer where the tile would not fit (0: not even one's)
int tgt_group(int m, int n, int k) {
    int G = TGT_THREADS / n;
    G = G < 1 ? 1 : G;
    G = G > m ? m : G;
    while (G > 0 && tgt_lds_bytes(G, n, k) > (size_t)TGT_LDS_BUDGET) --G;
    return G;
}

struct TargetWs {
    float *lam, *nstep;
    uint8_t *ok, *used;
    float *steve, *sweight, *smean, *svar;
    int32_t* scount;
    uint8_t* sfall;
    size_t off[CADM_TARGET_VIEWS];
};

// the outputs in the order of include/cadm_hip.h: ONE layout for the size, the offsets and the launch
size_t targets_carve(int m, int n, int k, int want_steve, char* base, TargetWs* w) {
    Carver c{base};
    TargetWs t{};
    const size_t rows = (size_t)m * n;
    size_t* o = t.off;
    *o++ = c.off; t.lam = c.take<float>((size_t)k * rows);
    *o++ = c.off; t.nstep = c.take<float>((size_t)k * rows);
    *o++ = c.off; t.ok = c.take<uint8_t>((size_t)k * rows);
    *o++ = c.off; t.used = c.take<uint8_t>((size_t)k * rows);
    if (want_steve) {
        *o++ = c.off; t.steve = c.take<float>((size_t)m);
        *o++ = c.off; t.sweight = c.take<float>((size_t)k * m);
        *o++ = c.off; t.smean = c.take<float>((size_t)k * m);
        *o++ = c.off; t.svar = c.take<float>((size_t)k * m);
        *o++ = c.off; t.scount = c.take<int32_t>((size_t)k * m);
        *o++ = c.off; t.sfall = c.take<uint8_t>((size_t)m);
    }
    if (w) *w = t;
    return c.off;
}

// the refusals of the shape: what both entry points share
int targets_shape_check(int m, int n, int k, int want_steve, const char* who) {
    CADM_REQUIRE(m >= 1 && n >= 1 && k >= 1, "%s: m, branches and horizon must be >= 1 (got m=%d branches=%d horizon=%d)", who, m, n, k);
    CADM_REQUIRE((unsigned long long)m * n <= 0x7fffffffull, "%s: m * branches = %llu rows are too many for one launch", who,
                 (unsigned long long)m * n);
    if (!want_steve) return CADM_OK;
    CADM_REQUIRE(n >= 2, "%s: the STEVE outputs need branches >= 2 (the variance is taken over the branches), got %d", who, n);
    CADM_REQUIRE(tgt_group(m, n, k) >= 1,
                 "%s: branches (%d) x horizon (%d) does not fit the STEVE reduction's LDS: one start state's tile of n * k targets and "
                 "flags and 2 k floats needs %zu bytes, the bound is %d; the scan without the STEVE outputs has no such limit", who, n, k,
                 tgt_lds_bytes(1, n, k), TGT_LDS_BUDGET);
    return CADM_OK;
}

}  // namespace

extern "C" size_t cadm_imagine_targets_workspace_bytes(cadm_ctx* ctx, int m, int n, int k, int want_steve, uint64_t* offsets_out) {
    if (!ctx || targets_shape_check(m, n, k, want_steve, "cadm_imagine_targets_workspace_bytes")) return 0;
    TargetWs w;
    const size_t bytes = targets_carve(m, n, k, want_steve, nullptr, &w);
    if (offsets_out)
        for (int i = 0; i < CADM_TARGET_VIEWS; ++i) offsets_out[i] = (uint64_t)w.off[i];
    return bytes;
}

extern "C" int cadm_imagine_targets(cadm_ctx* ctx, const float* rew, const uint8_t* valid, const uint8_t* done, const float* disagreement,
                                    const float* boot, int m, int n, int k, const cadm_target_params* prm, void* buffer, void* stream) {
    const char* who = "cadm_imagine_targets";
    CADM_REQUIRE(ctx && rew && valid && done && disagreement && boot && prm && buffer,
                 "%s: ctx / rew / valid / done / disagreement / boot / params / buffer is null", who);
    const int want_steve = prm->want_steve != 0;
    CADM_REQUIRE(prm->gamma > 0.0f && prm->gamma <= 1.0f, "%s: gamma %g is outside (0, 1]", who, (double)prm->gamma);
    CADM_REQUIRE(prm->lambda >= 0.0f && prm->lambda <= 1.0f, "%s: lambda %g is outside [0, 1]", who, (double)prm->lambda);
    CADM_REQUIRE(isfinite(prm->penalty) && prm->penalty >= 0.0f, "%s: penalty %g is negative or not finite", who, (double)prm->penalty);
    CADM_REQUIRE(prm->max_disagreement > 0.0f, "%s: max_disagreement %g is not > 0 (+inf: no bound)", who, (double)prm->max_disagreement);
    CADM_REQUIRE(!want_steve || (isfinite(prm->var_floor) && prm->var_floor > 0.0f), "%s: var_floor %g is not a finite number > 0", who,
                 (double)prm->var_floor);
    int rc;
    if ((rc = targets_shape_check(m, n, k, want_steve, who))) return rc;
    TargetWs w;
    targets_carve(m, n, k, want_steve, (char*)buffer, &w);
    TargetArgs a{};
    a.rew = rew; a.disag = disagreement; a.boot = boot; a.valid = valid; a.done = done;
    a.lam = w.lam; a.nstep = w.nstep; a.ok = w.ok; a.used = w.used;
    a.steve = w.steve; a.sweight = w.sweight; a.smean = w.smean; a.svar = w.svar; a.scount = w.scount; a.sfall = w.sfall;
    a.rows = (size_t)m * n; a.m = m; a.n = n; a.k = k; a.G = want_steve ? tgt_group(m, n, k) : 0;
    a.gamma = prm->gamma; a.lambda = prm->lambda; a.one_minus_lambda = 1.0f - prm->lambda; a.penalty = prm->penalty;
    a.max_disag = prm->max_disagreement; a.var_floor = prm->var_floor;
    const size_t blocks = want_steve ? ((size_t)m + a.G - 1) / a.G : (a.rows + TGT_THREADS - 1) / TGT_THREADS;
    CADM_ON_DEVICE(ctx);
    hipLaunchKernelGGL(imagine_targets_kernel, dim3((unsigned)blocks), dim3(TGT_THREADS), want_steve ? tgt_lds_bytes(a.G, n, k) : 0,
                       (hipStream_t)stream, a);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}
