// Imagined rollouts for a learner (no reference twin): short model rollouts branched from caller-supplied start states under the registered
// actor or the caller's open-loop actions, handed back as transitions (s, a, r, s', done) with the member that made each one and the
// ensemble's disagreement about it (MBPO / Dyna; MOPO / M2AC read the disagreement).  Two pieces: imagine_select_kernel, which stands
// BETWEEN two one-step rollouts -- it picks one particle per row, records the transition and re-seeds the row -- and cadm_launch_imagine,
// the serial chain  action -> one-step rollout -> select  over the k steps.  The rollout kernels are not touched: the chain calls
// cadm_launch_rollout with horizon 1 and per-row start states, as the proposal roll does (policy.hip).  The arithmetic is restated in
// include/cadm_hip.h ("Imagined rollouts").
//
// A "row" is one trajectory (start state mi, branch j), row = mi * n + j; its p particles cover every member p / E times (particle i
// belongs to member i / (p / E)), so one one-step rollout is every member's prediction and keeping one particle is MBPO's scheme.  Per row
// and step t, in this order:
//   sel = (uint64(w0) * p) >> 32, w0 = word 0 of Philox4x32-10 keyed (seed, call), counter (row, t, 0, CADM_STREAM_IMAGINE)
//         (cadm_imagine_select with sel_in: that value, clamped to 0 .. p - 1);   member = sel / (p / E)
//   s'  = next[row, sel, :];   r = rows1[row, sel]: the rollout's own one-step return of that particle
//   v_d = the epistemic variance over the row's p particles, uncertainty.hip's chain operation for operation (relative to particle 0,
//         members in member order; dims with w_d == 0 are not read);  u = w_d v_d added in ascending d from the first term; a non-finite u
//         is stored as +inf
//   finite  = no value of s' is NaN or +-inf;   healthy = s'[dim] > lo && s'[dim] < hi for every constraint (constrain.hip's test: a value
//         on a bound violates)
//   alive, finite, healthy:      valid 1, done 0, states[t+1] = s'
//   alive, finite, not healthy:  valid 1, done 1, states[t+1] = s', the row is dead afterwards
//   alive, not finite:           valid 0, done 0, rew 0, states[t+1] = states[t], the row is dead afterwards (member and u are kept: which
//                                member diverged)
//   dead:                        valid 0, done 0, rew 0, member -1, u 0, states[t+1] = states[t]
//   length += valid;  states[t+1] goes into all p slots of the row in the next rollout's start-state buffer, so a dead row is frozen at
//   a finite state and nothing non-finite is ever fed back.
// Mapping (uncertainty.hip's): a workgroup of 256 threads owns G consecutive rows, G chosen by the host from a 48 KiB LDS budget.  The
// group's G p D floats of `next` are ONE contiguous span, loaded lane-linear into an LDS tile (16-byte loads where the span is 16-byte
// aligned, scalar loads otherwise: odd p D at odd rows); every value of `next` is read from memory once.  Behind a barrier one thread per
// (row, dim) runs the variance chain out of LDS; behind another one thread per row sums, tests and writes the scalars (its draw and its
// reads of rows1 and alive were issued ahead of the tile); behind a third all threads write states[t + 1] and the p-fold broadcast out of
// the tile, coalesced.
// Reduction contract: every output is ONE thread's chain in the order above; no floating-point atomics; nothing depends on G, on the
// grid, on m or n: the same bits run to run, and at any row position for the same sel.
#include <math.h>

#include "planner.h"

namespace {

constexpr int IMG_THREADS = 256;
constexpr int IMG_GROUP = 16;                 // rows per workgroup at most (fewer where the tile would not fit)
constexpr int IMG_LDS_BUDGET = 48 * 1024;     // the tile of G * p * D floats, G * D variances, D weights, G ints; below the 64 KiB a kernel gets without an attribute

struct ImagineArgs {
    const float* next;         // [rows, p, D] the one-step rollout's post-step states
    const float* rows1;        // [rows, p] its one-step returns
    const float* state;        // [rows, D] states[t]
    const int32_t* sel_in;     // [rows] or null: drawn
    uint8_t* alive;            // [rows] in / out
    float* state_out;          // [rows, D] states[t + 1]
    float* rew;                // [rows]
    uint8_t *done, *valid;     // [rows]
    int32_t* member;           // [rows]
    float* disag;              // [rows]
    int32_t* length;           // [rows] in / out, or null
    float* bcast;              // [rows, p, D] or null (behind the last step nothing is rolled)
    size_t rows;
    int p, E, PE, D, G, t;
    uint32_t seed, call;
    cadm_constraint_params c;  // c.n == 0: no constraints (mode and weight are not read)
    float w[CADM_MAX_UNC_DIMS];      // [D], broadcast already
};

__device__ __forceinline__ int img_pad4(int v) { return (v + 3) & ~3; }
__device__ __forceinline__ bool img_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(IMG_THREADS) void imagine_select_kernel(const ImagineArgs a) {
    extern __shared__ __attribute__((aligned(16))) float img_smem[];
    const int D = a.D, p = a.p, E = a.E, PE = a.PE, pD = p * D, tid = threadIdx.x;
    float* tile = img_smem;                              // [ng, p, D] the rows' particles
    float* sv = tile + img_pad4(a.G * pD);               // [ng, D] the variances
    float* sw = sv + img_pad4(a.G * D);                  // [D] the weights, copied out of the kernel arguments once
    int* ssel = reinterpret_cast<int*>(sw + img_pad4(D));      // [ng] the particle states[t + 1] is taken from, -1: the row keeps states[t]
    const size_t c0 = (size_t)blockIdx.x * a.G;          // first row of this workgroup (c0 < rows: the grid is ceil(rows / G))
    const int ng = a.rows - c0 < (size_t)a.G ? (int)(a.rows - c0) : a.G;
    const int span = ng * pD;
    for (int d = tid; d < D; d += IMG_THREADS) sw[d] = a.w[d];
    // the row's draw and what it reads of the small arrays, issued ahead of the tile so that their latency hides behind its loads
    int sel = 0;
    bool was = false;
    float r1 = 0.0f;
    if (tid < ng) {                                      // (G <= IMG_GROUP <= IMG_THREADS)
        const size_t q = c0 + tid;
        if (a.sel_in) {
            sel = a.sel_in[q];
            sel = sel < 0 ? 0 : sel >= p ? p - 1 : sel;
        } else {
            uint32_t r[4];
            philox4x32_10((uint32_t)q, (uint32_t)a.t, 0u, CADM_STREAM_IMAGINE, a.seed, a.call, r);
            sel = (int)__umulhi(r[0], (uint32_t)p);      // (uint64(w0) * p) >> 32: 0 .. p - 1
        }
        was = a.alive[q] != 0;
        r1 = a.rows1[q * p + sel];
    }
    const float* src = a.next + c0 * pD;
    const int nvec = (reinterpret_cast<uintptr_t>(src) & 15) == 0 ? span >> 2 : 0;
    for (int i = tid; i < nvec; i += IMG_THREADS) reinterpret_cast<floatx4*>(tile)[i] = reinterpret_cast<const floatx4*>(src)[i];
    for (int i = 4 * nvec + tid; i < span; i += IMG_THREADS) tile[i] = src[i];
    __syncthreads();
    // the epistemic variance of a (row, dim): uncertainty_steps_kernel's chain, operation for operation
    for (int i = tid; i < ng * D; i += IMG_THREADS) {
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
        float epi = 0.0f;
        for (int e = 0; e < E; ++e) {
            float s = 0.0f;
            for (int j = 0; j < PE; ++j) s += x[(e * PE + j) * D] - x0;
            const float de = s / (float)PE - md;
            epi += de * de;
        }
        sv[i] = epi / (float)E;
    }
    __syncthreads();
    if (tid < ng) {
        const size_t q = c0 + tid;
        const float* x = tile + tid * pD + sel * D;
        bool finite = true;
        for (int d = 0; d < D; ++d) finite = finite && !img_nonfinite(x[d]);
        bool healthy = true;
        for (int k = 0; k < a.c.n; ++k) {
            const float v = x[a.c.dim[k]];
            healthy = healthy && (v > a.c.lo[k] && v < a.c.hi[k]);
        }
        float u = 0.0f;
        bool any = false;
        for (int d = 0; d < D; ++d) {
            const float w = sw[d];
            if (!(w > 0.0f)) continue;
            const float term = w * sv[tid * D + d];
            u = any ? u + term : term;
            any = true;
        }
        if (img_nonfinite(u)) u = INFINITY;
        const bool val = was && finite, dn = val && !healthy;
        a.valid[q] = val ? 1 : 0;
        a.done[q] = dn ? 1 : 0;
        a.rew[q] = val ? r1 : 0.0f;
        a.member[q] = was ? sel / PE : -1;
        a.disag[q] = was ? u : 0.0f;
        a.alive[q] = val && !dn ? 1 : 0;
        if (a.length && val) a.length[q] += 1;
        ssel[tid] = val ? sel : -1;
    }
    __syncthreads();
    // states[t + 1] of a row is its kept particle out of the tile, or states[t]; slot j of the broadcast is that value again, and the
    // thread of slot 0 writes states[t + 1] itself
    if (!a.bcast) {            // (uniform: behind the last step nothing is rolled)
        for (int i = tid; i < ng * D; i += IMG_THREADS) {
            const int c = i / D, d = i - c * D, s = ssel[c];
            a.state_out[c0 * D + i] = s >= 0 ? tile[c * pD + s * D + d] : a.state[(c0 + c) * D + d];
        }
        return;
    }
    // a thread keeps one dim and walks particle slots (row c, slot j), S = 256 / D of them per pass: consecutive threads write
    // consecutive floats, and no index is divided inside the loop (D <= CADM_MAX_UNC_DIMS <= IMG_THREADS / 2, so S >= 2)
    const int S = IMG_THREADS / D, sl = tid / D, d = tid - sl * D;
    if (sl >= S) return;
    const int dc = S / p, dj = S - dc * p;
    int c = sl / p, j = sl - c * p;
    for (int slot = sl; slot < ng * p; slot += S) {
        const int s = ssel[c];
        const float v = s >= 0 ? tile[c * pD + s * D + d] : a.state[(c0 + c) * D + d];
        a.bcast[(c0 * p + slot) * D + d] = v;
        if (j == 0) a.state_out[(c0 + c) * D + d] = v;
        c += dc;
        j += dj;
        if (j >= p) { j -= p; ++c; }
    }
}

// states[0] = the start state of the row's env, alive = 1, length = 0
__global__ void imagine_init_kernel(const float* __restrict__ obs, size_t rows, int n, int D, float* __restrict__ states0,
                                    uint8_t* __restrict__ alive, int32_t* __restrict__ length) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < rows * D; i += (size_t)gridDim.x * blockDim.x) {
        const size_t q = i / D;
        const int d = (int)(i - q * D);
        states0[i] = obs[(q / n) * D + d];
        if (d == 0) { alive[q] = 1; length[q] = 0; }
    }
}

// act[t, row, :] = clip(actions[row, t, :]) for every step at once
__global__ void imagine_actions_kernel(const float* __restrict__ actions, size_t rows, int k, int A, float lb, float ub,
                                       float* __restrict__ act) {
    const size_t total = rows * k * A;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t t = i / (rows * A), r = i - t * rows * A, q = r / A;
        const int d = (int)(r - q * A);
        act[i] = fminf(fmaxf(actions[(q * k + t) * A + d], lb), ub);
    }
}

size_t img_lds_bytes(int G, int p, int D) {
    return ((((size_t)G * p * D + 3) & ~(size_t)3) + (size_t)(((G * D + 3) & ~3) + ((D + 3) & ~3)) + (size_t)G) * sizeof(float);
}

// the largest group whose tile fits (0: not even one row's)
int img_group(int p, int D) {
    int G = IMG_GROUP;
    while (G > 0 && img_lds_bytes(G, p, D) > (size_t)IMG_LDS_BUDGET) --G;
    return G;
}

struct ImagineWs {
    float *states, *act, *rew;
    uint8_t *done, *valid;
    int32_t* member;
    float* disag;
    int32_t* length;
    uint8_t* alive;
    float *rows1, *cur, *next;
    float* logp;               // [k, rows] on the sampled route, else null
    size_t off[CADM_IMAGINE_SAMPLED_VIEWS];
};

// outputs first, in the order of include/cadm_hip.h, then the chain's own views: ONE layout for the size, the offsets and the launches.
// sampled (cadm_imagine_sampled): logp follows cadm_imagine's nine outputs, in front of the chain's views
size_t imagine_carve(const cadm_ctx* ctx, int m, int n, int k, bool sampled, char* base, ImagineWs* w) {
    Carver c{base};
    ImagineWs t{};
    const size_t rows = (size_t)m * n;
    size_t* o = t.off;
    *o++ = c.off; t.states = c.take<float>((size_t)(k + 1) * rows * ctx->D);
    *o++ = c.off; t.act = c.take<float>((size_t)k * rows * ctx->A);
    *o++ = c.off; t.rew = c.take<float>((size_t)k * rows);
    *o++ = c.off; t.done = c.take<uint8_t>((size_t)k * rows);
    *o++ = c.off; t.valid = c.take<uint8_t>((size_t)k * rows);
    *o++ = c.off; t.member = c.take<int32_t>((size_t)k * rows);
    *o++ = c.off; t.disag = c.take<float>((size_t)k * rows);
    *o++ = c.off; t.length = c.take<int32_t>(rows);
    *o++ = c.off; t.alive = c.take<uint8_t>(rows);
    if (sampled) { *o++ = c.off; t.logp = c.take<float>((size_t)k * rows); }
    t.rows1 = c.take<float>(rows * ctx->p);
    t.cur = c.take<float>(rows * ctx->p * ctx->D);
    t.next = c.take<float>(rows * ctx->p * ctx->D);
    if (w) *w = t;
    return c.off;
}

// the refusals of the stage's own inputs; fills the constraint and weight part of the arguments
int imagine_fill(const cadm_ctx* ctx, const cadm_constraint_params* cons, const cadm_uncertainty_params* dis, const char* who, ImagineArgs* a) {
    int rc;
    CADM_REQUIRE(!ctx->cfg.discrete && ctx->cfg.env_kind != CADM_ENV_CARTPOLE, "%s: imagined rollouts need a continuous-action ctx", who);
    CADM_REQUIRE(!cadm_sharded(ctx), "%s: imagined rollouts are not supported on a candidate-sharded ctx", who);
    CADM_REQUIRE(ctx->D <= CADM_MAX_UNC_DIMS, "%s: %d observation dims, the disagreement weights hold %d", who, ctx->D, CADM_MAX_UNC_DIMS);
    CADM_REQUIRE(img_group(ctx->p, ctx->D) >= 1,
                 "%s: p (%d) x D (%d) does not fit the select kernel's LDS: one row's tile of p * D floats, D variances and D weights need "
                 "%zu bytes, the bound is %d", who, ctx->p, ctx->D, img_lds_bytes(1, ctx->p, ctx->D), IMG_LDS_BUDGET);
    if (cons && (rc = cadm_constraint_check(ctx, cons, who))) return rc;
    if (dis && (rc = cadm_uncertainty_check(ctx, dis, who))) return rc;
    if (!a) return CADM_OK;
    a->p = ctx->p; a->E = ctx->E; a->PE = ctx->p / ctx->E; a->D = ctx->D; a->G = img_group(ctx->p, ctx->D);
    if (cons) a->c = *cons;
    for (int d = 0; d < ctx->D; ++d) a->w[d] = !dis ? 1.0f : dis->n_dims == 0 ? dis->w[0] : dis->w[d];
    return CADM_OK;
}

int imagine_select_launch(const ImagineArgs& a, hipStream_t s, const char* who) {
    const size_t blocks = (a.rows + a.G - 1) / a.G;
    CADM_REQUIRE(blocks <= 0x7fffffffull && a.rows <= 0xffffffffull, "%s: %zu rows are too many for one launch", who, a.rows);
    hipLaunchKernelGGL(imagine_select_kernel, dim3((unsigned)blocks), dim3(IMG_THREADS), img_lds_bytes(a.G, a.p, a.D), s, a);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

}  // namespace

int cadm_imagine_check(const cadm_ctx* ctx, int m, int n, int k, const cadm_constraint_params* cons, const cadm_uncertainty_params* dis,
                       const char* who) {
    CADM_REQUIRE(m >= 1 && n >= 1 && k >= 1, "%s: m, branches and horizon must be >= 1 (got m=%d branches=%d horizon=%d)", who, m, n, k);
    int rc;
    if ((rc = imagine_fill(ctx, cons, dis, who, nullptr))) return rc;
    const long long rows_p = (long long)m * n * ctx->p;
    CADM_REQUIRE(rows_p * ctx->A < (1ll << 31) && rows_p * ctx->D < (1ll << 31),
                 "%s: m * branches * p = %lld rows are more than one rollout launch takes (32-bit row indexing)", who, rows_p);
    CADM_REQUIRE(ctx->cfg.num_cem_iters <= CADM_IMAGINE_IT && CADM_IMAGINE_IT + 2 * ((long long)k - 1) < CADM_POLICY_IT,
                 "%s: num_cem_iters (%d) or the horizon (%d) leaves the iteration words %d .. %d of the imagined rollouts (at most %d steps)",
                 who, ctx->cfg.num_cem_iters, k, CADM_IMAGINE_IT, CADM_POLICY_IT - 2, (CADM_POLICY_IT - CADM_IMAGINE_IT) / 2);
    return CADM_OK;
}

// the chain: per step the action (the registered actor on states[t], or the given one), a one-step rollout under the even iteration word
// CADM_IMAGINE_IT + 2 t (the context layout of iteration 0; the head noise is drawn at the rollout's own t = 0, so the word is what
// tells the steps apart), and the select stage.  Nothing is evaluated behind the last step's record.  sampled: the action launch is the
// Gaussian head's step (policy_gauss.hip) in the place of policy.hip's, and logp[t] its second output; every other launch is the same.
int cadm_launch_imagine(cadm_ctx* ctx, const float* obs, const float* ctx_vec, const float* actions, int m, int n, int k, float noise_std,
                        const cadm_constraint_params* cons, const cadm_uncertainty_params* dis, uint32_t seed, uint32_t call, void* buffer,
                        hipStream_t s, const char* who, bool sampled) {
    ImagineWs w;
    imagine_carve(ctx, m, n, k, sampled, (char*)buffer, &w);
    ImagineArgs a{};
    int rc;
    if ((rc = imagine_fill(ctx, cons, dis, who, &a))) return rc;
    const size_t rows = (size_t)m * n;
    const int D = ctx->D, A = ctx->A;
    if (!ctx->packed && (rc = cadm_pack_streams(ctx, s))) return rc;
    const size_t gi = (rows * D + 255) / 256;
    hipLaunchKernelGGL(imagine_init_kernel, dim3((unsigned)(gi > 4096 ? 4096 : gi)), dim3(256), 0, s, obs, rows, n, D, w.states, w.alive, w.length);
    CADM_CHECK_HIP(hipGetLastError());
    if (actions) {
        const size_t ga = (rows * k * A + 255) / 256;
        hipLaunchKernelGGL(imagine_actions_kernel, dim3((unsigned)(ga > 4096 ? 4096 : ga)), dim3(256), 0, s, actions, rows, k, A,
                           ctx->cfg.lower_bound, ctx->cfg.upper_bound, w.act);
        CADM_CHECK_HIP(hipGetLastError());
    }
    a.rows1 = w.rows1; a.next = w.next; a.alive = w.alive; a.length = w.length; a.rows = rows; a.seed = seed; a.call = call;
    for (int t = 0; t < k; ++t) {
        float* act_t = w.act + (size_t)t * rows * A;
        const float* st = w.states + (size_t)t * rows * D;
        if (sampled) rc = cadm_launch_policy_gauss_step(ctx, st, rows, t, seed, call, act_t, w.logp + (size_t)t * rows, s, who);
        else rc = actions ? CADM_OK : cadm_launch_policy_step(ctx, st, rows, t, noise_std, seed, call, CADM_STREAM_IMAGINE_ACT, act_t, s, who);
        if (rc) return rc;
        if ((rc = cadm_launch_rollout(ctx, obs, t ? w.cur : nullptr, ctx_vec, act_t, nullptr, 1, seed, call, CADM_IMAGINE_IT + 2 * t, 0, n, m, n,
                                      w.rows1, w.next, s, 0, -1, /*horizon=*/1))) return rc;
        a.t = t; a.state = st; a.state_out = w.states + (size_t)(t + 1) * rows * D;
        a.rew = w.rew + (size_t)t * rows; a.done = w.done + (size_t)t * rows; a.valid = w.valid + (size_t)t * rows;
        a.member = w.member + (size_t)t * rows; a.disag = w.disag + (size_t)t * rows;
        a.bcast = t + 1 < k ? w.cur : nullptr;      // (the rollout that read w.cur is done in stream order; the kernel reads w.next only)
        if ((rc = imagine_select_launch(a, s, who))) return rc;
    }
    return CADM_OK;
}

extern "C" size_t cadm_imagine_workspace_bytes(cadm_ctx* ctx, int m, int n, int k, uint64_t* offsets_out) {
    if (!ctx || m <= 0 || n <= 0 || k <= 0) return 0;
    ImagineWs w;
    const size_t bytes = imagine_carve(ctx, m, n, k, false, nullptr, &w);
    if (offsets_out)
        for (int i = 0; i < CADM_IMAGINE_VIEWS; ++i) offsets_out[i] = (uint64_t)w.off[i];
    return bytes;
}

extern "C" size_t cadm_imagine_sampled_workspace_bytes(cadm_ctx* ctx, int m, int n, int k, uint64_t* offsets_out) {
    if (!ctx || m <= 0 || n <= 0 || k <= 0) return 0;
    ImagineWs w;
    const size_t bytes = imagine_carve(ctx, m, n, k, true, nullptr, &w);
    if (offsets_out)
        for (int i = 0; i < CADM_IMAGINE_SAMPLED_VIEWS; ++i) offsets_out[i] = (uint64_t)w.off[i];
    return bytes;
}

extern "C" int cadm_imagine_sampled(cadm_ctx* ctx, const float* obs, const float* ctx_vec, int m, int n, int k,
                                    const cadm_constraint_params* constraints, const cadm_uncertainty_params* disagreement, uint32_t seed,
                                    uint32_t call, void* buffer, void* stream) {
    const char* who = "cadm_imagine_sampled";
    CADM_REQUIRE(ctx && obs && buffer, "%s: ctx / obs / buffer is null", who);
    int rc;
    if ((rc = cadm_imagine_check(ctx, m, n, k, constraints, disagreement, who))) return rc;
    CADM_REQUIRE(ctx->C == 0 || ctx_vec, "%s: ctx_vec required for a context model", who);
    if ((rc = cadm_policy_gauss_check(ctx, who))) return rc;
    if ((rc = cadm_require_ready(ctx, who))) return rc;
    CADM_ON_DEVICE(ctx);
    return cadm_launch_imagine(ctx, obs, ctx_vec, nullptr, m, n, k, 0.0f, constraints, disagreement, seed, call, buffer, (hipStream_t)stream, who,
                               true);
}

extern "C" int cadm_imagine(cadm_ctx* ctx, const float* obs, const float* ctx_vec, const float* actions, int m, int n, int k, float noise_std,
                            const cadm_constraint_params* constraints, const cadm_uncertainty_params* disagreement, uint32_t seed,
                            uint32_t call, void* buffer, void* stream) {
    const char* who = "cadm_imagine";
    CADM_REQUIRE(ctx && obs && buffer, "%s: ctx / obs / buffer is null", who);
    int rc;
    if ((rc = cadm_imagine_check(ctx, m, n, k, constraints, disagreement, who))) return rc;
    CADM_REQUIRE(isfinite(noise_std) && noise_std >= 0.0f, "%s: noise_std %g is negative or not finite", who, (double)noise_std);
    CADM_REQUIRE(ctx->C == 0 || ctx_vec, "%s: ctx_vec required for a context model", who);
    if (!actions && !cadm_policy_dev(ctx, nullptr, nullptr)) {
        cadm_set_error("%s: neither actions nor a registered policy net (call cadm_set_policy_net)", who);
        return CADM_ESTATE;
    }
    if ((rc = cadm_require_ready(ctx, who))) return rc;
    CADM_ON_DEVICE(ctx);
    return cadm_launch_imagine(ctx, obs, ctx_vec, actions, m, n, k, noise_std, constraints, disagreement, seed, call, buffer, (hipStream_t)stream, who);
}

extern "C" int cadm_imagine_select(cadm_ctx* ctx, const float* next, const float* rows1, const float* state, const int32_t* sel_in, int rows,
                                   int t, const cadm_constraint_params* constraints, const cadm_uncertainty_params* disagreement,
                                   uint32_t seed, uint32_t call, uint8_t* alive_io, float* state_out, float* rew_out, uint8_t* done_out,
                                   uint8_t* valid_out, int32_t* member_out, float* disagreement_out, int32_t* length_io, float* bcast_out,
                                   void* stream) {
    const char* who = "cadm_imagine_select";
    CADM_REQUIRE(ctx && next && rows1 && state && alive_io && state_out && rew_out && done_out && valid_out && member_out && disagreement_out,
                 "%s: ctx / next / rows1 / state / alive_io / an output is null", who);
    CADM_REQUIRE(rows >= 1 && t >= 0, "%s: rows must be >= 1 and t >= 0 (got rows=%d t=%d)", who, rows, t);
    CADM_REQUIRE(bcast_out != next, "%s: bcast_out aliases next", who);
    ImagineArgs a{};
    int rc;
    if ((rc = imagine_fill(ctx, constraints, disagreement, who, &a))) return rc;
    a.next = next; a.rows1 = rows1; a.state = state; a.sel_in = sel_in; a.alive = alive_io; a.state_out = state_out; a.rew = rew_out;
    a.done = done_out; a.valid = valid_out; a.member = member_out; a.disag = disagreement_out; a.length = length_io; a.bcast = bcast_out;
    a.rows = (size_t)rows; a.t = t; a.seed = seed; a.call = call;
    CADM_ON_DEVICE(ctx);
    return imagine_select_launch(a, (hipStream_t)stream, who);
}
