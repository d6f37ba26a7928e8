// Run-time tracking targets of the opt-in planner loop (icem.hip): a cost on the predicted states that the caller sets per env and per
// step at call time -- "hold joint 3 at 0.4", "run at 2 m/s in env 0 and 5 m/s in env 1", "follow this reference" -- with no new env
// spec and no rebuild.  No reference twin: the reference's rewards are fixed when the model is built.  One kernel BEHIND the rollout,
// like the constraints (constrain.hip), the score (score.hip) and the forecast (forecast.hip): it reads the trajectories the rollout
// recorded (`traj_out`, [H, m, n, p, D]) and rewrites the rollout's returns (rows [m, n, p]); the rollout kernels are not touched.
//
// A term k reads one observation dim of the POST-step state traj[t] of step t = 0 .. H - 1 of env mi against the target
// g = targets[mi, clamp(offset[mi] + t, 0, T - 1), k]:  e = x[dim k] - g,  c = e^2 (SQUARE), |e| (ABS) or the Huber function of e with
// threshold delta_k,  cost += w_k c -- one thread's chain per row, steps in order, k ascending inside a step -- and rows' = rows - cost.
// A NaN target skips its (step, term); a row whose every (step, term) was skipped keeps its input bits.  With `first` (the constraint
// kernel's first_violation) steps t > first[row] are not counted: the step that leaves the region still pays, nothing behind it does.
// A non-finite value in a tracked dim at a counted step makes the row's return non-finite; other dims are not looked at.
// On a ctx with a discount over the horizon (cadm_set_discount, discount.hip): cost += disc[t] * (w_k c), the same order, the same skips.
//
// Mapping and traffic: constrain.hip's PENALTY mapping.  A workgroup owns TR_ROWS consecutive rows, one thread per row; its TR_THREADS
// threads (four waves) all load.  For a fixed step those rows' D values are ONE contiguous span of `traj`, loaded lane-linear into an
// LDS tile (16-byte loads where the span is 16-byte aligned, scalar loads otherwise); every value of `traj` is read at most once.  The
// rows of a workgroup belong to at most TR_ROWS consecutive envs: their target rows of the step (K floats each) are staged into LDS by
// the same threads in front of the same barrier, the envs' offsets and the terms once in front of the loop.  A step is a chain of load, barrier,
// cost.  With `first`, a workgroup whose rows have all been cut stops loading.
// Reduction contract: a row's cost is one thread's chain in step order; no floating-point atomics, nothing depends on the grid, on m
// or n, or on the row's position: the same bits run to run and inside any batch.
#include <math.h>

#include "planner.h"

namespace {

constexpr int TR_ROWS = 64;                  // rows per workgroup: the first wave's threads, one row each
constexpr int TR_THREADS = 256;              // threads per workgroup: all of them load
constexpr int TR_LDS_BUDGET = 48 * 1024;     // the tile of TR_ROWS * D floats, the targets, the offsets and the terms; below the 64 KiB a kernel gets without an attribute
constexpr int TR_TARGET_FLOATS = TR_ROWS * CADM_MAX_TRACK_TERMS;      // up to TR_ROWS envs' target rows of one step

struct TrackArgs {
    const float *traj, *targets, *rows_in;
    const float* disc;         // [H + 1] the ctx's discount table (DISC kernel only)
    const int32_t *offset, *first;
    float *rows_out, *cost_out;
    size_t total;              // m * n * p rows
    int np;                    // n * p: rows per env
    int H, D, T;
    cadm_track_params c;
};

// DISC: the ctx's discount over the horizon (discount.hip): cost = cost + disc[t] * (w_k c).  false: the undiscounted kernel as it was
template <bool DISC>
__global__ __launch_bounds__(TR_THREADS) void tracking_returns_kernel(const TrackArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tr_smem[];
    const int D = a.D, H = a.H, K = a.c.n, ts = (TR_ROWS * D + 3) & ~3, tid = threadIdx.x;
    float* tg = tr_smem + ts;                                      // [ne, K] the step's target rows of this workgroup's envs
    int32_t* toff = reinterpret_cast<int32_t*>(tg + TR_TARGET_FLOATS);      // [ne] their offsets
    // the terms, copied out of the kernel arguments once: LDS reads come back in order, so the step chain can keep several terms' reads in
    // flight, which scalar loads between them do not allow
    int32_t* sdim = toff + TR_ROWS;                                // [K]
    int32_t* skind = sdim + CADM_MAX_TRACK_TERMS;                  // [K]
    float* sw = reinterpret_cast<float*>(skind + CADM_MAX_TRACK_TERMS);      // [K]
    float* sdl = sw + CADM_MAX_TRACK_TERMS;                        // [K]
    const size_t q0 = (size_t)blockIdx.x * TR_ROWS;      // first row of this workgroup (q0 < total: the grid is ceil(total / TR_ROWS))
    const int nr = a.total - q0 < (size_t)TR_ROWS ? (int)(a.total - q0) : TR_ROWS;
    const int span = nr * D;
    const bool mine = tid < nr;
    const size_t q = q0 + tid;
    const size_t e0 = q0 / (size_t)a.np;                           // first env of this workgroup
    const int ne = (int)((q0 + nr - 1) / (size_t)a.np - e0) + 1;   // <= nr <= TR_ROWS: every env holds a row
    if (tid < ne) toff[tid] = a.offset ? a.offset[e0 + tid] : 0;
    if (tid < K) {
        sdim[tid] = a.c.dim[tid];
        skind[tid] = a.c.kind[tid];
        sw[tid] = a.c.w[tid];
        sdl[tid] = a.c.delta[tid];
    }
    const float* g = tg + (mine ? (int)(q / (size_t)a.np - e0) : 0) * K;
    const int cut = !mine ? -1 : a.first ? a.first[q] : H;         // steps t > cut are not counted
    __syncthreads();
    float cost = 0.0f;
    bool any = false;
    for (int t = 0; t < H; ++t) {
        const float* src = a.traj + ((size_t)t * a.total + q0) * D;
        const int nvec = (reinterpret_cast<uintptr_t>(src) & 15) == 0 ? span >> 2 : 0;
        for (int i = tid; i < nvec; i += TR_THREADS) reinterpret_cast<floatx4*>(tr_smem)[i] = reinterpret_cast<const floatx4*>(src)[i];
        for (int i = 4 * nvec + tid; i < span; i += TR_THREADS) tr_smem[i] = src[i];
        for (int i = tid; i < ne * K; i += TR_THREADS) {
            const int e = i / K;
            long long r = (long long)toff[e] + t;
            r = r < 0 ? 0 : (r > a.T - 1 ? a.T - 1 : r);
            tg[i] = a.targets[((e0 + e) * (size_t)a.T + (size_t)r) * K + (i - e * K)];
        }
        __syncthreads();
        if (mine && t <= cut) {
            const float* x = tr_smem + tid * D;
            const float dt = DISC ? a.disc[t] : 1.0f;
            // No branch on the data and nothing read under one: a term's parameters, its target and its value (all LDS reads) depend on
            // nothing the term before it computed, so the reads of several terms are in flight together.  With a branch per term and the
            // parameters read from the kernel arguments every term waited for five dependent loads in turn (measured: 106 us against
            // 27 us at K = 16 / K = 1)
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
                const float gk = g[k], w = sw[k], dl = sdl[k];
                const int kind = skind[k];
                const float e = x[sdim[k]] - gk, ae = fabsf(e);
                const float sq = e * e, hub = ae <= dl ? 0.5f * e * e : dl * (ae - 0.5f * dl);
                const float c = kind == CADM_TRACK_SQUARE ? sq : kind == CADM_TRACK_ABS ? ae : hub;
                const float next = DISC ? __fadd_rn(cost, __fmul_rn(dt, __fmul_rn(w, c))) : cost + w * c;
                const bool use = gk == gk;               // NaN: no target for this term at this step
                cost = use ? next : cost;
                any = any || use;
            }
        }
        // every read of the tile and the targets the next step loads over is done; with `first`: leave when no row counts a later step
        if (a.first) {
            if (__syncthreads_count(mine && t < cut) == 0) break;
        } else {
            __syncthreads();
        }
    }
    if (!mine) return;
    const float r_in = a.rows_in[q];
    a.rows_out[q] = any ? r_in - cost : r_in;
    if (a.cost_out) a.cost_out[q] = cost;
}

size_t tracking_lds_bytes(int D) {
    return ((((size_t)TR_ROWS * D + 3) & ~(size_t)3) + TR_TARGET_FLOATS + TR_ROWS + 4 * CADM_MAX_TRACK_TERMS) * sizeof(float);
}

}  // namespace

// the refusals of a set of tracking terms and its targets, before any HIP call
int cadm_track_check(const cadm_ctx* ctx, const cadm_track_params* c, const float* targets, int T, const char* who) {
    CADM_REQUIRE(c, "%s: the tracking parameters are null", who);
    CADM_REQUIRE(c->n >= 1 && c->n <= CADM_MAX_TRACK_TERMS, "%s: %d tracking terms, outside 1 .. %d", who, c->n, CADM_MAX_TRACK_TERMS);
    for (int k = 0; k < c->n; ++k) {
        CADM_REQUIRE(c->dim[k] >= 0 && c->dim[k] < ctx->D, "%s: tracking term %d reads dim %d, outside 0 .. %d", who, k, c->dim[k], ctx->D - 1);
        CADM_REQUIRE(c->kind[k] == CADM_TRACK_SQUARE || c->kind[k] == CADM_TRACK_ABS || c->kind[k] == CADM_TRACK_HUBER,
                     "%s: tracking term %d has an unknown kind %d", who, k, c->kind[k]);
        CADM_REQUIRE(isfinite(c->w[k]) && c->w[k] >= 0.0f, "%s: tracking term %d: w %g is not finite and >= 0", who, k, (double)c->w[k]);
        CADM_REQUIRE(c->kind[k] != CADM_TRACK_HUBER || (isfinite(c->delta[k]) && c->delta[k] > 0.0f),
                     "%s: tracking term %d: the Huber delta %g is not finite and > 0", who, k, (double)c->delta[k]);
    }
    CADM_REQUIRE(T >= 1, "%s: T = %d target rows per env, must be >= 1", who, T);
    CADM_REQUIRE(targets, "%s: targets is null", who);
    CADM_REQUIRE(!ctx->cfg.discrete && ctx->cfg.env_kind != CADM_ENV_CARTPOLE, "%s: tracking targets need a continuous-action ctx (discrete "
                 "actions are planned by random shooting)", who);
    CADM_REQUIRE(!cadm_sharded(ctx), "%s: tracking targets are not supported on a candidate-sharded ctx", who);
    CADM_REQUIRE(tracking_lds_bytes(ctx->D) <= (size_t)TR_LDS_BUDGET,
                 "%s: D (%d) does not fit the kernel's LDS: its tile of %d x D floats, the targets and the offsets need %zu bytes, the bound is %d",
                 who, ctx->D, TR_ROWS, tracking_lds_bytes(ctx->D), TR_LDS_BUDGET);
    return CADM_OK;
}

extern "C" int cadm_tracking_returns(cadm_ctx* ctx, const cadm_track_params* track, const float* traj, const float* targets, int T,
                                     const int32_t* offset, const int32_t* first, const float* rows_in, int m, int n, float* rows_out,
                                     float* cost_out, void* stream) {
    CADM_REQUIRE(ctx && track && traj && rows_in && rows_out, "cadm_tracking_returns: ctx / track / traj / rows_in / rows_out is null");
    int rc;
    if ((rc = cadm_track_check(ctx, track, targets, T, "cadm_tracking_returns"))) return rc;
    CADM_REQUIRE(m >= 1 && n >= 1, "cadm_tracking_returns: m, n must be >= 1 (got m=%d n=%d)", m, n);
    CADM_REQUIRE((long long)n * ctx->p <= 0x7fffffffLL, "cadm_tracking_returns: n * p = %lld rows per env are too many", (long long)n * ctx->p);
    const size_t total = (size_t)m * n * ctx->p, blocks = (total + TR_ROWS - 1) / TR_ROWS;
    CADM_REQUIRE(blocks <= 0x7fffffffull, "cadm_tracking_returns: %zu rows are too many for one launch", total);
    CADM_ON_DEVICE(ctx);
    TrackArgs a{};
    a.traj = traj; a.targets = targets; a.rows_in = rows_in; a.offset = offset; a.first = first; a.rows_out = rows_out; a.cost_out = cost_out;
    a.total = total; a.np = n * ctx->p; a.H = ctx->H; a.D = ctx->D; a.T = T;
    a.c = *track;
    a.disc = ctx->disc;
    if (a.disc) hipLaunchKernelGGL(tracking_returns_kernel<true>, dim3((unsigned)blocks), dim3(TR_THREADS), tracking_lds_bytes(ctx->D), (hipStream_t)stream, a);
    else hipLaunchKernelGGL(tracking_returns_kernel<false>, dim3((unsigned)blocks), dim3(TR_THREADS), tracking_lds_bytes(ctx->D), (hipStream_t)stream, a);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}
