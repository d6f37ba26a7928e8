// The planner loops of libcadm_hip.so: CEM (cadm_cem_plan), its one-call form from host arrays (cadm_cem_plan_staged) and random
// shooting (cadm_rs_plan), each a sequence of launches on the caller's stream.  (iCEM is a loop of its own: icem.hip.)
#include <string.h>
#include <time.h>

#include "planner.h"

// the path's one collective, bracketed by hipEvents when profiling is on
static int allgather_timed(cadm_ctx* ctx, const float* send, float* recv, size_t count, hipStream_t s) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc;
    if (ctx->prof) {
        if ((rc = cadm_prof_pair(ctx->prof_ag, ctx->prof_ag_used, &e0, &e1))) return rc;
        CADM_CHECK_HIP(hipEventRecord(e0, s));
    }
    rc = cadm_dist_allgather(ctx, send, recv, count, s);
    if (ctx->prof && rc == CADM_OK) CADM_CHECK_HIP(hipEventRecord(e1, s));
    return rc;
}

struct PlanWs {
    float *ctxv, *actions, *rows, *cand, *gath, *mean, *var;
    int32_t* raw;
    unsigned* chk;      // sharded planner: checksum of this call's replicated inputs
};

static size_t carve(cadm_ctx* ctx, int m, int n, char* base, PlanWs* w) {
    Carver c{base};
    PlanWs t;
    t.ctxv = c.take<float>((size_t)ctx->E * m * (ctx->C > 0 ? ctx->C : 1));
    t.actions = c.take<float>((size_t)m * n * ctx->H * ctx->A);
    t.rows = c.take<float>((size_t)m * n * ctx->p);
    t.cand = c.take<float>((size_t)m * n);
    t.gath = c.take<float>((size_t)m * n + 1024);      // (+ one checksum word per rank of a sharded call)
    t.mean = c.take<float>((size_t)m * ctx->H * ctx->A);
    t.var = c.take<float>((size_t)m * ctx->H * ctx->A);
    t.raw = c.take<int32_t>((size_t)m * n * ctx->H);
    t.chk = c.take<unsigned>(64);
    if (w) *w = t;
    return c.off;
}

extern "C" size_t cadm_plan_workspace_bytes(cadm_ctx* ctx, int m, int n) {
    if (!ctx || m <= 0 || n <= 0) return 0;
    return carve(ctx, m, n, nullptr, nullptr);
}

// What a CEM plan refuses before it touches the stream (have_cp: cp_obs and cp_act were supplied; who: the name an unready engine is reported under)
static int cem_plan_refuse(cadm_ctx* ctx, bool have_cp, int n, const char* who) {
    CADM_REQUIRE(ctx->C == 0 || have_cp, "cadm_cem_plan: cp_obs/cp_act required for a context model");
    const int G = cadm_sharded(ctx) ? ctx->nranks : 1;
    CADM_REQUIRE(n % G == 0, "cadm_cem_plan: n_candidates %d not divisible by %d ranks", n, G);
    CADM_REQUIRE(n >= ctx->cfg.num_elites, "cadm_cem_refit: n_candidates %d < num_elites %d (tf.nn.top_k would fail)", n, ctx->cfg.num_elites);
    return cadm_require_ready(ctx, who);
}

// head_done: the context vector and the candidates of iteration 0 are already in the workspace (cadm_cem_plan_staged's fused head);
// done: the completion flags the last refit raises (a staged call)
static int cem_plan_impl(cadm_ctx* ctx, const float* obs, const float* cp_obs, const float* cp_act,
                         const float* init_mean, const float* init_var, int m, int n, uint32_t seed,
                         uint32_t call, void* workspace, float* plan_out, void* stream, bool head_done, PlanDone done) {
    CADM_REQUIRE(ctx && obs && init_mean && init_var && workspace && plan_out && m > 0 && n > 0,
                 "cadm_cem_plan: bad arguments");
    if (int rd = cadm_refuse_discounted(ctx, "cadm_cem_plan")) return rd;
    CADM_ON_DEVICE(ctx);
    int rc = cem_plan_refuse(ctx, cp_obs && cp_act, n, "cadm_rollout_returns");      // (the call that has always reported an unready engine)
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    PlanWs w;
    carve(ctx, m, n, (char*)workspace, &w);
    if (ctx->C > 0 && !head_done && (rc = cadm_context_forward(ctx, cp_obs, cp_act, m, 0, w.ctxv, stream))) return rc;
    const int G = cadm_sharded(ctx) ? ctx->nranks : 1;
    const int nl = n / G, off = (cadm_sharded(ctx) ? ctx->rank : 0) * nl;
    const int iters = ctx->cfg.num_cem_iters;
    // Small candidate sets (rank-by-counting regime): the refit of iteration it and the sampling of iteration it + 1 are ONE
    // launch parallel over the plan's (t, a) elements (cem_refit_sample_kernel) -- sample(0), then rollout + fused step per
    // iteration, the last refit alone (it writes the clipped plan).  Larger sets: sample / rollout / refit per iteration.
    // (sharded: the stepwise form -- the refit REGENERATES the elites, which the fused refit + sample kernel does not do)
    const bool fuse = G == 1 && cadm_refit_sample_ok(ctx, n);
    CADM_REQUIRE(G <= 1024, "cadm_cem_plan: %d ranks", G);
    // Sharded call: every rank draws only ITS candidates (the draws are keyed by global element index) and the refit draws
    // the <= num_elites elite sequences again instead of reading them: the per-iteration work besides the rollout no longer grows with
    // the number of ranks.  The checksum of this rank's inputs rides at the end of its all-gather payload: every call is checked.
    if (G > 1 && (rc = cadm_launch_input_checksum(ctx, obs, ctx->C > 0 ? cp_obs : nullptr, ctx->C > 0 ? cp_act : nullptr, init_mean, init_var,
                                                  m, w.chk, s))) return rc;
    for (int it = 0; it < iters; ++it) {
        const bool first = it == 0, last = it + 1 == iters;
        // iteration 0 reads the caller's mean / var directly; the last refit also writes the clipped plan (dynamics.py:365-366)
        const float* mean_in = first ? init_mean : w.mean;
        const float* var_in = first ? init_var : w.var;
        float* plan = last ? plan_out : nullptr;
        // a rank draws ITS n / G candidates, at their global positions (counter-based RNG keyed by the global element index; the fused head of
        // cadm_cem_plan_staged has drawn all n of iteration 0 -- a superset, same values)
        if ((first && !head_done) || (!first && !fuse)) {
            if ((rc = cadm_sample_actions_shard(ctx, mean_in, var_in, nullptr, seed, call, it, m, n, off, nl, w.actions, stream))) return rc;
        }
        if ((rc = cadm_rollout_returns(ctx, obs, nullptr, ctx->C > 0 ? w.ctxv : nullptr, w.actions, nullptr, 1, seed,
                                       call, it, off, n, m, nl, w.rows, nullptr, stream))) return rc;
        const float* cand = nullptr;
        const float* rows = w.rows;
        if (G > 1) {   // the one collective of the path: [m, n/G] per rank -> [G, m, n/G] everywhere
            if ((rc = cadm_launch_particle_mean_tail(ctx, w.rows, m, nl, w.cand, w.chk, s))) return rc;
            if ((rc = allgather_timed(ctx, w.cand, w.gath, (size_t)m * nl + 1, s))) return rc;
            cand = w.gath;
            rows = nullptr;
        }              // (single rank: the particle mean is taken inside the refit kernels)
        if (fuse && !last) {
            if ((rc = cadm_launch_refit_sample(ctx, cand, rows, G, nl, w.actions, m, mean_in, var_in, w.mean, w.var, seed, call, it + 1, s))) return rc;
        } else {
            RefitRegen rg{};      // (read by a sharded call only)
            rg.on = 1; rg.seed = seed; rg.call = call; rg.it = it; rg.gstride = m * nl + 1; rg.my_rank = ctx->rank;
            rg.mismatch = ctx->dist_flag;
            rg.mismatch_host = (last && done.flags) ? done.flags + m : nullptr;      // (a staged call: m words behind its m completion flags)
            if ((rc = cadm_launch_refit(ctx, cand, rows, G, nl, w.actions, m, mean_in, var_in, w.mean, w.var, nullptr, plan, s, G > 1 ? &rg : nullptr, done))) return rc;
        }
    }
    return CADM_OK;
}

extern "C" int cadm_cem_plan(cadm_ctx* ctx, const float* obs, const float* cp_obs, const float* cp_act,
                             const float* init_mean, const float* init_var, int m, int n, uint32_t seed,
                             uint32_t call, void* workspace, float* plan_out, void* stream) {
    return cem_plan_impl(ctx, obs, cp_obs, cp_act, init_mean, init_var, m, n, seed, call, workspace, plan_out, stream, false, {});
}

// Per-call inputs of a small planner call travel as KERNEL ARGUMENTS: the runtime writes them into the kernarg segment with
// the launch packet, a one-workgroup kernel unpacks them into the device block.  Same queue as the planner kernels: no copy
// engine, no cross-engine dependency (hipMemcpyAsync of 2.5 KB cost ~10 us more per call; a kernel READING the pinned block
// over PCIe was 10x slower still).
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    asm volatile("" ::: "memory");
#endif
}
__global__ void ingest_kernel(const IngestBlock blk, float* __restrict__ dev_block, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dev_block[i] = blk.v[i];
}

// The class API's call (dynamics.py:344-367: numpy in -> numpy out) as ONE library call: the caller has packed the five
// per-call inputs into a host block; blocks of up to CADM_INGEST_MAX floats (every reference configuration: 618 at cfg2) travel
// as KERNEL ARGUMENTS of a one-workgroup ingest kernel -- same queue as the planner, no copy engine -- larger ones by an async
// H2D copy; then the whole planner, the plan written straight into the caller's pinned host buffer by the last refit kernel,
// and (optionally) the wait for its completion flags.
extern "C" int cadm_cem_plan_staged(cadm_ctx* ctx, const float* host_block, float* dev_block, const int32_t off[5], int nfloats,
                                    int m, int n, uint32_t seed, uint32_t call, void* workspace, float* plan_out_host, int sync,
                                    void* stream) {
    CADM_REQUIRE(ctx && host_block && dev_block && off && nfloats > 0 && plan_out_host && workspace && m > 0 && n > 0,
                 "cadm_cem_plan_staged: bad arguments");
    if (int rd = cadm_refuse_discounted(ctx, "cadm_cem_plan_staged")) return rd;
    CADM_ON_DEVICE(ctx);
    // refused before the fused head is enqueued (it carves the workspace and writes into it)
    CADM_REQUIRE(off[0] >= 0 && off[3] >= 0 && off[4] >= 0, "cadm_cem_plan_staged: obs / init_mean / init_var missing from the block");
    int rc = cem_plan_refuse(ctx, off[1] >= 0 && off[2] >= 0, n, "cadm_cem_plan_staged");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    bool head_done = false;
    // (the fused head runs the per-row encoder: from CADM_CONTEXT_BATCHED_MIN_ROWS envs on, the unfused call would take the batched one --
    //  not the same summation order -- so the head stays below it and a get_action means the same numbers either way)
    if (nfloats <= CADM_HEAD_INGEST_MAX && m < CADM_CONTEXT_BATCHED_MIN_ROWS) {
        // ONE launch: unpack the block, the context encoder on its history, the candidates of CEM iteration 0 (context.hip)
        PlanWs w;
        carve(ctx, m, n, (char*)workspace, &w);
        if ((rc = cadm_launch_plan_head(ctx, host_block, nfloats, off, dev_block, m, n, seed, call, w.ctxv, w.actions, s))) return rc;
        head_done = true;
    } else if (nfloats <= CADM_INGEST_MAX) {
        IngestBlock blk;
        memcpy(blk.v, host_block, (size_t)nfloats * sizeof(float));
        hipLaunchKernelGGL(ingest_kernel, dim3(1), dim3(256), 0, s, blk, dev_block, nfloats);
        CADM_CHECK_HIP(hipGetLastError());
    } else {
        CADM_CHECK_HIP(hipMemcpyAsync(dev_block, host_block, (size_t)nfloats * sizeof(float), hipMemcpyHostToDevice, s));
    }
    auto at = [&](int i) -> const float* { return off[i] < 0 ? nullptr : dev_block + off[i]; };      // obs, cp_obs, cp_act, mean, var
    // completion: [m] flag words behind the plan in the caller's pinned buffer, released by the last refit kernel with this
    // call's id; the host polls them (a sleeping hipStreamSynchronize wakes up ~10 us late on a 1 ms call)
    unsigned* flags = reinterpret_cast<unsigned*>(plan_out_host + (size_t)m * ctx->H * ctx->A);
    const unsigned val = call ^ 0x5ca1ab1eu;
    if (sync) { for (int i = 0; i < m; ++i) { flags[i] = ~val; flags[m + i] = 0u; } }      // (+ m mismatch words of a sharded call)
    if ((rc = cem_plan_impl(ctx, at(0), at(1), at(2), at(3), at(4), m, n, seed, call, workspace, plan_out_host, stream, head_done,
                            PlanDone{sync ? flags : nullptr, val}))) return rc;
    if (sync) {
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        volatile unsigned* vf = flags;
        bool ok = false;
        for (unsigned long spins = 0; !ok; ++spins) {
            ok = true;
            for (int i = 0; i < m; ++i) ok = ok && vf[i] == val;
            if (ok) break;
            cpu_relax();
            if ((spins & 4095) == 4095) {           // a kernel that faulted never raises the flag: fall back to the runtime's verdict
                clock_gettime(CLOCK_MONOTONIC, &t1);
                if ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec) > 0.25) break;
            }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        if (!ok) CADM_CHECK_HIP(hipStreamSynchronize(s));
    }
    return CADM_OK;
}

__global__ void gather_raw_first_kernel(const int32_t* raw, const int32_t* best, int m, int n, int H, int32_t* out) {
    const int mi = blockIdx.x * blockDim.x + threadIdx.x;
    if (mi < m) out[mi] = raw[((size_t)mi * n + best[mi]) * H];
}

extern "C" int cadm_rs_plan(cadm_ctx* ctx, const float* obs, const float* cp_obs, const float* cp_act, int m, int n,
                            uint32_t seed, uint32_t call, void* workspace, float* action_out, int32_t* raw_best_out,
                            void* stream) {
    CADM_REQUIRE(ctx && obs && workspace && action_out && m > 0 && n > 0, "cadm_rs_plan: bad arguments");
    if (int rd = cadm_refuse_discounted(ctx, "cadm_rs_plan")) return rd;
    CADM_ON_DEVICE(ctx);
    CADM_REQUIRE(ctx->C == 0 || (cp_obs && cp_act), "cadm_rs_plan: cp_obs/cp_act required for a context model");
    CADM_REQUIRE(!ctx->cfg.discrete || raw_best_out, "cadm_rs_plan: raw_best_out required for discrete actions");
    hipStream_t s = (hipStream_t)stream;
    PlanWs w;
    carve(ctx, m, n, (char*)workspace, &w);
    int rc;
    if (ctx->C > 0 && (rc = cadm_context_forward(ctx, cp_obs, cp_act, m, 0, w.ctxv, stream))) return rc;
    if ((rc = cadm_sample_uniform(ctx, seed, call, m, n, w.actions, w.raw, stream))) return rc;
    // it = 0: the RS graph transposes the context tensor once (core/utils.py:513) -> the even-iteration layout
    const int G = cadm_sharded(ctx) ? ctx->nranks : 1;
    CADM_REQUIRE(n % G == 0, "cadm_rs_plan: n_candidates %d not divisible by %d ranks", n, G);
    const int nl = n / G, off = (cadm_sharded(ctx) ? ctx->rank : 0) * nl;
    if ((rc = cadm_rollout_returns(ctx, obs, nullptr, ctx->C > 0 ? w.ctxv : nullptr, w.actions, nullptr,
                                   ctx->cfg.discrete ? 0 : 1, seed, call, 0, off, n, m, nl, w.rows, nullptr, stream))) return rc;
    if ((rc = cadm_particle_mean(ctx, w.rows, m, nl, w.cand, stream))) return rc;
    const float* cand = w.cand;
    if (G > 1) {
        if ((rc = allgather_timed(ctx, w.cand, w.gath, (size_t)m * nl, s))) return rc;
        cand = w.gath;
    }
    int32_t* best = (int32_t*)w.mean;  // scratch reuse: m ints
    if ((rc = cadm_rs_select(ctx, cand, G, nl, w.actions, m, action_out, best, stream))) return rc;
    if (ctx->cfg.discrete) {
        hipLaunchKernelGGL(gather_raw_first_kernel, dim3((m + 63) / 64), dim3(64), 0, s, w.raw, best, m, n, ctx->H, raw_best_out);
        CADM_CHECK_HIP(hipGetLastError());
    } else {
        if ((rc = cadm_launch_clip(action_out, action_out, m * ctx->A, ctx->cfg.lower_bound, ctx->cfg.upper_bound, 1, s))) return rc;
    }
    return CADM_OK;
}
