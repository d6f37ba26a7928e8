// Stochastic actor head (no reference twin): the registered policy net read as a SAC actor -- the net's own output layer is the mean
// mu [A] of a diagonal Gaussian, a second output layer on the same last hidden tile (cadm_set_policy_head) its log standard deviation
// l [A].  One kernel, policy_gauss_kernel, samples an action per row and returns its log-density; cadm_policy_sample is its launch on the
// caller's states and cadm_launch_policy_gauss_step the per-step action launch of cadm_imagine_sampled (imagine.hip).  policy.hip's
// kernel, the proposal roll and the critics' fused actor are not touched: they keep reading the mean columns alone, the mode actor.
// A roll flavour, policy_gauss_roll_kernel, is the policy step of cadm_policy_propose once cadm_set_policy_proposals has asked for
// proposals drawn from the head: it shares the draw and the log-std bound with the sampling kernel and computes no log-density.
//
// Arithmetic per row q = row0 + r and action dim d, all float32, every operation rounded on its own, nothing fused but the MFMA's own
// multiply-add (include/cadm_hip.h, "Stochastic actor head", restates it):
//   x, the hidden layers: policy.hip's, on the registered net's own packed copy;   mu_d, l_d: two identity-activation layers on the
//   last hidden tile (L = 0: on the input tile), each one column's chain in ascending k seeded with its bias
//   ls_d   CADM_LOGSTD_CLAMP: fminf(fmaxf(l_d, lo), hi)      CADM_LOGSTD_TANH: lo + (0.5f * (hi - lo)) * (tanhf(l_d) + 1.0f)
//   sig_d  = expf(ls_d)
//   xi_d   Philox4x32-10 keyed (seed, call), counter (q, t, d >> 2, CADM_STREAM_POLICY_SAMPLE), words to dims through Box-Muller exactly as
//          policy.hip's noise (words 0, 1 -> dims 4 g, 4 g + 1; words 2, 3 -> 4 g + 2, 4 g + 3)
//   u_d    = mu_d + sig_d * xi_d                              (one multiply, one add)
//   CADM_POLICY_TANH:  a_d = mid + half * tanhf(u_d);   J_d = logf(half) + 2 * ((LN2 - u_d) - softplus(-2 * u_d)),
//                      softplus(x) = fmaxf(x, 0) + log1pf(expf(-fabsf(x)))      (= log(half (1 - tanh^2 u)) with no epsilon inside a log)
//   CADM_POLICY_NONE:  a_d = u_d;   J_d = 0      (logp is the UNCLIPPED Gaussian's: the clip below is not part of the density)
//   a_d    = fminf(fmaxf(a_d, lb), ub)
//   term_d = (((-0.5f * xi_d) * xi_d - ls_d) - 0.9189385f) - J_d
//   logp   = term_0 + term_1 + ..   one thread per row, ascending d from term_0, out of LDS behind a barrier
//   mode_d = cadm_policy_eval's action of the row: fminf(fmaxf(squash(mu_d), lb), ub)
// A row with a non-finite value in its state: act = mode = clip(0, lb, ub) in every dim, logp = NaN.
// Mapping (policy.hip's): a workgroup of 4 waves owns 16 * RT consecutive rows, one state per row, activations resident in LDS as
// [unit][row]; the last hidden tile is read twice through mlp_layer, the two sets of A sums land in two LDS regions; one thread per
// (row, dim) then draws, squashes, stores act / mode and leaves term_d in the log-std's place; behind a barrier one thread per row sums.
// Reduction contract: every output is ONE thread's chain in the order above; no floating-point atomics; nothing depends on RT, the
// grid, R or the row's position for the same q: the same bits run to run.
#include "mlp_chain.h"

// the ctx-owned packed copy of the head's layer h_L -> A (mlp_chain.h's layer layout: mlp_pack_kernel) and its description
struct PolicyHead {
    bool set = false;
    MlpNet net;                    // buf / cap, W[0], b[0]; no statistics: the head reads the net's hidden tile
    cadm_policy_head_params prm{};
};

namespace {

constexpr float GAUSS_LN2 = 0.6931472f;
constexpr float GAUSS_HALF_LOG_2PI = 0.9189385f;

struct GaussArgs {
    MlpDev net;                    // D -> h_1 .. h_L -> A: the registered net, its output layer the mean
    const float *Wls, *bls;        // the head's packed layer h_L -> A
    const float* x;                // [total, D] one state per row
    int squash, bound, t;
    float lb, ub, mid, half, lo, hi;
    uint32_t seed, call, row0;
    float *act, *logp, *mode;      // [total, A], [total], [total, A] or null
    size_t total;
    int region0, region1;          // LDS floats of the two activation regions; the log-std's A sums follow them
};

__device__ __forceinline__ float gauss_softplus(float x) { return __fadd_rn(fmaxf(x, 0.0f), log1pf(expf(-fabsf(x)))); }

// what the sampling kernel and the roll flavour share per (row, dim): the bounded log-std of the raw l (hw = 0.5f * (hi - lo)) ..
__device__ __forceinline__ float gauss_log_std(float l, int bound, float lo, float hi, float hw) {
    return bound == CADM_LOGSTD_TANH ? __fadd_rn(lo, __fmul_rn(hw, __fadd_rn(tanhf(l), 1.0f))) : fminf(fmaxf(l, lo), hi);
}

// .. and the draw of Philox row q, step t, dim d under a stream word: policy.hip's word-to-dim mapping
__device__ __forceinline__ float gauss_xi(uint32_t q, int t, int d, uint32_t stream, uint32_t seed, uint32_t call) {
    uint32_t w[4];
    philox4x32_10(q, (uint32_t)t, (uint32_t)(d >> 2), stream, seed, call, w);
    float z0, z1;
    const int pair = d & 2;
    box_muller(u01(w[pair]), u01(w[pair + 1]), z0, z1);
    return (d & 1) ? z1 : z0;
}

template <int RT>
__global__ __launch_bounds__(MLP_THREADS) void policy_gauss_kernel(const GaussArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gauss_smem[];
    constexpr int R = 16 * RT;
    float* reg0 = gauss_smem;
    float* reg1 = reg0 + a.region0;
    const int A = a.net.dims[a.net.nlayers], A4 = (A + 3) & ~3;
    float* lsr = reg1 + a.region1;                               // [A4][R] the log-std's sums, later term_d
    int* bad = reinterpret_cast<int*>(lsr + A4 * R);             // [R] 1: a non-finite value in the row's state
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t q0 = (size_t)blockIdx.x * R;                    // (q0 < total: the grid is ceil(total / R))
    const int rows = a.total - q0 < (size_t)R ? (int)(a.total - q0) : R;
    if (tid < R) bad[tid] = 0;
    __syncthreads();
    // the input tile [k][row], normalised on the way in; rows behind the batch and the k behind D are zeros (policy.hip's prologue, p = 1)
    const int D = a.net.dims[0], D4 = (D + 3) & ~3;
    for (int idx = tid; idx < R * D4; idx += MLP_THREADS) {
        const int row = idx / D4, k = idx - row * D4;
        float x = 0.0f;
        if (k < D && row < rows) {
            const float est = a.x[(q0 + row) * D + k];
            if (mlp_nonfinite(est)) bad[row] = 1;                // (every writer stores the same 1)
            x = (est - a.net.mean[k]) * a.net.istd[k];
        }
        reg0[k * R + mlp_swz<RT>(row, k)] = x;
    }
    __syncthreads();
    // the hidden layers as mlp_forward walks them, then the last hidden tile twice: the net's own output layer and the head's
    const int L = a.net.nlayers - 1;
    const float* xin = reg0;
    for (int l = 0; l < L; ++l) {
        float* xout = (l & 1) ? reg0 : reg1;
        mlp_layer<RT>(a.net.W[l], a.net.b[l], a.net.dims[l], a.net.dims[l + 1], a.net.act, false, xin, xout, nullptr, wave, lane);
        __syncthreads();
        xin = xout;
    }
    float* mur = (L & 1) ? reg0 : reg1;
    mlp_layer<RT>(a.net.W[L], a.net.b[L], a.net.dims[L], A, MLP_ACT_NONE, false, xin, mur, nullptr, wave, lane);
    mlp_layer<RT>(a.Wls, a.bls, a.net.dims[L], A, MLP_ACT_NONE, false, xin, lsr, nullptr, wave, lane);
    __syncthreads();
    const float hw = __fmul_rn(0.5f, __fsub_rn(a.hi, a.lo));
    for (int idx = tid; idx < rows * A; idx += MLP_THREADS) {
        const int row = idx / A, d = idx - row * A;
        const size_t r = q0 + row;
        const int at = d * R + mlp_swz<RT>(row, d);
        float act, mode, term;
        if (bad[row]) {
            act = mode = fminf(fmaxf(0.0f, a.lb), a.ub);
            term = __builtin_nanf("");
        } else {
            const float mu = mur[at], l = lsr[at];
            mode = fminf(fmaxf(mlp_squash(mu, a.squash, a.mid, a.half), a.lb), a.ub);
            const float ls = gauss_log_std(l, a.bound, a.lo, a.hi, hw);
            const float sig = expf(ls);
            const float xi = gauss_xi(a.row0 + (uint32_t)r, a.t, d, CADM_STREAM_POLICY_SAMPLE, a.seed, a.call);
            const float u = __fadd_rn(mu, __fmul_rn(sig, xi));
            float J = 0.0f;
            act = u;
            if (a.squash == CADM_POLICY_TANH) {
                act = __fadd_rn(a.mid, __fmul_rn(a.half, tanhf(u)));
                J = __fadd_rn(logf(a.half), __fmul_rn(2.0f, __fsub_rn(__fsub_rn(GAUSS_LN2, u), gauss_softplus(__fmul_rn(-2.0f, u)))));
            }
            act = fminf(fmaxf(act, a.lb), a.ub);
            term = __fsub_rn(__fsub_rn(__fsub_rn(__fmul_rn(__fmul_rn(-0.5f, xi), xi), ls), GAUSS_HALF_LOG_2PI), J);
        }
        a.act[r * A + d] = act;
        if (a.mode) a.mode[r * A + d] = mode;
        lsr[at] = term;                                          // (this thread's own slot: read above, summed behind the barrier)
    }
    __syncthreads();
    if (tid < rows) {
        float s = lsr[mlp_swz<RT>(tid, 0)];
        for (int d = 1; d < A; ++d) s = __fadd_rn(s, lsr[d * R + mlp_swz<RT>(tid, d)]);
        a.logp[q0 + tid] = s;
    }
}

// The roll flavour (cadm_set_policy_proposals, CADM_PROPOSE_HEAD): one policy step of cadm_policy_propose whose sequences j >= 1 are
// draws of the head.  policy_step_kernel's prologue (obs or x [total, p, D], the particle mean, the states copy), this file's walk to
// mu and l, and an epilogue that consumes l where it is read: no term tile behind it, no logp phase, no barrier for one.  Per row
// q = mi * P + j and dim d (include/cadm_hip.h, "Proposals of the policy prior drawn from the head"):
//   s_d = std_scale * expf(ls_d);   j == 0 or std_scale == 0: u_d = mu_d, nothing drawn;   else u_d = mu_d + s_d * xi_d, xi under
//   counter (q, t, d >> 2, CADM_STREAM_POLICY): the noise route's draw;   a_d = clip(squash(u_d)).   A non-finite state: clip(0).
struct GaussRollArgs {
    MlpDev net;                    // D -> h_1 .. h_L -> A: the registered net, its output layer the mean
    const float *Wls, *bls;        // the head's packed layer h_L -> A
    const float* obs;              // [m, D]: the state of every row of env mi (t == 0), or null
    const float* x;                // [total, p, D]: the particle states of the rows (t >= 1), or null
    int squash, bound, P, p, t, H;
    float lb, ub, mid, half, lo, hi, std_scale;
    uint32_t seed, call;
    float* seqs;                   // [total, H, A] or null: a_t goes to [q, t, :]
    float* a1;                     // [total, A]: a_t
    float* states;                 // [total, p, D] or null: the particle states that were read
    size_t total;
    int region0, region1;          // LDS floats of the two activation regions; the log-std's A sums follow them
};

template <int RT>
__global__ __launch_bounds__(MLP_THREADS) void policy_gauss_roll_kernel(const GaussRollArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gauss_smem[];
    constexpr int R = 16 * RT;
    float* reg0 = gauss_smem;
    float* reg1 = reg0 + a.region0;
    const int A = a.net.dims[a.net.nlayers], A4 = (A + 3) & ~3;
    float* lsr = reg1 + a.region1;                               // [A4][R] the log-std's sums
    int* bad = reinterpret_cast<int*>(lsr + A4 * R);             // [R] 1: a non-finite value in the row's state
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t q0 = (size_t)blockIdx.x * R;                    // (q0 < total: the grid is ceil(total / R))
    const int rows = a.total - q0 < (size_t)R ? (int)(a.total - q0) : R;
    if (tid < R) bad[tid] = 0;
    __syncthreads();
    // the input tile [k][row]: policy_step_kernel's prologue, statement for statement
    const int D = a.net.dims[0], D4 = (D + 3) & ~3;
    for (int idx = tid; idx < R * D4; idx += MLP_THREADS) {
        const int row = idx / D4, k = idx - row * D4;
        float x = 0.0f;
        if (k < D && row < rows) {
            const size_t q = q0 + row;
            float est;
            bool nf;
            if (a.obs) {
                est = a.obs[(q / a.P) * D + k];
                nf = mlp_nonfinite(est);
                if (a.states)
                    for (int j = 0; j < a.p; ++j) a.states[(q * a.p + j) * D + k] = est;
            } else {
                const float* xp = a.x + q * a.p * D + k;
                float s = xp[0];
                nf = mlp_nonfinite(s);
                if (a.states) a.states[q * a.p * D + k] = s;
                for (int j = 1; j < a.p; ++j) {
                    const float v = xp[(size_t)j * D];
                    nf = nf || mlp_nonfinite(v);
                    if (a.states) a.states[(q * a.p + j) * D + k] = v;
                    s = __fadd_rn(s, v);
                }
                est = a.p > 1 ? __fdiv_rn(s, (float)a.p) : s;
            }
            if (nf) bad[row] = 1;                                // (every writer stores the same 1)
            x = (est - a.net.mean[k]) * a.net.istd[k];
        }
        reg0[k * R + mlp_swz<RT>(row, k)] = x;
    }
    __syncthreads();
    // the hidden layers, then the last hidden tile twice, as policy_gauss_kernel walks them -- but the head's layer is handed out from
    // wave 2 on: A <= 64 is one group of units, which mlp_layer gives to wave 0 (waves 0 and 1 with two row tiles), so the two output
    // layers run side by side instead of one behind the other.  A row's sums do not depend on the wave that takes them.
    const int L = a.net.nlayers - 1;
    const float* xin = reg0;
    for (int l = 0; l < L; ++l) {
        float* xout = (l & 1) ? reg0 : reg1;
        mlp_layer<RT>(a.net.W[l], a.net.b[l], a.net.dims[l], a.net.dims[l + 1], a.net.act, false, xin, xout, nullptr, wave, lane);
        __syncthreads();
        xin = xout;
    }
    float* mur = (L & 1) ? reg0 : reg1;
    mlp_layer<RT>(a.net.W[L], a.net.b[L], a.net.dims[L], A, MLP_ACT_NONE, false, xin, mur, nullptr, wave, lane);
    mlp_layer<RT>(a.Wls, a.bls, a.net.dims[L], A, MLP_ACT_NONE, false, xin, lsr, nullptr, wave ^ 2, lane);
    __syncthreads();
    const float hw = __fmul_rn(0.5f, __fsub_rn(a.hi, a.lo));
    for (int idx = tid; idx < rows * A; idx += MLP_THREADS) {
        const int row = idx / A, d = idx - row * A;
        const size_t q = q0 + row;
        const int at = d * R + mlp_swz<RT>(row, d);
        float v;
        if (bad[row]) {
            v = 0.0f;
        } else {
            float u = mur[at];
            if (a.std_scale > 0.0f && q % a.P != 0) {
                const float sc = __fmul_rn(a.std_scale, expf(gauss_log_std(lsr[at], a.bound, a.lo, a.hi, hw)));
                u = __fadd_rn(u, __fmul_rn(sc, gauss_xi((uint32_t)q, a.t, d, CADM_STREAM_POLICY, a.seed, a.call)));
            }
            v = mlp_squash(u, a.squash, a.mid, a.half);
        }
        v = fminf(fmaxf(v, a.lb), a.ub);
        if (a.seqs) a.seqs[(q * a.H + a.t) * A + d] = v;
        a.a1[q * A + d] = v;
    }
}

// LDS of a workgroup with RT row tiles: policy.hip's two activation regions (the mean's A sums in one of them), the log-std's A sums, the flags
size_t gauss_lds_bytes(const int* dims, int nlayers, int RT, int* region0, int* region1) {
    const size_t A4 = (size_t)((dims[nlayers] + 3) & ~3);
    return (mlp_region_floats(dims, nlayers + 1, RT, region0, region1) + 16 * (size_t)RT * A4 + 16 * (size_t)RT) * sizeof(float);
}

bool gauss_bounds_ok(float lo, float hi) { return isfinite(lo) && isfinite(hi) && lo < hi && hi <= 10.0f; }

// the registered net's description out of its kernel arguments, for cadm_policy_check
void gauss_policy_params(const MlpDev& d, int squash, cadm_policy_params* p) {
    *p = cadm_policy_params{};
    p->n_hidden = d.nlayers - 1;
    for (int l = 0; l < p->n_hidden; ++l) p->hidden[l] = d.dims[1 + l];
    p->activation = d.act; p->squash = squash; p->n_samples = 1; p->noise_std = 0.0f;
}

// what every entry point asks of the ctx's state: a registered net (CADM_ESTATE), and with need_head a head on it (CADM_ESTATE); then
// what cadm_policy_check refuses, lb < ub, and the kernel's LDS at one row tile
int gauss_ready(const cadm_ctx* ctx, bool need_head, MlpDev* d, int* squash, const char* who) {
    if (!cadm_policy_dev(ctx, d, squash)) { cadm_set_error("%s: no policy net is registered (call cadm_set_policy_net)", who); return CADM_ESTATE; }
    if (need_head && !(ctx->policy_head && ctx->policy_head->set)) {
        cadm_set_error("%s: the registered policy net has no Gaussian head (call cadm_set_policy_head)", who);
        return CADM_ESTATE;
    }
    cadm_policy_params p;
    gauss_policy_params(*d, *squash, &p);
    int rc;
    if ((rc = cadm_policy_check(ctx, &p, who))) return rc;
    CADM_REQUIRE(ctx->cfg.lower_bound < ctx->cfg.upper_bound, "%s: the action bounds [%g, %g] leave no range (half > 0 is required)", who,
                 (double)ctx->cfg.lower_bound, (double)ctx->cfg.upper_bound);
    const size_t lds = gauss_lds_bytes(d->dims, d->nlayers, 1, nullptr, nullptr);
    CADM_REQUIRE(lds <= (size_t)MLP_LDS_MAX, "%s: the sampling kernel's activation tiles need %zu bytes of LDS at one row tile, the bound is %d",
                 who, lds, MLP_LDS_MAX);
    return CADM_OK;
}

// one launch over `total` rows x [total, D] whose Philox rows are row0 + 0 .. total - 1 (checked by the callers)
int gauss_launch(cadm_ctx* ctx, const MlpDev& net, int squash, const float* x, size_t total, uint32_t row0, int t, uint32_t seed, uint32_t call,
                 float* act, float* logp, float* mode, hipStream_t s, const char* who) {
    const PolicyHead& h = *ctx->policy_head;
    GaussArgs a{};
    a.net = net; a.squash = squash;
    a.Wls = h.net.W[0]; a.bls = h.net.b[0];
    a.x = x; a.bound = h.prm.bound; a.t = t;
    a.lb = ctx->cfg.lower_bound; a.ub = ctx->cfg.upper_bound;
    a.mid = 0.5f * (a.ub + a.lb); a.half = 0.5f * (a.ub - a.lb);
    a.lo = h.prm.log_std_min; a.hi = h.prm.log_std_max;
    a.seed = seed; a.call = call; a.row0 = row0;
    a.act = act; a.logp = logp; a.mode = mode; a.total = total;
    // two row tiles where the rows are many (mlp_many_tiles) and their LDS fits; else one: policy_launch's rule
    int RT = mlp_many_tiles(ctx, total) ? 2 : 1;
    size_t lds = gauss_lds_bytes(a.net.dims, a.net.nlayers, RT, &a.region0, &a.region1);
    if (lds > (size_t)MLP_LDS_MAX) { RT = 1; lds = gauss_lds_bytes(a.net.dims, a.net.nlayers, RT, &a.region0, &a.region1); }
    return mlp_launch(ctx, policy_gauss_kernel<1>, policy_gauss_kernel<2>, RT, lds, total, a, s, who);
}

}  // namespace

void cadm_policy_head_drop(cadm_ctx* ctx) { if (ctx->policy_head) ctx->policy_head->set = false; }

void cadm_policy_head_free(cadm_ctx* ctx) {
    if (!ctx->policy_head) return;
    mlp_net_release(&ctx->policy_head->net);
    delete ctx->policy_head;
    ctx->policy_head = nullptr;
}

// policy_logp.hip's view of the head: false while the registered net has none; else the packed layer and its description, where asked for
bool cadm_policy_head_dev(const cadm_ctx* ctx, const float** W_ls, const float** b_ls, cadm_policy_head_params* prm) {
    if (!(ctx->policy_head && ctx->policy_head->set)) return false;
    if (W_ls) *W_ls = ctx->policy_head->net.W[0];
    if (b_ls) *b_ls = ctx->policy_head->net.b[0];
    if (prm) *prm = ctx->policy_head->prm;
    return true;
}

// imagine.hip's sampled step: the refusals (CADM_ESTATE without a net or a head), before any HIP call ..
int cadm_policy_gauss_check(const cadm_ctx* ctx, const char* who) {
    MlpDev d;
    int squash;
    return gauss_ready(ctx, true, &d, &squash, who);
}

// .. and the launch on states x [total, D], rows 0 .. total - 1: a1 [total, A] the sampled action, logp [total]
int cadm_launch_policy_gauss_step(cadm_ctx* ctx, const float* x, size_t total, int t, uint32_t seed, uint32_t call, float* a1, float* logp,
                                  hipStream_t s, const char* who) {
    MlpDev d;
    int squash, rc;
    if ((rc = gauss_ready(ctx, true, &d, &squash, who))) return rc;
    CADM_REQUIRE(total <= 0xffffffffull, "%s: %zu rows are too many for one launch", who, total);      // (xi's Philox counter takes the row)
    return gauss_launch(ctx, d, squash, x, total, 0u, t, seed, call, a1, logp, nullptr, s, who);
}

// policy.hip's plan check under CADM_PROPOSE_HEAD, behind its own refusals and before any HIP call: one source per call, lb < ub (ahead
// of the head's check: no head can be set on a ctx without a range), then what every sampling entry point asks of the ctx
int cadm_policy_proposals_check(const cadm_ctx* ctx, const cadm_policy_params* p, const char* who) {
    if (ctx->propose_source != CADM_PROPOSE_HEAD) return CADM_OK;
    CADM_REQUIRE(!(p->noise_std > 0.0f), "%s: the proposals are drawn from the head (cadm_set_policy_proposals) and noise_std is %g: one source "
                 "of proposals per call", who, (double)p->noise_std);
    CADM_REQUIRE(ctx->cfg.lower_bound < ctx->cfg.upper_bound, "%s: the action bounds [%g, %g] leave no range (half > 0 is required)", who,
                 (double)ctx->cfg.lower_bound, (double)ctx->cfg.upper_bound);
    MlpDev d;
    int squash;
    return gauss_ready(ctx, true, &d, &squash, who);
}

// .. and ONE policy step of the roll under it (policy.hip's policy_launch with the head's draws): obs [m, D] (t == 0) or x [total, p, D];
// seqs [total, H, A] or null; a1 [total, A]; states or null.  The caller has passed cadm_policy_proposals_check.
int cadm_launch_policy_gauss_roll(cadm_ctx* ctx, const float* obs, const float* x, int P, int p, int t, uint32_t seed, uint32_t call, float* seqs,
                                  float* a1, float* states, size_t total, hipStream_t s, const char* who) {
    const PolicyHead& h = *ctx->policy_head;
    GaussRollArgs a{};
    cadm_policy_dev(ctx, &a.net, &a.squash);
    a.Wls = h.net.W[0]; a.bls = h.net.b[0];
    a.obs = obs; a.x = x; a.bound = h.prm.bound; a.P = P; a.p = p; a.t = t; a.H = ctx->H;
    a.lb = ctx->cfg.lower_bound; a.ub = ctx->cfg.upper_bound;
    a.mid = 0.5f * (a.ub + a.lb); a.half = 0.5f * (a.ub - a.lb);
    a.lo = h.prm.log_std_min; a.hi = h.prm.log_std_max; a.std_scale = ctx->propose_scale;
    a.seed = seed; a.call = call;
    a.seqs = seqs; a.a1 = a1; a.states = states; a.total = total;
    // two row tiles where the rows are many (mlp_many_tiles) and their LDS fits; else one: gauss_launch's rule
    int RT = mlp_many_tiles(ctx, total) ? 2 : 1;
    size_t lds = gauss_lds_bytes(a.net.dims, a.net.nlayers, RT, &a.region0, &a.region1);
    if (lds > (size_t)MLP_LDS_MAX) { RT = 1; lds = gauss_lds_bytes(a.net.dims, a.net.nlayers, RT, &a.region0, &a.region1); }
    CADM_REQUIRE(total <= 0xffffffffull, "%s: %zu rows are too many for one launch", who, total);      // (xi's Philox counter takes the row)
    return mlp_launch(ctx, policy_gauss_roll_kernel<1>, policy_gauss_roll_kernel<2>, RT, lds, total, a, s, who);
}

extern "C" int cadm_set_policy_proposals(cadm_ctx* ctx, int32_t source, float std_scale) {
    const char* who = "cadm_set_policy_proposals";
    CADM_REQUIRE(ctx, "%s: ctx is null", who);
    CADM_REQUIRE(source == CADM_PROPOSE_NOISE || source == CADM_PROPOSE_HEAD, "%s: unknown source of proposals %d", who, source);
    CADM_REQUIRE(isfinite(std_scale) && std_scale >= 0.0f, "%s: the std_scale %g is negative or not finite", who, (double)std_scale);
    ctx->propose_source = source;
    ctx->propose_scale = std_scale;
    return CADM_OK;
}

extern "C" int cadm_set_policy_head(cadm_ctx* ctx, const cadm_policy_head_params* params, const float* W_ls, const float* b_ls, void* stream) {
    const char* who = "cadm_set_policy_head";
    CADM_REQUIRE(ctx, "%s: ctx is null", who);
    if (!params) { cadm_policy_head_drop(ctx); return CADM_OK; }
    CADM_REQUIRE(W_ls && b_ls, "%s: W_ls / b_ls is null", who);
    CADM_REQUIRE(params->kind == CADM_HEAD_GAUSSIAN, "%s: unknown head kind %d", who, params->kind);
    CADM_REQUIRE(params->bound == CADM_LOGSTD_CLAMP || params->bound == CADM_LOGSTD_TANH, "%s: unknown log-std bound %d", who, params->bound);
    CADM_REQUIRE(gauss_bounds_ok(params->log_std_min, params->log_std_max),
                 "%s: the log-std bounds (%g, %g) must be finite with min < max <= 10 (expf must stay finite)", who,
                 (double)params->log_std_min, (double)params->log_std_max);
    MlpDev d;
    int squash, rc;
    if ((rc = gauss_ready(ctx, false, &d, &squash, who))) return rc;
    CADM_ON_DEVICE(ctx);
    if (!ctx->policy_head) {
        ctx->policy_head = new (std::nothrow) PolicyHead();
        if (!ctx->policy_head) { cadm_set_error("%s: out of host memory", who); return CADM_ENOMEM; }
    }
    PolicyHead& h = *ctx->policy_head;
    h.set = false;
    const int K = d.dims[d.nlayers - 1], A = d.dims[d.nlayers];
    const size_t wf = mlp_w_floats(K, A), need = wf + mlp_b_floats(A);
    if (need > h.net.cap) {
        if (h.net.buf) CADM_CHECK_HIP(hipFree(h.net.buf));      // (waits for every launch that still reads the old copy)
        h.net.buf = nullptr; h.net.cap = 0;
        if (hipMalloc(&h.net.buf, need * sizeof(float)) != hipSuccess) { cadm_set_error("%s: hipMalloc failed", who); return CADM_ENOMEM; }
        h.net.cap = need;
    }
    h.net.W[0] = h.net.buf;
    h.net.b[0] = h.net.buf + wf;
    const size_t g = (wf + 255) / 256;
    hipLaunchKernelGGL(mlp_pack_kernel, dim3((unsigned)(g > 1024 ? 1024 : g)), dim3(256), 0, (hipStream_t)stream, W_ls, b_ls, K, A, h.net.W[0],
                       h.net.b[0]);
    CADM_CHECK_HIP(hipGetLastError());
    h.prm = *params;
    h.set = true;
    return CADM_OK;
}

extern "C" int cadm_policy_sample(cadm_ctx* ctx, const float* states, int R, uint32_t row0, int t, uint32_t seed, uint32_t call, float* act_out,
                                  float* logp_out, float* mode_out, void* stream) {
    const char* who = "cadm_policy_sample";
    CADM_REQUIRE(ctx && states && act_out && logp_out, "%s: ctx / states / act_out / logp_out is null", who);
    CADM_REQUIRE(R >= 1, "%s: R must be >= 1 (got %d)", who, R);
    CADM_REQUIRE(t >= 0, "%s: t must be >= 0 (got %d)", who, t);
    CADM_REQUIRE((uint64_t)row0 + (uint64_t)R <= (1ull << 32), "%s: row0 + R = %llu is beyond the 2^32 rows of the Philox counter", who,
                 (unsigned long long)row0 + (unsigned long long)R);
    MlpDev d;
    int squash, rc;
    if ((rc = gauss_ready(ctx, true, &d, &squash, who))) return rc;
    CADM_ON_DEVICE(ctx);
    return gauss_launch(ctx, d, squash, states, (size_t)R, row0, t, seed, call, act_out, logp_out, mode_out, (hipStream_t)stream, who);
}
