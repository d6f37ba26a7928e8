// Terminal value of the opt-in planner loop (icem.hip): a caller-supplied value net V, an MLP D -> h_1 -> .. -> h_L -> 1, evaluated on
// the LAST state of every particle's trajectory and added to the particle's return: rows' = rows + weight * V(s_H).  No reference twin:
// the reference's planner scores the H step rewards and nothing else.  One kernel BEHIND the rollout, like the constraints
// (constrain.hip) and the tracking terms (tracking.hip); the rollout kernels are not touched.  Unlike those it is not a per-row scan of
// `traj` but a GEMM chain over thousands of rows, so it runs on the fp32 matrix pipe, in the pattern of context_batched_kernel
// (context.hip): transposed evaluation, activations resident in LDS as [unit][row], weights through a register ring.
//
// Arithmetic of one row (all fp32, nothing fused but the MFMA's own multiply-add):
//   x_k = (s_k - mean_k) * inv_std_k                       k = 0 .. D-1 (one subtract, one multiply)
//   a layer with K inputs:  acc = b_u;  for k = 0 .. K4-1 ascending: acc = fma(W[k][u], x_k, acc)      K4 = K rounded up to 4
//   (v_mfma_f32_16x16x4_f32 adds its 4 products in ascending k onto the accumulator, as context.hip relies on; the bias SEEDS the
//   accumulator; for K <= k < K4 both W and x are exact zeros)
//   hidden: relu max(z, 0), tanhf(z), or swish z / (1 + expf(-z));  output: linear.
//   rows' = rows + weight * V: one multiply, then one add.  On a ctx with a discount over the horizon (cadm_set_discount, discount.hip)
//   the launcher passes weight * disc[H], one fp32 product on the host; the kernel is the same.
// A row whose terminal state holds a non-finite value gets V = NaN explicitly (relu would otherwise hide it) and so a NaN return.  With
// `first` (the constraint kernel's first_violation) a row with first < H keeps its input bits, its V reads NaN, and its terminal
// state is not loaded.
//
// Mapping, packed weights and the host path (description checks, registration, launch): mlp_chain.h.  A workgroup of 4 waves owns
// 16 * RT consecutive rows (RT = 1 or 2) and takes them through every layer; rows behind the batch compute on zeros and store nothing.
// Rows are the B / D columns of the MFMAs: a value of one row never meets a value of another.
// Reduction contract: a row's V is one column's chain in ascending k, the same instruction sequence wherever the row sits; no
// floating-point atomics; nothing depends on the grid, on RT, on m or n: the same bits run to run, inside any batch, and from
// cadm_value_eval as from the planner stage.
#include "mlp_chain.h"

namespace {

struct ValueArgs {
    MlpDev net;                    // D -> h_1 .. h_L -> 1
    const float* x;                // [total, D] row-major states
    const int32_t* first;          // [total] or null
    int H;
    const float* rows_in;          // [total] or null (cadm_value_eval)
    float *rows_out, *v_out;       // [total] or null each
    float weight;
    size_t total;
    int region0, region1;          // LDS floats of the two activation regions
};

template <int RT>
__global__ __launch_bounds__(MLP_THREADS) void value_kernel(const ValueArgs a) {
    extern __shared__ __attribute__((aligned(16))) float val_smem[];
    constexpr int R = 16 * RT;
    float* reg0 = val_smem;
    float* reg1 = reg0 + a.region0;
    float* vres = reg1 + a.region1;                              // [R] the output layer's sums
    int* flag = reinterpret_cast<int*>(vres + R);                // [R] 0: a row to evaluate, 1: cut by `first`, 2: behind the batch
    int* bad = flag + R;                                         // [R] 1: a non-finite value in the terminal state
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t q0 = (size_t)blockIdx.x * R;                    // (q0 < total: the grid is ceil(total / R))
    const int rows = a.total - q0 < (size_t)R ? (int)(a.total - q0) : R;
    if (tid < R) {
        flag[tid] = tid >= rows ? 2 : (a.first && a.first[q0 + tid] < a.H) ? 1 : 0;
        bad[tid] = 0;
    }
    __syncthreads();
    // the input tile [k][row], normalised on the way in; rows that are not evaluated and the k behind D are zeros
    const int D = a.net.dims[0], D4 = (D + 3) & ~3;
    for (int idx = tid; idx < R * D4; idx += MLP_THREADS) {
        const int row = idx / D4, k = idx - row * D4;
        float x = 0.0f;
        if (k < D && flag[row] == 0) {
            const float v = a.x[(q0 + row) * D + k];
            if (mlp_nonfinite(v)) bad[row] = 1;                  // (every writer stores the same 1)
            x = (v - a.net.mean[k]) * a.net.istd[k];
        }
        reg0[k * R + mlp_swz<RT>(row, k)] = x;
    }
    __syncthreads();
    mlp_forward<RT>(a.net, true, reg0, reg1, reg0, vres, wave, lane);
    if (tid >= rows) return;
    const size_t q = q0 + tid;
    const float nan = __uint_as_float(0x7fc00000u);
    const bool cut = flag[tid] == 1;
    const float v = (cut || bad[tid]) ? nan : vres[tid];
    if (a.v_out) a.v_out[q] = v;
    if (a.rows_out) {
        const float r_in = a.rows_in[q];
        const float wv = __fmul_rn(a.weight, v);                 // (one multiply, then one add: never an fma)
        a.rows_out[q] = cut ? r_in : __fadd_rn(r_in, wv);
    }
}

// LDS of a workgroup with RT row tiles: region 0 (the input tile, later the outputs of the odd layers), region 1 (the outputs of the even
// layers), the output sums and the two flag arrays
size_t value_lds_bytes(const int* dims, int nlayers, int RT, int* region0, int* region1) {
    return (mlp_region_floats(dims, nlayers, RT, region0, region1) + 3 * 16 * (size_t)RT) * sizeof(float);
}

}  // namespace

// the ctx-owned packed copy of the registered net (the weight of its prm is not used: every call brings its own)
struct ValueNet : MlpOwned<cadm_value_params> {};

void cadm_value_free(cadm_ctx* ctx) { mlp_free(ctx->value); }

// the refusals of a value net's description, before any HIP call
int cadm_value_check(const cadm_ctx* ctx, const cadm_value_params* p, const char* who) {
    int rc;
    if ((rc = mlp_shape_check(mlp_shape(p), "value", who))) return rc;
    CADM_REQUIRE(isfinite(p->weight), "%s: the value weight %g is not finite", who, (double)p->weight);
    CADM_REQUIRE(ctx->D <= CADM_MAX_VALUE_DIMS, "%s: D (%d) is beyond the value net's %d input dims", who, ctx->D, CADM_MAX_VALUE_DIMS);
    if ((rc = mlp_ctx_check(ctx, "a terminal value", who))) return rc;
    int dims[MLP_NL + 1];
    mlp_dims(mlp_shape(p), ctx->D, 1, dims);
    const size_t lds = value_lds_bytes(dims, p->n_hidden + 1, 1, nullptr, nullptr);
    CADM_REQUIRE(lds <= (size_t)MLP_LDS_MAX, "%s: the value net's activation tiles need %zu bytes of LDS at one row tile, the bound is %d", who,
                 lds, MLP_LDS_MAX);
    return CADM_OK;
}

// `p` must describe the registered net
static int value_match(const cadm_ctx* ctx, const cadm_value_params* p, const char* who) {
    if (!mlp_registered(ctx->value)) { cadm_set_error("%s: no value net is registered (call cadm_set_value_net)", who); return CADM_ESTATE; }
    CADM_REQUIRE(mlp_shape_same(mlp_shape(p), mlp_shape(&ctx->value->prm)), "%s: the value parameters do not describe the registered net (layers, widths or activation differ)", who);
    return CADM_OK;
}

int cadm_value_plan_check(const cadm_ctx* ctx, const cadm_value_params* p, const char* who) {
    int rc;
    if ((rc = cadm_value_check(ctx, p, who))) return rc;
    return value_match(ctx, p, who);
}

// x [total, D]; first [total] or null; rows_in / rows_out [total] or both null; v_out [total] or null
static int value_launch(cadm_ctx* ctx, float weight, const float* x, const int32_t* first, size_t total, const float* rows_in, float* rows_out,
                        float* v_out, hipStream_t s, const char* who) {
    const ValueNet& net = *ctx->value;
    ValueArgs a{};
    mlp_dev(a.net, net.net[0], mlp_shape(&net.prm), ctx->D, 1);
    a.x = x; a.first = first; a.H = ctx->H; a.rows_in = rows_in; a.rows_out = rows_out; a.v_out = v_out; a.weight = weight; a.total = total;
    // two row tiles where the rows are many (mlp_many_tiles) and their LDS fits; else one
    int RT = mlp_many_tiles(ctx, total) ? 2 : 1;
    size_t lds = value_lds_bytes(a.net.dims, a.net.nlayers, RT, &a.region0, &a.region1);
    if (lds > (size_t)MLP_LDS_MAX) { RT = 1; lds = value_lds_bytes(a.net.dims, a.net.nlayers, RT, &a.region0, &a.region1); }
    return mlp_launch(ctx, value_kernel<1>, value_kernel<2>, RT, lds, total, a, s, who);
}

// the planner's stage: rows [m, n, p] in place, behind a rollout's traj [H, m, n, p, D] (n the PACKED candidate count)
int cadm_launch_value(cadm_ctx* ctx, const cadm_value_params* p, const float* traj, const int32_t* first, int m, int n, float* rows,
                      hipStream_t s) {
    const size_t total = (size_t)m * n * ctx->p;
    return value_launch(ctx, cadm_discounted_weight(ctx, p->weight), traj + (size_t)(ctx->H - 1) * total * ctx->D, first, total, rows, rows, nullptr, s, "cadm_valued_plan");
}

extern "C" int cadm_set_value_net(cadm_ctx* ctx, const cadm_value_params* params, const float* const* W, const float* const* b,
                                  const float* mean, const float* std_inv, void* stream) {
    const char* who = "cadm_set_value_net";
    CADM_REQUIRE(ctx, "%s: ctx is null", who);
    if (!params) { mlp_clear(ctx->value); return CADM_OK; }
    int rc;
    if ((rc = cadm_value_check(ctx, params, who))) return rc;
    int dims[MLP_NL + 1];
    mlp_dims(mlp_shape(params), ctx->D, 1, dims);
    if ((rc = mlp_register(ctx, ctx->value, 1, nullptr, dims, params->n_hidden + 1, W, b, mean, std_inv, stream, who))) return rc;
    ctx->value->prm = *params;
    return CADM_OK;
}

extern "C" int cadm_value_eval(cadm_ctx* ctx, const float* states, int R, float* v_out, void* stream) {
    CADM_REQUIRE(ctx && states && v_out, "cadm_value_eval: ctx / states / v_out is null");
    CADM_REQUIRE(R >= 1, "cadm_value_eval: R must be >= 1 (got %d)", R);
    if (!mlp_registered(ctx->value)) { cadm_set_error("cadm_value_eval: no value net is registered (call cadm_set_value_net)"); return CADM_ESTATE; }
    CADM_ON_DEVICE(ctx);
    return value_launch(ctx, 0.0f, states, nullptr, (size_t)R, nullptr, nullptr, v_out, (hipStream_t)stream, "cadm_value_eval");
}

extern "C" int cadm_value_returns(cadm_ctx* ctx, const cadm_value_params* params, const float* traj, const int32_t* first, int m, int n,
                                  const float* rows_in, float* rows_out, float* v_out, void* stream) {
    CADM_REQUIRE(ctx && params && traj && rows_in && rows_out, "cadm_value_returns: ctx / params / traj / rows_in / rows_out is null");
    int rc;
    if ((rc = cadm_value_plan_check(ctx, params, "cadm_value_returns"))) return rc;
    CADM_REQUIRE(m >= 1 && n >= 1, "cadm_value_returns: m, n must be >= 1 (got m=%d n=%d)", m, n);
    CADM_ON_DEVICE(ctx);
    const size_t total = (size_t)m * n * ctx->p;
    return value_launch(ctx, cadm_discounted_weight(ctx, params->weight), traj + (size_t)(ctx->H - 1) * total * ctx->D, first, total, rows_in, rows_out, v_out,
                        (hipStream_t)stream, "cadm_value_returns");
}
