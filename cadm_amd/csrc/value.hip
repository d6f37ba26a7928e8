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
// Mapping: a workgroup of 4 waves owns 16 * RT consecutive rows (RT = 1 or 2) and takes them through every layer.  A layer's 64-unit
// groups go to the waves (all row tiles each, so a weight fragment is used RT times); with fewer groups than waves the (group, row tile)
// pairs do (mlp_chain.h, shared with reward.hip).  The weights are a ctx-owned packed copy (mlp_pack_kernel): per layer [group of 64 units][k-step][lane][4], so that the A
// operands of FOUR 16-unit tiles (tile t = units {64 g + 4 i + t}) are one 16-byte load per lane and a wave's k-step is 1 KiB contiguous;
// K is zero-padded to 4 and the units to 64 there, the biases to 64.  Activation units behind N up to the next multiple of 4 are
// written as exact zeros, rows behind the batch compute on zeros and store nothing.  Rows are the B / D columns of the MFMAs: a value
// of one row never meets a value of another.
// Reduction contract: a row's V is one column's chain in ascending k, the same instruction sequence wherever the row sits; no
// floating-point atomics; nothing depends on the grid, on RT, on m or n: the same bits run to run, inside any batch, and from
// cadm_value_eval as from the planner stage.
#include "mlp_chain.h"

namespace {

struct ValueArgs {
    const float* W[MLP_NL];        // packed, per layer
    const float* b[MLP_NL];        // padded to 64 units
    int dims[MLP_NL + 1];          // D, h_1 .. h_L, 1
    int nlayers;                   // dense layers including the output
    int act;
    const float *mean, *istd;      // [D]
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
    const int D = a.dims[0], D4 = (D + 3) & ~3;
    for (int idx = tid; idx < R * D4; idx += MLP_THREADS) {
        const int row = idx / D4, k = idx - row * D4;
        float x = 0.0f;
        if (k < D && flag[row] == 0) {
            const float v = a.x[(q0 + row) * D + k];
            if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) bad[row] = 1;      // (every writer stores the same 1)
            x = (v - a.mean[k]) * a.istd[k];
        }
        reg0[k * R + mlp_swz<RT>(row, k)] = x;
    }
    __syncthreads();
    const float* xin = reg0;
    for (int l = 0; l < a.nlayers; ++l) {
        float* xout = (l & 1) ? reg0 : reg1;
        mlp_layer<RT>(a.W[l], a.b[l], a.dims[l], a.dims[l + 1], a.act, l + 1 == a.nlayers, xin, xout, vres, wave, lane);
        __syncthreads();
        xin = xout;
    }
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

void value_dims(const cadm_ctx* ctx, const cadm_value_params* p, int* dims) {
    dims[0] = ctx->D;
    for (int l = 0; l < p->n_hidden; ++l) dims[1 + l] = p->hidden[l];
    dims[1 + p->n_hidden] = 1;
}

}  // namespace

// the ctx-owned packed copy of the registered net
struct ValueNet : MlpNet {
    cadm_value_params prm{};       // what was registered (its weight is not used: every call brings its own)
};

void cadm_value_free(cadm_ctx* ctx) {
    if (!ctx->value) return;
    mlp_net_release(ctx->value);
    delete ctx->value;
    ctx->value = nullptr;
}

// the refusals of a value net's description, before any HIP call
int cadm_value_check(const cadm_ctx* ctx, const cadm_value_params* p, const char* who) {
    CADM_REQUIRE(p, "%s: the value parameters are null", who);
    CADM_REQUIRE(p->n_hidden >= 0 && p->n_hidden <= CADM_MAX_VALUE_LAYERS, "%s: %d hidden layers, outside 0 .. %d", who, p->n_hidden,
                 CADM_MAX_VALUE_LAYERS);
    for (int l = 0; l < p->n_hidden; ++l)
        CADM_REQUIRE(p->hidden[l] >= 1 && p->hidden[l] <= CADM_MAX_VALUE_WIDTH, "%s: hidden layer %d has width %d, outside 1 .. %d", who, l,
                     p->hidden[l], CADM_MAX_VALUE_WIDTH);
    CADM_REQUIRE(p->activation == CADM_VALUE_RELU || p->activation == CADM_VALUE_TANH || p->activation == CADM_VALUE_SWISH,
                 "%s: unknown value activation %d", who, p->activation);
    CADM_REQUIRE(isfinite(p->weight), "%s: the value weight %g is not finite", who, (double)p->weight);
    CADM_REQUIRE(ctx->D <= CADM_MAX_VALUE_DIMS, "%s: D (%d) is beyond the value net's %d input dims", who, ctx->D, CADM_MAX_VALUE_DIMS);
    CADM_REQUIRE(!ctx->cfg.discrete && ctx->cfg.env_kind != CADM_ENV_CARTPOLE, "%s: a terminal value needs a continuous-action ctx (discrete "
                 "actions are planned by random shooting)", who);
    CADM_REQUIRE(!cadm_sharded(ctx), "%s: a terminal value is not supported on a candidate-sharded ctx", who);
    int dims[MLP_NL + 1];
    value_dims(ctx, p, dims);
    const size_t lds = value_lds_bytes(dims, p->n_hidden + 1, 1, nullptr, nullptr);
    CADM_REQUIRE(lds <= (size_t)MLP_LDS_MAX, "%s: the value net's activation tiles need %zu bytes of LDS at one row tile, the bound is %d", who,
                 lds, MLP_LDS_MAX);
    return CADM_OK;
}

// `p` must describe the registered net
static int value_match(const cadm_ctx* ctx, const cadm_value_params* p, const char* who) {
    if (!ctx->value || !ctx->value->set) { cadm_set_error("%s: no value net is registered (call cadm_set_value_net)", who); return CADM_ESTATE; }
    const cadm_value_params& r = ctx->value->prm;
    bool same = p->n_hidden == r.n_hidden && p->activation == r.activation;
    for (int l = 0; same && l < p->n_hidden; ++l) same = p->hidden[l] == r.hidden[l];
    CADM_REQUIRE(same, "%s: the value parameters do not describe the registered net (layers, widths or activation differ)", who);
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
    value_dims(ctx, &net.prm, a.dims);
    a.nlayers = net.prm.n_hidden + 1;
    a.act = net.prm.activation;
    for (int l = 0; l < a.nlayers; ++l) { a.W[l] = net.W[l]; a.b[l] = net.b[l]; }
    a.mean = net.mean; a.istd = net.istd;
    a.x = x; a.first = first; a.H = ctx->H; a.rows_in = rows_in; a.rows_out = rows_out; a.v_out = v_out; a.weight = weight; a.total = total;
    // two row tiles halve the weight stream per row; one tile keeps every CU busy while the rows are few
    int RT = (total + 15) / 16 > 2 * (size_t)ctx->n_cus ? 2 : 1;
    size_t lds = value_lds_bytes(a.dims, a.nlayers, RT, &a.region0, &a.region1);
    if (lds > (size_t)MLP_LDS_MAX) { RT = 1; lds = value_lds_bytes(a.dims, a.nlayers, RT, &a.region0, &a.region1); }
    const size_t R = 16 * (size_t)RT, blocks = (total + R - 1) / R;
    CADM_REQUIRE(blocks <= 0x7fffffffull, "%s: %zu rows are too many for one launch", who, total);
    const void* fn = RT == 2 ? reinterpret_cast<const void*>(&value_kernel<2>) : reinterpret_cast<const void*>(&value_kernel<1>);
    if (lds > 64 * 1024 && !ctx->attr_done.count(fn)) {
        CADM_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, MLP_LDS_MAX));
        ctx->attr_done.insert(fn);
    }
    if (RT == 2) hipLaunchKernelGGL(value_kernel<2>, dim3((unsigned)blocks), dim3(MLP_THREADS), lds, s, a);
    else hipLaunchKernelGGL(value_kernel<1>, dim3((unsigned)blocks), dim3(MLP_THREADS), lds, s, a);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

// the planner's stage: rows [m, n, p] in place, behind a rollout's traj [H, m, n, p, D] (n the PACKED candidate count)
int cadm_launch_value(cadm_ctx* ctx, const cadm_value_params* p, const float* traj, const int32_t* first, int m, int n, float* rows,
                      hipStream_t s) {
    const size_t total = (size_t)m * n * ctx->p;
    return value_launch(ctx, cadm_discounted_weight(ctx, p->weight), traj + (size_t)(ctx->H - 1) * total * ctx->D, first, total, rows, rows, nullptr, s, "cadm_valued_plan");
}

extern "C" int cadm_set_value_net(cadm_ctx* ctx, const cadm_value_params* params, const float* const* W, const float* const* b,
                                  const float* mean, const float* std_inv, void* stream) {
    CADM_REQUIRE(ctx, "cadm_set_value_net: ctx is null");
    if (!params) {
        if (ctx->value) ctx->value->set = false;
        return CADM_OK;
    }
    int rc;
    if ((rc = cadm_value_check(ctx, params, "cadm_set_value_net"))) return rc;
    CADM_REQUIRE(W && b && mean && std_inv, "cadm_set_value_net: W / b / mean / std_inv is null");
    const int nl = params->n_hidden + 1;
    for (int l = 0; l < nl; ++l) CADM_REQUIRE(W[l] && b[l], "cadm_set_value_net: the weights or the biases of layer %d are null", l);
    int dims[MLP_NL + 1];
    value_dims(ctx, params, dims);
    CADM_ON_DEVICE(ctx);
    if (!ctx->value) {
        ctx->value = new (std::nothrow) ValueNet();
        if (!ctx->value) { cadm_set_error("cadm_set_value_net: out of host memory"); return CADM_ENOMEM; }
    }
    ValueNet& net = *ctx->value;
    if ((rc = mlp_net_upload(net, dims, nl, W, b, mean, std_inv, (hipStream_t)stream, "cadm_set_value_net"))) return rc;
    net.prm = *params;
    return CADM_OK;
}

extern "C" int cadm_value_eval(cadm_ctx* ctx, const float* states, int R, float* v_out, void* stream) {
    CADM_REQUIRE(ctx && states && v_out, "cadm_value_eval: ctx / states / v_out is null");
    CADM_REQUIRE(R >= 1, "cadm_value_eval: R must be >= 1 (got %d)", R);
    if (!ctx->value || !ctx->value->set) { cadm_set_error("cadm_value_eval: no value net is registered (call cadm_set_value_net)"); return CADM_ESTATE; }
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
