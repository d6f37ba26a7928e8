// What the caller-supplied nets of the opt-in planner share (value.hip: the terminal value; reward.hip: the learned step reward;
// policy.hip: the policy prior; critic.hip: the Q critics): an MLP K -> h_1 -> .. -> h_L -> N evaluated transposed on the fp32 matrix
// pipe -- activations resident in LDS as [unit][row], rows as the B / D columns of v_mfma_f32_16x16x4_f32, weights from a ctx-owned
// packed copy through a register ring -- the packed copy itself, and the host path around both.  Each of the four files is its own
// translation unit: everything here but the types has internal linkage.
//
// The host path, once for the four files:
//   description   mlp_shape() views the common prefix of the four parameter structs (n_hidden, hidden, activation); mlp_shape_check,
//                 mlp_ctx_check and mlp_shape_same are the refusals and the comparison every net has.  What a net has of its own
//                 (inputs, squash, n_critics, its LDS bound) and the ORDER of its refusals stay in its file.
//   registration  mlp_register: null checks, the ctx-owned MlpOwned on first use, the packed copies (mlp_net_upload).  `set` is false
//                 from the first upload until the last one is queued; mlp_clear / mlp_registered / mlp_free are the rest of its life.
//   launch        mlp_dev fills the net's half of a kernel's arguments (MlpDev); each file chooses its row tiles (mlp_many_tiles is
//                 the clause they share) and sizes its LDS; mlp_launch bounds the grid, raises the dynamic-LDS attribute above 64 KiB
//                 once per ctx, launches and asks for the launch error.
// On the device mlp_forward is the walk through the layers (critic.hip writes its two walks out and keeps its argument struct flat: with
// either shared, its kernel or its short launch changed: profiles/mlp_host_refactor.md);
// mlp_nonfinite and mlp_squash are what the prologues and the actor's epilogues share.
//
// Arithmetic of one row through one layer with K inputs (all fp32, nothing fused but the MFMA's own multiply-add):
//   acc = b_u;  for k = 0 .. K4-1 ascending: acc = fma(W[k][u], x_k, acc)      K4 = K rounded up to 4
//   (the MFMA adds its 4 products in ascending k onto the accumulator, as context.hip relies on; the bias SEEDS the accumulator; for
//   K <= k < K4 both W and x are exact zeros)
//   hidden: relu max(z, 0), tanhf(z), or swish z / (1 + expf(-z));  output: linear.
// An output layer of N > 1 units (policy.hip: the A action dims) runs as one more hidden-type layer whose activation is the identity
// MLP_ACT_NONE: its sums land in LDS as [unit][row] like any layer's outputs.  The N = 1 `last` path of the two nets above is as it was.
// A workgroup of 4 waves owns 16 * RT consecutive rows (RT = 1 or 2) and takes them through every layer.  A layer's 64-unit groups go
// to the waves (all row tiles each, so a weight fragment is used RT times); with fewer groups than waves the (group, row tile) pairs do.
// (Four row tiles were built and measured for reward.hip and lost to one and two at every width: see its header.)
// Packed weights: per layer [group of 64 units][k-step][lane][4], so that the A operands of FOUR 16-unit tiles (tile t = units {64 g + 4 i + t}) are one 16-byte load per lane and a wave's k-step is
// 1 KiB contiguous; K is zero-padded to 4 and the units to 64 there, the biases to 64.  Activation units behind N up to the next multiple
// of 4 are written as exact zeros.  With two row tiles the rows of odd k are stored with bit 4 flipped, so that the two k of a
// half-wave's B read fall into different banks.  A row's result is one column's chain in ascending k, the same instruction sequence
// wherever the row sits and whichever wave takes it: nothing depends on RT or on the grid.
#pragma once
#include <math.h>

#include "planner.h"

constexpr int MLP_THREADS = 256;
constexpr int MLP_WAVES = 4;
constexpr int MLP_PF = 6;                    // k-steps of weight fragments in flight per wave
constexpr int MLP_LDS_MAX = 160 * 1024;      // the CU's LDS; above 64 KiB a kernel's dynamic-LDS attribute is raised
constexpr int MLP_NL = CADM_MAX_VALUE_LAYERS + 1;
constexpr int MLP_ACT_NONE = 3;              // the identity: a linear output layer written to LDS (behind CADM_VALUE_RELU / _TANH / _SWISH)

// a ctx-owned packed copy of a registered net
struct MlpNet {
    float* buf = nullptr;          // one allocation: mean, inv_std, then per layer the packed weights and the padded biases
    size_t cap = 0;                // floats allocated
    float *mean = nullptr, *istd = nullptr;
    float* W[MLP_NL] = {};
    float* b[MLP_NL] = {};
};

// what a ctx owns of a registration: the packed copies of its N nets (one description, one set of input statistics) and the description
template <class Prm, int N = 1>
struct MlpOwned {
    bool set = false;
    MlpNet net[N];
    Prm prm{};                     // what was registered
};

// the net's half of a kernel's arguments
struct MlpDev {
    const float* W[MLP_NL];        // packed, per layer
    const float* b[MLP_NL];        // padded to 64 units
    int dims[MLP_NL + 1];          // K, h_1 .. h_L, N
    int nlayers;                   // dense layers including the output
    int act;
    const float *mean, *istd;      // [K]
};

// the common prefix of cadm_value_params, cadm_reward_params, cadm_policy_params and cadm_critic_params; hidden == null: null parameters
struct MlpShape {
    int n_hidden;
    const int32_t* hidden;
    int activation;
};

namespace {

template <class Prm>
MlpShape mlp_shape(const Prm* p) { return p ? MlpShape{p->n_hidden, p->hidden, p->activation} : MlpShape{0, nullptr, 0}; }

// where row `row` of input k sits inside its [k] line of 16 * RT rows
template <int RT>
__device__ __forceinline__ int mlp_swz(int row, int k) { return row ^ (RT == 2 ? 16 * (k & 1) : 0); }

__device__ __forceinline__ float mlp_act(float z, int act) {
    if (act == CADM_VALUE_RELU) return fmaxf(z, 0.0f);
    if (act == CADM_VALUE_TANH) return tanhf(z);
    if (act == MLP_ACT_NONE) return z;
    return z / (1.0f + expf(-z));
}

// One work item of a layer: NT tiles of 16 units of group g x NRT row tiles, the whole K.  The k loop is straight-line code: one ring
// slot consumed, one refilled, NRT LDS reads, NT * NRT MFMAs; everything it could branch on is a template parameter.
template <int RT, int NRT, int NT>
__device__ __forceinline__ void mlp_item(const float* __restrict__ Wg, const float* __restrict__ bias, int nsteps, int N, int act, bool last,
                                         const float* xin, float* xout, float* vres, int g, int rt0, int lane) {
    constexpr int R = 16 * RT;
    const int i = lane & 15, q = lane >> 4;
    floatx4 acc[NT][NRT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        floatx4 b4;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) b4[rr] = bias[g * 64 + 4 * (4 * q + rr) + t];
#pragma unroll
        for (int r = 0; r < NRT; ++r) acc[t][r] = b4;
    }
    // A operand of k-step s: row k = 4 s + q of W, units 64 g + 4 i + (0 .. 3)
    const floatx4* wp = reinterpret_cast<const floatx4*>(Wg) + lane;
    auto fetch = [&](int s) -> floatx4 { return wp[(size_t)s * 64]; };
    // B operand of k-step s for row tile r: X[k = 4 s + q][row = 16 (rt0 + r) + i]
    int boff[NRT];
#pragma unroll
    for (int r = 0; r < NRT; ++r) boff[r] = q * R + mlp_swz<RT>(16 * (rt0 + r) + i, q);      // (k & 1 == q & 1)
    constexpr int bstep = 4 * R;
    auto bread = [&](float (&bv)[NRT], int s) {
#pragma unroll
        for (int r = 0; r < NRT; ++r) bv[r] = xin[boff[r] + s * bstep];
    };
    auto mfmas = [&](const floatx4& av, const float (&bv)[NRT]) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < NRT; ++r) acc[t][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv[r], acc[t][r], 0, 0, 0);
    };
    floatx4 ring[MLP_PF];
#pragma unroll
    for (int u = 0; u < MLP_PF; ++u) ring[u] = fetch(u < nsteps ? u : nsteps - 1);
    int s0 = 0;
    for (; s0 + MLP_PF <= nsteps; s0 += MLP_PF) {
        float bv[MLP_PF][NRT];
#pragma unroll
        for (int u = 0; u < MLP_PF; ++u) bread(bv[u], s0 + u);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < MLP_PF; ++u) {
            mfmas(ring[u], bv[u]);
            const int sn = s0 + u + MLP_PF;
            ring[u] = fetch(sn < nsteps ? sn : nsteps - 1);      // (past the end: a re-read of the last step, never consumed)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int u = 0; u < MLP_PF - 1; ++u)                         // the last nsteps % PF steps are already in the ring
        if (s0 + u < nsteps) { float bv[NRT]; bread(bv, s0 + u); mfmas(ring[u], bv); }
    // D layout: lane (i -> data row, q), register rr -> unit 64 g + 4 (4 q + rr) + t
    const int N4 = (N + 3) & ~3;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int unit = g * 64 + 4 * (4 * q + rr) + t;
#pragma unroll
            for (int r = 0; r < NRT; ++r) {
                const float z = acc[t][r][rr];
                const int row = 16 * (rt0 + r) + i;
                if (last) { if (unit == 0) vres[row] = z; }
                else if (unit < N4) xout[unit * R + mlp_swz<RT>(row, unit)] = unit < N ? mlp_act(z, act) : 0.0f;
            }
        }
}

template <int RT>
__device__ __forceinline__ void mlp_layer(const float* __restrict__ W, const float* __restrict__ bias, int K, int N, int act, bool last,
                                          const float* xin, float* xout, float* vres, int wave, int lane) {
    const int NG = (N + 63) >> 6, nsteps = (K + 3) >> 2;
    const size_t gfl = (size_t)nsteps * 256;                     // packed floats of one group
    if (last) {                                                  // one unit: the first tile of group 0, a row tile per wave
        for (int rt0 = wave; rt0 < RT; rt0 += MLP_WAVES) mlp_item<RT, 1, 1>(W, bias, nsteps, N, act, true, xin, xout, vres, 0, rt0, lane);
    } else if (RT == 1 || NG >= MLP_WAVES) {                     // a wave takes whole groups, all row tiles
        for (int g = wave; g < NG; g += MLP_WAVES) mlp_item<RT, RT, 4>(W + g * gfl, bias, nsteps, N, act, false, xin, xout, vres, g, 0, lane);
    } else {                                                     // few groups: the row tiles of a group go to different waves
        for (int item = wave; item < NG * RT; item += MLP_WAVES) {
            const int g = item % NG, rt0 = item / NG;
            mlp_item<RT, 1, 4>(W + g * gfl, bias, nsteps, N, act, false, xin, xout, vres, g, rt0, lane);
        }
    }
}

// The net's layers over the input tile xin, their outputs alternating between reg1 and reg0; returns where the last layer's outputs are.
// last_is_scalar: the output layer is the one-unit `last` path into vres; else it is one more layer with the identity activation into LDS.
template <int RT>
__device__ __forceinline__ const float* mlp_forward(const MlpDev& d, bool last_is_scalar, float* reg0, float* reg1, const float* xin,
                                                    float* vres, int wave, int lane) {
    for (int l = 0; l < d.nlayers; ++l) {
        float* xout = (l & 1) ? reg0 : reg1;
        // (two calls, not one with selected arguments: under the constant a kernel passes one plain call is left, and the loop compiles
        // as if it stood in the kernel: profiles/mlp_host_refactor.md)
        if (last_is_scalar) mlp_layer<RT>(d.W[l], d.b[l], d.dims[l], d.dims[l + 1], d.act, l + 1 == d.nlayers, xin, xout, vres, wave, lane);
        else mlp_layer<RT>(d.W[l], d.b[l], d.dims[l], d.dims[l + 1], l + 1 == d.nlayers ? MLP_ACT_NONE : d.act, false, xin, xout, vres, wave, lane);
        __syncthreads();
        xin = xout;
    }
    return xin;
}

// Inf or NaN
__device__ __forceinline__ bool mlp_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// the actor's output z under its squash: mid + half * tanhf(z), one multiply, then one add: never an fma.  (The clip follows at the call
// site: the policy kernel's noise goes between the two.)
__device__ __forceinline__ float mlp_squash(float z, int squash, float mid, float half) {
    return squash == CADM_POLICY_TANH ? __fadd_rn(mid, __fmul_rn(half, tanhf(z))) : z;
}

// dst [NG][nsteps][64 lanes][4]: lane (i = lane & 15, q = lane >> 4), t -> W[k = 4 s + q][unit = 64 g + 4 i + t], 0 outside [K, N);
// bdst [NG * 64]: the biases, 0 behind N
__global__ void mlp_pack_kernel(const float* __restrict__ W, const float* __restrict__ b, int K, int N, float* __restrict__ dst,
                                float* __restrict__ bdst) {
    const int nsteps = (K + 3) >> 2, NG = (N + 63) >> 6;
    const size_t total = (size_t)NG * nsteps * 256;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(e & 3), lane = (int)((e >> 2) & 63);
        const size_t gs = e >> 8;
        const int s = (int)(gs % nsteps), g = (int)(gs / nsteps);
        const int k = 4 * s + (lane >> 4), unit = 64 * g + 4 * (lane & 15) + t;
        dst[e] = (k < K && unit < N) ? W[(size_t)k * N + unit] : 0.0f;
        if (e < (size_t)NG * 64) bdst[e] = e < (size_t)N ? b[e] : 0.0f;
    }
}

__global__ void mlp_copy_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, float* __restrict__ da, float* __restrict__ db) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { da[i] = a[i]; db[i] = b[i]; }
}

size_t mlp_w_floats(int K, int N) { return (size_t)((N + 63) >> 6) * ((K + 3) >> 2) * 256; }
size_t mlp_b_floats(int N) { return (size_t)((N + 63) >> 6) * 64; }

// LDS floats of a workgroup's two activation regions with RT row tiles: region 0 (the input tile, later the outputs of the odd layers)
// and region 1 (the outputs of the even layers); returns their sum
size_t mlp_region_floats(const int* dims, int nlayers, int RT, int* region0, int* region1) {
    const size_t R = 16 * (size_t)RT;
    size_t r0 = R * (size_t)((dims[0] + 3) & ~3), r1 = 0;
    for (int l = 0; l + 1 < nlayers; ++l) {
        const size_t need = R * (size_t)((dims[l + 1] + 3) & ~3);
        if (l & 1) r0 = need > r0 ? need : r0; else r1 = need > r1 ? need : r1;
    }
    if (region0) *region0 = (int)r0;
    if (region1) *region1 = (int)r1;
    return r0 + r1;
}

void mlp_net_release(MlpNet* net) {
    if (net && net->buf) (void)hipFree(net->buf);
}

// packs the net dims[0] -> .. -> dims[nl] (W[l] [in,out] row-major, b[l] [out], mean / std_inv [dims[0]]: device pointers) into memory
// `net` owns, on `s`; a net that fits the allocation it has allocates nothing
int mlp_net_upload(MlpNet& net, const int* dims, int nl, const float* const* W, const float* const* b, const float* mean, const float* std_inv,
                   hipStream_t s, const char* who) {
    const size_t K64 = (size_t)((dims[0] + 63) & ~63);
    size_t need = 2 * K64;
    for (int l = 0; l < nl; ++l) need += mlp_w_floats(dims[l], dims[l + 1]) + mlp_b_floats(dims[l + 1]);
    if (need > net.cap) {
        if (net.buf) CADM_CHECK_HIP(hipFree(net.buf));      // (waits for every launch that still reads the old copy)
        net.buf = nullptr; net.cap = 0;
        if (hipMalloc(&net.buf, need * sizeof(float)) != hipSuccess) { cadm_set_error("%s: hipMalloc failed", who); return CADM_ENOMEM; }
        net.cap = need;
    }
    float* q = net.buf;
    net.mean = q; q += K64;
    net.istd = q; q += K64;
    hipLaunchKernelGGL(mlp_copy_kernel, dim3((dims[0] + 127) / 128), dim3(128), 0, s, mean, std_inv, dims[0], net.mean, net.istd);
    CADM_CHECK_HIP(hipGetLastError());
    for (int l = 0; l < nl; ++l) {
        const size_t wf = mlp_w_floats(dims[l], dims[l + 1]);
        net.W[l] = q; q += wf;
        net.b[l] = q; q += mlp_b_floats(dims[l + 1]);
        const size_t g = (wf + 255) / 256;
        hipLaunchKernelGGL(mlp_pack_kernel, dim3((unsigned)(g > 1024 ? 1024 : g)), dim3(256), 0, s, W[l], b[l], dims[l], dims[l + 1], net.W[l],
                           net.b[l]);
        CADM_CHECK_HIP(hipGetLastError());
    }
    return CADM_OK;
}

// ---- the host path of a net ----

// the first refusals of every description
int mlp_shape_check(const MlpShape& v, const char* noun, const char* who) {
    CADM_REQUIRE(v.hidden, "%s: the %s parameters are null", who, noun);
    CADM_REQUIRE(v.n_hidden >= 0 && v.n_hidden <= CADM_MAX_VALUE_LAYERS, "%s: %d hidden layers, outside 0 .. %d", who, v.n_hidden,
                 CADM_MAX_VALUE_LAYERS);
    for (int l = 0; l < v.n_hidden; ++l)
        CADM_REQUIRE(v.hidden[l] >= 1 && v.hidden[l] <= CADM_MAX_VALUE_WIDTH, "%s: hidden layer %d has width %d, outside 1 .. %d", who, l,
                     v.hidden[l], CADM_MAX_VALUE_WIDTH);
    CADM_REQUIRE(v.activation == CADM_VALUE_RELU || v.activation == CADM_VALUE_TANH || v.activation == CADM_VALUE_SWISH,
                 "%s: unknown %s activation %d", who, noun, v.activation);
    return CADM_OK;
}

// the two kinds of ctx no net plans on; phrase: "a terminal value", ..
int mlp_ctx_check(const cadm_ctx* ctx, const char* phrase, const char* who) {
    CADM_REQUIRE(!ctx->cfg.discrete && ctx->cfg.env_kind != CADM_ENV_CARTPOLE, "%s: %s needs a continuous-action ctx (discrete actions are "
                 "planned by random shooting)", who, phrase);
    CADM_REQUIRE(!cadm_sharded(ctx), "%s: %s is not supported on a candidate-sharded ctx", who, phrase);
    return CADM_OK;
}

bool mlp_shape_same(const MlpShape& a, const MlpShape& b) {
    bool same = a.n_hidden == b.n_hidden && a.activation == b.activation;
    for (int l = 0; same && l < a.n_hidden; ++l) same = a.hidden[l] == b.hidden[l];
    return same;
}

// dims[0 .. n_hidden + 1] of the net in -> h_1 .. h_L -> out
void mlp_dims(const MlpShape& v, int in, int out, int* dims) {
    dims[0] = in;
    for (int l = 0; l < v.n_hidden; ++l) dims[1 + l] = v.hidden[l];
    dims[1 + v.n_hidden] = out;
}

template <class Owned> bool mlp_registered(const Owned* o) { return o && o->set; }
template <class Owned> void mlp_clear(Owned* o) { if (o) o->set = false; }
template <class Owned> void mlp_free(Owned*& o) {
    if (!o) return;
    for (MlpNet& n : o->net) mlp_net_release(&n);
    delete o;
    o = nullptr;
}

// What the cadm_set_* entry points share behind their description's check: the null checks of the arrays and of every layer, the
// ctx-owned object on first use, the packed copies of `count` nets of the dims given (W, b: count * nl pointers, net by net; one mean /
// std_inv for all) on `stream`.  member: null, or what the nets of a count are called in the refusal ("critic").  `set` is false from
// the first upload on and true behind the last; the caller then stores its prm.
template <class Owned>
int mlp_register(cadm_ctx* ctx, Owned*& slot, int count, const char* member, const int* dims, int nl, const float* const* W,
                 const float* const* b, const float* mean, const float* std_inv, void* stream, const char* who) {
    CADM_REQUIRE(W && b && mean && std_inv, "%s: W / b / mean / std_inv is null", who);
    for (int i = 0; i < count * nl; ++i) {
        if (member) CADM_REQUIRE(W[i] && b[i], "%s: the weights or the biases of layer %d of %s %d are null", who, i % nl, member, i / nl);
        else CADM_REQUIRE(W[i] && b[i], "%s: the weights or the biases of layer %d are null", who, i);
    }
    CADM_ON_DEVICE(ctx);
    if (!slot) {
        slot = new (std::nothrow) Owned();
        if (!slot) { cadm_set_error("%s: out of host memory", who); return CADM_ENOMEM; }
    }
    slot->set = false;
    for (int c = 0; c < count; ++c) {
        const int rc = mlp_net_upload(slot->net[c], dims, nl, W + (size_t)c * nl, b + (size_t)c * nl, mean, std_inv, (hipStream_t)stream, who);
        if (rc) return rc;
    }
    slot->set = true;
    return CADM_OK;
}

// the net's half of a kernel's arguments, from its packed copy and its description: in -> h_1 .. h_L -> out
void mlp_dev(MlpDev& d, const MlpNet& net, const MlpShape& v, int in, int out) {
    mlp_dims(v, in, out, d.dims);
    d.nlayers = v.n_hidden + 1;
    d.act = v.activation;
    for (int l = 0; l < d.nlayers; ++l) { d.W[l] = net.W[l]; d.b[l] = net.b[l]; }
    d.mean = net.mean; d.istd = net.istd;
}

// the clause every row-tile rule shares: more than two sixteen-row tiles per CU.  (Two row tiles halve the weight stream per row; one
// tile keeps every CU busy while the rows are few.)
bool mlp_many_tiles(const cadm_ctx* ctx, size_t rows) { return (rows + 15) / 16 > 2 * (size_t)ctx->n_cus; }

// the launch of k1 (RT == 1) or k2 (RT == 2) over `rows` rows with `lds` bytes of dynamic LDS
template <class Args>
int mlp_launch(cadm_ctx* ctx, void (*k1)(const Args), void (*k2)(const Args), int RT, size_t lds, size_t rows, const Args& a, hipStream_t s,
               const char* who) {
    const size_t R = 16 * (size_t)RT, blocks = (rows + R - 1) / R;
    CADM_REQUIRE(blocks <= 0x7fffffffull, "%s: %zu rows are too many for one launch", who, rows);
    void (*const k)(const Args) = RT == 2 ? k2 : k1;
    const void* fn = reinterpret_cast<const void*>(k);
    if (lds > 64 * 1024 && !ctx->attr_done.count(fn)) {
        CADM_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, MLP_LDS_MAX));
        ctx->attr_done.insert(fn);
    }
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(MLP_THREADS), lds, s, a);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

}  // namespace
