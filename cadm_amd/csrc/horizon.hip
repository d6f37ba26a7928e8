// Open-loop prediction error of the ensemble along the horizon: trajectories of a rollout (`traj_out` of the rollout kernel,
// [F, m, 1, p, D]) against held-out next observations, reduced on the device to per-step sums (cadm_horizon_error;
// cadm_eval_horizon in capi.hip strings encoder, rollout and this kernel together chunk by chunk).
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
#include "common.h"

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
