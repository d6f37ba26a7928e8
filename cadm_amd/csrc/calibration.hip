// Calibration of the ensemble's predictive distribution: the particles of a rollout (`traj_out` of the rollout kernel, [F, m, 1, p, D])
// against held-out next observations, reduced on the device to rank histograms and proper scores (cadm_calibration_stats;
// cadm_eval_calibration in horizon.hip strings encoder, rollout and this kernel together chunk by chunk).  A sibling of horizon.hip:
// the same inputs, the same rule for which pairs count, the same reduction contract for the float sums.
//
// Per (window i, step h) that is VALID -- future_bool[i, 0..h] all non-zero -- and whose p * D trajectory values are all finite (else
// the pair only counts in diverged[h]), per dim d, with particles x_0 .. x_{p-1}, truth y, every comparison in float32:
//     rank_hist[h, d, r]           += 1   at r = #{j : x_j < y}                       (Talagrand histogram, p + 1 bins)
//     rank_hist_member[e, h, d, r] += 1   the same over member e's own p / E particles   (particle j belongs to member j / (p / E))
//     ties[h, d]                   += 1   where some x_j == y
//     degenerate[h, d]             += 1   where the biased particle variance v is exactly 0; such a pair is in neither z2 nor nll
//     crps[h, d] += (1/p) sum_j |x_j - y| - (1/p^2) sum_j sum_{k<j} |x_j - x_k|       (= the usual 1/(2 p^2) over all ordered pairs)
//     z2[h, d]   += (xbar - y)^2 / v
//     nll[h, d]  += 0.5 (log 2 pi + log v + (xbar - y)^2 / v)                          (moment-matched Gaussian)
//     count[h]   += 1
// xbar and v are formed relative to particle 0, members first, the variance in a second pass -- the very operations of
// horizon_error_kernel, so v is bit for bit the per-window term of its `spread` (and std_total^2 of the forecast).
// Sums and counts only; the caller divides.
//
// Reduction contract.
//   integers  exact in any order: LDS integer atomics per workgroup, then one global atomicAdd per non-zero LDS counter.  The entry
//             point clears them when window0 == 0.  A workgroup sees at most 64 windows, so a histogram bin of its own never exceeds
//             64: the LDS histograms are 8-bit counters packed four to a word (atomicAdd of 1 << 8 (bin & 3); no carry can cross).
//   floats    no floating-point atomics.  Stage 1: one workgroup per (block of 64 consecutive windows, step) writes ONE partial; block
//             boundaries are multiples of 64 in the GLOBAL window index (window0 % 64 == 0), window w adds into slot w % WT in window
//             order, the WT slots are then added in slot order.  Stage 2: one thread per entry adds the blocks' partials in block order.
//             Bit-identical run to run, and independent of how the caller cuts the windows into launches.
//
// Rounding chains (fp32, u = 2^-24; the library is built without contraction, logf is OCML's, documented at 1 ulp):
//   per window   A = (1/p) sum_j |x_j - y|: 1 (difference) + p (sum) + 1 (division) roundings of non-negative terms
//                B = (1/p^2) sum_j sum_{k<j} |x_j - x_k|: 1 + (p - 1) (row sum) + p (rows) + 1 (division); p^2 is exact in fp32
//                crps_i = A - B: 1 more, of a difference: its error scales with A + B, not with crps_i
//                xbar - y: the member sums (p / E), the total (E), the division, x0 + md and the subtraction -- as in horizon.hip, an
//                absolute error of at most 3 u (max_j |x_j| + |y|) that does not shrink where xbar lands near y
//                v: x_j - x0 and - md (2 roundings of each deviation, absolute), the square, p adds, the division
//                z2_i = (xbar - y)^2 / v: square and division, 2 more on top of its two operands' errors
//                nll_i = 0.5 ((log 2 pi + log v) + z2_i): logf, 2 adds (of terms of either sign), the halving is exact
//   over windows 64 / WT adds into a slot, WT slot adds, (blocks - 1) block adds: 64 / WT + WT + (blocks - 1) roundings of the running
//                sum, which for nll is bounded by the sum of the |nll_i| (its terms change sign), for crps and z2 by the sum itself.
//
// Tile.  Like horizon.hip: a (block, step)'s windows are one contiguous span of traj, loaded lane-linear into LDS with 16-byte loads
// (scalar loads where the span is not 16-byte aligned), WT windows at a time; one thread per (window, dim) walks its p values at
// stride D (consecutive lanes read consecutive words: conflict-free but for the seam between two windows).  The pair term is a plain
// triangular loop over LDS, p (p - 1) / 2 reads per thread against p values loaded: at p = 20 the kernel stays bound by the read of traj.
// WT is the largest power of two <= 16 with
//     WT * (4 D (p + 3) + 8)  +  D (2 p + E + 1) + 8 D + 32   <=  48 KiB
// (tile + three float slots + flags per window; the two byte histograms, ties / degenerate and the counters once), below the 64 KiB a
// kernel gets without an attribute.  p = 20, D = 45: WT = 8; p = 130, D = 45: WT = 1.  CADM_EINVAL when not even one window fits.
#include "planner.h"

namespace {

constexpr int CS_BLOCK = 64;                 // windows per partial
constexpr int CS_THREADS = 256;
constexpr int CS_MAX_WT = 16;                // windows per LDS tile
constexpr int CS_LDS_BUDGET = 48 * 1024;
constexpr float CS_LOG_2PI = 1.8378770664093453f;

struct CalibrationArgs {
    const float *traj, *truth, *mask;
    long long truth_ld;                      // floats between the truth rows of consecutive windows
    int m, F, p, E, D, PE, WT;
    long long block0;                        // window0 / 64: global index of this launch's first block
    float* partials;                         // [blocks][F][3 D]: crps, z2, nll
    cadm_calibration_out out;                // the int32 outputs are added to from here
};

__device__ __forceinline__ bool non_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
// 8-bit counters, four to a word
__device__ __forceinline__ void bump(unsigned* hist, int bin) { atomicAdd(&hist[bin >> 2], 1u << (8 * (bin & 3))); }
__device__ __forceinline__ int bin_count(const unsigned* hist, int bin) { return (int)((hist[bin >> 2] >> (8 * (bin & 3))) & 255u); }

__global__ __launch_bounds__(CS_THREADS) void calibration_kernel(const CalibrationArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cs_smem[];
    const int D = a.D, p = a.p, E = a.E, PE = a.PE, WT = a.WT, pD = p * D, KD = 3 * D;
    const int nh = D * (p + 1), nhm = E * D * (PE + 1), hw = (nh + 3) >> 2, hmw = (nhm + 3) >> 2;
    float* tile = cs_smem;                                   // [WT][p][D]: the trajectory values of WT windows at this step
    float* acc = tile + ((WT * pD + 3) & ~3);                // [WT][3][D]: slot w % WT of crps, z2, nll
    unsigned* hist = reinterpret_cast<unsigned*>(acc + WT * KD);     // [D][p + 1] bytes
    unsigned* histm = hist + hw;                             // [E][D][PE + 1] bytes
    int* ties = reinterpret_cast<int*>(histm + hmw);         // [D]
    int* degen = ties + D;                                   // [D]
    int* ok = degen + D;                                     // [WT] the window exists and the step is valid
    int* bad = ok + WT;                                      // [WT] a non-finite value was loaded
    int* cnt = bad + WT;                                     // count, diverged
    const int blk = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    const int wb0 = blk * CS_BLOCK;
    for (int i = tid; i < WT * KD; i += CS_THREADS) acc[i] = 0.0f;
    for (int i = tid; i < hw + hmw + 2 * D; i += CS_THREADS) hist[i] = 0u;      // hist, histm, ties, degen are contiguous
    if (tid < 2) cnt[tid] = 0;
    for (int t0 = 0; t0 < CS_BLOCK && wb0 + t0 < a.m; t0 += WT) {
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
        for (int i = tid; i < nvec; i += CS_THREADS) {
            const floatx4 v = reinterpret_cast<const floatx4*>(src)[i];
            reinterpret_cast<floatx4*>(tile)[i] = v;
            if (non_finite(v[0]) || non_finite(v[1]) || non_finite(v[2]) || non_finite(v[3])) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (non_finite(v[c])) atomicOr(&bad[(4 * i + c) / pD], 1);
            }
        }
        for (int i = 4 * nvec + tid; i < len; i += CS_THREADS) {
            const float v = src[i];
            tile[i] = v;
            if (non_finite(v)) atomicOr(&bad[i / pD], 1);
        }
        __syncthreads();
        if (tid < nw && ok[tid]) atomicAdd(&cnt[bad[tid] ? 1 : 0], 1);
        for (int it = tid; it < nw * D; it += CS_THREADS) {
            const int w = it / D, d = it - w * D;
            if (!ok[w] || bad[w]) continue;
            const float* x = tile + w * pD + d;
            const float y = a.truth[(size_t)(w0 + w) * a.truth_ld + (size_t)h * D + d];
            float* ac = acc + w * KD + d;
            // mean and variance exactly as horizon_error_kernel forms them: relative to particle 0, members first, two passes
            const float x0 = x[0];
            float tot = 0.0f;
            int r = 0, tie = 0;
            for (int e = 0; e < E; ++e) {
                float s = 0.0f;
                int re = 0;
                for (int j = 0; j < PE; ++j) {
                    const float xj = x[(e * PE + j) * D];
                    s += xj - x0;
                    re += xj < y ? 1 : 0;
                    tie |= xj == y ? 1 : 0;
                }
                tot += s;
                r += re;
                bump(histm, (e * D + d) * (PE + 1) + re);
            }
            bump(hist, d * (p + 1) + r);
            if (tie) atomicAdd(&ties[d], 1);
            const float md = tot / (float)p;
            float var = 0.0f;
            for (int j = 0; j < p; ++j) {
                const float dv = (x[j * D] - x0) - md;
                var += dv * dv;
            }
            const float v = var / (float)p;
            const float dt = (x0 + md) - y;
            // crps: the distance term, and the pair term as row sums in index order
            float sa = 0.0f, sb = 0.0f;
            for (int j = 0; j < p; ++j) {
                const float xj = x[j * D];
                sa += fabsf(xj - y);
                float row = 0.0f;
                for (int k = 0; k < j; ++k) row += fabsf(xj - x[k * D]);
                sb += row;
            }
            ac[0] += sa / (float)p - sb / ((float)p * (float)p);
            if (v == 0.0f) {
                atomicAdd(&degen[d], 1);
            } else {
                const float z = dt * dt / v;
                ac[D] += z;
                ac[2 * D] += 0.5f * ((CS_LOG_2PI + logf(v)) + z);
            }
        }
    }
    __syncthreads();
    float* out = a.partials + ((size_t)(a.block0 + blk) * a.F + h) * KD;
    for (int i = tid; i < KD; i += CS_THREADS) {
        float s = 0.0f;
        for (int w = 0; w < WT; ++w) s += acc[w * KD + i];
        out[i] = s;
    }
    // integers: one global add per LDS counter that moved
    int32_t* gh = a.out.rank_hist + (size_t)h * nh;
    for (int i = tid; i < nh; i += CS_THREADS) {
        const int c = bin_count(hist, i);
        if (c) atomicAdd(&gh[i], c);
    }
    const int per_member = D * (PE + 1);
    for (int i = tid; i < nhm; i += CS_THREADS) {
        const int c = bin_count(histm, i);
        if (c) {
            const int e = i / per_member;
            atomicAdd(&a.out.rank_hist_member[((size_t)e * a.F + h) * per_member + (i - e * per_member)], c);
        }
    }
    for (int i = tid; i < D; i += CS_THREADS) {
        if (ties[i]) atomicAdd(&a.out.ties[(size_t)h * D + i], ties[i]);
        if (degen[i]) atomicAdd(&a.out.degenerate[(size_t)h * D + i], degen[i]);
    }
    if (tid < 2 && cnt[tid]) atomicAdd(&(tid == 0 ? a.out.count : a.out.diverged)[h], cnt[tid]);
}

// stage 2: one thread per float output entry, blocks added in index order
__global__ __launch_bounds__(CS_THREADS) void calibration_finalize_kernel(const float* __restrict__ partials, long long nblocks, int F, int D,
                                                                          float* crps, float* z2, float* nll) {
    const int KD = 3 * D;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= F * KD) return;
    const int h = idx / KD, i = idx - h * KD;
    const float* src = partials + (size_t)h * KD + i;
    const size_t step = (size_t)F * KD;
    float s = 0.0f;
    for (long long b = 0; b < nblocks; ++b) s += src[b * step];
    const int k = i / D, d = i - k * D;
    (k == 0 ? crps : k == 1 ? z2 : nll)[h * D + d] = s;
}

long long fixed_bytes(int p, int E, int D) { return (long long)D * (2 * p + E + 1) + 8LL * D + 32; }

// windows per LDS tile: the largest power of two <= CS_MAX_WT that fits the budget (0: not even one window)
int tile_windows(int p, int E, int D) {
    const long long per_window = 4LL * D * (p + 3) + 8;
    int wt = CS_MAX_WT;
    while (wt >= 1 && wt * per_window + fixed_bytes(p, E, D) > CS_LDS_BUDGET) wt >>= 1;
    return wt;
}

}  // namespace

extern "C" int cadm_calibration_stats(const float* traj, const float* truth, long long truth_row_stride, const float* mask, int m, int F, int p,
                                      int E, int D, long long window0, float* partials, long long partials_blocks,
                                      const cadm_calibration_out* out, int finalize, void* stream) {
    CADM_REQUIRE(traj, "cadm_calibration_stats: traj is null");
    CADM_REQUIRE(truth && mask && partials, "cadm_calibration_stats: truth / mask / partials is null");
    CADM_REQUIRE(out && out->rank_hist && out->rank_hist_member && out->ties && out->degenerate && out->crps && out->z2 && out->nll &&
                     out->count && out->diverged, "cadm_calibration_stats: out or one of its pointers is null");
    CADM_REQUIRE(F >= 1 && m >= 1 && p >= 1 && D >= 1, "cadm_calibration_stats: F, m, p, D must be >= 1 (got F=%d m=%d p=%d D=%d)", F, m, p, D);
    CADM_REQUIRE(E >= 1 && p % E == 0, "cadm_calibration_stats: p (%d) must be a multiple of E (%d)", p, E);
    CADM_REQUIRE(window0 >= 0 && window0 % CS_BLOCK == 0, "cadm_calibration_stats: window0 (%lld) must be a non-negative multiple of %d", window0,
                 CS_BLOCK);
    CADM_REQUIRE(D <= 64, "cadm_calibration_stats: D (%d) must be <= 64", D);
    CADM_REQUIRE(F <= 65535, "cadm_calibration_stats: F (%d) must be <= 65535", F);
    CADM_REQUIRE(truth_row_stride >= (long long)F * D, "cadm_calibration_stats: truth_row_stride (%lld) is below F * D = %d", truth_row_stride,
                 F * D);
    const int wt = tile_windows(p, E, D);
    CADM_REQUIRE(wt >= 1, "cadm_calibration_stats: p (%d) x D (%d) does not fit an LDS tile (4 D (p + 3) + D (2 p + E + 9) + 40 <= %d bytes)", p, D,
                 CS_LDS_BUDGET);
    const long long nblk = ((long long)m + CS_BLOCK - 1) / CS_BLOCK, block0 = window0 / CS_BLOCK;
    CADM_REQUIRE(block0 + nblk <= partials_blocks, "cadm_calibration_stats: partials_blocks (%lld) is below the %lld blocks of windows [0, %lld)",
                 partials_blocks, block0 + nblk, window0 + m);
    hipStream_t s = (hipStream_t)stream;
    const int PE = p / E;
    if (window0 == 0) {
        const size_t fd = (size_t)F * D * sizeof(int32_t);
        CADM_CHECK_HIP(hipMemsetAsync(out->rank_hist, 0, fd * (p + 1), s));
        CADM_CHECK_HIP(hipMemsetAsync(out->rank_hist_member, 0, fd * E * (PE + 1), s));
        CADM_CHECK_HIP(hipMemsetAsync(out->ties, 0, fd, s));
        CADM_CHECK_HIP(hipMemsetAsync(out->degenerate, 0, fd, s));
        CADM_CHECK_HIP(hipMemsetAsync(out->count, 0, F * sizeof(int32_t), s));
        CADM_CHECK_HIP(hipMemsetAsync(out->diverged, 0, F * sizeof(int32_t), s));
    }
    CalibrationArgs a{};
    a.traj = traj; a.truth = truth; a.mask = mask; a.truth_ld = truth_row_stride;
    a.m = m; a.F = F; a.p = p; a.E = E; a.D = D; a.PE = PE; a.WT = wt;
    a.block0 = block0; a.partials = partials; a.out = *out;
    const size_t words = (size_t)((wt * p * D + 3) & ~3) + (size_t)wt * 3 * D + (size_t)((D * (p + 1) + 3) >> 2) +
                         (size_t)((E * D * (PE + 1) + 3) >> 2) + 2 * (size_t)D + 2 * (size_t)wt + 2;
    hipLaunchKernelGGL(calibration_kernel, dim3((unsigned)nblk, (unsigned)F), dim3(CS_THREADS), words * 4, s, a);
    CADM_CHECK_HIP(hipGetLastError());
    if (finalize) {
        const int total = F * 3 * D;
        hipLaunchKernelGGL(calibration_finalize_kernel, dim3((total + CS_THREADS - 1) / CS_THREADS), dim3(CS_THREADS), 0, s, partials, block0 + nblk,
                           F, D, out->crps, out->z2, out->nll);
        CADM_CHECK_HIP(hipGetLastError());
    }
    return CADM_OK;
}
