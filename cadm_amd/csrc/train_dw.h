// Grouped weight-gradient kernel of the training step, Adam fused into its epilogue.  Part of train.hip's translation unit (overview there).
#pragma once
#include "train_pack.h"
#include "train_chain.h"

namespace {
// ---------------------------------------------------------------------------------------------
// grouped weight-gradient GEMM with the Adam update fused into its epilogue
// ---------------------------------------------------------------------------------------------
struct DwJob {                       // W[e] (M x N) <- Adam(W, X[e]^T dZ[e] + wdc W);  b[e] <- Adam(b, colsum dZ[e])
    const float *X, *dZ;             // X [E][B][ldx] (first M columns), dZ [E][B][N]
    const float* dZ2;                // optional second gradient, added on load (the context encoder's, from the two dynamics nets)
    float *W, *Mw, *Vw, *bW, *bM, *bV;
    int ldx, M, N, tile0;            // tile0: first workgroup (blockIdx.x) of this job
    int ldz, pad;                    // row stride of dZ (>= N: the head / context gradients are stored with rows padded to 16 bytes)
    float wdc;
    int tn;                          // column tiles
    PackDst pf, pb;                  // the chain kernel's packed copies of W (forward / transposed operand), kept current here
};
#define DW_MAXJOBS 20
struct DwArgs {
    int tile0s[DW_MAXJOBS];          // the jobs' first tiles again, compact: the job search reads two 64-byte lines of the argument block
                                     // instead of one line per job it steps over (each a dependent scalar-memory round trip)
    DwJob job[DW_MAXJOBS];
    int njobs, B, tiles, E;          // tiles: work items per member
    float lr_t, b1, b2, eps;
    ReduceP lossr; int loss_slots;   // the step's loss partials (chain_loss_phase), summed by a spare workgroup of this launch
    unsigned long long* tbuf;        // cadm_dev_set_timing_buffer (tools/chain_timing.py): per workgroup [1024 + 2 b] start / end,
                                     // [4096 + b] job and flavour, [5200 + b] end of the slab loop (s_memrealtime, 100 MHz)
};
static_assert(sizeof(DwArgs) <= 4096, "kernel argument block");

#define TN 64
#define TM 48
#define TK 32
#define LDA (TM + 4)
#define LDB (TN + 4)
#define DW_NSLAB 1                   // slabs per K panel in flight (registers): one keeps the kernel at 120 VGPRs = 4 workgroups per CU

// One 48 x 64 tile of one job per workgroup, reduction over the batch: the whole step's ~925 tiles then fit the chip's
// 1024 workgroup slots (4 per CU) in ONE round (32 x 64 tiles needed 1330 = two rounds).  K is walked in 32-deep slabs:
// stash the slab's loads into LDS as they land, barrier, MFMA sweep; 4 waves side by side, each 48 x 16.  Occupancy beats
// panel depth here: 2-slab panels (156 VGPRs, 3 per CU) and register double-buffering (178 VGPRs) both measured slower.
__global__ __launch_bounds__(256) void dw_adam_kernel(const DwArgs a) {
    constexpr int LDK = TK + 4;                          // fast path: slabs stored [feature][k]
    constexpr int DW_SLAB = (TM + TN) * LDK;             // ... in TWO buffers, so that a slab costs one barrier (see the slab loop)
    constexpr int DW_SMEM = DW_NSLAB * TK * (LDA + LDB) > 2 * DW_SLAB ? DW_NSLAB * TK * (LDA + LDB) : 2 * DW_SLAB;
    __shared__ __attribute__((aligned(16))) float dw_smem[DW_SMEM];
    float* const As = dw_smem;
    float* const Bs = dw_smem + DW_NSLAB * TK * LDA;
    constexpr int LDC = TN + 4;                          // the finished tile, staged for the vectorised Adam epilogue
    static_assert(TM * LDC <= DW_NSLAB * TK * (LDA + LDB), "the C tile must fit the slab buffers");
    // Workgroups are dispatched round-robin over the 8 XCDs (linear id % 8), each with its own L2.  Consecutive work items
    // (member-major, then job, then tile) re-read the same X / dZ panels, so XCD x gets the x-th CONTIGUOUS eighth of them:
    // a panel is then fetched into one L2 instead of up to eight (W, m, v alone are 44 MB of traffic per launch; measured later: the placement of the panels makes no difference).
    if (blockIdx.x >= gridDim.x - 8) {                   // (eight spare workgroups keep the XCD arithmetic below; one works)
        if (blockIdx.x == gridDim.x - 8 && a.loss_slots > 0) loss_finalize<256, false>(a.lossr, a.loss_slots, dw_smem, threadIdx.x);
        return;
    }
    const int per_xcd = (a.tiles * a.E + 7) >> 3;
    const int item = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (item >= a.tiles * a.E) return;
    const int e = item / a.tiles, tile = item - e * a.tiles;
#ifdef CADM_DW_TIMING       // (developer build only, tools/chain_timing.py: the stamps cost registers -- 132 VGPRs = 3 workgroups per CU)
    const bool tstamp = a.tbuf && threadIdx.x == 0 && blockIdx.x < 1000;
    if (tstamp) a.tbuf[1024 + 2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
#endif
    int ji = 0;
#pragma unroll 1
    while (ji + 1 < a.njobs && tile >= a.tile0s[ji + 1]) ++ji;
    const DwJob& jb = a.job[ji];
    const int t = tile - jb.tile0;
    const int mb = (t / jb.tn) * TM, nb = (t % jb.tn) * TN;
    const int M = jb.M, N = jb.N, K = a.B;
    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
    const float* A = jb.X + (long)e * K * jb.ldx;       // A(m = k_in, k = b) = X[b][k_in]
    const float* Bm = jb.dZ + (long)e * K * jb.ldz;     // B(k = b, n)        = dZ[b][n]
    constexpr int MI = TM / 16;
    floatx4 acc[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    float colsum = 0.0f;                                // bias gradient (threads < 64 of the m-tile-0 blocks)
    constexpr int NLA = TM * TK / 256, NLB = TN * TK / 256;
    float ra[DW_NSLAB][NLA], rb[DW_NSLAB][NLB];
    // Loads are UNCONDITIONAL (addresses clamped into the matrix, out-of-range elements zeroed afterwards): a
    // `cond ? *p : 0` select makes hipcc branch around every load and wait for each one in turn.
    const float* pa[NLA];
    const float* pb[NLB];
    int ka[NLA], kb[NLB], la[NLA], lb[NLB];
    bool va[NLA], vb[NLB];
#pragma unroll
    for (int it = 0; it < NLA; ++it) {
        const int idx = tid + it * 256;
        const int ak = idx / TM, am = idx - ak * TM;
        ka[it] = ak; la[it] = ak * LDA + am;
        va[it] = mb + am < M;
        pa[it] = A + (va[it] ? mb + am : 0);
    }
#pragma unroll
    for (int it = 0; it < NLB; ++it) {
        const int idx = tid + it * 256;
        const int bn = idx & (TN - 1), bk = idx / TN;
        kb[it] = bk; lb[it] = bk * LDB + bn;
        vb[it] = nb + bn < N;
        pb[it] = Bm + (vb[it] ? nb + bn : 0);
    }
    const int kmax = K - 1;
    const bool two = jb.dZ2 != nullptr;
    const long d2 = two ? jb.dZ2 - jb.dZ : 0;            // (same shape and member stride as dZ)
    const bool do_colsum = jb.bW && mb == 0 && tid < TN;

    // The loads of slab s+1 are issued right after slab s has been stashed into LDS -- into the SAME registers, which are
    // dead by then -- so their latency runs under slab s's MFMAs at no register cost.
    static_assert(DW_NSLAB == 1, "the slab pipeline below keeps one slab of loads in flight");
    const int KP = jb.X ? K : 0;                                       // X == null: L2-only job, gradient = wdc * W
    auto issue = [&](int k0) {
#pragma unroll
        for (int it = 0; it < NLA; ++it) {
            const int k = k0 + ka[it];
            ra[0][it] = pa[it][(long)(k < kmax ? k : kmax) * jb.ldx];
        }
#pragma unroll
        for (int it = 0; it < NLB; ++it) {
            const int k = k0 + kb[it];
            const long o = (long)(k < kmax ? k : kmax) * jb.ldz;
            const float v1 = pb[it][o], v2 = pb[it][o + d2];        // (both loads unconditional: d2 = 0 without a second gradient)
            rb[0][it] = two ? v1 + v2 : v1;
        }
    };
    // Fast path (whole slabs, 16-byte rows): a slab is fetched with 16-byte loads -- a lane takes 4 consecutive features of one
    // batch row, 8 lanes 128 contiguous bytes of it (lanes along the batch instead -- conflict-free stores without a swizzle --
    // fetch a 64-byte line per 16 bytes used: 0.225 ms per step) -- and stashed TRANSPOSED ([feature][k], k contiguous), so that
    // an MFMA operand for 4 k-steps is one ds_read_b128: per slab and wave 4 global loads, 14 LDS writes and
    // 8 LDS reads next to the 24 MFMAs, where the generic path below spends 14 + 14 + 32 and a clamp / select per element.
    // (On this part the matrix pipe does not overlap with another wave's VALU work: every instruction saved is MFMA time.)
    // k-steps are taken in the order k = 16 g + 4 q + u (lane group q, u = 0..3) -- any order, as long as A and B agree.
    // (rows are read in 16-byte pieces up to the next multiple of 4 columns: the workspace pads the odd-width tensors -- the
    //  normalised inputs, the head and context gradients -- with zero columns, so that the few jobs on them do not fall back to
    //  the scalar loop: they were the launch's tail, 25-28 us of slab loop against 13-17)
    const int Mq = (M + 3) & ~3, Nq = (N + 3) & ~3;
    const bool vec = KP > 0 && (K % TK) == 0 && ((jb.ldx | jb.ldz) & 3) == 0 && Mq <= jb.ldx && Nq <= jb.ldz &&
                     ((reinterpret_cast<size_t>(jb.X) | reinterpret_cast<size_t>(jb.dZ) | reinterpret_cast<size_t>(jb.dZ2)) & 15) == 0;
    // Slabs by LDS-DMA (one gradient source; the jobs that add a second one on load keep the register path below): a slab goes
    // global -> LDS in 16 buffer_load_dwordx4 .. lds of the workgroup (4 per wave: 4 batch rows x 12 / 16 quads each), no registers, no
    // ds_write, in the tensors' own [row][feature] order; operands are then single dwords (lane (c, q): feature c of row q of a 4-row
    // group).  The 4 rows of one MFMA come from 4 DIFFERENT groups -- each group starts 16 floats further round the banks -- so the
    // four lane groups of a ds_read hit four different quarter-sets of banks: k-steps are taken in the order (t, r) -> rows
    // {4 (4 t + q) + r : q = 0..3}, any order as long as A and B agree.
    const bool dma = vec && !two && (size_t)K * jb.ldx * 4 < (1ull << 32) && (size_t)K * jb.ldz * 4 < (1ull << 32);
    if (dma) {
        constexpr int AG = 4 * TM + 16, BG = 4 * TN + 16, DBUF = 8 * (AG + BG);      // floats per 4-row group of A / B, per slab buffer
        static_assert(TK == 32 && 2 * DBUF <= DW_SMEM && TM * LDC <= DBUF, "slab buffers of the LDS-DMA path");
        typedef __attribute__((address_space(3))) void* ldsp;
        const int c = lane & 15, kq = lane >> 4, wu = __builtin_amdgcn_readfirstlane(wn);
        const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, (unsigned)((size_t)K * jb.ldx * 4), 0x00020000);
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)Bm, 0, (unsigned)((size_t)K * jb.ldz * 4), 0x00020000);
        const int ar = lane / 12, aq = lane - 12 * ar;                               // (lanes 0..47: 4 rows x 12 quads of A)
        const int ma = mb + 4 * aq < Mq ? mb + 4 * aq : Mq - 4, nq = nb + 4 * c < Nq ? nb + 4 * c : Nq - 4;
        const unsigned va = (unsigned)((ar * jb.ldx + ma) * 4), vb = (unsigned)((kq * jb.ldz + nq) * 4);
        const bool n_ok = nb + 16 * wn < N;
        auto request = [&](int k0, int par) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = 2 * wu + u;
                float* const ga = dw_smem + par * DBUF + j * AG;
                float* const gb = dw_smem + par * DBUF + 8 * AG + j * BG;
                const unsigned sa = (unsigned)(k0 + 4 * j) * (unsigned)jb.ldx * 4u, sb = (unsigned)(k0 + 4 * j) * (unsigned)jb.ldz * 4u;
                if (lane < 48) __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (ldsp)ga, 16, va, sa, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (ldsp)gb, 16, vb, sb, 0, 0);
            }
        };
        auto compute = [&](int par) {
            const float* Ab = dw_smem + par * DBUF + kq * AG + c;
            const float* Bb = dw_smem + par * DBUF + 8 * AG + kq * BG + 16 * wn + c;
            if (do_colsum) {
                const float* Bc = dw_smem + par * DBUF + 8 * AG + tid;
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) colsum += Bc[j * BG + r * TN];
            }
            if (n_ok) {
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float b = Bb[4 * t * BG + r * TN];
#pragma unroll
                        for (int i = 0; i < MI; ++i) {
                            if (mb + 16 * i >= M) continue;
                            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ab[4 * t * AG + r * TM + 16 * i], b, acc[i], 0, 0, 0);
                        }
                    }
            }
        };
        request(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int par = 0;
        for (int k0 = 0; k0 < KP; k0 += TK, par ^= 1) {
            if (k0 + TK < KP) request(k0 + TK, par ^ 1);       // (the buffer computed from one iteration ago: every wave is past that iteration's barrier)
            compute(par);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
    if (vec && !dma) {
        float* const At = dw_smem;
        float* const Bt = dw_smem + TM * LDK;
        const int c = lane & 15, q = lane >> 4;
        // quads of a slab: A 32 rows x 12 (8 per row for every thread, the other 4 for threads 0..127), B 32 rows x 16 (8 + 8):
        // a wave reads 8 rows x 128 bytes (or 16 x 64) per load.  LDS position of (feature f, k): f * LDK + 4 * ((k >> 2) ^
        // ((f >> 2) & 7)) + (k & 3) -- the XOR spreads a wave's transposed stores over all banks (2 lanes per bank)
        const int kl = tid >> 3, ql = tid & 7, kl2 = (tid >> 2) & 31, ql2 = 8 + (tid & 3);
        const bool a1 = tid < 128;
        const int ma0 = mb + 4 * ql < Mq ? mb + 4 * ql : Mq - 4, ma1 = mb + 4 * ql2 < Mq ? mb + 4 * ql2 : Mq - 4;
        const int nb0 = nb + 4 * ql < Nq ? nb + 4 * ql : Nq - 4, nb1 = nb + 32 + 4 * ql < Nq ? nb + 32 + 4 * ql : Nq - 4;
        const floatx4* pA0 = reinterpret_cast<const floatx4*>(A + (long)kl * jb.ldx + ma0);
        const floatx4* pA1 = reinterpret_cast<const floatx4*>(A + (long)kl2 * jb.ldx + ma1);
        const floatx4* pB0 = reinterpret_cast<const floatx4*>(Bm + (long)kl * jb.ldz + nb0);
        const floatx4* pB1 = reinterpret_cast<const floatx4*>(Bm + (long)kl * jb.ldz + nb1);
        const long sA = (long)TK * jb.ldx / 4, sB = (long)TK * jb.ldz / 4;    // slab strides in float4
        float* const wA0 = At + (4 * ql) * LDK + 4 * ((kl >> 2) ^ (ql & 7)) + (kl & 3);
        float* const wA1 = At + (4 * ql2) * LDK + 4 * ((kl2 >> 2) ^ (ql2 & 7)) + (kl2 & 3);
        float* const wB0 = Bt + (4 * ql) * LDK + 4 * ((kl >> 2) ^ (ql & 7)) + (kl & 3);
        float* const wB1 = Bt + (32 + 4 * ql) * LDK + 4 * ((kl >> 2) ^ ((8 + ql) & 7)) + (kl & 3);
        const bool n_ok = nb + 16 * wn < N;                              // units past the matrix edge are skipped
        // two slabs of loads in flight (registers): slab s + 2 is requested when slab s has been stashed
        struct Slab { floatx4 a0, a1, b0, b1, c0, c1; } r[2];      // (c: the second gradient, added when the slab is stashed)
        auto fetch = [&](Slab& d) {
            d.a0 = *pA0; d.a1 = a1 ? *pA1 : floatx4{0.f, 0.f, 0.f, 0.f}; d.b0 = *pB0; d.b1 = *pB1;
            if (two) { d.c0 = pB0[d2 / 4]; d.c1 = pB1[d2 / 4]; }     // (used at the stash only: the branch costs no wait)
            pA0 += sA; pA1 += sA; pB0 += sB; pB1 += sB;
        };
        // One barrier per slab: slab s is stashed into buffer s & 1 while the slower waves may still be reading slab s - 1 out of the other
        // one; the stores of slab s + 1 (same buffer as s - 1) come behind the barrier of slab s, which every wave passes only after its
        // reads of slab s - 1.  (Single-buffered until round 5: two barriers per 24 MFMAs.)
        auto slab = [&](Slab& d, int k0, int par) {
            const int bo = par * DW_SLAB;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                wA0[bo + j * LDK] = d.a0[j];
                if (a1) wA1[bo + j * LDK] = d.a1[j];
                wB0[bo + j * LDK] = two ? d.b0[j] + d.c0[j] : d.b0[j];
                wB1[bo + j * LDK] = two ? d.b1[j] + d.c1[j] : d.b1[j];
            }
            __syncthreads();
            if (k0 + 2 * TK < KP) fetch(d);
            if (do_colsum) {
#pragma unroll
                for (int x = 0; x < TK / 4; ++x) {
                    const floatx4 v = *reinterpret_cast<const floatx4*>(Bt + bo + tid * LDK + 4 * (x ^ ((tid >> 2) & 7)));
                    colsum += v[0]; colsum += v[1]; colsum += v[2]; colsum += v[3];
                }
            }
            if (n_ok) {
                const int fb = 16 * wn + c;
#pragma unroll
                for (int g = 0; g < TK / 16; ++g) {
                    const floatx4 b4 = *reinterpret_cast<const floatx4*>(Bt + bo + fb * LDK + 4 * ((4 * g + q) ^ ((fb >> 2) & 7)));
#pragma unroll
                    for (int i = 0; i < MI; ++i) {
                        if (mb + 16 * i >= M) continue;
                        const int fa = 16 * i + c;
                        const floatx4 a4 = *reinterpret_cast<const floatx4*>(At + bo + fa * LDK + 4 * ((4 * g + q) ^ ((fa >> 2) & 7)));
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u], b4[u], acc[i], 0, 0, 0);
                    }
                }
            }
        };
        fetch(r[0]);
        if (KP > TK) fetch(r[1]);
        for (int k0 = 0; k0 < KP; k0 += 2 * TK) {
            slab(r[0], k0, 0);
            if (k0 + TK < KP) slab(r[1], k0 + TK, 1);
        }
    }
    if (!vec && KP > 0) issue(0);
    for (int k0 = 0; !vec && k0 < KP; k0 += TK) {
        if (k0 > 0) __syncthreads();               // previous slab fully consumed before its LDS is overwritten
#pragma unroll
        for (int it = 0; it < NLA; ++it) As[la[it]] = (va[it] && k0 + ka[it] <= kmax) ? ra[0][it] : 0.0f;
#pragma unroll
        for (int it = 0; it < NLB; ++it) Bs[lb[it]] = (vb[it] && k0 + kb[it] <= kmax) ? rb[0][it] : 0.0f;
        __syncthreads();
        if (k0 + TK < KP) issue(k0 + TK);
        if (do_colsum) {
#pragma unroll
            for (int kk = 0; kk < TK; ++kk) colsum += Bs[kk * LDB + tid];
        }
#pragma unroll
        for (int ks = 0; ks < TK / 4; ++ks) {
            const int kr = ks * 4 + (lane >> 4);
            const float b = Bs[kr * LDB + wn * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < MI; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(As[kr * LDA + i * 16 + (lane & 15)], b, acc[i], 0, 0, 0);
        }
    }

    // ---- epilogue: D layout col = lane & 15 -> n, row = (lane >> 4) * 4 + r -> m.  Adam touches W, m and v once each
    // (read + write): that traffic, not the GEMM, is most of this kernel, so the tile goes through LDS and every thread
    // updates 4 consecutive columns with 16-byte accesses (a D-layout thread would touch 12 scattered dwords x 6) ----
#ifdef CADM_DW_TIMING
    if (tstamp) a.tbuf[5200 + blockIdx.x] = __builtin_amdgcn_s_memrealtime();
#endif
    if ((N & 3) == 0) {
        __syncthreads();                                 // every wave is done reading the slab buffers
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) dw_smem[(i * 16 + (lane >> 4) * 4 + r) * LDC + wn * 16 + (lane & 15)] = acc[i][r];
        __syncthreads();
        // W, m, v of the thread's three column quads are requested TOGETHER (addresses clamped into the layer, never predicated:
        // with a branch around each quad hipcc waits for one quad's loads before it issues the next -- three dependent round trips)
        constexpr int NQD = TM * TN / 4 / 256;
        floatx4 w3[NQD], m3[NQD], v3[NQD];
#pragma unroll
        for (int it = 0; it < NQD; ++it) {
            const int idx = tid + it * 256;
            const int ml = idx / (TN / 4), n4 = (idx % (TN / 4)) * 4;
            const int mc = mb + ml < M ? mb + ml : M - 1, nc = nb + n4 < N ? nb + n4 : N - 4;
            const long o = ((long)e * M + mc) * N + nc;
            w3[it] = *reinterpret_cast<const floatx4*>(jb.W + o); m3[it] = *reinterpret_cast<const floatx4*>(jb.Mw + o);
            v3[it] = *reinterpret_cast<const floatx4*>(jb.Vw + o);
        }
#pragma unroll
        for (int it = 0; it < NQD; ++it) {
            const int idx = tid + it * 256;
            const int ml = idx / (TN / 4), n4 = (idx % (TN / 4)) * 4;
            const int m = mb + ml, n = nb + n4;
            if (m >= M || n >= N) continue;
            const long o = ((long)e * M + m) * N + n;
            const floatx4 g = *reinterpret_cast<const floatx4*>(dw_smem + ml * LDC + n4);
            floatx4 w = w3[it], mo = m3[it], vo = v3[it];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float wc = w[c], mc = mo[c], vc = vo[c];
                adam_update(wc, mc, vc, g[c] + jb.wdc * wc, a.lr_t, a.b1, a.b2, a.eps);
                w[c] = wc; mo[c] = mc; vo[c] = vc;
            }
            *reinterpret_cast<floatx4*>(jb.W + o) = w;
            *reinterpret_cast<floatx4*>(jb.Mw + o) = mo;
            *reinterpret_cast<floatx4*>(jb.Vw + o) = vo;
            // packed copies: forward operand (k = m, column n): the 4 columns are 4 lanes of one block; transposed operand
            // (k = n, column m - row0): the 4 columns are one lane's 4 k
            if (jb.pf.P) {
                float* q = jb.pf.P + (long)e * jb.pf.sP + pack_index(jb.pf, m, n);
#pragma unroll
                for (int c = 0; c < 4; ++c) q[4 * c] = w[c];
            }
            if (jb.pb.P) {
                const int np = m - jb.pb.row0;
                if (np >= 0 && np < jb.pb.ncols) *reinterpret_cast<floatx4*>(jb.pb.P + (long)e * jb.pb.sP + pack_index(jb.pb, n, np)) = w;
            }
        }
    } else {
        // (odd N: the heads, the context vector) -- the loads of all 12 elements first, clamped, for the same reason
        float ws_[MI][4], ms_[MI][4], vs_[MI][4];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = mb + i * 16 + (lane >> 4) * 4 + r, n = nb + wn * 16 + (lane & 15);
                const long o = ((long)e * M + (m < M ? m : M - 1)) * N + (n < N ? n : N - 1);
                ws_[i][r] = jb.W[o]; ms_[i][r] = jb.Mw[o]; vs_[i][r] = jb.Vw[o];
            }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = mb + i * 16 + (lane >> 4) * 4 + r;
                const int n = nb + wn * 16 + (lane & 15);
                if (m >= M || n >= N) continue;
                const long o = ((long)e * M + m) * N + n;
                float w = ws_[i][r], mo = ms_[i][r], vo = vs_[i][r];
                adam_update(w, mo, vo, acc[i][r] + jb.wdc * w, a.lr_t, a.b1, a.b2, a.eps);
                jb.W[o] = w; jb.Mw[o] = mo; jb.Vw[o] = vo;
                if (jb.pf.P) jb.pf.P[(long)e * jb.pf.sP + pack_index(jb.pf, m, n)] = w;
                const int np = m - jb.pb.row0;
                if (jb.pb.P && np >= 0 && np < jb.pb.ncols) jb.pb.P[(long)e * jb.pb.sP + pack_index(jb.pb, n, np)] = w;
            }
    }
#ifdef CADM_DW_TIMING
    if (tstamp) { a.tbuf[1024 + 2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime(); a.tbuf[4096 + blockIdx.x] = ji * 2 + (vec ? 1 : 0); }
#endif
    if (do_colsum && nb + tid < N) {
        const long o = (long)e * N + nb + tid;
        float w = jb.bW[o], mo = jb.bM[o], vo = jb.bV[o];
        adam_update(w, mo, vo, colsum, a.lr_t, a.b1, a.b2, a.eps);
        jb.bW[o] = w; jb.bM[o] = mo; jb.bV[o] = vo;
    }
}

// log-variance head output -> the clamped log-variance the loss phase uses (cadm_predict).
// It belongs to neither kernel of this header: it is defined here, behind dw_adam_kernel, only because that is where the single file had
// it and the code object keeps its kernels in the order of their definitions.  It may move whenever the device code changes anyway.
__global__ void clamp_logvar_kernel(const float* lv, const float* maxlv, const float* minlv, float* out, long n, int D) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int d = (int)(i % D);
    const float u = maxlv[d] - tf_softplus(maxlv[d] - lv[i]);      // core/utils.py:356
    out[i] = minlv[d] + tf_softplus(u - minlv[d]);                 // core/utils.py:357
}

}  // namespace
