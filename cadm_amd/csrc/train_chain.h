// Chain kernel of the training step: a workgroup walks a whole layer chain (forward or transposed) over a 16-row batch tile held
// in LDS; the forward launch of a training step closes with the loss phase.  Part of train.hip's translation unit (overview there).
#pragma once
#include "common.h"

namespace {
enum { ACT_NONE = 0, ACT_SWISH = 1, ACT_RELU = 2, ACT_TANH = 3, ACT_SIGMOID = 4 };      // stage-table codes (see dyn_act)

// v_exp_f32 / v_rcp_f32 sigmoid like the planner's swish_f.
__device__ __forceinline__ float sigmoid_fast(float z) { return __builtin_amdgcn_rcpf(1.0f + __expf(-z)); }

__device__ __forceinline__ void adam_update(float& w, float& m, float& v, float g, float lr_t, float b1, float b2,
                                            float eps) {
    // tf.compat.v1.train.AdamOptimizer (training_ops ApplyAdam): m,v EMA; w -= lr_t * m / (sqrt(v) + eps)
    m = b1 * m + (1.0f - b1) * g;
    v = b2 * v + (1.0f - b2) * g * g;
    w -= lr_t * m / (sqrtf(v) + eps);
}

// ---------------------------------------------------------------------------------------------
// input assembly (core/utils.py:372-379 and :619-621 of the reference): done by the forward chain's input tiles
// ---------------------------------------------------------------------------------------------
// Where batch row (e, b) lives in the caller's tensors.  Direct: row r of [E*B, .] tensors.  Indexed (`fit`'s windowed
// dataset, cadm_train_step_rows): rid = idx[r], window w = row_w[rid], future offset f = row_f[rid]; per-step tensors are
// [N, F, .] (source row w*F + f), history tensors [N, .] (source row w).
struct RowMap {
    const long long *idx, *row_w, *row_f;
    int F, B;
    long long idx_ld;                 // idx[e * idx_ld + b]: a batch is a column slice of the [E, n_train] bootstrap matrix
};
__device__ __forceinline__ void map_row(const RowMap& m, long r, long& srow, long& swin) {
    if (!m.idx) { srow = r; swin = r; return; }
    const long long rid = m.idx[(r / m.B) * m.idx_ld + r % m.B];
    swin = m.row_w[rid];
    srow = swin * m.F + m.row_f[rid];
}

struct ChainAsm {         // raw batch -> normalised network inputs
    RowMap map;
    const float *act, *cp_obs, *cp_act;
    const float *obs_mean, *obs_std, *act_mean, *act_std, *cp_obs_mean, *cp_obs_std, *cp_act_mean, *cp_act_std;
    int D, A, P, ncpo, ncpa, env;
    const int* spec_feat;     // CADM_ENV_SPEC: per feature, source obs dim | op << 8 (cadm_set_env_spec); else null
};

// ---------------------------------------------------------------------------------------------
// loss terms and their reductions (dynamics.py:269-314): parameters of the forward chain's closing phase (chain_loss_phase)
// ---------------------------------------------------------------------------------------------
struct LossP {
    RowMap map;
    const float *mu, *lv, *bmu;              // head outputs [E*B, D]
    const float *delta, *back_delta;         // raw targets [E*B, D] (or through map)
    const float *dmean, *dstd, *bdmean, *bdstd, *maxlv, *minlv;
    float *dMu, *dLv, *dBmu;                 // d loss / d head pre-activation
    long n;                                  // E*B*D
    int D, B, det, has_back;
    float back_coeff;
    int Dp;                                  // row stride of dMu / dLv / dBmu (D rounded up to 4: zero columns behind D)
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// Deterministic reductions of the loss terms.  out: [4 + 2D] = {mse, mu_loss, var_loss, back_mse, d/d max_logvar [D],
// d/d min_logvar [D]}.  The workgroup that finishes last turns the sums into losses_out = [mse, back_mse, recon]
// (dynamics.py:505-507: recon = loss - reg - coeff * l2) and, when training a probabilistic model, applies Adam to
// max/min_logvar (data term + the 0.01 regulariser of dynamics.py:308) -- nothing else reads them until the next step.
struct ReduceP {
    float* part;                                   // [workgroups][4 + 2D] per-workgroup partial sums
    int D; float* out; unsigned* counter;
    int det, has_back; float back_coeff; float* losses_out;
    int adam_mm;                                   // 1: update max/min_logvar
    float *maxlv, *minlv, *mx_m, *mx_v, *mn_m, *mn_v;
    float lr_t, b1, b2, eps;
};

__device__ __forceinline__ float wave_sum_fixed(float v) {            // xor butterfly: the same order on every run
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------
// chain kernel: a list of GEMM stages over a 16-row batch tile held in LDS
// ---------------------------------------------------------------------------------------------
// Pointers read out of a stage table are generic to the compiler (flat_load: slower, and it ties the vector-memory
// counter to the LDS one); they all point to device memory, so say so.
typedef __attribute__((address_space(1))) const float* gcptr;
typedef __attribute__((address_space(1))) float* gptr;
__device__ __forceinline__ gcptr as_global(const float* p) { return (gcptr)p; }
__device__ __forceinline__ gptr as_global(float* p) { return (gptr)p; }
#define CH_ROWS 16
// Two flavours of the chain kernel (template parameter NW = waves per workgroup), chosen per launch by the number of work items:
//   NW = 8  ONE workgroup per CU, two waves per SIMD: one wave's LDS / load / scalar work overlaps the other's MFMAs.  The latency
//           flavour: a step at the reference's batch size (256 rows x 5 members x 2 nets = 160 work items) is one partial round of the chip.
//   NW = 4  THREE workgroups per CU (168 registers per wave, 53.6 KB of LDS each): three independent 16-row chains per CU, so one
//           chain's epilogue / barrier / stage start (36 % of a stage, chain_timing) runs beside the others' MFMAs.  The throughput
//           flavour, for launches of more work items than CUs: B = 4096 1.633 -> 1.200 ms per step (0.177 -> 0.241 of the fp32
//           matrix peak), B = 1024 0.410 -> 0.340; at B = 256 it would be 0.144 instead of 0.120 ms (profiles/r5_train_scaling.md).
//           With the work items spread over all eight XCDs (xcd_spread_item: the member-affine mapping left three idle) 0.88 ms = 0.328.
#define CH_WAVES_MAX 8
#define CH_THREADS_MAX (64 * CH_WAVES_MAX)
#define CH_RING 8             // operand blocks (16 k x 2 tiles) of a wave's ring; CH_RING - 1 are in flight
#define CH_MAXSTAGE 20
#define CH_BLK_FLOATS 256     // one operand block of one tile: 64 lanes x float4

// A GEMM stage computes acc[16 rows x N] = src[16 x K] * Bop[K x N] for up to two column SEGMENTS (e.g. the mu and
// logvar heads side by side), each with its own operand stream, bias and outputs.  The operand stream is a packed copy
// of the layer (train_pack_kernel; kept current by dw_adam_kernel's epilogue): per member [k-block][tile][lane] float4,
// tile = 16 output columns, k-block = 16 k, lane (c, kq) holds Bop(16 t + 4 kq + i, 16 tile + c), i = 0..3 -- exactly
// the A operand of four v_mfma_f32_16x16x4_f32 k-steps, zero-padded in both directions.  A wave reads the 2 KB of its
// tile pair per k-block; the workgroup's waves -- and the member's other workgroups, which walk the same stages at the
// same time -- together read one contiguous window of the stream per k-block (all of the L2's channels, not the few
// that per-tile streams a fixed stride apart would hit).  The same load shape in every stage of every chain, forward
// or transposed.
struct ChainSeg {
    const float* P;        // packed operand [E][KB][tiles (even)][64][4]
    long sP;               // member stride (floats)
    const float *bias, *zprev;                           // bias [E][N]; zprev [E][B][ldz]: pre-activation whose act' scales the result
    float *out0, *out1;                                  // [E][B][ldo]: value before act_o / after
    int N, ldo, ldz, vec;                                // vec: N, ldo, ldz, dk0 all multiples of 4 -> 16-byte accesses
    int nt;                                              // tiles of the stream
    int pkB, pkC, pad;                                   // (host, finish of sync_programs) vec | nt << 8;  N | ldz << 16: the lookup of a wave's next
                                                         //  group reads these instead of the four fields (registers: see chain_group)
};
struct ChainStage {
    int KB, src, dst, dk0, act_d, act_o, ntp, tp1;       // KB: k-blocks; ntp: tile pairs (all segments); tp1: first pair of segment 1
    int zfill;                                           // zfill: columns N .. of the last tile are written as zeros
    unsigned char nxt[8];                                // wave slot w's next stage behind this one (index inside the chain; 31: none) | 0x80 if its
                                                         //  pair there (tile pair w) belongs to segment 1 -- filled by finish_chain_table (host)
    int pkA;                                             // (host) KB | src << 8 | tp1 << 16 | ntp << 24
    int pad[4];
    ChainSeg seg[2];
};
struct ChainLoad {        // input tile -> LDS: K columns of g0 (+ g1) [E][B][ld_in] become rows dk0 .. dk0 + K - 1 of buffer dst,
    const float *g0, *g1; // zeros up to row zero_to (the consumer's k loop runs whole 16-row blocks without masking)
    float* gsum;          // echo of the sum [E][B][ldg]
    int ld_in, ldg, K, dst, dk0, zero_to;
    int mode, pad;        // 0: as stored;  1..4: assembled from the raw batch (ChainAsm; formerly assemble_kernel): 1 = obs_preproc of
                          //    the g0 rows (obs or next obs), 2 = action, 3 / 4 = the context encoder's (obs, act) history
};
struct ChainArgs {
    const ChainStage* prog;
    int first[2], count[2];                              // stage range per chain (y)
    ChainLoad pre[2][4]; int npre[2];                    // the chain's inputs (kernel arguments: they are requested before the table is)
    ChainAsm asmp;
    int loss_on, loss_buf, loss_lv0, loss_slots, loss_final;   // forward launch of a training step: losses + head gradients behind the
                                                         //  heads; loss_final: this launch also sums the partials (evaluation)
    LossP lossp; ReduceP lossr;                          //  (head outputs in LDS buffer loss_buf: mu at rows 0.., logvar at rows loss_lv0..)
    int B, bufsz;                                        // rows per member, floats per LDS activation buffer
    int E, ny, ntiles, G, ips;                           // work decomposition, see chain_kernel
    int spread, per_xcd;                                 // spread: XCD x takes the x-th contiguous eighth of the (member-major) work items
    int y_base, slot_ny;                                 // loss phase: this launch's chain y counts as y + y_base of slot_ny (a forward pass split
                                                         //  into one launch per net, forward_nets: same terms, same partial-sum slots as the joint launch)
    unsigned long long* tfine;                           // (same item) wave 0's epilogue, per GEMM stage: [6 si ..] activation math done, LDS tile
                                                         // stored, global stores issued, next group looked up, its operands requested
    unsigned long long* tbuf;                            // cadm_dev_set_timing_buffer: clocks of member 0's first work item:
                                                         // [0..63] stage boundaries, [64 + 4 si ..] wave 0: group start, k loop end,
                                                         // epilogue end, barrier reached
};

typedef __attribute__((address_space(1))) const char* gcbytes;
typedef __attribute__((address_space(1))) const floatx4* gcptr4;
typedef float floatx2 __attribute__((ext_vector_type(2)));

// The operand ring lives in a[0:63], named literally: slot s holds block i (i % 8 == s) of the wave's two tiles in
// a[8 s : 8 s + 3] and a[8 s + 4 : 8 s + 7].  Loads and MFMAs on it are inline asm, for two reasons:
//  * hipcc cannot pipeline loads across a loop back edge (its s_waitcnt placement waits for every outstanding load at the
//    first use behind it), let alone across a stage boundary; asm loads are invisible to its counters and are ordered
//    with explicit `s_waitcnt vmcnt(n)`: vector-memory operations of a wave complete in issue order, so "at most n
//    younger operations outstanding" is exact when the n youngest are ring loads and conservative when compiler-issued
//    accesses (epilogue operands, z / h stores) sit between them;
//  * a ring held in compiler-allocated registers gets MOVED at control-flow merges (the stage loop, the conditional
//    refills): a copy of a register with a load in flight reads stale data, the hardware does not interlock that.
//    Registers the compiler never sees cannot be moved.  (It has no reason to touch AGPRs in this kernel -- the ISA
//    hygiene test checks that it does not.)
// Wait states the hazard recognizer cannot place inside asm (cdna_hip_programming.md 5.7): `s_nop 4` between a
// readfirstlane'd base and the load that reads it, `s_nop 1` between a VALU-written operand and the MFMA (ring_begin), 12 states between
// the last MFMA and the first reader of its accumulator (ring_done).
#define CH_RING_REGS                                                                                                                   \
    "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18", "a19",   \
        "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35", "a36", "a37",  \
        "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55",  \
        "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63"
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N < 63 ? N : 63) : "memory");
}
// Values read out of the LDS stage table are wave-uniform, but the compiler cannot know: make them scalar.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ gcbytes uni(gcbytes p) {
    const unsigned long long u = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return (gcbytes)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ gcbytes uni_ptr(const float* p) { return uni((gcbytes)as_global(p)); }

// LDS activation tile: element (k, row m) at ((k >> 2) * 16 + m) * 4 + (k & 3): the B operand of a k-block is one
// lane-linear ds_read_b128 (lane (m, kq) <- k = 16 t + 4 kq + 0..3), and a D fragment of the transposed product
// (lane (m, q) holds columns 4 q + 0..3 of its tile) is written back as one lane-linear ds_write_b128.
__device__ __forceinline__ int lds_at(int k, int m) { return ((k >> 2) * CH_ROWS + m) * 4 + (k & 3); }

struct ChainGroup {       // one wave's work in one stage: a tile pair
    int si, tp;           // stage, pair index (si < 0: none)
    int KB;
    gcbytes w0;           // block 0 of the pair (tile 1 right behind tile 0)
    int bstep;            // bytes from one k-block to the next
    int sg, nb, src;      // its segment, first column inside the segment, LDS buffer of the stage's input: looked up with the
                          // group (one stage ahead), so that nothing the k loop needs is read out of the table at stage start
    int ntp; unsigned nx; // the stage's tile pairs; ChainStage::nxt of this wave slot: what the NEXT lookup starts from (scalars, no LDS read)
};

// block i of the group -> ring slot S (both tiles); (uniform 64-bit base in SGPRs) + (32-bit per-lane byte offset)
template <int S>
__device__ __forceinline__ void ring_issue(const ChainGroup& g, int i, unsigned loff) {
    gcbytes p0 = g.w0 + (long)i * g.bstep;
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 a[%2*8:%2*8+3], %0, %1\n\tglobal_load_dwordx4 a[%2*8+4:%2*8+7], %0, %1 offset:1024"
                 :: "v"(loff), "s"(p0), "n"(S) : "memory", CH_RING_REGS);
}
// the first CH_RING - 1 blocks of a group: issued one stage ahead (before the previous group's stores and the barrier)
template <int S>
__device__ __forceinline__ void ring_prologue_from(const ChainGroup& g, unsigned loff) {
    if (S < g.KB) {
        ring_issue<S>(g, S, loff);
        if constexpr (S + 1 < CH_RING - 1) ring_prologue_from<S + 1>(g, loff);
    }
}
__device__ __forceinline__ void ring_prologue(const ChainGroup& g, unsigned loff) {
    if (g.si >= 0) ring_prologue_from<0>(g, loff);
}
// tail of a group (nothing left to issue): at most `rem` younger blocks may still be outstanding.  Three levels instead of
// seven: a taken scalar branch costs more than the MFMA it delays, and the blocks a coarser wait adds were issued at least
// four block times ago.
__device__ __forceinline__ void wait_blocks(int rem) {
    if (rem >= 4) wait_vmcnt<8>();
    else if (rem >= 2) wait_vmcnt<4>();
    else wait_vmcnt<0>();
}
static_assert(CH_RING == 8, "wait_blocks, the ring's register names and the slot arithmetic assume a ring of 8");
// acc += (weights of ring slot S, tile J, k-step U) x (activation column x): weights are the A operand, so a lane (m, q)
// of D holds columns 4 q + 0..3 of the tile for batch row m
template <int S, int J, int U>
__device__ __forceinline__ void ring_mfma(floatx4& acc, float x) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, a[%2], %1, %0" : "+v"(acc) : "v"(x), "n"(S * 8 + J * 4 + U));
}
// consume block i (slot S): refill the slot freed by block i - 1, wait for block i, 8 MFMAs
template <int S>
__device__ __forceinline__ void ring_step(const ChainGroup& g, int i, unsigned loff, const float* abase, floatx4 (&xa)[4],
                                          floatx4 (&acc)[2]) {
    const int rem = g.KB - 1 - i;
    if (rem >= CH_RING - 1) {
        ring_issue<(S + CH_RING - 1) % CH_RING>(g, i + CH_RING - 1, loff);
        wait_vmcnt<2 * (CH_RING - 1)>();
    } else {
        wait_blocks(rem);
    }
    const int ia = i + 2 < g.KB ? i + 2 : g.KB - 1;
    xa[(S + 2) & 3] = *reinterpret_cast<const floatx4*>(abase + CH_BLK_FLOATS * ia);
    __builtin_amdgcn_sched_barrier(0);     // keep the LDS read two blocks ahead of its use
    const floatx4 x = xa[S & 3];
    ring_mfma<S, 0, 0>(acc[0], x[0]); ring_mfma<S, 1, 0>(acc[1], x[0]);
    ring_mfma<S, 0, 1>(acc[0], x[1]); ring_mfma<S, 1, 1>(acc[1], x[1]);
    ring_mfma<S, 0, 2>(acc[0], x[2]); ring_mfma<S, 1, 2>(acc[1], x[2]);
    ring_mfma<S, 0, 3>(acc[0], x[3]); ring_mfma<S, 1, 3>(acc[1], x[3]);
}
template <int S>
__device__ __forceinline__ void ring_steps(const ChainGroup& g, int i0, unsigned loff, const float* abase, floatx4 (&xa)[4],
                                           floatx4 (&acc)[2]) {
    if (S == 0 || i0 + S < g.KB) {
        ring_step<S>(g, i0 + S, loff, abase, xa, acc);
        if constexpr (S + 1 < CH_RING) ring_steps<S + 1>(g, i0, loff, abase, xa, acc);
    }
}
// VALU-written accumulators (the zeroing moves) -> first MFMA.  The MFMAs' other operands never come out of a VALU
// instruction: weights are written by the ring's loads, activations by ds_read_b128 (tests/test_isa_hygiene.py checks the
// instruction in front of every MFMA of this kernel).
__device__ __forceinline__ void ring_begin(floatx4 (&acc)[2]) { asm volatile("s_nop 1" : "+v"(acc[0]), "+v"(acc[1])); }
__device__ __forceinline__ void ring_done(floatx4 (&acc)[2]) {   // last MFMA -> first VALU read of its accumulator (8-pass op)
    asm volatile("s_nop 11" : "+v"(acc[0]), "+v"(acc[1]));
}

__device__ __forceinline__ ChainGroup group_of(const ChainStage* stg, int si, int tp, int e, int wave) {
    const ChainStage& st = stg[si];
    const int tp1 = uni(st.tp1);
    const int sg = tp >= tp1 ? 1 : 0;
    const ChainSeg& seg = st.seg[sg];
    ChainGroup g;
    g.si = si; g.tp = tp; g.KB = uni(st.KB);
    g.sg = sg; g.nb = 32 * (tp - (sg ? tp1 : 0)); g.src = uni(st.src);
    g.w0 = uni((gcbytes)(as_global(seg.P) + (long)e * seg.sP + (long)(2 * (tp - (sg ? tp1 : 0))) * CH_BLK_FLOATS));
    g.bstep = uni(seg.nt) * (CH_BLK_FLOATS * 4);
    g.ntp = uni(st.ntp); g.nx = (unsigned)uni((int)st.nxt[wave]);
    return g;
}
// the wave's next tile pair behind (si, tp): the next pass of the same stage, else its pair in the next GEMM stage
template <int NW>
__device__ __forceinline__ ChainGroup next_group(const ChainStage* stg, int nst, int si, int tp, int wave, int e) {
    if (si >= 0 && tp + NW < uni(stg[si].ntp)) return group_of(stg, si, tp + NW, e, wave);
    for (int sj = si + 1; sj < nst; ++sj)
        if (wave < uni(stg[sj].ntp)) return group_of(stg, sj, wave, e, wave);
    ChainGroup g;
    g.si = -1; g.tp = 0; g.KB = 0; g.w0 = nullptr; g.bstep = 0; g.sg = 0; g.nb = 0; g.src = 0; g.ntp = 0; g.nx = 31;
    return g;
}

// Epilogue operands of a group (bias, act'(z) source): lane (m, q) needs columns 4 q + 0..3 of both tiles for row m.
// Requested one stage ahead, right before the group's first ring blocks -- so that, in issue order, nothing but ring
// loads follows a ring load and the k loop's vmcnt counts are exact (clamped, never predicated).
struct ChainOps { floatx4 bv[2], zp[2]; };
__device__ __forceinline__ void load_ops(const ChainStage* stg, const ChainGroup& g, int e, int B, int row0, int lane, ChainOps& o) {
    if (g.si < 0) return;
    const ChainStage& st = stg[g.si];
    const int m = lane & 15, q = lane >> 4;
    const int tp1 = uni(st.tp1);
    const int sg = g.tp >= tp1 ? 1 : 0;
    const ChainSeg& seg = st.seg[sg];
    const int nb = 32 * (g.tp - (sg ? tp1 : 0));
    const int N = uni(seg.N), ldz = uni(seg.ldz);
    const bool VEC = uni(seg.vec) != 0;
    gcbytes p_bias = uni_ptr(seg.bias), p_z = uni_ptr(seg.zprev);
    const bool has_z = p_z != nullptr, has_b = p_bias != nullptr;
    const long mrow = (long)e * B;
    const int row = row0 + m, rowc = row < B ? row : B - 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n0 = nb + 16 * j + 4 * q;
        if (VEC) {
            const int nc = n0 < N ? n0 : 0;
            gcbytes bb = has_b ? p_bias + ((long)e * N + nc) * 4 : g.w0;
            gcbytes zb = has_z ? p_z + ((mrow + rowc) * ldz + nc) * 4 : g.w0;
            o.bv[j] = *reinterpret_cast<gcptr4>(bb);
            o.zp[j] = *reinterpret_cast<gcptr4>(zb);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + r, nc = n < N ? n : N - 1;
                gcbytes bb = has_b ? p_bias + ((long)e * N + nc) * 4 : g.w0;
                gcbytes zb = has_z ? p_z + ((mrow + rowc) * ldz + nc) * 4 : g.w0;
                o.bv[j][r] = *reinterpret_cast<gcptr>(bb);
                o.zp[j][r] = *reinterpret_cast<gcptr>(zb);
            }
        }
    }
}

// One tile pair of a GEMM stage: k loop over the ring, epilogue.  At the end of the epilogue -- behind this group's
// stores -- the NEXT group's operands and first ring blocks are requested: by the time the stage-end barrier has been
// passed they have landed, so a stage starts with MFMAs instead of an L2 round trip.
template <int NW>
__device__ __forceinline__ void chain_group(const ChainStage* stg, int nst, int wave, const ChainGroup& g, ChainGroup& nxt, ChainOps& ops,
                                            float* bufs, int bufsz, int e, int B, int row0, int lane, unsigned long long* dbg,
                                            unsigned long long* fine) {
    if (dbg) dbg[0] = __builtin_readcyclecounter();
    const ChainStage& st = stg[g.si];
    const int m = lane & 15, q = lane >> 4;
    const unsigned loff = 16u * (unsigned)lane;
    const int sg = g.sg, rtp1 = st.tp1;
    const ChainSeg& seg = st.seg[sg];
    const int nb = g.nb;                                  // first column of the pair inside its segment
    // The epilogue's stage constants are REQUESTED here (plain LDS reads into VGPRs, all independent) and made scalar behind the
    // k loop: read and used in front of it, their two or three dependent LDS round trips delayed every stage's first MFMA.
    const int rN = seg.N, rldo = seg.ldo, rdk0 = st.dk0, rdst = st.dst, ract_d = st.act_d, ract_o = st.act_o, rzf = st.zfill, rvec = seg.vec;
    const float *rbias = seg.bias, *rz = seg.zprev;
    float *ro0 = seg.out0, *ro1 = seg.out1;
    const long mrow = (long)e * B;                        // first row of this member in the [E][B][.] tensors
    const int row = row0 + m;
    const floatx4 bv[2] = {ops.bv[0], ops.bv[1]}, zp[2] = {ops.zp[0], ops.zp[1]};
    const int n0[2] = {nb + 4 * q, nb + 16 + 4 * q};
    floatx4 acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
    {   // ---- k loop: block i of the pair sits in ring slot i % 8; its loads were issued 7 blocks earlier ----
        const float* abase = bufs + g.src * bufsz + 4 * lane;             // activation block i: + 256 i floats
        floatx4 xa[4];
        xa[0] = *reinterpret_cast<const floatx4*>(abase);
        xa[1] = *reinterpret_cast<const floatx4*>(abase + CH_BLK_FLOATS * (g.KB > 1 ? 1 : 0));
        ring_begin(acc);
#pragma unroll 1
        for (int i0 = 0; i0 < g.KB; i0 += CH_RING) ring_steps<0>(g, i0, loff, abase, xa, acc);
        ring_done(acc);
    }
    if (dbg) dbg[1] = __builtin_readcyclecounter();
    // stage constants -> SGPRs: scalar address bases, uniform branches on the activation kinds
    const int N = uni(rN), ldo = uni(rldo), dk0 = uni(rdk0), dsti = uni(rdst), tp1 = uni(rtp1);
    const int act_d = uni(ract_d), act_o = uni(ract_o), zfill = uni(rzf);
    const bool VEC = uni(rvec) != 0;
    gcbytes p_o0 = uni_ptr(ro0), p_o1 = uni_ptr(ro1);
    const bool has_z = uni_ptr(rz) != nullptr, has_b = uni_ptr(rbias) != nullptr, s0 = p_o0 != nullptr, s1 = p_o1 != nullptr;
    floatx4 v0[2];                                // [tile][r]: before the output activation
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) v0[j][r] = acc[j][r] + (has_b ? bv[j][r] : 0.0f);
    if (has_z) {
        if (act_d == ACT_SWISH) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float z = zp[j][r], sg_ = sigmoid_fast(z);
                    v0[j][r] *= sg_ * (1.0f + z * (1.0f - sg_));
                }
        } else if (act_d == ACT_RELU) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) v0[j][r] = zp[j][r] > 0.0f ? v0[j][r] : 0.0f;
        } else if (act_d == ACT_TANH) {          // 1 - tanh(z)^2 = 4 s (1 - s), s = sigmoid(2z)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) { const float sg_ = sigmoid_fast(2.0f * zp[j][r]); v0[j][r] *= 4.0f * sg_ * (1.0f - sg_); }
        } else if (act_d == ACT_SIGMOID) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) { const float sg_ = sigmoid_fast(zp[j][r]); v0[j][r] *= sg_ * (1.0f - sg_); }
        }
    }
    // global stores: (uniform base of this member) + 32-bit byte offset (host checks B * ldo * 4 < 2^32).  The value before the output
    // activation is stored as soon as it exists -- not next to the activated one: eight registers fewer are live through the activation math.
    typedef __attribute__((address_space(1))) float* gfp;
    typedef __attribute__((address_space(1))) floatx4* gf4p;
    auto store_rows = [&](gcbytes base, const floatx4 (&v)[2]) {
        if (row >= B) return;
        if (VEC) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (n0[j] >= N) continue;
                *(gf4p)(base + 4u * (unsigned)(row * ldo + n0[j])) = v[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0[j] + r;
                    if (n >= N) continue;
                    *(gfp)(base + 4u * (unsigned)(row * ldo + n)) = v[j][r];
                }
        }
    };
    if (s0) store_rows(p_o0 + mrow * ldo * 4, v0);
    floatx4 v1[2];                                // ... and after
    if (act_o == ACT_SWISH) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) v1[j][r] = v0[j][r] * sigmoid_fast(v0[j][r]);
    } else if (act_o == ACT_RELU) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) v1[j][r] = fmaxf(v0[j][r], 0.0f);
    } else if (act_o == ACT_TANH) {              // as the planner: 2 sigmoid(2z) - 1, odd series near 0 where that cancels
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x = v0[j][r], x2 = x * x;
                const float ser = x * fmaf(x2, fmaf(x2, fmaf(x2, -0.05396825396825397f, 0.13333333333333333f), -0.3333333333333333f), 1.0f);
                v1[j][r] = fabsf(x) < 0.1f ? ser : fmaf(2.0f, sigmoid_fast(2.0f * x), -1.0f);
            }
    } else if (act_o == ACT_SIGMOID) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) v1[j][r] = sigmoid_fast(v0[j][r]);
    } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) v1[j] = v0[j];
    }
    // The wave's next group -- the next pass of this stage (tile pair tp + NW), else its pair in the stage the table names (ChainStage::nxt,
    // precomputed on the host) -- is known from scalars that came with THIS group's descriptor, so its whole descriptor is ONE batch of LDS reads,
    // requested here -- behind the activation math, whose registers it would compete for: hipcc parks values in the ring's AGPRs otherwise -- and
    // consumed behind this group's stores, which run under its latency.  (Until round 5 the
    // lookup walked the table behind the stores -- stage's pair count, next stage's, the group's fields, the operands' fields: three to four
    // dependent LDS round trips, 2-3 k of an epilogue's 5-6 k cycles under load, tools/chain_timing.py.)
    const unsigned nx = g.nx;
    const bool same_stage = g.tp + NW < g.ntp;
    const int nsi = same_stage ? g.si : ((nx & 31u) == 31u ? -1 : (int)(nx & 31u));
    const int ntpp = same_stage ? g.tp + NW : wave;
    const int nsg = same_stage ? (ntpp >= tp1 ? 1 : 0) : (int)(nx >> 7);
    struct { int A, B, C, nx; const float *P, *bias, *z; long sP; } rq;
    auto request_next = [&]() {
        const ChainStage& ns = stg[nsi < 0 ? 0 : nsi];
        const ChainSeg& nseg = ns.seg[nsg];
        rq.A = ns.pkA; rq.B = nseg.pkB; rq.C = nseg.pkC; rq.nx = ns.nxt[wave];
        rq.P = nseg.P; rq.bias = nseg.bias; rq.z = nseg.zprev; rq.sP = nseg.sP;
    };
    if constexpr (NW == 8) request_next();
    if (fine) fine[0] = __builtin_readcyclecounter();
    if (dsti >= 0) {
        float* dst = bufs + dsti * bufsz;
        const int sg0 = sg ? 32 * tp1 : 0;                // a second segment's columns follow the first's tile pairs
        if (VEC) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                *reinterpret_cast<floatx4*>(dst + lds_at(dk0 + sg0 + n0[j], m)) = n0[j] < N ? v1[j] : floatx4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0[j] + r;
                    if (n < N || zfill) dst[lds_at(dk0 + sg0 + n, m)] = n < N ? v1[j][r] : 0.0f;
                }
        }
    }
    if constexpr (NW != 8) request_next();      // (the 4-wave flavour has 84 VGPRs: requested in front of the activation tile's stores, hipcc parks values in the ring's AGPRs)
    if (fine) fine[1] = __builtin_readcyclecounter();
    if (s1) store_rows(p_o1 + mrow * ldo * 4, v1);
    if (fine) fine[2] = __builtin_readcyclecounter();
    // ---- the wave's next group: descriptor (requested behind the k loop, see above) -> scalars, its epilogue operands and first ring blocks ----
    nxt.si = nsi; nxt.tp = ntpp; nxt.sg = nsg;
    if (nsi >= 0) {
        const int pA = uni(rq.A), pB = uni(rq.B), pC = uni(rq.C);
        const int qtp1 = (pA >> 16) & 255, qN = pC & 0xffff, qldz = (int)((unsigned)pC >> 16);
        const bool qVEC = (pB & 1) != 0;
        const int tp_in = ntpp - (nsg ? qtp1 : 0);                         // pair index inside its segment
        nxt.KB = pA & 255; nxt.src = (pA >> 8) & 255; nxt.nb = 32 * tp_in;
        nxt.w0 = uni((gcbytes)(as_global(rq.P) + (long)e * rq.sP + (long)(2 * tp_in) * CH_BLK_FLOATS));
        nxt.bstep = (pB >> 8) * (CH_BLK_FLOATS * 4);
        nxt.ntp = (int)((unsigned)pA >> 24); nxt.nx = (unsigned)uni(rq.nx);
        gcbytes p_bias = uni_ptr(rq.bias), p_z = uni_ptr(rq.z);
        const bool hz = p_z != nullptr, hb = p_bias != nullptr;
        const int rowc = row < B ? row : B - 1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c0 = nxt.nb + 16 * j + 4 * q;
            if (qVEC) {
                const int nc = c0 < qN ? c0 : 0;
                gcbytes bb = hb ? p_bias + ((long)e * qN + nc) * 4 : nxt.w0;
                gcbytes zb = hz ? p_z + ((mrow + rowc) * qldz + nc) * 4 : nxt.w0;
                ops.bv[j] = *reinterpret_cast<gcptr4>(bb);
                ops.zp[j] = *reinterpret_cast<gcptr4>(zb);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = c0 + r, nc = n < qN ? n : qN - 1;
                    gcbytes bb = hb ? p_bias + ((long)e * qN + nc) * 4 : nxt.w0;
                    gcbytes zb = hz ? p_z + ((mrow + rowc) * qldz + nc) * 4 : nxt.w0;
                    ops.bv[j][r] = *reinterpret_cast<gcptr>(bb);
                    ops.zp[j][r] = *reinterpret_cast<gcptr>(zb);
                }
            }
        }
    } else {
        nxt.KB = 0; nxt.w0 = nullptr; nxt.bstep = 0; nxt.nb = 0; nxt.src = 0; nxt.ntp = 0; nxt.nx = 31;
    }
    if (fine) fine[3] = fine[4] = __builtin_readcyclecounter();      // (one stamp for both: a per-thread branch inside the uniform one above makes hipcc treat the group's scalars as per-lane values)
    ring_prologue(nxt, loff);
    if (dbg) dbg[2] = __builtin_readcyclecounter();
}

// The chain's input tiles.  Element idx of a tile = (16-column block, row, column in the block): a wave covers 4 rows x 16
// columns -- 4 segments of 64 bytes per load (the LDS-linear order, 16 rows x 4 columns, costs 16 segments per load and
// made this prologue slower than the separate assembly kernel it replaces), a 4-way bank conflict on the LDS side.
// Two phases, so that the loads of ALL of a chain's tiles (and the stage table's) are in flight together: fetch requests the
// raw operands of a tile's elements -- the value, and for the assembled tiles its mean and std --, commit turns them into
// inputs.  One global round trip for the whole kernel prologue instead of one per tile and operand.  A tile has ONE source
// per operand (the assembled inputs are two tiles each: observation columns, action columns), so an element's addresses are
// base + column: nothing for hipcc to branch on between the loads.
template <int NU>
struct ChainIn { float x[NU], a[NU]; };      // (the third operand -- the std of an assembled column -- is fetched at commit time: an L2 hit by then,
                                             //  and a third fewer registers per element in flight across the one HBM round trip)
struct ChainInSrc {
    gcptr x0, a0, b0;
    int hc;                   // half-cheetah obs_preproc (columns 0..2 <- o[1], sin o[2], cos o[2])
    int shift;                // ant obs_preproc: column f <- o[f + 1]
    const int* sf;            // env spec: column f <- op(o[sf[f] & 255]), op = sf[f] >> 8 (0 id, 1 sin, 2 cos)
    bool rok, two;
    long grow;
};
__device__ __forceinline__ ChainInSrc chain_input_src(const ChainLoad& d, const ChainAsm& ap, int e, int B, int row0, int tid) {
    ChainInSrc r;
    const int row = row0 + ((tid >> 4) & 15);                 // (a thread's elements are 256 apart: it keeps its row)
    r.rok = row < B;
    r.grow = (long)e * B + (r.rok ? row : 0);
    long srow = r.grow, swin = r.grow;
    if (d.mode) map_row(ap.map, r.grow, srow, swin);
    r.hc = 0; r.shift = 0; r.sf = nullptr; r.two = false;
    if (d.mode == 0) {
        r.x0 = as_global(d.g0) + r.grow * d.ld_in;
        r.two = d.g1 != nullptr;
        r.a0 = r.two ? as_global(d.g1) + r.grow * d.ld_in : r.x0;
        r.b0 = r.x0;
    } else if (d.mode == 1) {          // preprocessed observation columns of (next) obs rows
        r.x0 = as_global(d.g0) + srow * ap.D; r.a0 = as_global(ap.obs_mean); r.b0 = as_global(ap.obs_std);
        r.hc = ap.env == CADM_ENV_HALFCHEETAH;
        r.shift = ap.env == CADM_ENV_ANT;
        r.sf = ap.spec_feat;
    } else if (d.mode == 2) {          // action columns
        r.x0 = as_global(ap.act) + srow * ap.A; r.a0 = as_global(ap.act_mean); r.b0 = as_global(ap.act_std);
    } else if (d.mode == 3) {          // context encoder: observation history
        r.x0 = as_global(ap.cp_obs) + swin * ap.ncpo; r.a0 = as_global(ap.cp_obs_mean); r.b0 = as_global(ap.cp_obs_std);
    } else {                           // context encoder: action history
        r.x0 = as_global(ap.cp_act) + swin * ap.ncpa; r.a0 = as_global(ap.cp_act_mean); r.b0 = as_global(ap.cp_act_std);
    }
    return r;
}
template <int NT, int NU>
__device__ __forceinline__ void chain_input_fetch(const ChainLoad& d, const ChainInSrc& r, int base, int tid, ChainIn<NU>& q) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int idx = base + u * NT + tid;
        const int k = (idx >> 8) * 16 + (idx & 15);
        const int j = k < d.K ? k : 0;
        const int jx = r.sf ? (r.sf[j] & 255) : r.hc ? (j == 0 ? 1 : j <= 2 ? 2 : j) : j + r.shift;     // obs_preproc's source column of feature j
        q.x[u] = r.x0[jx];
        q.a[u] = r.a0[j];
    }
}
template <int NT, int NU>
__device__ __forceinline__ void chain_input_commit(const ChainLoad& d, const ChainInSrc& r, int base, int tid, const ChainIn<NU>& q,
                                                   float* bufs, int bufsz) {
    float* dst = bufs + d.dst * bufsz;
    const int m = (tid >> 4) & 15;
    float sd[NU];
    if (d.mode != 0) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int idx = base + u * NT + tid;
            const int k = (idx >> 8) * 16 + (idx & 15);
            sd[u] = r.b0[k < d.K ? k : 0];
        }
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int idx = base + u * NT + tid;
        const int k = (idx >> 8) * 16 + (idx & 15);
        const bool ok = k < d.K && r.rok;
        float x;
        if (d.mode == 0) {
            x = r.two ? q.x[u] + q.a[u] : q.x[u];
        } else {
            float t = q.x[u];
            if (u == 0 && r.hc && base == 0) {              // (columns 1 and 2 only exist in a thread's first element; hc: mode 1)
                if (k == 1) t = sinf(t);
                else if (k == 2) t = cosf(t);
            }
            if (r.sf) {                                     // env spec (mode 1): the same sinf / cosf as the half-cheetah path
                const int op = r.sf[k < d.K ? k : 0] >> 8;
                if (op == 1) t = sinf(t);
                else if (op == 2) t = cosf(t);
            }
            x = (t - q.a[u]) / (sd[u] + 1e-10f);
        }
        x = ok ? x : 0.0f;
        if (d.dk0 + k < d.zero_to) dst[lds_at(d.dk0 + k, m)] = x;
        if (ok && d.gsum) as_global(d.gsum)[r.grow * d.ldg + k] = x;
    }
}

// Work decomposition.  Workgroups are dispatched round-robin over the 8 XCDs (linear id % 8), and every XCD has
// its own L2, so the launch is 1-D and a member's work items (batch tile x chain) are all sent to the same
// G = 8 / E XCDs (E <= 8; one XCD per member for the 5-member ensemble: 32 items on its 32 CUs): a member's
// weights are then filled into exactly one L2 instead of eight.
__device__ __forceinline__ bool xcd_affine_item(int E, int G, int ips, int per, int& e, int& item) {
    const int lin = blockIdx.x, xcd = lin & 7, j = lin >> 3;
    e = xcd / G + 8 * (j / ips);
    item = (j % ips) * G + xcd % G;
    return e < E && item < per;
}
// More work items than the affine mapping's XCDs can hold in one round (large batches): that mapping leaves 8 - G E XCDs idle -- three
// of eight for the 5-member ensemble, found in round 5 with the per-item clocks: an item took 160 k cycles, the launch 6 rounds of them.
// Then XCD x takes the x-th CONTIGUOUS eighth of the member-major item list instead (as dw_adam_kernel does): every XCD is busy, and
// its L2 still holds the weights of at most two members (E <= 8).
__device__ __forceinline__ bool xcd_spread_item(int E, int per_xcd, int per, int& e, int& item) {
    const int g = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (g >= E * per) return false;
    e = g / per;
    item = g - e * per;
    return true;
}

// Sums of the workgroups' partials in a fixed order (G groups of threads take contiguous chunks of slots -- loads eight at a
// time: one after the other they are 160 dependent round trips, + 48 us measured --, then the chunks are added in order), the
// three reported losses, and Adam on max / min_logvar (data term + the 0.01 regulariser of dynamics.py:308).
template <int NT, bool COHERENT>
__device__ __forceinline__ void loss_finalize(const ReduceP& r, int slots, float* scr, int tid) {
    const int D = r.D, NQ = 4 + 2 * D;
    float* red = r.out;
    const int W = NQ < NT ? NQ : NT, G = NT / W, CS = (slots + G - 1) / G;
    for (int q0 = 0; q0 < NQ; q0 += NT) {
        const int q = q0 + tid % W, g = tid / W;
        if (g < G && q < NQ) {
            float v = 0.0f;
            const int w1 = (g + 1) * CS < slots ? (g + 1) * CS : slots;
            for (int w0 = g * CS; w0 < w1; w0 += 8) {
                float x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float* src = r.part + (size_t)(w0 + u < w1 ? w0 + u : w1 - 1) * NQ + q;
                    x[u] = COHERENT ? __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *src;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) v += w0 + u < w1 ? x[u] : 0.0f;
            }
            scr[g * W + (q - q0)] = v;
        }
        __syncthreads();
        if (tid < W && q0 + tid < NQ) {
            float tot = 0.0f;
            for (int gg = 0; gg < G; ++gg) tot += scr[gg * W + tid];
            red[q0 + tid] = tot;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float mse = red[0], mu_loss = red[1], var_loss = red[2], back = red[3];
        float recon = r.det ? mse : mu_loss + var_loss;
        if (r.has_back) recon += r.back_coeff * back;
        r.losses_out[0] = mse;
        r.losses_out[1] = r.has_back ? back : 0.0f;
        r.losses_out[2] = recon;
    }
    if (r.adam_mm && tid < 2 * D) {
        const bool mx = tid < D;
        const int d = mx ? tid : tid - D;
        float* w = (mx ? r.maxlv : r.minlv) + d;
        float* m = (mx ? r.mx_m : r.mn_m) + d;
        float* v = (mx ? r.mx_v : r.mn_v) + d;
        float ww = *w, mm = *m, vv = *v;
        adam_update(ww, mm, vv, red[4 + tid] + (mx ? 0.01f : -0.01f), r.lr_t, r.b1, r.b2, r.eps);
        *w = ww; *m = mm; *v = vv;
    }
}

// Closing phase of the forward launch of a training step: the workgroup's 16 rows x D head outputs are still in LDS, so the
// loss terms, the head gradients and the workgroup's share of every reduction are taken here instead of in a launch of their
// own (9 us of pure latency).  Forward-net workgroups own terms {mse, mu_loss, var_loss, d/d max_logvar,
// d/d min_logvar}, backward-model workgroups back_mse.  Reductions in a fixed order throughout: a workgroup's partials
// (rows ascending), then -- by the workgroup that arrives last -- all partials in slot order: no float atomics, the result
// does not depend on which workgroup is last.  That one also finalises (losses_out, Adam on max / min_logvar), exactly as
// the separate loss / reduction launch of earlier rounds did.
// The normalised target of a thread's FIRST element (el = tid; the only one when 16 D <= 512): requested in the kernel prologue,
// a whole forward pass before it is needed -- its memory latency used to sit at the end of the launch.
__device__ __forceinline__ float chain_loss_target(const LossP& p, int e, int y, int row0, int el) {
    const int D = p.D, m = el / D, d = el - m * D, row = row0 + m;
    if (el >= CH_ROWS * D || row >= p.B) return 0.0f;
    long srow, swin;
    map_row(p.map, (long)e * p.B + row, srow, swin);
    const long si = srow * D + d;                                      // this element in the caller's target tensors
    return y == 0 ? (p.delta[si] - p.dmean[d]) / (p.dstd[d] + 1e-10f) : (p.back_delta[si] - p.bdmean[d]) / (p.bdstd[d] + 1e-10f);
}

template <int NW>
__device__ __forceinline__ void chain_loss_phase(const ChainArgs& a, float* bufs, float* scr, int e, int y, int row0, int tid, float tgt0) {
    constexpr int CH_THREADS = 64 * NW;
    const LossP& p = a.lossp;
    const ReduceP& r = a.lossr;
    const int D = p.D, B = p.B, nel = CH_ROWS * D, lane = tid & 63, wave = tid >> 6;
    const float* hb = bufs + a.loss_buf * a.bufsz;
    for (int el = tid; el < nel; el += CH_THREADS) {
        const int m = el / D, d = el - m * D, row = row0 + m;
        float tm[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (row < B) {
            const long grow = (long)e * B + row, i = grow * p.Dp + d;
            const float s = 1.0f / ((float)B * (float)D);             // reduce_mean over b then d; reduce_sum over e
            const float mu = hb[lds_at(d, m)];
            const float tgt = el == tid ? tgt0 : chain_loss_target(p, e, y, row0, el);     // (normalised target)
            if (y == 0) {
                const float t = tgt;
                const float diff = mu - t;
                tm[0] = diff * diff * s;                                                  // mse            (:273-274)
                if (p.det) {
                    p.dMu[i] = 2.0f * s * diff;
                    p.dLv[i] = 0.0f;
                } else {
                    const float mx = p.maxlv[d], mn = p.minlv[d], lv0 = hb[lds_at(a.loss_lv0 + d, m)];
                    const float u = mx - tf_softplus(mx - lv0);                           // core/utils.py:356
                    const float lvc = mn + tf_softplus(u - mn);                           // core/utils.py:357
                    const float invvar = expf(-lvc);                                      // :303
                    tm[1] = diff * diff * invvar * s;                                     // mu_loss        (:304-305)
                    tm[2] = lvc * s;                                                      // var_loss       (:306-307)
                    const float g_lvc = s * (1.0f - diff * diff * invvar);
                    const float s1 = sigmoidf_(u - mn), s2 = sigmoidf_(mx - lv0);         // softplus' = sigmoid
                    p.dMu[i] = 2.0f * s * diff * invvar;
                    p.dLv[i] = g_lvc * s1 * s2;
                    // 1 - sigmoid(x) = sigmoid(-x), evaluated as such: with min_logvar = -10 the factor is ~5e-5 and `1 - s1`
                    // would keep 3 of its digits (the autodiff graph's g - g s1 does cancel like that; this is the exact value)
                    tm[4] = g_lvc * s1 * sigmoidf_(lv0 - mx);                             // d / d max_logvar (without the 0.01 reg)
                    tm[5] = g_lvc * sigmoidf_(mn - u);                                    // d / d min_logvar
                }
            } else {
                const float tb = tgt;
                const float db = mu - tb;
                tm[3] = db * db * s;                                                      // back_mse       (:280-281)
                p.dBmu[i] = p.back_coeff * 2.0f * s * db;
            }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) scr[q * nel + el] = tm[q];
    }
    __syncthreads();
    const int NQ = 4 + 2 * D;
    const int slot = (e * a.slot_ny + y) * a.ntiles + row0 / CH_ROWS;      // (y: the caller passes y + y_base)
    float* part = r.part + (size_t)slot * NQ;
    if (wave < 4) {                                                // scalar terms: wave q sums scr[q][*]
        float v = 0.0f;
        for (int j = lane; j < nel; j += 64) v += scr[wave * nel + j];
        v = wave_sum_fixed(v);
        if (lane == 0) {
            if (a.loss_final) __hip_atomic_store(part + wave, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else part[wave] = v;
        }
    }
    {                                                              // per-dim terms: one thread per (bound, dim), rows ascending
        for (int o = (NW > 4 ? tid - 256 : tid); o >= 0 && o < 2 * D; o += 256) {
            const int which = o / D, d = o - which * D;
            float v = 0.0f;
            for (int m = 0; m < CH_ROWS; ++m) v += scr[(4 + which) * nel + m * D + d];
            if (a.loss_final) __hip_atomic_store(part + 4 + o, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else part[4 + o] = v;
        }
    }
    // Training step: the partials are ordinary stores; the sums are taken by a spare workgroup of the weight-gradient launch
    // (loss_finalize in dw_adam_kernel: the kernel boundary orders the two, nothing waits for anybody, and the reduction is off
    // the step's critical path).  Evaluation (no further launch): hand-off to the last workgroup WITHOUT an agent-scope fence --
    // a release fence writes back the XCD's whole L2, which at this point holds the megabytes of z / h the chain has just
    // stored (measured: + 48 us on the launch).  There the partials are device-coherent stores (sc1: written through, past
    // the non-coherent L2s) that have completed (vmcnt) before the arrival counter is bumped, and the last workgroup reads them
    // with device-coherent loads.  This is the "sc1 payload -> asm vmcnt(0) -> agent atomic flag / sc1 loads on the consumer" form
    // MI355X_MICROARCH.md lists as valid for gfx950 (handoff-flag, "drained sc1"); it is a statement about THIS target, which is
    // the only one the library is built for (Makefile: ARCH = gfx950), not about the HIP memory model in general.  Compiler side:
    // the asm wait carries a "memory" clobber and both __syncthreads() are workgroup fences, so no access moves across them.
    // tests/test_gpu_train.py::test_eval_losses_equal_the_training_steps_reduction pins the result (bit-equal to the two-launch
    // reduction, under load, many repetitions).
    if (!a.loss_final) return;
    int* const flag = reinterpret_cast<int*>(scr + (6 * nel > CH_THREADS ? 6 * nel : CH_THREADS));     // (launch_chain sizes scr)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) *flag = atomicInc(r.counter, a.loss_slots - 1) == (unsigned)(a.loss_slots - 1);     // wraps back to 0 for the next step
    __syncthreads();
    if (!*flag) return;
    loss_finalize<256, true>(r, a.loss_slots, scr, tid);      // (256 threads' chunking in BOTH flavours -- and in dw_adam_kernel's copy: the same sums, bit for bit)
}

template <int NW>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 3) void chain_kernel(const ChainArgs a) {
    constexpr int CH_THREADS = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) float chain_smem[];
    ChainStage* const stg = reinterpret_cast<ChainStage*>(chain_smem);
    float* const bufs = chain_smem + (CH_MAXSTAGE * sizeof(ChainStage)) / sizeof(float);
    const int tid = threadIdx.x, lane = tid & 63, wave = uni(tid >> 6);
    // The argument block is ~1 KB (input tiles, assembly pointers): read where it is used, its 64-byte lines arrive one
    // dependent scalar-memory round trip after the other (4.7 k cycles of prologue were measured that way even for the
    // smallest chain).  Touch every line now, in one batch.
    {
        typedef __attribute__((address_space(4))) const int* kargp;
        kargp ka = (kargp)__builtin_amdgcn_kernarg_segment_ptr();
        int sink = 0;
#pragma unroll
        for (unsigned o = 0; o < sizeof(ChainArgs); o += 64) sink += ka[o / 4];
        asm volatile("" ::"s"(sink));
    }
    int e, item;
    const int per = a.ntiles * a.ny;
    if (a.spread ? !xcd_spread_item(a.E, a.per_xcd, per, e, item) : !xcd_affine_item(a.E, a.G, a.ips, per, e, item)) return;
    const int y = item / a.ntiles, row0 = (item - y * a.ntiles) * CH_ROWS, B = a.B;
    const int nst = y ? a.count[1] : a.count[0];
    const bool timed0 = a.tbuf && item == 0 && e == 0 && tid == 0;
    if (timed0) a.tbuf[200] = __builtin_readcyclecounter();
    // stage table of this chain -> LDS (one memory latency instead of one per stage); requested first, stored behind the
    // input tiles, which are described by kernel arguments and so are on their way before the table has arrived
    constexpr int TW = (CH_MAXSTAGE * (int)(sizeof(ChainStage) / sizeof(int)) + CH_THREADS - 1) / CH_THREADS;
    int tv[TW];
    const int nw = nst * (int)(sizeof(ChainStage) / sizeof(int));
    {
        const int* g = reinterpret_cast<const int*>(a.prog + (y ? a.first[1] : a.first[0]));
#pragma unroll
        for (int u = 0; u < TW; ++u) {
            const int i = tid + u * CH_THREADS;
            tv[u] = g[i < nw ? i : 0];
        }
    }
    {
        // (descriptors by value at static kernel-argument offsets: indexing them with the runtime y makes every field access
        //  a scalar memory load of its own -- 13 k cycles of prologue were measured that way)
        const int np = y ? a.npre[1] : a.npre[0];
        const ChainLoad d0 = y ? a.pre[1][0] : a.pre[0][0], d1 = y ? a.pre[1][1] : a.pre[0][1], d2 = y ? a.pre[1][2] : a.pre[0][2],
                        d3 = y ? a.pre[1][3] : a.pre[0][3];
        // elements per thread requested in one go -- two registers each: value and mean (or second summand); the std follows at commit
        // time --: 8 / 4 / 2 / 2 (8 waves: 128 / 64 / 32 / 32 columns) and 12 / 4 / 2 / 2 (4 waves: 192 / 64 / 32 / 32): the reference's
        // input tiles (180 + 60 history columns, 20 + 6) in ONE round trip to HBM; wider tiles loop.  The 4-wave flavour's 84 VGPRs do not
        // hold that: hipcc parks values in AGPRs here -- harmless in front of the first ring load, and only there
        // (tests/test_isa_hygiene.py checks from the first ring load on).
        constexpr int Q0 = NW == 8 ? 8 : 12, Q1 = 4, Q2 = 2;
        ChainIn<Q0> q0;
        ChainIn<Q1> q1;
        ChainIn<Q2> q2, q3;
        const ChainInSrc r0 = chain_input_src(d0, a.asmp, e, B, row0, tid), r1 = chain_input_src(np > 1 ? d1 : d0, a.asmp, e, B, row0, tid),
                         r2 = chain_input_src(np > 2 ? d2 : d0, a.asmp, e, B, row0, tid), r3 = chain_input_src(np > 3 ? d3 : d0, a.asmp, e, B, row0, tid);
        chain_input_fetch<CH_THREADS>(d0, r0, 0, tid, q0);
        if (np > 1) chain_input_fetch<CH_THREADS>(d1, r1, 0, tid, q1);
        if (np > 2) chain_input_fetch<CH_THREADS>(d2, r2, 0, tid, q2);
        if (np > 3) chain_input_fetch<CH_THREADS>(d3, r3, 0, tid, q3);
        if (timed0) a.tbuf[201] = __builtin_readcyclecounter();
        chain_input_commit<CH_THREADS>(d0, r0, 0, tid, q0, bufs, a.bufsz);
        if (np > 1) chain_input_commit<CH_THREADS>(d1, r1, 0, tid, q1, bufs, a.bufsz);
        if (np > 2) chain_input_commit<CH_THREADS>(d2, r2, 0, tid, q2, bufs, a.bufsz);
        if (np > 3) chain_input_commit<CH_THREADS>(d3, r3, 0, tid, q3, bufs, a.bufsz);
        for (int i = 0; i < np; ++i) {                        // the rest of wide tiles, one round trip per 32 columns
            const ChainLoad& d = i == 0 ? d0 : i == 1 ? d1 : i == 2 ? d2 : d3;
            const ChainInSrc& r = i == 0 ? r0 : i == 1 ? r1 : i == 2 ? r2 : r3;
            const int done = (i == 0 ? Q0 : i == 1 ? Q1 : Q2) * CH_THREADS;
            // (four elements per thread and round trip: one at a time, the 4-wave flavour took 13 dependent round trips for the context
            //  encoder's 240-column tile -- 30 k cycles of prologue under load, tools/chain_timing.py)
            constexpr int QR = 4;
            ChainIn<QR> qr;
            for (int base = done; base < ((d.zero_to - d.dk0 + 15) & ~15) * CH_ROWS; base += QR * CH_THREADS) {
                chain_input_fetch<CH_THREADS>(d, r, base, tid, qr);
                chain_input_commit<CH_THREADS>(d, r, base, tid, qr, bufs, a.bufsz);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < TW; ++u)
        if (tid + u * CH_THREADS < nw) reinterpret_cast<int*>(stg)[tid + u * CH_THREADS] = tv[u];
    if (timed0) a.tbuf[202] = __builtin_readcyclecounter();
    __syncthreads();
    const bool timed = a.tbuf && item == 0 && e == 0 && tid == 0;
    if (timed) a.tbuf[0] = __builtin_readcyclecounter();
    const float tgt0 = a.loss_on ? chain_loss_target(a.lossp, e, y + a.y_base, row0, tid) : 0.0f;
    ChainOps ops;
    ChainGroup cur = next_group<NW>(stg, nst, -1, 0, wave, e);
    load_ops(stg, cur, e, B, row0, lane, ops);
    ring_prologue(cur, 16u * (unsigned)lane);
    for (int si = 0; si < nst; ++si) {
        while (cur.si == si) {
            ChainGroup nxt;
            unsigned long long* dbg = timed ? a.tbuf + 64 + si * 4 : nullptr;
            chain_group<NW>(stg, nst, wave, cur, nxt, ops, bufs, a.bufsz, e, B, row0, lane, dbg, timed ? a.tfine + si * 6 : nullptr);
            cur = nxt;
        }
        if (timed) a.tbuf[64 + si * 4 + 3] = __builtin_readcyclecounter();
        __syncthreads();
        if (timed) a.tbuf[si + 1] = __builtin_readcyclecounter();
    }
    // (the loss terms' scratch: an activation buffer the chain is done with -- the head outputs sit in loss_buf, the other two are dead;
    //  a region of its own behind the buffers cost the third workgroup per CU its LDS)
    if (a.loss_on) chain_loss_phase<NW>(a, bufs, bufs + ((a.loss_buf + 1) % 3) * a.bufsz, e, y + a.y_base, row0, tid, tgt0);
}

}  // namespace
