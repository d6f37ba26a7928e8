// Weight-stream pack kernel of the training step: (re)builds the chain kernel's packed operand streams from the master weights.
#pragma once
#include "common.h"

namespace {
// ---------------------------------------------------------------------------------------------
// packed operand streams of the chain kernel (layout: ChainSeg)
// ---------------------------------------------------------------------------------------------
struct PackDst {          // where element (m, n) of a layer W [M][N] lives in one stream (tr: 0 forward, 1 transposed)
    float* P; long sP;    // stream base, member stride (floats); P == null: no stream
    int KB, kb0;          // k-blocks of the whole stream; this layer's first one (streams concatenated along k)
    int row0, ncols;      // forward: Bop(k, n') = W[k][n'];  transposed: Bop(k, n') = W[row0 + n'][k];  n' < ncols
    int nt, pad;          // tiles of the stream (even)
};
__device__ __forceinline__ long pack_index(const PackDst& d, int k, int np) {    // float index inside a member's stream
    return (((long)(d.kb0 + (k >> 4)) * d.nt + (np >> 4)) * 64 + ((k >> 2) & 3) * 16 + (np & 15)) * 4 + (k & 3);
}

struct PackJob {
    const float* W; int M, N;        // [E][M][N]
    PackDst d; int tr, nk, ntile;    // nk: valid k; ntile: tiles of the stream (even)
};
// Full (re)build of one layer's part of a stream, zero padding included: one float4 per thread.
__global__ void train_pack_kernel(const PackJob j, int E) {
    const int KBl = (j.nk + 15) >> 4;
    const long per = (long)j.ntile * KBl * 64, idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (idx >= per * E) return;
    const int e = (int)(idx / per);
    const long r = idx - e * per;
    const int lane = (int)(r & 63), t = (int)((r >> 6) % KBl), tile = (int)((r >> 6) / KBl);
    const int c = lane & 15, kq = lane >> 4, np = 16 * tile + c;
    const float* W = j.W + (long)e * j.M * j.N;
    floatx4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = 16 * t + 4 * kq + i;
        v[i] = (k < j.nk && np < j.d.ncols) ? (j.tr ? W[(long)(j.d.row0 + np) * j.N + k] : W[(long)k * j.N + np]) : 0.0f;
    }
    *reinterpret_cast<floatx4*>(j.d.P + (long)e * j.d.sP + (((long)(j.d.kb0 + t) * j.d.nt + tile) * 64 + lane) * 4) = v;
}

}  // namespace
