// Plans on knots (no reference twin, OPT-IN): action sequences of the opt-in loop (icem.hip) that are piecewise constant or piecewise
// linear on a fixed grid of knot steps -- the search runs over fewer decisions than the horizon has steps.  The grid is restated in
// include/cadm_hip.h (cadm_shape_actions).  The shaped sequences are a linear subspace that holds the knot values unchanged, so the
// loop only overwrites its candidates onto it between sampling and rollout; every kernel behind that sees sequences already on the grid.
#include "planner.h"

// One thread per (env, candidate, step, dim) element, lane-linear over the H A floats of a sequence.  A knot step is left alone; any
// other step is recomputed from knot steps only: reads come from knot steps, writes go to other steps, so the kernel works in place
// without synchronisation.  The segment arithmetic is 64-bit: a spacing near 2^31 is legal (one knot, or two).
__global__ void knot_shape_kernel(float* __restrict__ seqs, const int32_t* __restrict__ phase, size_t total, int n, int H, int A, int r,
                                  int interp) {
    const int HA = H * A;
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(q % HA);
        const size_t mc = q / HA;                        // mi * n + c
        const int t = e / A;
        int phi = phase ? phase[mc / n] % r : 0;
        if (phi < 0) phi += r;
        const long long j = ((long long)t + phi) / r;
        const long long kj = j * r - phi;
        const int k = kj > 0 ? (int)kj : 0;
        if (t == k) continue;
        const long long k1 = (j + 1) * r - phi;          // the next knot; > t
        float* col = seqs + mc * HA + (e - t * A);       // this sequence's action dim, step 0
        const float a0 = col[(size_t)k * A];
        float v = a0;
        if (interp == CADM_KNOT_LINEAR && k1 <= H - 1) {
            const float w = (float)(t - k) / (float)((int)k1 - k);
            v = fmaf(w, col[(size_t)k1 * A] - a0, a0);
        }
        col[(size_t)t * A] = v;
    }
}

int cadm_knot_check(const cadm_knot_params* knots, const char* who) {
    CADM_REQUIRE(knots->spacing >= 1, "%s: knot spacing %d must be >= 1", who, knots->spacing);
    CADM_REQUIRE(knots->interp == CADM_KNOT_HOLD || knots->interp == CADM_KNOT_LINEAR, "%s: knot interp %d is not CADM_KNOT_HOLD or CADM_KNOT_LINEAR",
                 who, knots->interp);
    return CADM_OK;
}

int cadm_launch_shape_actions(cadm_ctx* ctx, const cadm_knot_params* knots, const int32_t* phase, int m, int n, float* seqs, hipStream_t s) {
    const size_t total = (size_t)m * n * ctx->H * ctx->A, g = (total + 255) / 256;
    hipLaunchKernelGGL(knot_shape_kernel, dim3((unsigned)(g > 65536 ? 65536 : g)), dim3(256), 0, s, seqs, phase, total, n, ctx->H, ctx->A,
                       knots->spacing, knots->interp);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

extern "C" int cadm_shape_actions(cadm_ctx* ctx, const cadm_knot_params* knots, const int32_t* phase, int m, int n, float* seqs_io,
                                  void* stream) {
    CADM_REQUIRE(ctx && knots && seqs_io && m > 0 && n > 0, "cadm_shape_actions: bad arguments");
    int rc = cadm_knot_check(knots, "cadm_shape_actions");
    if (rc) return rc;
    if (knots->spacing == 1) return CADM_OK;             // every step is a knot
    CADM_ON_DEVICE(ctx);
    return cadm_launch_shape_actions(ctx, knots, phase, m, n, seqs_io, (hipStream_t)stream);
}
