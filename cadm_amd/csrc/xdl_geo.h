// Geometry of the split-f16 ("xdl") rollout weight stream, shared by the packer (host + pack kernel) and the
// rollout kernel so that the two can never disagree.  See DESIGN.md "rollout kernel".
//
//   * A dense layer is evaluated transposed (OUT^T = W^T * IN^T) with v_mfma_f32_16x16x32_f16: the weights are
//     the A operand (16 output units x 32 input features), 16 data rows are the B / D columns.
//   * fp32 accuracy on the f16 matrix pipe: a WEIGHT is split as  w = w1 + 2^-11 * w2,  w1 = f16_rn(w), w2 = f16_rn((w - w1) * 2^11)
//     (the 2^11 keeps the low part a NORMAL f16 number); an ACTIVATION as  x = x1 + x2,  x1 = f16_rn(x), x2 = f16_rn(x - x1), unscaled
//     (round 4: the scaling cost the epilogue 2 of its 28 instructions per tile, and the kernels are bound by their VALU instructions as
//     much as by their MFMAs; a low part below the f16 normal range is a subnormal: 3e-8 ABSOLUTE error on an activation below 0.25).
//     A product  w * x  is evaluated as  w1*x1 + w1*x2  (accumulator HI)  +  2^-11 * w2*x1  (accumulator LO); the dropped term
//     w2*x2 is <= 2^-22 |w x| (layers wider than 256 add it to LO).  3 MFMAs at 16x the fp32-MFMA rate instead of 8.
//   * swish layers (the reference's default): log2(e) is folded into the packed weights -- layer 0's W and every hidden bias are
//     multiplied by it, the head's W divided -- so a hidden pre-activation arrives as  p' = log2(e) * p,  sigmoid(p) = 1 / (1 + exp2(-p'))
//     needs no multiply, and the activation handed on is  p' * sigmoid(p) = log2(e) * swish(p)  (2 more instructions per tile saved).
//   * An output tile is 16 units; the K dimension of the layers that consume a hidden layer is cut in chunks of
//     32 = one PAIR of producer tiles, so a lane's D fragments (units 4g..4g+3 of tiles 2c, 2c+1) ARE its B fragment
//     for chunk c: activations cross layers through LDS without any cross-lane movement.
//   * Hidden tiles are distributed over the CADM_XDL_WAVES waves of a workgroup contiguously (wave w: BASE + (w < EXTRA)
//     tiles; XdlGeo::tile_of maps a wave's local tile to the global one -- a HALF tile, below, may change owner); head tiles
//     (8 obs dims: mu0 mu1 lv0 lv1 per lane) go to the waves with the fewest hidden tiles first.
//   * A "fragment" = one (tile, chunk) of weights = 2 split parts x 64 lanes x 16 B = 2 KB.  Per (member, wave) the
//     stream stores the fragments in EXACTLY the order that wave consumes them during one rollout step:
//     [layer 0][hidden 1 .. NH-1][head]; inside a layer tiles go in groups of xdl_group(), chunk-major inside a group
//     (xdl_frag_index), so the kernel addresses the stream linearly.
#pragma once

#define CADM_XDL_FRAG_BYTES 2048
#define CADM_XDL_LOG2E 1.4426950408889634f
#define CADM_XDL_WAVES 8          // two waves per SIMD: one wave's waits (LDS, L2, epilogue chains) hide behind the other's MFMAs

// Narrow nets: the 8-wave tile split needs at least 8 hidden tiles (113 units).  A narrower net (the reference accepts any
// --hidden_size, e.g. 64) runs on the 128-wide instantiation with zero-padded units: a padded unit has zero weights and bias on
// both sides, so whatever the nonlinearity makes of its zero pre-activation is multiplied by zero in the next layer.  HID is the
// KERNEL's width (tiles, chunks, stream layout), HIDR the model's (bounds and strides of the master weights in the packer).
#define CADM_XDL_MIN_HID 113
#define CADM_XDL_NARROW_HID 128
__host__ __device__ constexpr int xdl_kernel_hid(int hid) { return hid < CADM_XDL_MIN_HID ? CADM_XDL_NARROW_HID : hid; }

// HALF LAST HIDDEN TILE.  When the last hidden tile holds at most 8 real units (HID % 16 in 1..8; HID = 200: units 192..199 of tile 12) half
// of its A operand is zero rows, and with three products per block the w2 rows fit there.  The cooperative stream packs that tile's fragments as
//     part 0 = [ w1(u0..u7) ; w2(u0..u7) ]      acc += part0 * x1     rows 0-7: HI += w1 x1    rows 8-15: LO += w2 x1
//     part 1 = [ w1(u0..u7) ;     0      ]      acc += part1 * x2     rows 0-7: HI += w1 x2    rows 8-15: += 0
// (A-operand lane (grp, m) holds row m: m < 8 is unit 16 tile + m, m >= 8 is the low part of unit 16 tile + m - 8 in part 0, zero in part 1)
// in every layer that OUTPUTS hidden units, layer 0's invariant-chunk fragment included: TWO MFMAs per (tile, chunk) into ONE accumulator
// instead of three into two.  Every real output element sees the same dot products over the same k positions added in the same order as in the
// three-MFMA form -- HI: w1 x1 then w1 x2, chunk by chunk; LO: w2 x1, chunk by chunk -- so the result is that form's bit for bit, with two
// caveats nobody can observe: the zero rows of part 1 add +-0 to LO, which can only change the sign of a LO that is exactly zero (and then
// fma(LO, 2^-11, HI) is HI either way unless HI is a zero too, whose sign swish / the f16 split pass on to a product with a finite weight), and a
// NaN activation makes both forms NaN.  In the D fragment HI of units 4g..4g+3 sits in lane groups g = 0, 1, LO of the same units in groups
// 2, 3: the epilogue exchanges half waves between register pairs (rollout_xdl.h: xdl_half_pairs), after which every lane holds (HI, LO) of
// TWO real units -- half a full tile's epilogue arithmetic -- and stores them as 2-byte pieces; the slots of the units that do not exist are
// written by nobody and keep the zeros of the workgroup's LDS fill.  (A first form -- LO brought down to lanes 0-31, lanes 32-63 idle and
// storing zeros -- lengthened the owner's exposed epilogue by what the MFMAs saved: no gain, profiles/half_tile_ab.md.)  The bias tile needs
// nothing: its lanes 32-63 are zero already, LO's initial value.  Fragment size, stream order and wave_frags are those of a full tile.  The wave-tile stream (NW = 1) keeps the three-MFMA form: it is what this one is tested against.
// Units are NOT permuted among k positions (an MFMA's summation order depends on them).
__host__ __device__ constexpr bool xdl_half(int hid_kernel, int nw) {
    return nw == CADM_XDL_WAVES && hid_kernel <= 256 && hid_kernel % 16 >= 1 && hid_kernel % 16 <= 8;
}
// TILE OWNERSHIP.  Wave w runs on SIMD w mod 4, and a hidden layer ends when the busiest SIMD is done.  Where ONE SIMD carries more tiles
// than every other (EXTRA mod 4 == 1: HID 200 is 13 tiles, 4 / 3 / 3 / 3) the half tile's saving counts only there, so it becomes the
// LAST local tile of the last wave with an extra tile (wave EXTRA - 1, on that SIMD) and the full tiles are dealt contiguously around it:
// HID 200: waves 0-3 {0,1} {2,3} {4,5} {6,7}, wave 4 {8, 12}, waves 5-7 {9} {10} {11} -- per hidden layer 2 x 21 + 21 + 14 = 77 MFMAs on
// SIMD 0 against 63 on the others (84 before).  Everywhere else no placement lowers the busiest SIMD's count (no extra tiles, or two SIMDs
// tied with full tiles only), and the last tile stays the last wave's.  xdl_half_wave: the owner, or -1 without a half tile.
__host__ __device__ constexpr bool xdl_half_moved(int hid_kernel, int nw) {
    return xdl_half(hid_kernel, nw) && (((hid_kernel + 15) / 16) % nw) % 4 == 1;
}
__host__ __device__ constexpr int xdl_half_wave(int hid_kernel, int nw) {
    return !xdl_half(hid_kernel, nw) ? -1 : xdl_half_moved(hid_kernel, nw) ? ((hid_kernel + 15) / 16) % nw - 1 : nw - 1;
}
// global tile of local tile ti of wave w (nt tiles over nw waves)
__host__ __device__ constexpr int xdl_tile_of(int nt, int nw, bool moved, int w, int ti) {
    const int base = nt / nw, extra = nt % nw;
    if (!moved) return w * base + (w < extra ? w : extra) + ti;
    if (w == extra - 1 && ti == base) return nt - 1;
    return w * base + (w < extra - 1 ? w : extra - 1) + ti;
}
__host__ __device__ constexpr bool xdl_owners_ok(int hid_kernel, int nw) {       // every tile has exactly one owner
    const int nt = (hid_kernel + 15) / 16, base = nt / nw, extra = nt % nw;
    for (int t = 0; t < nt; ++t) {
        int n = 0;
        for (int w = 0; w < nw; ++w)
            for (int ti = 0; ti < base + (w < extra ? 1 : 0); ++ti) n += xdl_tile_of(nt, nw, xdl_half_moved(hid_kernel, nw), w, ti) == t ? 1 : 0;
        if (n != 1) return false;
    }
    const int hw = xdl_half_wave(hid_kernel, nw);      // the half tile is its owner's LAST local tile
    return hw < 0 || xdl_tile_of(nt, nw, xdl_half_moved(hid_kernel, nw), hw, base + (hw < extra ? 1 : 0) - 1) == nt - 1;
}
static_assert(xdl_owners_ok(128, CADM_XDL_WAVES) && xdl_owners_ok(200, CADM_XDL_WAVES) && xdl_owners_ok(256, CADM_XDL_WAVES) &&
              xdl_owners_ok(512, CADM_XDL_WAVES) && xdl_owners_ok(200, 1), "hidden tile ownership: every tile exactly one owner");
static_assert(!xdl_half(128, CADM_XDL_WAVES) && xdl_half(200, CADM_XDL_WAVES) && !xdl_half(256, CADM_XDL_WAVES) && !xdl_half(512, CADM_XDL_WAVES) &&
              xdl_half_wave(200, CADM_XDL_WAVES) == 4 && xdl_tile_of(13, CADM_XDL_WAVES, true, 4, 1) == 12 && xdl_tile_of(13, CADM_XDL_WAVES, true, 7, 0) == 11 &&
              xdl_half_wave(120, CADM_XDL_WAVES) == 7 && xdl_half_wave(196, CADM_XDL_WAVES) == 4, "half tile: of the compiled-in widths only 200");

// INVARIANT LAST CHUNK OF LAYER 0 (round 6).  Layer 0's inputs are [obs features | action | context]; the context vector does not change
// over a rollout, so a layer-0 chunk that holds ONLY context features (halfcheetah CaDM: K0 = 18 + 6 + 10 = 34, chunk 1 = context features
// 8 and 9; slim humanoid: chunk 2 of 3) contributes the same products in all H steps.  Where that holds (xdl_inv0) EVERY flavour accumulates
// that chunk FIRST -- (bias + chunk NC0-1) + chunk 0 + .. -- and the cooperative kernel runs it ONCE per row tile: the tile prologue leaves
// (HI, LO) of "bias + last chunk" in LDS per tile, the step loop starts its layer-0 accumulators from them and sweeps NC0 - 1 chunks.  The same
// instructions on the same operands in the same order as a flavour that runs the chunk in every step (the wave-tile kernel): bit-identical.
// Stream of the cooperative kernels: layer 0 holds NC0 - 1 chunks per tile; the invariant chunk's fragments (one per tile) follow the head's.
// A timing build on a vanilla model (K0 = 24: one chunk): cfg2 152.8 -> 144.9 us per rollout (tools/ctx_fold_bound.py).
__host__ __device__ constexpr bool xdl_inv0(int k0, int kdyn, int hid_kernel) {      // kdyn = P + A: the inputs that change from step to step
    return k0 > kdyn && (k0 + 31) / 32 >= 2 && ((k0 + 31) / 32 - 1) * 32 >= kdyn && (hid_kernel + 15) / 16 <= 13;
}

struct XdlGeo {
    int K0, HID, D, NH, HIDR;
    int INV;     // 1: the cooperative kernels' stream keeps layer 0's invariant chunk apart (above); the wave-tile stream (NW = 1) never does
    int NC0, NT, NCH, NTO, BASE, EXTRA, NTOW;
    int NW;      // waves the tiles are dealt to: CADM_XDL_WAVES (cooperative kernel), 1 (wave-tile kernel, rollout_wt.h: every wave owns ALL tiles)
    int HALF;    // 1: the last hidden tile is packed as a half tile (above); HALFW its owner (-1: none)
    int HALFW;
    __host__ __device__ int ntw(int w) const { return BASE + (w < EXTRA ? 1 : 0); }
    __host__ __device__ int tile_of(int w, int ti) const { return xdl_tile_of(NT, NW, HALF && xdl_half_moved(HID, NW), w, ti); }
    __host__ __device__ int head_tile(int w, int s) const { return (NW - 1 - w) + NW * s; }          // slot s of wave w (valid if < NTO)
    __host__ __device__ int nhead(int w) const {
        int n = 0;
        for (int s = 0; s < NTOW; ++s) n += head_tile(w, s) < NTO ? 1 : 0;
        return n;
    }
    __host__ __device__ int wave_frags(int w) const { return ntw(w) * NC0 + (NH - 1) * ntw(w) * NCH + nhead(w) * NCH; }      // (INV: NC0 - 1 chunks in front, 1 behind the head)
    __host__ __device__ int member_frags() const {
        int n = 0;
        for (int w = 0; w < NW; ++w) n += wave_frags(w);
        return n;
    }
    __host__ __device__ int bias_tiles() const { return NH * NT + NTO; }
};

inline XdlGeo make_xdl_geo(int K0, int hid_model, int D, int NH, int nw = CADM_XDL_WAVES, int kdyn = -1) {
    XdlGeo g;
    g.NW = nw;
    g.INV = (nw == CADM_XDL_WAVES && kdyn >= 0 && xdl_inv0(K0, kdyn, xdl_kernel_hid(hid_model))) ? 1 : 0;
    const int HID = xdl_kernel_hid(hid_model);
    g.K0 = K0; g.HID = HID; g.HIDR = hid_model; g.D = D; g.NH = NH;
    g.NC0 = (K0 + 31) / 32;
    g.NT = (HID + 15) / 16;
    g.NCH = (g.NT + 1) / 2;
    g.NTO = (D + 7) / 8;
    g.BASE = g.NT / nw;
    g.EXTRA = g.NT % nw;
    g.NTOW = (g.NTO + nw - 1) / nw;
    g.HALF = xdl_half(HID, nw) ? 1 : 0;
    g.HALFW = xdl_half_wave(HID, nw);
    return g;
}

// Tiles a wave accumulates at a time: every wave takes its tiles two at a time, and a group's epilogue runs stage by stage between the
// MFMAs of the next group (rollout_xdl.h: xdl_sweep).  Measured and dropped: the second wave of each SIMD going tile by tile, each tile's
// epilogue right behind its MFMAs, to put the two waves out of phase (211 against 203 us per launch at cfg2).
__host__ __device__ constexpr int xdl_group() { return 2; }

// position of fragment (local tile ti, chunk c) in a layer's consumption order, for a wave with ntw tiles taken in
// groups of gsz: chunk-major inside a group
__host__ __device__ constexpr int xdl_frag_index(int ntw, int nchl, int ti, int c, int gsz) {
    const int g = ti / gsz;
    const int gs = (ntw - gsz * g) < gsz ? (ntw - gsz * g) : gsz;
    return gsz * g * nchl + c * gs + (ti - gsz * g);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The launcher's plan (rollout_xdl.h: xdl_launch): how a member's row tiles are cut between the kernel flavours.
//   flavour 0: cooperative kernel, one row tile per workgroup   cap 1 unit   cost 1
//           1: cooperative kernel, two row tiles per workgroup  cap 2        xdl_costs(..).c[1]
//           2: wave-tile kernel, 4 tiles per workgroup           cap 4        .c[2]   (one wave per SIMD: never wins, exists for the tests)
//           3: wave-tile kernel, 8 tiles per workgroup           cap 8        .c[3]   (per round)
// 1 unit = one CU share of the member (n_cus / E tiles); costs in units of the one-tile launch (halfcheetah at the cfg2 / cfg3 geometry,
// 51 workgroups per member: 165 / 261 / 600 / 876 us, profiles/r4_s3_flavour_table.txt).  The cheapest cover is a small
// dynamic programme, f(u) = min over flavours (cost + f(u - cap)); count[o] = launches (rounds) of flavour o.
// The costs are a property of the INSTANTIATION (env kind -> observation width -> state phase and head; hidden width -> tiles per wave):
// xdl_costs(env, hid) is a constexpr of the launcher's template arguments, filled from tools/flavour_table.py runs (round 6,
// profiles/r6_flavour_table.txt; us per rollout / the one-tile launch's):
//   halfcheetah, HID 200:    two tiles 1.59 (260.7 per full round)   wave-tile 4: 3.15-3.2 (517)   wave-tile 8: 5.19 (851.9)
//   slim humanoid, HID 200:  two tiles 1.62 (304.0)                  wave-tile 4: 3.62   wave-tile 8: 5.5
// A wave-tile round that is NOT full is cheaper than a full one -- its workgroups run 5, 6 or 7 waves instead of 8 (wt_launch gives a
// partly filled round the member's whole CU share): wt8p[k - 5] = cost of a round that covers k = 5, 6, 7 units (halfcheetah 735.6 /
// 741.8 / 794.0 us: 4.48 / 4.52 / 4.84; at 6 units one partial round beats three two-tile launches, 741.8 against 776.9 us).
// Geometries nobody measured use halfcheetah's, user-declared envs (CADM_ENV_SPEC) included.
struct XdlCosts { float c[4]; float wt8p[3]; };
__host__ __device__ constexpr XdlCosts xdl_costs(int env_kind, int hid) {
    return env_kind == 2 /* CADM_ENV_SLIM_HUMANOID */ ? XdlCosts{{1.0f, 1.62f, 3.62f, 5.5f}, {4.78f, 4.80f, 5.15f}}
                                                      : XdlCosts{{1.0f, 1.59f, 3.2f, 5.19f}, {4.48f, 4.52f, 4.84f}};
}
inline void xdl_plan_units(int units, bool mt2_ok, bool wt_ok, int (&count)[4], XdlCosts costs = xdl_costs(0, 200)) {
    const int capu[4] = {1, mt2_ok ? 2 : 0, wt_ok ? 4 : 0, wt_ok ? 8 : 0};
    const float* cost = costs.c;
    for (int o = 0; o < 4; ++o) count[o] = 0;
    // beyond 64 units the answer is "rounds of the biggest flavour" plus the plan of the rest
    const int big = capu[3] ? 3 : capu[1] ? 1 : 0;
    int u = units;
    if (u > 64) { const int k = (u - 56) / capu[big]; count[big] += k; u -= k * capu[big]; }
    float f[65];
    int pick[65];
    f[0] = 0.0f;
    pick[0] = -1;
    for (int v = 1; v <= u; ++v) {
        f[v] = 1e30f;
        for (int o = 0; o < 4; ++o) {
            if (!capu[o]) continue;
            // (a wave-tile-8 round that covers only 5, 6 or 7 units -- the LAST launch of a plan takes the ragged rest -- at its own cost)
            const float co = (o == 3 && v >= 5 && v <= 7) ? costs.wt8p[v - 5] : cost[o];
            const float c = co + f[v > capu[o] ? v - capu[o] : 0];
            if (c < f[v] - 1e-6f) { f[v] = c; pick[v] = o; }
        }
    }
    for (int v = u; v > 0; v -= capu[pick[v]]) ++count[pick[v]];
}
