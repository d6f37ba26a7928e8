// Training step of the ensemble (reference cadm/dynamics/mlp_cadm_ensemble_cem_dynamics.py:269-317;
// vanilla twin mlp_ensemble_cem_dynamics.py:148-170): forward of the context / forward / backward
// nets on one [E,B,.] bootstrap batch, the losses, hand-written backward and TF1-semantics Adam.
//
// The batch is tiny (B = 256 rows x 5 members, < 3 GFLOP per step), so a step is bound by dependent-
// launch overhead (~4.5 us per kernel on this part) and by per-workgroup latency chains, not by
// throughput.  The step is therefore built from THREE fat kernels instead of one GEMM per layer:
//   chain_kernel (forward)   a workgroup owns 16 batch rows of one member of one net and walks the whole
//                            layer chain (context encoder -> dynamics net -> heads) with the activations
//                            resident in LDS; weights stream from L2 straight into the MFMA B operand
//                            through rotating register blocks (no LDS staging: a weight is used by exactly
//                            one wave; 8 waves, two per SIMD).  z / h of every layer are stored for the
//                            backward pass.
//   chain_kernel (backward)  same kernel, transposed weight indexing: dZ_{l-1} = (dZ_l W_l^T) * act'(z_{l-1})
//                            down the chain; once for the forward+backward nets, once for the context net.
//   dw_adam_kernel           every layer's W <- Adam(W, X^T dZ + c*wd*W), b <- Adam(b, colsum dZ) as ONE
//                            grouped launch over a tile table (the gradient never touches HBM).
// A chain is described by a small stage table in device memory (LOAD / GEMM stages, rebuilt only when
// a pointer changes).  Everything is launch-ordered on one stream: the backward chains (which read W)
// run before the grouped DW launch (which overwrites W).
#include <math.h>
#include <string.h>

#include "common.h"
#include "train_pack.h"
#include "train_chain.h"
#include "train_dw.h"

// hidden nonlinearity of the dynamics nets (cadm_config.hidden_act, CADM_ACT_*) as a stage-table code
static int dyn_act(const cadm_ctx* ctx) {
    switch (ctx->cfg.hidden_act) {
        case CADM_ACT_RELU: return ACT_RELU;
        case CADM_ACT_TANH: return ACT_TANH;
        case CADM_ACT_SIGMOID: return ACT_SIGMOID;
        case CADM_ACT_NONE: return ACT_NONE;
        default: return ACT_SWISH;
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
namespace {      // (host records of this file only)
struct NetBufs {
    std::vector<float*> z, h, dz;     // per hidden layer [E,B,width]; dz: gradient w.r.t. the pre-activation
    float *mu = nullptr, *lv = nullptr;
    float* dctx = nullptr;            // this net's gradient w.r.t. its context input columns [E,B,C]
};

struct AdamSlot { float *m = nullptr, *v = nullptr; size_t n = 0; };

// One of the three nets, TrainState::net[CADM_NET_FF / CADM_NET_BACK / CADM_NET_CTX]
struct TrainNet {
    const std::vector<DenseRef>* L = nullptr;   // its registered layers (ctx->ff / ctx->back / ctx->cp); null: this model has no such net
    NetBufs nb;
    float* X = nullptr;                         // echo of its normalised input [E,B,K0p] (context net: [E,B,cpinp]): layer 0's weight-gradient operand
    std::vector<AdamSlot> adam;                 // Adam moments, same order as the registered layers: W then b (2 per layer)
    std::vector<PackDst> pf, pb;                // packed operand streams of the chain kernel, per registered layer (forward / transposed)
    std::vector<int> pt, ptb;                   // tiles (even) of the forward / transposed stream
};
}  // namespace

struct TrainState {
    cadm_train_hparams hp{};
    bool configured = false;
    int B = 0;                    // workspace capacity (rows per member)
    long step = 0;
    float* ws = nullptr;          // one workspace allocation (the nets' buffers and the views below)
    TrainNet net[3];
    std::vector<float*> cp_dz2;   // the context encoder's dz as propagated from the backward model's chain (net[CADM_NET_CTX].nb.dz: from the forward net's)
    float *dMu = nullptr, *dLv = nullptr, *dBmu = nullptr, *terms = nullptr, *red = nullptr;
    AdamSlot a_mx, a_mn;          // max / min_logvar
    float* adam_buf = nullptr;    // one allocation: the nets' moments in net order, then a_mx, a_mn
    float* pack_buf = nullptr;    // one allocation: the nets' streams in net order
    // chain programs: [fwd ff | fwd back | bwd ff | bwd back | bwd context]
    std::vector<ChainStage> prog_host;
    ChainStage* prog_dev = nullptr;
    int prog_first[8] = {0, 0, 0, 0, 0, 0, 0, 0}, prog_count[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ChainLoad pre[8][4]; int npre[8] = {0, 0, 0, 0, 0, 0, 0, 0};         // the programs' input tiles (kernel arguments of the launch)
    ChainAsm asmp{};                                            // raw batch of the current call (forward launch)
    int loss_buf = 0, loss_lv0 = 0;                             // where the forward chains leave the head outputs in LDS
    int K0p = 0, cpinp = 0, Dp = 0, Cp = 0;                     // padded row strides of the dynamics nets' X, the context net's X, dMu / dLv / dBmu, the dctx buffers
    int chain_bufsz = 0;
};

void cadm_train_free(cadm_ctx* ctx) {
    if (!ctx->train) return;
    if (ctx->train->ws) (void)hipFree(ctx->train->ws);
    if (ctx->train->adam_buf) (void)hipFree(ctx->train->adam_buf);
    if (ctx->train->prog_dev) (void)hipFree(ctx->train->prog_dev);
    if (ctx->train->pack_buf) (void)hipFree(ctx->train->pack_buf);
    delete ctx->train;
    ctx->train = nullptr;
}

static int alloc_adam(cadm_ctx* ctx) {
    TrainState* t = ctx->train;
    size_t total = 0;
    for (TrainNet& n : t->net)
        if (n.L) for (auto& d : *n.L) total += 2 * ((size_t)ctx->E * d.din * d.dout + (size_t)ctx->E * d.dout);
    total += 4 * (size_t)ctx->D;
    CADM_CHECK_HIP(hipMalloc(&t->adam_buf, total * sizeof(float)));
    CADM_CHECK_HIP(hipMemset(t->adam_buf, 0, total * sizeof(float)));
    float* q = t->adam_buf;
    for (TrainNet& n : t->net) {
        n.adam.clear();
        if (!n.L) continue;
        for (auto& d : *n.L) {
            AdamSlot w, b;
            w.n = (size_t)ctx->E * d.din * d.dout; w.m = q; q += w.n; w.v = q; q += w.n;
            b.n = (size_t)ctx->E * d.dout; b.m = q; q += b.n; b.v = q; q += b.n;
            n.adam.push_back(w); n.adam.push_back(b);
        }
    }
    t->a_mx.n = t->a_mn.n = ctx->D;
    t->a_mx.m = q; q += ctx->D; t->a_mx.v = q; q += ctx->D;
    t->a_mn.m = q; q += ctx->D; t->a_mn.v = q; q += ctx->D;
    return CADM_OK;
}

int cadm_train_adam_slot(cadm_ctx* ctx, int net, int layer, int is_bias, float** m, float** v, size_t* n) {
    *m = *v = nullptr; *n = 0;
    TrainState* t = ctx->train;
    if (!t || !t->adam_buf) return CADM_ESTATE;
    const AdamSlot* s = nullptr;
    if (layer < 0) {
        if (net != CADM_NET_FF || layer < -2) return CADM_EINVAL;
        s = layer == -1 ? &t->a_mx : &t->a_mn;
    } else {
        if (net < 0 || net > CADM_NET_CTX) return CADM_EINVAL;
        const std::vector<AdamSlot>& v_ = t->net[net].adam;
        const size_t i = 2 * (size_t)layer + (is_bias ? 1 : 0);
        if (i >= v_.size()) return CADM_EINVAL;
        s = &v_[i];
    }
    *m = s->m; *v = s->v; *n = s->n;
    return CADM_OK;
}

static inline int kblocks(int k) { return (k + 15) >> 4; }
static inline int even_tiles(int n) { return 2 * ((((n + 15) >> 4) + 1) / 2); }

// Streams of the chain kernel's stages (geometry only; filled by pack_streams and kept current by dw_adam_kernel):
//   forward    every layer: Bop(k, n) = W[k][n]
//   transposed hidden layers l >= 1 and the context net's layers l >= 1: Bop(k, n') = W[n'][k];
//              layer 0 of a dynamics net: only its context rows (row0 = P + A, C of them) carry a gradient;
//              the heads mu (| logvar) of a net share ONE stream, concatenated along k: dz = [dMu | dLv] [Wmu | Wlv]^T
static int alloc_packs(cadm_ctx* ctx) {
    TrainState* t = ctx->train;
    const int E = ctx->E, NH = ctx->NH, D = ctx->D, C = ctx->C, PA = ctx->P + ctx->A;
    const bool has_cp = C > 0, det = ctx->cfg.deterministic != 0;
    size_t total = 0;
    auto region = [&](PackDst& d, int ntile) { d.nt = ntile; d.sP = (long)ntile * d.KB * CH_BLK_FLOATS; d.P = reinterpret_cast<float*>(total + 1); total += (size_t)E * d.sP; };
    auto net = [&](TrainNet& tn, bool dyn, bool with_lv) {
        const std::vector<DenseRef>& L = *tn.L;
        auto &pf = tn.pf, &pb = tn.pb; auto &pt = tn.pt, &ptb = tn.ptb;
        const int n = (int)L.size();
        pf.assign(n, PackDst{}); pb.assign(n, PackDst{}); pt.assign(n, 0); ptb.assign(n, 0);
        for (int l = 0; l < n; ++l) {
            if (dyn && l == NH + 1 && !with_lv) continue;          // logvar head outside the data path
            PackDst& f = pf[l];
            f.KB = kblocks(L[l].din); f.kb0 = 0; f.row0 = 0; f.ncols = L[l].dout;
            pt[l] = even_tiles(L[l].dout);
            region(f, pt[l]);
            PackDst& b = pb[l];
            if (dyn && l == 0) {
                if (!has_cp) continue;
                b.KB = kblocks(L[0].dout); b.kb0 = 0; b.row0 = PA; b.ncols = C;
                ptb[0] = even_tiles(C);
                region(b, ptb[0]);
            } else if (dyn && l >= NH) {
                const int KBd = kblocks(D);
                b.KB = KBd * (with_lv ? 2 : 1); b.kb0 = (l - NH) * KBd; b.row0 = 0; b.ncols = L[l].din;
                ptb[l] = even_tiles(L[l].din);
                if (l == NH) region(b, ptb[l]);
                else { b.P = pb[NH].P; b.sP = pb[NH].sP; b.nt = pb[NH].nt; }
            } else if (l >= 1) {
                b.KB = kblocks(L[l].dout); b.kb0 = 0; b.row0 = 0; b.ncols = L[l].din;
                ptb[l] = even_tiles(L[l].din);
                region(b, ptb[l]);
            }
        }
    };
    for (int id = 0; id < 3; ++id)
        if (t->net[id].L) net(t->net[id], id != CADM_NET_CTX, id == CADM_NET_FF && !det);
    CADM_CHECK_HIP(hipMalloc(&t->pack_buf, total * sizeof(float)));
    for (TrainNet& tn : t->net)
        for (auto* v : {&tn.pf, &tn.pb})
            for (auto& d : *v)
                if (d.P) d.P = t->pack_buf + (reinterpret_cast<size_t>(d.P) - 1);
    ctx->train_packs_stale = true;
    return CADM_OK;
}

// (Re)build every stream from the registered master weights: after cadm_set_weights / cadm_repack, i.e. whenever the
// caller may have written the weights; the training step itself updates them in dw_adam_kernel's epilogue.
static int pack_streams(cadm_ctx* ctx, hipStream_t s) {
    TrainState* t = ctx->train;
    auto one = [&](const DenseRef& L, const PackDst& d, int tr, int nk, int ntile) -> int {
        if (!d.P) return CADM_OK;
        PackJob j{};
        j.W = L.W; j.M = L.din; j.N = L.dout; j.d = d; j.tr = tr; j.nk = nk; j.ntile = ntile;
        const long n = (long)ctx->E * ntile * kblocks(nk) * 64;
        hipLaunchKernelGGL(train_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, j, ctx->E);
        CADM_CHECK_HIP(hipGetLastError());
        return CADM_OK;
    };
    int rc;
    for (TrainNet& n : t->net)
        for (size_t l = 0; l < n.pf.size(); ++l) {
            const DenseRef& L = (*n.L)[l];
            if ((rc = one(L, n.pf[l], 0, L.din, n.pt[l]))) return rc;
            if ((rc = one(L, n.pb[l], 1, L.dout, n.ptb[l]))) return rc;
        }
    ctx->train_packs_stale = false;
    return CADM_OK;
}

static inline int r4(int n) { return (n + 3) & ~3; }

static int ensure_workspace(cadm_ctx* ctx, int B) {
    TrainState* t = ctx->train;
    if (B <= t->B && t->ws) return CADM_OK;
    if (t->ws) { (void)hipFree(t->ws); t->ws = nullptr; }
    const size_t R = (size_t)ctx->E * B;
    const int NH = ctx->NH, HID = ctx->HID, D = ctx->D, K0 = ctx->K0;
    const int ncp = ctx->C > 0 ? ctx->cfg.n_cp_hidden : 0;
    const int cpin = (ctx->D + ctx->A) * ctx->cfg.history_length;
    const size_t Cw = ctx->C > 0 ? ctx->C : 1;
    size_t total = 0;
    auto need = [&](size_t n) { size_t o = total; total += (n + 63) & ~(size_t)63; return o; };
    // odd-width tensors that the weight-gradient launch reads get rows padded to a multiple of 4 floats (zero columns: the
    // buffer is cleared once, nothing writes them): dw_adam_kernel then takes its 16-byte loop on them too
    const int K0p = r4(K0), cpinp = r4(cpin > 0 ? cpin : 1), Dp = r4(D), Cp = r4((int)Cw);
    t->K0p = K0p; t->cpinp = cpinp; t->Dp = Dp; t->Cp = Cp;
    const size_t oXff = need(R * K0p), oXbk = need(R * K0p), oXcp = need(R * cpinp);
    const size_t odCff = need(R * Cp), odCbk = need(R * Cp);
    std::vector<size_t> oz_ff(NH), oh_ff(NH), od_ff(NH), oz_bk(NH), oh_bk(NH), od_bk(NH), oz_cp(ncp), oh_cp(ncp), od_cp(ncp), od_cpb(ncp);
    for (int l = 0; l < NH; ++l) {
        oz_ff[l] = need(R * HID); oh_ff[l] = need(R * HID); od_ff[l] = need(R * HID);
        oz_bk[l] = need(R * HID); oh_bk[l] = need(R * HID); od_bk[l] = need(R * HID);
    }
    for (int l = 0; l < ncp; ++l) {
        const size_t w = ctx->cfg.cp_hidden[l];
        oz_cp[l] = need(R * w); oh_cp[l] = need(R * w); od_cp[l] = need(R * w); od_cpb[l] = need(R * w);
    }
    const size_t omu = need(R * D), olv = need(R * D), obmu = need(R * D), oblv = need(R * D);
    const size_t odMu = need(R * Dp), odLv = need(R * Dp), odBmu = need(R * Dp);
    const size_t oterms = need((size_t)ctx->E * 2 * ((B + CH_ROWS - 1) / CH_ROWS) * (4 + 2 * (size_t)D)), ored = need(4 + 2 * (size_t)D + 8);   // a slot per forward workgroup
    CADM_CHECK_HIP(hipMalloc(&t->ws, total * sizeof(float)));
    CADM_CHECK_HIP(hipMemset(t->ws, 0, total * sizeof(float)));
    float* w = t->ws;
    NetBufs &ff = t->net[CADM_NET_FF].nb, &bk = t->net[CADM_NET_BACK].nb, &cp = t->net[CADM_NET_CTX].nb;
    t->net[CADM_NET_FF].X = w + oXff; t->net[CADM_NET_BACK].X = w + oXbk; t->net[CADM_NET_CTX].X = w + oXcp; ff.dctx = w + odCff; bk.dctx = w + odCbk;
    for (NetBufs* nb : {&ff, &bk}) { nb->z.resize(NH); nb->h.resize(NH); nb->dz.resize(NH); }
    cp.z.resize(ncp); cp.h.resize(ncp); cp.dz.resize(ncp);
    for (int l = 0; l < NH; ++l) {
        ff.z[l] = w + oz_ff[l]; ff.h[l] = w + oh_ff[l]; ff.dz[l] = w + od_ff[l];
        bk.z[l] = w + oz_bk[l]; bk.h[l] = w + oh_bk[l]; bk.dz[l] = w + od_bk[l];
    }
    t->cp_dz2.resize(ncp);
    for (int l = 0; l < ncp; ++l) { cp.z[l] = w + oz_cp[l]; cp.h[l] = w + oh_cp[l]; cp.dz[l] = w + od_cp[l]; t->cp_dz2[l] = w + od_cpb[l]; }
    ff.mu = w + omu; ff.lv = w + olv; bk.mu = w + obmu; bk.lv = w + oblv;
    t->dMu = w + odMu; t->dLv = w + odLv; t->dBmu = w + odBmu;
    t->terms = w + oterms; t->red = w + ored;
    CADM_CHECK_HIP(hipMemset(t->red, 0, (4 + 2 * (size_t)D + 8) * sizeof(float)));   // incl. the reduction's arrival counter
    t->B = B;
    return CADM_OK;
}

static int ensure_state(cadm_ctx* ctx) {
    if (ctx->train) return CADM_OK;
    ctx->train = new (std::nothrow) TrainState();
    if (!ctx->train) { cadm_set_error("out of host memory"); return CADM_ENOMEM; }
    TrainNet* n = ctx->train->net;      // the nets this model has (fixed at cadm_create)
    n[CADM_NET_FF].L = &ctx->ff;
    if (ctx->cfg.back_model) n[CADM_NET_BACK].L = &ctx->back;
    if (ctx->C > 0) n[CADM_NET_CTX].L = &ctx->cp;
    return CADM_OK;
}

extern "C" int cadm_train_configure(cadm_ctx* ctx, const cadm_train_hparams* hp, int max_batch) {
    CADM_REQUIRE(ctx && hp, "cadm_train_configure: null argument");
    CADM_ON_DEVICE(ctx);
    for (auto& d : ctx->ff) CADM_REQUIRE(d.W && d.b, "cadm_train_configure: ff_model weights not registered");
    if (ctx->cfg.back_model) for (auto& d : ctx->back) CADM_REQUIRE(d.W && d.b, "cadm_train_configure: backward_model weights not registered");
    if (ctx->C > 0) for (auto& d : ctx->cp) CADM_REQUIRE(d.W && d.b, "cadm_train_configure: context_model weights not registered");
    int rc0 = ensure_state(ctx);
    if (rc0) return rc0;
    if (!ctx->train->adam_buf && (rc0 = alloc_adam(ctx))) return rc0;
    ctx->train->hp = *hp;
    ctx->train->configured = true;
    if (max_batch > 0) return ensure_workspace(ctx, max_batch);
    return CADM_OK;
}

extern "C" int cadm_train_reset(cadm_ctx* ctx, void* stream) {
    CADM_REQUIRE(ctx && ctx->train, "cadm_train_reset: training not configured");
    CADM_ON_DEVICE(ctx);
    TrainState* t = ctx->train;
    size_t total = 0;
    for (TrainNet& n : t->net) for (auto& s : n.adam) total += 2 * s.n;
    total += 4 * (size_t)ctx->D;
    CADM_CHECK_HIP(hipMemsetAsync(t->adam_buf, 0, total * sizeof(float), (hipStream_t)stream));
    t->step = 0;
    return CADM_OK;
}

namespace {

enum { PROG_FWD_FF = 0, PROG_FWD_BK = 1, PROG_BWD_FF = 2, PROG_BWD_BK = 3,
       PROG_FWD_BK_NOCP = 4,                                  // large batches: the backward model's forward chain with the context columns read back (fwd_prog)
       PROG_BWD_FF_NOCP = 5, PROG_BWD_BK_NOCP = 6, PROG_BWD_CP = 7,   // ... and the backward chains cut in front of the context encoder + ONE pass down it (bwd_prog)
       NPROG = 8 };

ChainLoad input_tile(const float* g0, const float* g1, float* gsum, int ld_in, int ldg, int K, int dst, int dk0, int zero_to, int mode = 0) {
    ChainLoad d{};
    d.mode = mode;
    d.g0 = g0; d.g1 = g1; d.gsum = gsum; d.ld_in = ld_in; d.ldg = ldg; d.K = K; d.dst = dst; d.dk0 = dk0; d.zero_to = zero_to;
    return d;
}

ChainStage gemm_stage(int src, int dst, int dk0, int act_d, int act_o) {
    ChainStage g{};
    g.src = src; g.dst = dst; g.dk0 = dk0; g.act_d = act_d; g.act_o = act_o; g.zfill = dst >= 0 && dk0 == 0;
    return g;
}

bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// appends a column segment (its packed operand `d` with `ntile` tiles) to a GEMM stage
void add_seg(ChainStage& g, const PackDst& d, int ntile, const float* bias, const float* zprev, float* out0, float* out1, int N,
             int ldo, int ldz) {
    const int si = g.ntp == 0 ? 0 : 1;
    ChainSeg& sg = g.seg[si];
    sg.P = d.P; sg.sP = d.sP; sg.nt = d.nt; sg.bias = bias; sg.zprev = zprev; sg.out0 = out0; sg.out1 = out1; sg.N = N; sg.ldo = ldo; sg.ldz = ldz;
    sg.vec = (N & 3) == 0 && ((!out0 && !out1) || (ldo & 3) == 0) && (!zprev || (ldz & 3) == 0) && (g.dst < 0 || (g.dk0 & 3) == 0) &&
             aligned16(bias) && aligned16(zprev) && aligned16(out0) && aligned16(out1);
    g.KB = d.KB;
    g.ntp += ntile / 2;
    if (si == 0) g.tp1 = g.ntp;          // (a second segment starts here)
}

// Builds the five stage lists for the current pointers and uploads them if anything changed.
int sync_programs(cadm_ctx* ctx, hipStream_t s) {
    TrainState* t = ctx->train;
    const bool has_back = ctx->cfg.back_model != 0, has_cp = ctx->C > 0, det = ctx->cfg.deterministic != 0;
    const int NH = ctx->NH, HID = ctx->HID, D = ctx->D, K0 = ctx->K0, C = ctx->C, PA = ctx->P + ctx->A;
    const int ncp = has_cp ? ctx->cfg.n_cp_hidden : 0;
    const int cpin = (ctx->D + ctx->A) * ctx->cfg.history_length;
    std::vector<ChainStage> prog;
    int first[NPROG], count[NPROG];
    int maxk = 16;                       // k extent of the widest LDS activation buffer
    int cur_prog = 0;
    TrainNet &ff = t->net[CADM_NET_FF], &bk = t->net[CADM_NET_BACK], &cp = t->net[CADM_NET_CTX];
    for (int i = 0; i < NPROG; ++i) t->npre[i] = 0;
    auto push = [&](const ChainStage& g) {
        const int ext = g.dst >= 0 ? g.dk0 + 32 * g.ntp : 0;       // whole tile pairs are written (zeros behind N)
        maxk = ext > maxk ? ext : maxk;
        prog.push_back(g);
    };
    auto input = [&](const ChainLoad& d) {
        maxk = d.zero_to > maxk ? d.zero_to : maxk;
        t->pre[cur_prog][t->npre[cur_prog]++] = d;
    };

    // ctx_from: the context vector is not computed by this chain but read back from the forward net's input echo (its context columns,
    // written by the forward net's launch in front of this one): large batches, forward_nets
    auto fwd_prog = [&](TrainNet& n, bool store_cp, bool want_lv, const float* ctx_from = nullptr) {
        const std::vector<DenseRef>& net = *n.L;
        const auto &pf = n.pf; const auto &pt = n.pt; float* const X = n.X; NetBufs& nb = n.nb;
        int cur;
        if (has_cp && ctx_from) {      // (buffer 2, as the chain with the encoder in front: the same walk through the buffers, the same loss_buf)
            input(input_tile(nullptr, nullptr, X, 0, t->K0p, ctx->P, 2, 0, ctx->P, 1));
            input(input_tile(nullptr, nullptr, X + ctx->P, 0, t->K0p, ctx->A, 2, ctx->P, PA, 2));
            input(input_tile(ctx_from, nullptr, X + PA, t->K0p, t->K0p, C, 2, PA, 16 * kblocks(K0)));
            cur = 2;
        } else if (has_cp) {
            // both inputs at once: the context encoder's history in buffer 0, this net's (obs, act) columns in buffer 2,
            // where the encoder's last stage drops the context vector behind them
            // (assembled from the raw batch on the way in; the forward net's workgroups also leave the normalised copies that
            //  the weight-gradient launch reads as layer-0 inputs.  g0 of the raw tiles is set per call: forward_nets)
            const int ncpo = D * ctx->cfg.history_length;
            input(input_tile(nullptr, nullptr, store_cp ? cp.X : nullptr, 0, t->cpinp, ncpo, 0, 0, ncpo, 3));
            input(input_tile(nullptr, nullptr, store_cp ? cp.X + ncpo : nullptr, 0, t->cpinp, cpin - ncpo, 0, ncpo, 16 * kblocks(cpin), 4));
            input(input_tile(nullptr, nullptr, X, 0, t->K0p, ctx->P, 2, 0, ctx->P, 1));
            input(input_tile(nullptr, nullptr, X + ctx->P, 0, t->K0p, ctx->A, 2, ctx->P, 16 * kblocks(K0), 2));
            cur = 0;
            for (int l = 0; l <= ncp; ++l) {
                const DenseRef& L = ctx->cp[l];
                if (l < ncp) {
                    ChainStage g = gemm_stage(cur, cur ^ 1, 0, ACT_NONE, ACT_RELU);
                    add_seg(g, cp.pf[l], cp.pt[l], L.b, nullptr, store_cp ? cp.nb.z[l] : nullptr, store_cp ? cp.nb.h[l] : nullptr,
                            L.dout, L.dout, 0);
                    push(g);
                    cur ^= 1;
                } else {   // context vector -> the ctx columns of this net's input (LDS and global)
                    ChainStage g = gemm_stage(cur, 2, PA, ACT_NONE, ACT_NONE);
                    add_seg(g, cp.pf[l], cp.pt[l], L.b, nullptr, nullptr, X + PA, L.dout, t->K0p, 0);
                    push(g);
                }
            }
            cur = 2;
        } else {
            input(input_tile(nullptr, nullptr, X, 0, t->K0p, ctx->P, 0, 0, ctx->P, 1));
            input(input_tile(nullptr, nullptr, X + ctx->P, 0, t->K0p, ctx->A, 0, ctx->P, 16 * kblocks(K0), 2));
            cur = 0;
        }
        for (int l = 0; l < NH; ++l) {
            const int dst = cur == 0 ? 1 : 0;
            ChainStage g = gemm_stage(cur, dst, 0, ACT_NONE, dyn_act(ctx));
            add_seg(g, pf[l], pt[l], net[l].b, nullptr, nb.z[l], nb.h[l], HID, HID, 0);
            push(g);
            cur = dst;
        }
        {   // the heads side by side: mu on the first tile pairs, logvar behind them; also left in LDS for the loss phase
            const int hd = cur == 0 ? 1 : 0;
            t->loss_buf = hd; t->loss_lv0 = 16 * pt[NH];
            ChainStage g = gemm_stage(cur, hd, 0, ACT_NONE, ACT_NONE);
            g.zfill = 0;
            add_seg(g, pf[NH], pt[NH], net[NH].b, nullptr, nullptr, nb.mu, D, D, 0);
            if (want_lv) add_seg(g, pf[NH + 1], pt[NH + 1], net[NH + 1].b, nullptr, nullptr, nb.lv, D, D, 0);
            push(g);
        }
    };
    // the backward chain's way down the context encoder, from the context gradient in LDS buffer `cur`: dz of its hidden layers -> dz
    auto cp_down = [&](int cur, std::vector<float*>& dz) {
        for (int l = ncp; l >= 1; --l) {
            const DenseRef& L = ctx->cp[l];
            const int dst = (cur + 1) % 3;
            ChainStage h = gemm_stage(cur, dst, 0, ACT_RELU, ACT_NONE);
            add_seg(h, cp.pb[l], cp.ptb[l], nullptr, cp.nb.z[l - 1], nullptr, dz[l - 1], L.din, L.din, L.din);
            push(h);
            cur = dst;
        }
    };
    auto bwd_prog = [&](TrainNet& n, const float* dMu, const float* dLv, std::vector<float*>& cp_dz, bool with_cp = true) {
        const std::vector<DenseRef>& net = *n.L;
        const auto &pb = n.pb; const auto &ptb = n.ptb; NetBufs& nb = n.nb;
        const int KBd = kblocks(D);
        // [dMu | dLv] side by side along k (the heads' transposed operands are concatenated the same way)
        input(input_tile(dMu, nullptr, nullptr, t->Dp, 0, D, 0, 0, 16 * KBd));
        if (dLv) input(input_tile(dLv, nullptr, nullptr, t->Dp, 0, D, 0, 16 * KBd, 32 * KBd));
        {   // d z_{NH-1} = (dMu W_mu^T (+ dLv W_lv^T)) * act'(z_{NH-1})
            ChainStage g = gemm_stage(0, 1, 0, dyn_act(ctx), ACT_NONE);
            add_seg(g, pb[NH], ptb[NH], nullptr, nb.z[NH - 1], nullptr, nb.dz[NH - 1], HID, HID, HID);
            push(g);
        }
        int cur = 1;
        for (int l = NH - 1; l >= 1; --l) {
            const int dst = (cur + 1) % 3;
            ChainStage g = gemm_stage(cur, dst, 0, dyn_act(ctx), ACT_NONE);
            add_seg(g, pb[l], ptb[l], nullptr, nb.z[l - 1], nullptr, nb.dz[l - 1], net[l].din, HID, HID);
            push(g);
            cur = dst;
        }
        if (has_cp) {   // only the context columns of the input carry a gradient ...
            const int dst = (cur + 1) % 3;
            ChainStage g = gemm_stage(cur, dst, 0, ACT_NONE, ACT_NONE);
            add_seg(g, pb[0], ptb[0], nullptr, nullptr, nullptr, nb.dctx, C, t->Cp, 0);
            push(g);
            // ... and it goes on down the context encoder in the same chain: backpropagation is linear in the incoming
            // gradient, so each dynamics net carries ITS share (cp_dz) and the weight-gradient launch adds the two on load --
            // no third chain launch, no pass of the context gradient through global memory
            // (with_cp = false, large batches: the chain ends here, with its share of the context gradient in nb.dctx; cp_bwd_prog)
            if (with_cp) cp_down(dst, cp_dz);
        }
    };

    // one program of the table: its stages are whatever `build` pushes (none when the model has no use for it)
    auto program = [&](int id, bool on, auto build) {
        cur_prog = id; first[id] = (int)prog.size();
        if (on) build();
        count[id] = (int)prog.size() - first[id];
    };
    float* const dLv = det ? nullptr : t->dLv;
    program(PROG_FWD_FF, true, [&] { fwd_prog(ff, true, !det); });
    program(PROG_FWD_BK, has_back, [&] { fwd_prog(bk, false, false); });
    program(PROG_BWD_FF, true, [&] { bwd_prog(ff, t->dMu, dLv, cp.nb.dz); });
    program(PROG_BWD_BK, has_back, [&] { bwd_prog(bk, t->dBmu, nullptr, t->cp_dz2); });
    // Large batches: ONE pass down the context encoder on the SUM of the two dynamics nets' context gradients (an input tile adds the two on
    // the way in) instead of one pass per net inside its backward chain: a third launch of short items, half the context-encoder work.
    // Linear in the incoming gradient, so the same gradient -- summed before the pass instead of behind it (in dw_adam_kernel's loads):
    // equal to fp32 roundoff, not bit for bit; the gradient bars against fp64 are asserted for both forms.
    auto cp_bwd_prog = [&]() {
        input(input_tile(ff.nb.dctx, bk.nb.dctx, nullptr, t->Cp, 0, C, 0, 0, 16 * kblocks(C)));
        cp_down(0, cp.nb.dz);
    };
    const bool can_merge = has_back && has_cp && ncp >= 1;
    program(PROG_BWD_FF_NOCP, can_merge, [&] { bwd_prog(ff, t->dMu, dLv, cp.nb.dz, false); });
    program(PROG_BWD_BK_NOCP, can_merge, [&] { bwd_prog(bk, t->dBmu, nullptr, t->cp_dz2, false); });
    program(PROG_BWD_CP, can_merge, cp_bwd_prog);
    program(PROG_FWD_BK_NOCP, has_back && has_cp, [&] { fwd_prog(bk, false, false, ff.X + PA); });
    for (int i = 0; i < NPROG; ++i) CADM_REQUIRE(count[i] <= CH_MAXSTAGE, "training chain too long (more than 20 stages): too many layers");
    static_assert(CH_MAXSTAGE < 31, "ChainStage::nxt keeps a stage index in 5 bits (31: none)");
    for (int i = 0; i < NPROG; ++i)      // where each wave slot goes behind a stage (chain_group looks it up in ONE LDS read instead of walking the table)
        for (int k = 0; k < count[i]; ++k)
            for (int w = 0; w < CH_WAVES_MAX; ++w) {
                unsigned char v = 31;
                for (int j = k + 1; j < count[i]; ++j)
                    if (w < prog[first[i] + j].ntp) { v = (unsigned char)(j | (w >= prog[first[i] + j].tp1 ? 0x80 : 0)); break; }
                prog[first[i] + k].nxt[w] = v;
            }
    for (ChainStage& g : prog) {          // packed copies of the fields a lookup needs (fewer registers in flight across an epilogue)
        CADM_REQUIRE(g.KB < 256 && g.src < 256 && g.tp1 < 256 && g.ntp < 128, "training chain: stage too wide for the packed descriptor");
        g.pkA = g.KB | g.src << 8 | g.tp1 << 16 | g.ntp << 24;
        for (ChainSeg& sg : g.seg) {
            CADM_REQUIRE(sg.nt < (1 << 23) && sg.N < 65536 && sg.ldz < 32768, "training chain: layer too wide for the packed descriptor");
            sg.pkB = (sg.vec ? 1 : 0) | sg.nt << 8;
            sg.pkC = sg.N | sg.ldz << 16;
        }
    }

    const bool same = t->prog_dev && prog.size() == t->prog_host.size() &&
                      memcmp(prog.data(), t->prog_host.data(), prog.size() * sizeof(ChainStage)) == 0;
    if (!same) {
        if (t->prog_dev && prog.size() > t->prog_host.size()) { (void)hipFree(t->prog_dev); t->prog_dev = nullptr; }
        if (!t->prog_dev) CADM_CHECK_HIP(hipMalloc(&t->prog_dev, prog.size() * sizeof(ChainStage)));
        CADM_CHECK_HIP(hipStreamSynchronize(s));   // nothing in flight may still read the old table
        CADM_CHECK_HIP(hipMemcpy(t->prog_dev, prog.data(), prog.size() * sizeof(ChainStage), hipMemcpyHostToDevice));
        t->prog_host = prog;
    }
    for (int i = 0; i < NPROG; ++i) { t->prog_first[i] = first[i]; t->prog_count[i] = count[i]; }
    t->chain_bufsz = CH_ROWS * ((maxk + 15) & ~15);
    {   // (an activation buffer doubles as the loss phase's scratch: 6 term arrays of 16 x D elements, or 512 chunk sums, + a flag)
        const int terms = 6 * CH_ROWS * ctx->D, need = ((terms > CH_THREADS_MAX ? terms : CH_THREADS_MAX) + 4 + 63) & ~63;
        if (t->chain_bufsz < need) t->chain_bufsz = need;
    }
    return CADM_OK;
}

struct ChainLossCfg { LossP lp; ReduceP rp; int final; };

int launch_chain(cadm_ctx* ctx, int B, int p0, int p1, hipStream_t s, const ChainLossCfg* loss = nullptr, int y_base = 0, int slot_ny = 0) {
    TrainState* t = ctx->train;
    ChainArgs a{};
    a.prog = t->prog_dev;
    a.first[0] = t->prog_first[p0]; a.count[0] = t->prog_count[p0];
    a.ny = 1;
    if (p1 >= 0 && t->prog_count[p1] > 0) { a.first[1] = t->prog_first[p1]; a.count[1] = t->prog_count[p1]; a.ny = 2; }
    a.npre[0] = t->npre[p0];
    for (int i = 0; i < t->npre[p0]; ++i) a.pre[0][i] = t->pre[p0][i];
    if (a.ny == 2) { a.npre[1] = t->npre[p1]; for (int i = 0; i < t->npre[p1]; ++i) a.pre[1][i] = t->pre[p1][i]; }
    a.asmp = t->asmp;
    a.B = B; a.bufsz = t->chain_bufsz;
    a.tbuf = ctx->tbuf ? ctx->tbuf + 256 * (p0 / 2) : nullptr;   // [fwd | bwd] x 256 stamps (tools/chain_timing.py)
    a.tfine = ctx->tbuf ? ctx->tbuf + 512 + 128 * (p0 / 2) : nullptr;
    if (p0 >= PROG_FWD_BK_NOCP) a.tbuf = a.tfine = nullptr;      // (the extra launches of the large-batch path are not clocked)
    a.E = ctx->E; a.ntiles = (B + CH_ROWS - 1) / CH_ROWS;
    a.y_base = y_base; a.slot_ny = slot_ny ? slot_ny : a.ny;
    a.G = ctx->E <= 8 ? 8 / ctx->E : 1;
    const int per = a.ntiles * a.ny;
    a.ips = (per + a.G - 1) / a.G;
    const int rounds = (ctx->E + 7) / 8;
    const size_t lds = CH_MAXSTAGE * sizeof(ChainStage) + 3 * (size_t)t->chain_bufsz * sizeof(float);
    if (loss) {     // closing loss phase: 6 term arrays of the workgroup's 16 x D elements + a flag, in an activation buffer the chain is done with
        a.loss_on = 1; a.loss_final = loss->final; a.loss_buf = t->loss_buf; a.loss_lv0 = t->loss_lv0; a.loss_slots = ctx->E * a.slot_ny * a.ntiles;
        a.lossp = loss->lp; a.lossr = loss->rp;
        const size_t terms = 6 * (size_t)CH_ROWS * ctx->D;          // (the final reduction reuses it for up to 512 chunk sums)
        CADM_REQUIRE(((terms > CH_THREADS_MAX ? terms : CH_THREADS_MAX) + 4) * sizeof(float) <= (size_t)t->chain_bufsz * sizeof(float),
                     "training chain: loss scratch does not fit an activation buffer");
    }
    CADM_REQUIRE(lds <= 160 * 1024, "training chain: layer too wide for the LDS-resident activation tile");
    CADM_REQUIRE((long long)B * (t->chain_bufsz / CH_ROWS) * 4 < (1LL << 32),
                 "training chain: batch of %d rows too large for 32-bit per-member offsets", B);
    // more work items than CUs: the throughput flavour (three 4-wave workgroups per CU), if three of them fit the LDS
    const long items = (long)ctx->E * per;
    const bool wide = ctx->train_force_nw ? ctx->train_force_nw == 4 : (items > ctx->n_cus && 3 * lds <= 160 * 1024);
    const void* fn = wide ? reinterpret_cast<const void*>(&chain_kernel<4>) : reinterpret_cast<const void*>(&chain_kernel<8>);
    size_t& attr = wide ? ctx->chain_attr_lds4 : ctx->chain_attr_lds;
    if (lds > attr) {      // per ctx = per device (a process-wide flag would leave a second GPU's attribute unset)
        CADM_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr = lds;
    }
    // member -> XCD affinity while one round of it holds the launch; beyond that every XCD takes a contiguous eighth of the items
    const int affine_slots = (ctx->n_cus / 8) * (wide ? 3 : 1);        // workgroups an XCD holds at once
    a.spread = ctx->train_force_spread ? ctx->train_force_spread == 1 : (ctx->E * a.G < 8 && a.ips > affine_slots);
    a.per_xcd = (int)((items + 7) / 8);
    const unsigned grid = a.spread ? 8u * (unsigned)a.per_xcd : 8u * (unsigned)(a.ips * rounds);
    if (wide) hipLaunchKernelGGL(chain_kernel<4>, dim3(grid), dim3(256), lds, s, a);
    else hipLaunchKernelGGL(chain_kernel<8>, dim3(grid), dim3(512), lds, s, a);
    CADM_CHECK_HIP(hipGetLastError());
    return CADM_OK;
}

// forward of the context / forward (/ backward) nets on one [E,B,.] batch into the workspace
// The large-batch training path (one forward launch per net; ONE pass of the summed context gradient down the encoder) changes the
// arithmetic in the last bits (a sum taken before a linear pass instead of behind it), so WHEN it is taken must be a property of the
// batch, not of the device the step happens to run on: the rule "work items >= 1.5 rounds of three workgroups per CU" is
// evaluated for the part this library is written for -- MI355X, 256 CUs -- whatever ctx->n_cus says: with 5 members + backward model the
// switch is at B = 1856 (1843.2 rounded up to the 16-row tile).  INTEGRATION.md, "numeric envelope"; tests/test_gpu_train.py pins it.
#define CADM_LARGE_BATCH_CUS 256
bool large_batch(const cadm_ctx* ctx, int B) {
    const long items = (long)ctx->E * 2 * ((B + CH_ROWS - 1) / CH_ROWS);
    return 2 * items >= 9L * CADM_LARGE_BATCH_CUS;      // (>= 1.5 rounds of three workgroups per CU: B = 2048 0.4485 -> 0.4445 ms, B = 1024 0.249 -> 0.280)
}

int forward_nets(cadm_ctx* ctx, const RowMap& map, const float* obs, const float* act, const float* obs_next, const float* cp_obs,
                 const float* cp_act, int B, bool has_back, hipStream_t s, const ChainLossCfg* loss = nullptr) {
    TrainState* t = ctx->train;
    const int D = ctx->D;
    int rc;
    if (!t->pack_buf && (rc = alloc_packs(ctx))) return rc;
    if (ctx->train_packs_stale && (rc = pack_streams(ctx, s))) return rc;
    if ((rc = sync_programs(ctx, s))) return rc;
    ChainAsm& ap = t->asmp;
    ap.map = map;
    ap.act = act; ap.cp_obs = cp_obs; ap.cp_act = cp_act;
    ap.obs_mean = ctx->st.obs_mean; ap.obs_std = ctx->st.obs_std; ap.act_mean = ctx->st.act_mean; ap.act_std = ctx->st.act_std;
    ap.cp_obs_mean = ctx->st.cp_obs_mean; ap.cp_obs_std = ctx->st.cp_obs_std;
    ap.cp_act_mean = ctx->st.cp_act_mean; ap.cp_act_std = ctx->st.cp_act_std;
    ap.D = D; ap.A = ctx->A; ap.P = ctx->P;
    ap.ncpo = D * ctx->cfg.history_length; ap.ncpa = ctx->A * ctx->cfg.history_length;
    ap.env = ctx->cfg.env_kind;
    if (ap.env == CADM_ENV_SPEC && !ctx->spec_set) {
        cadm_set_error("training / prediction on a CADM_ENV_SPEC ctx needs its tables first (cadm_set_env_spec)");
        return CADM_ESTATE;
    }
    ap.spec_feat = ap.env == CADM_ENV_SPEC ? ctx->spec_feat : nullptr;
    for (int p : {PROG_FWD_FF, PROG_FWD_BK, PROG_FWD_BK_NOCP})      // the forward net reads obs, the backward model next obs
        for (int i = 0; i < t->npre[p]; ++i) if (t->pre[p][i].mode == 1) t->pre[p][i].g0 = p == PROG_FWD_FF ? obs : obs_next;
    // Large batches: one launch per net, the backward model's behind the forward net's -- its chains then READ the context vector the
    // forward net's chains have left in their input echo instead of running the context encoder a second time on the same histories
    // (4 of a chain's 9 stages; in the joint launch -- the reference's batch: one partial round of the chip -- the two chains of a
    // row tile run side by side and the recomputation costs nothing).  Same arithmetic, same loss partials in the same slots.
    const bool split = has_back && ctx->C > 0 && t->prog_count[PROG_FWD_BK_NOCP] > 0 &&
                       (ctx->train_force_spread ? ctx->train_force_spread == 1 : large_batch(ctx, B));
    if (!split) return launch_chain(ctx, B, PROG_FWD_FF, has_back ? PROG_FWD_BK : -1, s, loss);
    if ((rc = launch_chain(ctx, B, PROG_FWD_FF, -1, s, loss, 0, 2))) return rc;
    return launch_chain(ctx, B, PROG_FWD_BK_NOCP, -1, s, loss, 1, 2);
}

}  // namespace

static int train_step_impl(cadm_ctx* ctx, const RowMap& map, const float* obs, const float* act, const float* delta,
                           const float* obs_next, const float* back_delta, const float* cp_obs, const float* cp_act, int B,
                           int train, float* losses_out, void* stream) {
    CADM_REQUIRE(ctx && obs && act && delta && losses_out && B > 0, "cadm_train_step: bad arguments");
    CADM_REQUIRE(ctx->train && ctx->train->configured, "cadm_train_step: call cadm_train_configure first");
    CADM_REQUIRE(ctx->st.set, "cadm_train_step: normalisation stats not set");
    const bool has_back = ctx->cfg.back_model != 0, has_cp = ctx->C > 0, det = ctx->cfg.deterministic != 0;
    CADM_REQUIRE(!has_back || (obs_next && back_delta), "cadm_train_step: obs_next / back_delta required (backward model)");
    CADM_REQUIRE(!has_cp || (cp_obs && cp_act), "cadm_train_step: cp_obs / cp_act required (context model)");
    CADM_REQUIRE(ctx->ff_maxlv && ctx->ff_minlv, "cadm_train_step: logvar bounds not registered");
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_workspace(ctx, B);
    if (rc) return rc;
    TrainState* t = ctx->train;
    const cadm_train_hparams& hp = t->hp;
    const int E = ctx->E, NH = ctx->NH, HID = ctx->HID, D = ctx->D;
    const int ncp = has_cp ? ctx->cfg.n_cp_hidden : 0;
    const long R = (long)E * B;
    TrainNet &ff = t->net[CADM_NET_FF], &bk = t->net[CADM_NET_BACK], &cp = t->net[CADM_NET_CTX];

    // ---- forward + losses + head gradients ----
    LossP lp{};
    lp.map = map;
    lp.mu = ff.nb.mu; lp.lv = ff.nb.lv; lp.bmu = bk.nb.mu; lp.delta = delta; lp.back_delta = back_delta;
    lp.dmean = ctx->st.delta_mean; lp.dstd = ctx->st.delta_std; lp.bdmean = ctx->st.back_delta_mean; lp.bdstd = ctx->st.back_delta_std;
    lp.maxlv = ctx->ff_maxlv; lp.minlv = ctx->ff_minlv;
    lp.dMu = t->dMu; lp.dLv = t->dLv; lp.dBmu = t->dBmu;
    lp.n = R * D; lp.D = D; lp.Dp = t->Dp; lp.B = B; lp.det = det; lp.has_back = has_back; lp.back_coeff = hp.back_coeff;
    // lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t)  (TF1 Adam)
    if (train) t->step += 1;
    const float lr_t = (float)(hp.learning_rate * sqrt(1.0 - pow((double)hp.beta2, (double)t->step)) /
                               (1.0 - pow((double)hp.beta1, (double)t->step)));
    ReduceP rp{};
    rp.part = t->terms; rp.D = D; rp.out = t->red; rp.counter = reinterpret_cast<unsigned*>(t->red + 4 + 2 * D);
    rp.det = det; rp.has_back = has_back; rp.back_coeff = hp.back_coeff; rp.losses_out = losses_out;
    rp.adam_mm = train && !det;
    rp.maxlv = ctx->ff_maxlv; rp.minlv = ctx->ff_minlv;
    rp.mx_m = t->a_mx.m; rp.mx_v = t->a_mx.v; rp.mn_m = t->a_mn.m; rp.mn_v = t->a_mn.v;
    rp.lr_t = lr_t; rp.b1 = hp.beta1; rp.b2 = hp.beta2; rp.eps = hp.epsilon;
    CADM_REQUIRE(lp.n < (1L << 31), "cadm_train_step: E*B*D too large");
    // forward chains; their closing phase takes the losses, the head gradients and the reductions (chain_loss_phase)
    ChainLossCfg lc{lp, rp, train ? 0 : 1};
    if ((rc = forward_nets(ctx, map, obs, act, obs_next, cp_obs, cp_act, B, has_back, s, &lc))) return rc;
    if (!train) return CADM_OK;

    // ---- backward + Adam ----
    const float coeff = hp.weight_decay_coeff;
    auto wd_dyn = [&](int l) { return coeff * (l < NH ? hp.weight_decays[l] : hp.weight_decays[NH]); };

    // backward chains (read W) ...
    const bool merge = has_back && has_cp && t->prog_count[PROG_BWD_CP] > 0 &&
                       (ctx->train_force_merge ? ctx->train_force_merge == 1 : large_batch(ctx, B));      // (forward_nets' rule)
    if (!merge) {
        if ((rc = launch_chain(ctx, B, PROG_BWD_FF, has_back ? PROG_BWD_BK : -1, s))) return rc;
    } else {
        if ((rc = launch_chain(ctx, B, PROG_BWD_FF_NOCP, PROG_BWD_BK_NOCP, s))) return rc;
        if ((rc = launch_chain(ctx, B, PROG_BWD_CP, -1, s))) return rc;
    }

    // ... then every layer's weight gradient + Adam as one grouped launch (overwrites W)
    DwArgs da{};
    da.B = B; da.lr_t = lr_t; da.b1 = hp.beta1; da.b2 = hp.beta2; da.eps = hp.epsilon;
    int tiles = 0;
    // layer l of a net;  X == dZ == null: a job without data -- the gradient is the L2 term alone, no bias, no packed copies to keep current
    auto add_job = [&](TrainNet& n, int l, const float* X, int ldx, const float* dZ, int ldz, float wdc) -> int {
        CADM_REQUIRE(da.njobs < DW_MAXJOBS, "cadm_train_step: too many layers for the grouped weight-gradient launch");
        const DenseRef& L = (*n.L)[l];
        const AdamSlot &aw = n.adam[2 * l], &ab = n.adam[2 * l + 1];
        DwJob& j = da.job[da.njobs++];
        j.X = X; j.dZ = dZ; j.dZ2 = nullptr; j.W = L.W; j.Mw = aw.m; j.Vw = aw.v;
        if (X) { j.bW = L.b; j.bM = ab.m; j.bV = ab.v; j.pf = n.pf[l]; j.pb = n.pb[l]; }
        j.ldx = ldx; j.ldz = ldz; j.M = L.din; j.N = L.dout; j.tile0 = tiles; j.wdc = wdc; j.tn = (L.dout + TN - 1) / TN;
        tiles += j.tn * ((L.din + TM - 1) / TM);
        return CADM_OK;
    };
    auto net_jobs = [&](TrainNet& n, const float* dMu, const float* dLv) -> int {      // a dynamics net: hidden layers, mu head (, logvar head)
        NetBufs& nb = n.nb;
        int r;
        for (int l = 0; l < NH; ++l)
            if ((r = add_job(n, l, l == 0 ? n.X : nb.h[l - 1], l == 0 ? t->K0p : HID, nb.dz[l], HID, wd_dyn(l)))) return r;
        if ((r = add_job(n, NH, nb.h[NH - 1], HID, dMu, t->Dp, wd_dyn(NH)))) return r;
        if (dLv && (r = add_job(n, NH + 1, nb.h[NH - 1], HID, dLv, t->Dp, wd_dyn(NH + 1)))) return r;
        return CADM_OK;
    };
    if ((rc = net_jobs(ff, t->dMu, det ? nullptr : t->dLv))) return rc;
    if (has_back && (rc = net_jobs(bk, t->dBmu, nullptr))) return rc;
    if (has_cp) {
        auto wd_cp = [&](int l) { return coeff * (l < ncp ? hp.context_weight_decays[l] : hp.context_weight_decays[ncp]); };
        for (int l = 0; l <= ncp; ++l) {      // gradient = the forward net's share (+ the backward model's), added on load
            if ((rc = add_job(cp, l, l == 0 ? cp.X : cp.nb.h[l - 1], l == 0 ? t->cpinp : ctx->cp[l - 1].dout, l == ncp ? ff.nb.dctx : cp.nb.dz[l],
                                l == ncp ? t->Cp : ctx->cp[l].dout, wd_cp(l)))) return rc;
            if (has_back && !(merge && l < ncp)) da.job[da.njobs - 1].dZ2 = l == ncp ? bk.nb.dctx : t->cp_dz2[l];      // (merged: cp.nb.dz holds the sum)
        }
    }
    // output_logvar outside the data path (deterministic forward net / backward net): its weight only sees the L2 term
    // (a job without data: X = null), its bias has no gradient at all and is skipped like TF does
    if (det && (rc = add_job(ff, NH + 1, nullptr, 0, nullptr, 0, wd_dyn(NH + 1)))) return rc;
    if (has_back && (rc = add_job(bk, NH + 1, nullptr, 0, nullptr, 0, wd_dyn(NH + 1)))) return rc;
    da.tiles = tiles; da.E = E;
    da.tbuf = ctx->tbuf;
    for (int i = 0; i < da.njobs; ++i) da.tile0s[i] = da.job[i].tile0;
    da.lossr = rp; da.loss_slots = E * (has_back ? 2 : 1) * ((B + CH_ROWS - 1) / CH_ROWS);
    hipLaunchKernelGGL(dw_adam_kernel, dim3(8 * ((tiles * E + 7) / 8) + 8), dim3(256), 0, s, da);
    CADM_CHECK_HIP(hipGetLastError());
    ctx->packed = false;   // planner streams are stale until cadm_repack
    return CADM_OK;
}

extern "C" int cadm_train_step(cadm_ctx* ctx, const float* obs, const float* act, const float* delta,
                               const float* obs_next, const float* back_delta, const float* cp_obs,
                               const float* cp_act, int B, int train, float* losses_out, void* stream) {
    return train_step_impl(ctx, RowMap{}, obs, act, delta, obs_next, back_delta, cp_obs, cp_act, B, train, losses_out, stream);
}

// The same step on rows of a WINDOWED dataset resident on the device (fit(), dynamics.py:382-569 + :676-696): per-step
// tensors [N, F, .], history tensors [N, .]; training row rid = (row_w[rid], row_f[rid]); the batch is idx[e * idx_ld + b].
extern "C" int cadm_train_step_rows(cadm_ctx* ctx, const float* ds_obs, const float* ds_act, const float* ds_delta,
                                    const float* ds_obs_next, const float* ds_back_delta, const float* ds_cp_obs,
                                    const float* ds_cp_act, int F, const long long* row_w, const long long* row_f,
                                    const long long* idx, long long idx_ld, int B, int train, float* losses_out,
                                    void* stream) {
    CADM_REQUIRE(F >= 1 && row_w && row_f && idx && idx_ld >= B, "cadm_train_step_rows: bad row index arguments");
    RowMap map{idx, row_w, row_f, F, B, idx_ld};
    return train_step_impl(ctx, map, ds_obs, ds_act, ds_delta, ds_obs_next, ds_back_delta, ds_cp_obs, ds_cp_act, B, train, losses_out,
                           stream);
}

// One-step prediction heads of every member on an [E,B,.] batch (the vanilla reference's `_get_pred`,
// mlp_ensemble_cem_dynamics.py:185-189: [mlp.mu, mlp.logvar]): normalised mean and clamped log-variance.
extern "C" int cadm_predict(cadm_ctx* ctx, const float* obs, const float* act, const float* cp_obs, const float* cp_act,
                            int B, float* mu_out, float* logvar_out, void* stream) {
    CADM_REQUIRE(ctx && obs && act && mu_out && B > 0, "cadm_predict: bad arguments");
    CADM_ON_DEVICE(ctx);
    CADM_REQUIRE(ctx->st.set, "cadm_predict: normalisation stats not set");
    CADM_REQUIRE(ctx->C == 0 || (cp_obs && cp_act), "cadm_predict: cp_obs / cp_act required (context model)");
    for (auto& d : ctx->ff) CADM_REQUIRE(d.W && d.b, "cadm_predict: ff_model weights not registered");
    if (ctx->C > 0) for (auto& d : ctx->cp) CADM_REQUIRE(d.W && d.b, "cadm_predict: context_model weights not registered");
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_state(ctx);
    if (rc) return rc;
    if ((rc = ensure_workspace(ctx, B))) return rc;
    if ((rc = forward_nets(ctx, RowMap{}, obs, act, nullptr, cp_obs, cp_act, B, false, s))) return rc;
    TrainState* t = ctx->train;
    const long n = (long)ctx->E * B * ctx->D;
    CADM_CHECK_HIP(hipMemcpyAsync(mu_out, t->net[CADM_NET_FF].nb.mu, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (logvar_out) {
        CADM_REQUIRE(!ctx->cfg.deterministic, "cadm_predict: a deterministic model has no log-variance head output");
        hipLaunchKernelGGL(clamp_logvar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t->net[CADM_NET_FF].nb.lv, ctx->ff_maxlv,
                           ctx->ff_minlv, logvar_out, n, ctx->D);
        CADM_CHECK_HIP(hipGetLastError());
    }
    return CADM_OK;
}
