// Step reward of one particle from recorded states, for the kernels that run BEHIND the rollout (forecast.hip, constrain.hip): one
// definition, so that a forecast's step rewards and a terminated candidate's partial return are the same numbers.
#pragma once
#include "planner.h"
#include "rollout_env.h"

// a CADM_ENV_SPEC ctx's reward tables (cadm_env_spec), evaluated at run time: the library holds no compile-time table for them
struct ForecastSpec {
    int n_terms;
    int kind[CADM_SPEC_MAX_TERMS], dim[CADM_SPEC_MAX_TERMS], when[CADM_SPEC_MAX_TERMS];
    float w[CADM_SPEC_MAX_TERMS], lo[CADM_SPEC_MAX_TERMS], hi[CADM_SPEC_MAX_TERMS];
    float ctrl, bonus;
};

// the ctx's uploaded spec as the kernels read it (a ctx of a built-in kind: left zeroed, never read)
inline void forecast_spec_fill(const cadm_ctx* ctx, ForecastSpec* out) {
    if (ctx->cfg.env_kind != CADM_ENV_SPEC) return;
    const cadm_env_spec& sp = ctx->spec;
    out->n_terms = sp.n_terms;
    for (int k = 0; k < sp.n_terms; ++k) {
        out->kind[k] = sp.term_kind[k]; out->dim[k] = sp.term_dim[k]; out->when[k] = sp.term_when[k];
        out->w[k] = sp.term_w[k]; out->lo[k] = sp.term_lo[k]; out->hi[k] = sp.term_hi[k];
    }
    out->ctrl = sp.ctrl_cost; out->bonus = sp.bonus;
}

__device__ __forceinline__ float fc_term(int kind, float x, float w, float lo, float hi) {
    switch (kind) {
        case CADM_SPEC_TERM_LINEAR: return spec_term_value<CADM_SPEC_TERM_LINEAR>(x, w, lo, hi);
        case CADM_SPEC_TERM_SQUARE: return spec_term_value<CADM_SPEC_TERM_SQUARE>(x, w, lo, hi);
        case CADM_SPEC_TERM_ABS: return spec_term_value<CADM_SPEC_TERM_ABS>(x, w, lo, hi);
        case CADM_SPEC_TERM_INSIDE: return spec_term_value<CADM_SPEC_TERM_INSIDE>(x, w, lo, hi);
        default: return spec_term_value<CADM_SPEC_TERM_OUTSIDE>(x, w, lo, hi);
    }
}

// Step reward of one particle: pre / post = its D pre- and post-step values, act = the step's raw action (A values).
// Built-in kinds: the pair parts of rollout_env.h (the terms the rollout adds), summed in ascending pair order.
// CADM_ENV_SPEC: the grouping of env_spec.py EnvDecl.reward -- ((pre-step terms of the first term's dim pair) - c ctrl) + bonus,
// then the other terms in declaration order.
template <int ENV>
__device__ __forceinline__ float step_reward(const ForecastSpec& sp, int D, int A, const float* pre, const float* post, const float* act) {
    const float ctrl = ctrl_term<ENV>(act, A);
    if constexpr (ENV == CADM_ENV_SPEC) {
        const int first_pair = sp.n_terms > 0 ? sp.dim[0] >> 1 : 0;
        float r = 0.0f;
        bool any = false;
        for (int k = 0; k < sp.n_terms; ++k) {
            if ((sp.dim[k] >> 1) != first_pair || sp.when[k] != CADM_SPEC_WHEN_OBS) continue;
            const float v = fc_term(sp.kind[k], pre[sp.dim[k]], sp.w[k], sp.lo[k], sp.hi[k]);
            r = any ? r + v : v;
            any = true;
        }
        if (sp.ctrl != 0.0f) r = r - sp.ctrl * ctrl;
        if (sp.bonus != 0.0f) r = r + sp.bonus;
        for (int k = 0; k < sp.n_terms; ++k) {
            const bool next = sp.when[k] != CADM_SPEC_WHEN_OBS;
            if ((sp.dim[k] >> 1) == first_pair && !next) continue;
            r = r + fc_term(sp.kind[k], (next ? post : pre)[sp.dim[k]], sp.w[k], sp.lo[k], sp.hi[k]);
        }
        return r;
    } else {
        float r = 0.0f;
        const int pairs = (D + 1) >> 1;
        for (int dp = 0; dp < pairs; ++dp) {
            const float part = reward_part<ENV>(dp, pre[2 * dp], 2 * dp + 1 < D ? pre[2 * dp + 1] : 0.0f, ctrl);
            r = dp == 0 ? part : r + part;
        }
        return r;
    }
}
