// Env tables: the closures of an env kind as compile-time data (dims, per-dim preprocessing / postprocessing masks, single-dim reward
// terms, control cost, bonus) -- the vocabulary of a user-declared env (include/cadm_hip.h cadm_env_spec, cadm_amd/env_spec.py EnvDecl).
// rollout_env.h evaluates the table of its template parameter; a kind without a table keeps hand-written closures there.
#pragma once
#include "../../include/cadm_hip.h"

struct EnvTerm { int kind, dim, when; float w, lo, hi; };

// no table: the five built-in kinds, and CADM_ENV_SPEC inside the library, which never instantiates a kernel for it (its dims are
// 0 here and come from the ctx config, cadm_ctx_create)
template <int ENV> struct EnvTable {
    static constexpr bool is_table = false;
    static constexpr int D = 0, A = 0, P = 0;
    static constexpr unsigned long long drop = 0, sincos = 0, replace = 0;
    static constexpr int nterms = 0;
    static constexpr EnvTerm terms[1] = {{0, 0, 0, 0.0f, 0.0f, 0.0f}};
    static constexpr float ctrl = 0.0f, bonus = 0.0f;
};

// a side module built for one user-declared env (cadm_amd/jit.py, -DCADM_JIT_SPEC): the table of its generated cadm_spec_tables.h
#ifdef CADM_JIT_SPEC
#include "cadm_spec_tables.h"
template <> struct EnvTable<CADM_ENV_SPEC> {
    static constexpr bool is_table = true;
    static constexpr int D = CADM_SPEC_D, A = CADM_SPEC_A, P = CADM_SPEC_P;
    static constexpr unsigned long long drop = CADM_SPEC_DROP_MASK;        // bit d: obs dim d feeds no feature
    static constexpr unsigned long long sincos = CADM_SPEC_SINCOS_MASK;    // bit d: obs dim d feeds sin, cos
    static constexpr unsigned long long replace = CADM_SPEC_REPLACE_MASK;  // bit d: next[d] = delta[d] (else obs[d] + delta[d])
    static constexpr int nterms = CADM_SPEC_NTERMS;
    static constexpr EnvTerm terms[CADM_SPEC_NTERMS + 1] = {CADM_SPEC_TERMS {0, 0, 0, 0.0f, 0.0f, 0.0f}};
    static constexpr float ctrl = CADM_SPEC_CTRL, bonus = CADM_SPEC_BONUS;
};
#endif

// halfcheetah, ant and slim humanoid are expressible as tables (env_spec.py restate()) but keep hand-written closures in rollout_env.h:
// the table form of their kernels timed slower than the A/A' spread of one box (profiles/env_tables_ab.md)
__host__ __device__ constexpr int env_D(int k) { return k == CADM_ENV_SPEC ? EnvTable<CADM_ENV_SPEC>::D : k == 0 ? 18 : k == 1 ? 28 : k == 2 ? 45 : k == 3 ? 4 : 3; }
__host__ __device__ constexpr int env_A(int k) { return k == CADM_ENV_SPEC ? EnvTable<CADM_ENV_SPEC>::A : k == 0 ? 6 : k == 1 ? 8 : k == 2 ? 17 : k == 3 ? 2 : 1; }
__host__ __device__ constexpr int env_P(int k) { return k == CADM_ENV_SPEC ? EnvTable<CADM_ENV_SPEC>::P : k == 0 ? 18 : k == 1 ? 27 : k == 2 ? 45 : k == 3 ? 4 : 3; }
