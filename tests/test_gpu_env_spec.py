"""GPU: user-declared envs (cadm_amd/env_spec.py EnvDecl) end to end.

* Restated built-ins (halfcheetah with and without context, ant, slim humanoid) run through a spec-built rollout module and the spec
  path of the training kernels: every rollout flavour, the CEM plan, a training step and predict() are BIT-IDENTICAL to the
  compiled-in kind's.
* Two envs no built-in covers -- a hopper-like one (odd D, two sincos dims that are not dim 2, a replace dim, every term kind on
  both states) and a small deterministic vanilla one (next-state terms only) -- against the oracle (duck-typed on env objects).
* The class API on the hopper-like spec, and the library's checks with a live ctx (malformed tables, a module of another spec)."""
import ctypes

import numpy as np
import pytest

from cadm_amd import _lib, jit, synth
from cadm_amd import planner as hplanner
from cadm_amd.env_spec import EnvDecl, restate
from helpers import (FLAVOURS, _np, assert_close, check_class_api_on_spec, check_spec_training_step, close_but_jumps, make_engine,
                     threshold_jump, trunc_z)
from helpers import SPEC_CWD as CWD
from helpers import SPEC_WD as WD
from helpers import run_flavour as _run
from helpers import spec_oracle as _oracle
from oracle import nets as onets
from oracle import planner as oplanner

pytestmark = pytest.mark.gpu


def hopper_like():
    return EnvDecl(11, 3, preproc=["drop", "sincos", "id", "id", "sincos", "id", "id", "id", "id", "id", "id"],
                   postproc=["add"] * 5 + ["replace"] + ["add"] * 5,
                   reward=[dict(kind="linear", dim=5), dict(kind="square", dim=3, w=-0.5, when="next_obs"),
                           dict(kind="abs", dim=10, w=-0.1), dict(kind="inside", dim=0, w=1.0, lo=-0.5, hi=0.5, when="next_obs"),
                           dict(kind="outside", dim=2, w=-1.0, lo=-0.2, hi=0.2), dict(kind="linear", dim=4, w=0.3, when="next_obs"),
                           dict(kind="square", dim=7, w=-0.05), dict(kind="abs", dim=6, w=0.2, when="next_obs"),
                           dict(kind="outside", dim=9, w=-0.5, lo=-1.0, hi=1.0, when="next_obs"),
                           dict(kind="inside", dim=8, w=0.25, lo=-0.3, hi=0.8)],
                   ctrl_cost=0.001, bonus=1.0)


def small_vanilla():
    return EnvDecl(7, 1, preproc=["id", "id", "sincos", "id", "drop", "id", "id"],
                   reward=[dict(kind="linear", dim=0, when="next_obs"), dict(kind="square", dim=2, w=-0.1, when="next_obs"),
                           dict(kind="outside", dim=1, w=-1.0, lo=-1.5, hi=1.5, when="next_obs")], ctrl_cost=0.01)


# ------------------------------------------------------------------------------------------------------------------------------
# restated built-ins: bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,context,p", [("halfcheetah", True, 20), ("halfcheetah", False, 5), ("ant", True, 20), ("slim_humanoid", True, 20)])
def test_restated_builtin_is_bit_identical(gpu, kind, context, p):
    E, m, n, H, B = 5, 2, 13, 8, 37                  # 13 candidates x 4 rows per member: ragged row tiles
    spec = restate(kind)
    prob = synth.make_problem(env=kind, context=context, E=E, m=m, H=H, trained_like=True, with_back=context, seed=31)
    sprob = synth.make_problem(env=spec, context=context, E=E, m=m, H=H, trained_like=True, with_back=context, seed=31)
    for k in ("ff", "stats"):
        assert all(np.array_equal(prob[k][x], sprob[k][x]) for x in prob[k])
    dev = _lib.load_dev()
    eb, es = make_engine(prob, p=p, lib=dev), make_engine(sprob, p=p, lib=dev)
    assert eb.lib.cadm_rollout_builtin(eb._ctx) and not es.lib.cadm_rollout_builtin(es._ctx)
    rng = np.random.default_rng(7)
    D, A = prob["D"], prob["A"]
    acts = rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32)
    eps = rng.standard_normal((H, m, n, p, D)).astype(np.float32)
    obs_rows = rng.standard_normal((m, n, p, D)).astype(np.float32)
    cb = eb.context_forward(prob["cp_obs"], prob["cp_act"]) if context else None
    cs = es.context_forward(prob["cp_obs"], prob["cp_act"]) if context else None
    if context:
        np.testing.assert_array_equal(_np(cs), _np(cb))
    for kw in (dict(eps=eps), dict(seed=5, call=3, it=1), dict(obs_rows=obs_rows, seed=9, call=1)):
        for fl in FLAVOURS:
            rb, tb = _run(eb, fl, prob["obs"], cb, acts, **kw)
            rs, ts = _run(es, fl, prob["obs"], cs, acts, **kw)
            assert np.isfinite(rb).all()
            np.testing.assert_array_equal(ts, tb, err_msg="traj_out, flavour %s, %s" % (fl, sorted(kw)))
            np.testing.assert_array_equal(rs, rb, err_msg="returns, flavour %s, %s" % (fl, sorted(kw)))
    n_plan = 64
    pb = _np(eb.cem_plan(prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], n_plan, seed=4, call=2))
    ps = _np(es.cem_plan(prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], n_plan, seed=4, call=2))
    np.testing.assert_array_equal(ps, pb, err_msg="CEM plan")
    # one training step (losses, every updated weight) and the prediction heads
    batch = synth.make_train_batch(prob, B=B, seed=2)
    keys = ["obs", "act", "delta"] + (["obs_next", "back_delta", "cp_obs", "cp_act"] if context else [])
    bc = 0.5 if context else 0.0
    out = []
    for eng in (eb, es):
        eng.train_configure(1e-3, WD, CWD, 1.0, bc, max_batch=B)
        losses = _np(eng.train_step({k: eng._t(batch[k]) for k in keys}, train=True))
        mu, lv = eng.predict_heads(batch["obs"], batch["act"], batch["cp_obs"] if context else None, batch["cp_act"] if context else None)
        out.append((losses, {(nn, k): _np(v) for nn in eng.net_names() for k, v in eng.nets[nn].items()}, _np(mu), _np(lv)))
    np.testing.assert_array_equal(out[1][0], out[0][0], err_msg="losses")
    for key in out[0][1]:
        np.testing.assert_array_equal(out[1][1][key], out[0][1][key], err_msg="trained %s/%s" % key)
    np.testing.assert_array_equal(out[1][2], out[0][2], err_msg="predict mu")
    np.testing.assert_array_equal(out[1][3], out[0][3], err_msg="predict logvar")
    eb.close(); es.close()


# ------------------------------------------------------------------------------------------------------------------------------
# new envs against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
NEW = [  # name, spec factory, context, E, p, deterministic
    ("hopper", hopper_like, True, 5, 10, False),
    ("small", small_vanilla, False, 5, 5, True),
]


@pytest.mark.parametrize("name,make,context,E,p,det", NEW)
def test_new_env_rollouts_match_oracle(gpu, name, make, context, E, p, det):
    spec = make()
    m, n = 2, 9
    dev = _lib.load_dev()
    rng = np.random.default_rng(11)
    for H in (1, 30):
        prob = synth.make_problem(env=spec, context=context, E=E, m=m, H=H, trained_like=H == 1, seed=12)
        eng = make_engine(prob, p=p, H=H, deterministic=det, lib=dev)
        D, A = prob["D"], prob["A"]
        acts = rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32)
        eps = rng.standard_normal((H, m, n, p, D)).astype(np.float32)
        obs_rows = rng.standard_normal((m, n, p, D)).astype(np.float32) if H == 1 else None
        ctx = eng.context_forward(prob["cp_obs"], prob["cp_act"]) if context else None
        o = _oracle(prob, spec)
        T = oplanner.context_table_indexed(onets.context_forward(o["cp"], o["cp_obs"], o["cp_act"], o["st"]), 0) if context else None
        r_ref, t_ref = oplanner.rollout_indexed(spec, o["ff"], o["st"], o["obs"], T, acts, eps, E, p, det, obs_rows=obs_rows, return_traj=True)
        kw = dict(obs_rows=obs_rows) if H == 1 else {}
        if not det:
            kw["eps"] = eps
        first = None
        for fl in FLAVOURS:
            rows, traj = _run(eng, fl, prob["obs"], ctx, acts, **kw)
            assert_close(traj, t_ref, 1e-5, "%s H=%d next obs, flavour %s" % (name, H, fl))
            assert_close(rows, r_ref, 1e-5, "%s H=%d returns, flavour %s" % (name, H, fl))
            if first is None:
                first = (rows, traj)
            np.testing.assert_array_equal(rows, first[0])
            np.testing.assert_array_equal(traj, first[1])
        eng.close()


@pytest.mark.parametrize("name,make,context,E,p,det", NEW)
def test_new_env_planners_match_oracle(gpu, name, make, context, E, p, det):
    spec = make()
    m, n, H = 2, 64, 8
    prob = synth.make_problem(env=spec, context=context, E=E, m=m, H=H, seed=8)
    eng = make_engine(prob, p=p, deterministic=det)
    rng = np.random.default_rng(12)
    D, A = prob["D"], prob["A"]
    z = trunc_z(rng, (5, m, n, H, A)).astype(np.float32)
    eps = rng.standard_normal((5, H, m, n, p, D)).astype(np.float32)
    plan, info, ctx = hplanner.cem_plan(eng, prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], n,
                                        z=eng._t(z), eps=None if det else eng._t(eps), return_info=True)
    o = _oracle(prob, spec)
    ref, rinfo, _ = oplanner.cem_plan(spec, o["ff"], o["cp"], o["st"], o["obs"], o["cp_obs"], o["cp_act"], o["init_mean"], o["init_var"],
                                      z, eps, E, p, deterministic=det, return_info=True)
    jump = threshold_jump(spec, H, p)
    for it in range(5):
        np.testing.assert_array_equal(np.sort(_np(info[it]["elites"]), axis=1), np.sort(rinfo[it]["elites"], axis=1),
                                      err_msg="%s: elite set differs at CEM iteration %d" % (name, it))
        close_but_jumps(_np(info[it]["cand"])[0], rinfo[it]["cand_returns"], jump, "candidate returns it=%d" % it)
    assert_close(_np(plan), oplanner.get_action_clip(ref), 1e-4, "%s final CEM plan" % name)
    acts = rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32)
    first, cand = hplanner.rs_plan(eng, prob["obs"], prob["cp_obs"], prob["cp_act"], n, actions=acts, eps=None if det else eng._t(eps[0]))
    rfirst, rcand = oplanner.rs_plan(spec, o["ff"], o["cp"], o["st"], o["obs"], o["cp_obs"], o["cp_act"], acts, eps[0], E, p, deterministic=det)
    close_but_jumps(_np(cand)[0], rcand, jump, "%s RS candidate returns" % name)
    np.testing.assert_array_equal(_np(first), np.clip(rfirst, -1, 1))
    eng.close()


@pytest.mark.parametrize("name,make,context,E,p,det", NEW)
def test_new_env_training_step_matches_oracle(gpu, name, make, context, E, p, det):
    """Losses and gradients against oracle/train (helpers.check_spec_training_step)."""
    spec = make()
    prob = synth.make_problem(env=spec, context=context, E=E, trained_like=True, with_back=True, seed=61)
    check_spec_training_step(spec, prob, E, det, name)


# ------------------------------------------------------------------------------------------------------------------------------
# the class API on a spec env
# ------------------------------------------------------------------------------------------------------------------------------
def test_class_api_on_a_spec_env(gpu, tmp_path):
    check_class_api_on_spec(hopper_like(), tmp_path, epochs=3)


def test_vanilla_class_on_a_spec_env(gpu):
    from cadm_amd.dynamics.mlp_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as Vanilla
    spec = small_vanilla()
    D, A, H = 7, 1, 5
    model = Vanilla("dyn", spec, hidden_nonlinearity="swish", n_forwards=H, n_candidates=64, ensemble_size=5, n_particles=5, use_cem=True,
                    batch_size=32, normalize_input=True, deterministic=True, weight_decays=WD)
    rng = np.random.default_rng(1)
    obs = rng.standard_normal((200, D))
    model.fit(obs, rng.uniform(-1, 1, (200, A)), obs + 0.1 * rng.standard_normal((200, D)), epochs=2)
    plan = model.get_action(obs[:3], np.zeros((3, H, A)), np.full((3, H, A), 0.25))
    assert plan.shape == (3, H, A) and np.isfinite(plan).all()
    nxt = model.predict(obs[:3], plan[:, 0])
    assert nxt.shape == (5, 3, D) and np.isfinite(nxt).all()


# ------------------------------------------------------------------------------------------------------------------------------
# the library's checks with a live ctx
# ------------------------------------------------------------------------------------------------------------------------------
def test_library_refuses_malformed_tables_and_foreign_modules(gpu):
    spec, other = hopper_like(), small_vanilla()
    prob = synth.make_problem(env=spec, context=True, E=5, m=1, H=4, seed=3)
    eng = make_engine(prob, p=10)
    lib = eng.lib
    bad = spec.to_c()
    bad.term_dim[2] = 11                                # a term that reads a dim past D
    assert lib.cadm_set_env_spec(eng._ctx, ctypes.byref(bad)) == -1
    assert b"past D=11" in lib.cadm_last_error()
    bad = spec.to_c()
    bad.preproc[3] = 2                                  # one more sincos dim: more features than P
    assert lib.cadm_set_env_spec(eng._ctx, ctypes.byref(bad)) == -1 and b"features" in lib.cadm_last_error()
    bad = spec.to_c()
    bad.hash_lo ^= 1
    assert lib.cadm_set_env_spec(eng._ctx, ctypes.byref(bad)) == -1 and b"hash" in lib.cadm_last_error()
    assert lib.cadm_set_env_spec(eng._ctx, ctypes.byref(spec.to_c())) == 0
    # a module built for another spec of the same shape is refused by hash
    same_shape = EnvDecl(11, 3, preproc=list(spec.preproc), postproc=list(spec.postproc), reward=[dict(kind="linear", dim=5, w=2.0)])
    path = jit.build(_lib.ENV_SPEC, 10, 200, 4, 0, _lib.NOISE_INJECT, spec=same_shape)
    mod = ctypes.CDLL(path)
    desc = (ctypes.c_int * 10)()
    mod.cadm_jit_describe(desc)
    rc = lib.cadm_register_rollout(eng._ctx, _lib.NOISE_INJECT, ctypes.cast(mod.cadm_jit_rollout, ctypes.c_void_p), desc)
    assert rc == -1 and b"env spec" in lib.cadm_last_error()
    # a spec ctx without a module of its own: no kernel in the library
    assert lib.cadm_rollout_check(eng._ctx, _lib.NOISE_INJECT, 1, 4) == -5
    assert b"user-declared" in lib.cadm_last_error()
    # the spec's own module registers, and a set of tables is required before training
    eng.ensure_rollout(_lib.NOISE_INJECT)
    eng.close()
    cfg = _lib.Config.from_buffer_copy(eng.cfg)
    ctx = ctypes.c_void_p()
    assert lib.cadm_ctx_create(ctypes.byref(cfg), ctypes.byref(ctx)) == 0
    try:
        assert lib.cadm_set_env_spec(ctx, ctypes.byref(other.to_c())) == -1 and b"differ" in lib.cadm_last_error()
    finally:
        lib.cadm_ctx_destroy(ctx)
