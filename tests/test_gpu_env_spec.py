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
import torch

from cadm_amd import _lib, jit, synth
from cadm_amd import planner as hplanner
from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
from cadm_amd.env_spec import EnvDecl, restate
from cadm_amd.policies.mpc_controller import MPCController
from cadm_amd.samplers.model_sample_processor import ModelSampleProcessor
from helpers import assert_close, make_engine, trunc_z
from oracle import nets as onets
from oracle import planner as oplanner
from oracle import train as otrain

pytestmark = pytest.mark.gpu

WD = (0.000025, 0.00005, 0.000075, 0.000075, 0.0001)
CWD = (0.000025, 0.00005, 0.000075)
FLAVOURS = ("1", "2", "3", "4")      # cooperative kernel with one / two row tiles, wave-tile kernel with 8 / 4 tiles per workgroup


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


def _np(t):
    return t.detach().cpu().numpy()


def _oracle(prob, spec, dt=np.float32):
    o = dict(env=spec, ff=onets.cast_params(prob["ff"], dt), cp=None if prob["cp"] is None else onets.cast_params(prob["cp"], dt),
             st=onets.cast_stats(prob["stats"], dt))
    for k in ("obs", "cp_obs", "cp_act", "init_mean", "init_var"):
        o[k] = prob[k].astype(dt)
    return o


def _run(eng, flavour, obs, ctx, acts, **kw):
    eng.dev_set_rollout("xdl", row_tiles=int(flavour))
    try:
        rows, traj = eng.rollout_returns(obs, ctx, acts, want_traj=True, **kw)
        torch.cuda.synchronize()
        return _np(rows), _np(traj)
    finally:
        eng.dev_set_rollout("xdl", row_tiles=0)


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
    # An indicator term (inside / outside) jumps by its weight where a state sits on its threshold: a particle whose state lands
    # within rounding of it may take the other side in the oracle.  Such a candidate is off by a multiple of w / p -- allowed for at
    # most 1 % of the candidates, everything else at the usual bar (and the elite sets exactly).
    jump = sum(abs(t[3]) for t in spec.terms if t[0] in ("inside", "outside")) * H / p

    def close_but_jumps(got, want, what):
        bad = np.abs(got - want) > 1e-4 * np.maximum(np.abs(want), np.sqrt(np.mean(want ** 2)))
        assert bad.sum() <= 0.01 * bad.size, "%s: %d/%d candidates off" % (what, bad.sum(), bad.size)
        assert (np.abs(got - want)[bad] <= jump + 1e-3).all(), "%s: off by more than one threshold flip" % what
    for it in range(5):
        np.testing.assert_array_equal(np.sort(_np(info[it]["elites"]), axis=1), np.sort(rinfo[it]["elites"], axis=1),
                                      err_msg="%s: elite set differs at CEM iteration %d" % (name, it))
        close_but_jumps(_np(info[it]["cand"])[0], rinfo[it]["cand_returns"], "candidate returns it=%d" % it)
    assert_close(_np(plan), oplanner.get_action_clip(ref), 1e-4, "%s final CEM plan" % name)
    acts = rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32)
    first, cand = hplanner.rs_plan(eng, prob["obs"], prob["cp_obs"], prob["cp_act"], n, actions=acts, eps=None if det else eng._t(eps[0]))
    rfirst, rcand = oplanner.rs_plan(spec, o["ff"], o["cp"], o["st"], o["obs"], o["cp_obs"], o["cp_act"], acts, eps[0], E, p, deterministic=det)
    close_but_jumps(_np(cand)[0], rcand, "%s RS candidate returns" % name)
    np.testing.assert_array_equal(_np(first), np.clip(rfirst, -1, 1))
    eng.close()


@pytest.mark.parametrize("name,make,context,E,p,det", NEW)
def test_new_env_training_step_matches_oracle(gpu, name, make, context, E, p, det):
    """Losses and gradients against oracle/train.  The oracle's obs_preproc is picked by env name, so it is handed the spec's
    preprocessed observations under an identity-preproc name: the same network inputs."""
    spec = make()
    B = 48
    prob = synth.make_problem(env=spec, context=context, E=E, trained_like=True, with_back=True, seed=61)
    batch = synth.make_train_batch(prob, B=B, seed=2)
    cfg = dict(deterministic=det, back_coeff=0.5, weight_decay_coeff=1.0, weight_decays=WD, context_weight_decays=CWD,
               n_hidden=len(prob["hidden_sizes"]), n_cp_hidden=len(prob["cp_hidden_sizes"]))
    keys = ["obs", "act", "delta", "obs_next", "back_delta"] + (["cp_obs", "cp_act"] if context else [])
    tb = {k: torch.tensor(v, dtype=torch.float64) for k, v in batch.items()}
    tb["obs"] = torch.tensor(spec.obs_preproc(batch["obs"]), dtype=torch.float64)
    tb["obs_next"] = torch.tensor(spec.obs_preproc(batch["obs_next"]), dtype=torch.float64)

    def oracle_nets(rg):
        return (otrain.to_torch(prob["ff"], torch.float64, rg), otrain.to_torch(prob["back"], torch.float64, rg),
                otrain.to_torch(prob["cp"], torch.float64, rg) if context else None, otrain.to_torch(prob["stats"], torch.float64))
    eng = make_engine(prob, p=E, deterministic=det)
    eng.train_configure(1e-3, WD, CWD, 1.0, 0.5, max_batch=B)
    got = _np(eng.train_step({k: eng._t(batch[k]) for k in keys}, train=False))
    ff, back, cp, st = oracle_nets(False)
    ref = otrain.train_losses("slim_humanoid", ff, back, cp, st, tb, cfg)       # (identity obs_preproc)
    np.testing.assert_allclose(got, [float(ref["mse"]), float(ref["back_mse"]), float(ref["recon"])], rtol=5e-5, atol=5e-5)
    eng.close()
    eng = make_engine(prob, p=E, deterministic=det)
    eng.train_configure(1e6, WD, CWD, 1.0, 0.5, max_batch=B, beta1=0.0, beta2=0.0, epsilon=1e6)    # linearised Adam: g = w_before - w_after
    before = {nn: {k: v.clone() for k, v in eng.nets[nn].items()} for nn in eng.net_names()}
    eng.train_step({k: eng._t(batch[k]) for k in keys}, train=True)
    ff, back, cp, st = oracle_nets(True)
    out = otrain.train_losses("slim_humanoid", ff, back, cp, st, tb, cfg)
    grads = otrain.grads_of(out["loss"], {"ff_model": ff, "backward_model": back, "context_model": cp})
    for net in eng.net_names():
        for pname, w0 in before[net].items():
            g_ref = grads[net][pname]
            g_hip = (w0 - eng.nets[net][pname]).cpu().numpy().astype(np.float64)
            if g_ref is None:
                assert np.abs(g_hip).max() == 0.0
                continue
            g_ref = g_ref.numpy()
            err = np.abs(g_hip - g_ref).max() / max(np.abs(g_ref).max(), 1e-12)
            assert err < 2e-3, "%s %s/%s gradient off: %.3e" % (name, net, pname, err)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the class API on a spec env
# ------------------------------------------------------------------------------------------------------------------------------
def test_class_api_on_a_spec_env(gpu, tmp_path):
    spec = hopper_like()

    class HopperSim:                                     # a user's simulator: declares its closures, is no built-in class
        cadm_env_spec = spec
        observation_space, action_space, proc_observation_space_dims = spec.observation_space, spec.action_space, spec.proc_obs_dim
        obs_preproc, obs_postproc, targ_proc, reward = spec.obs_preproc, spec.obs_postproc, spec.targ_proc, spec.reward

    class Normalized:                                    # the reference's NormalizedEnv wrapper shape
        def __init__(self, e):
            self.wrapped_env = e
            for k in ("observation_space", "action_space", "proc_observation_space_dims", "obs_preproc", "obs_postproc", "targ_proc", "reward"):
                setattr(self, k, getattr(e, k))
    env = Normalized(HopperSim())
    D, A, Hh, F, H = 11, 3, 10, 10, 6
    kw = dict(hidden_nonlinearity="swish", context_out_dim=10, n_forwards=H, n_candidates=64, ensemble_size=5, n_particles=10, use_cem=True,
              batch_size=32, state_diff=1, normalize_input=True, back_coeff=0.5, weight_decays=WD, weight_decay_coeff=1.0,
              context_weight_decays=CWD + (0.0001,), history_length=Hh, future_length=F)
    model = MLPEnsembleCEMDynamicsModel("dyn", env, **kw)
    assert model.engine.spec == spec
    rng = np.random.default_rng(0)
    paths = []
    for L in (30, 45, 12):
        obs = rng.standard_normal((L, D)).astype(np.float32)
        paths.append(dict(observations=obs, actions=rng.uniform(-1, 1, (L, A)).astype(np.float32), rewards=rng.standard_normal(L),
                          cp_obs=0.1 * rng.standard_normal((L, D * Hh)).astype(np.float32),
                          cp_act=rng.uniform(-1, 1, (L, A * Hh)).astype(np.float32)))
    d = ModelSampleProcessor(context=True, future_length=F).process_samples(paths)
    model.fit(d["concat_obs"], d["concat_act"], d["concat_next_obs"], d["cp_observations"], d["cp_actions"], d["concat_bool"], epochs=3)
    policy = MPCController("mpc", env, model, use_cem=True, n_candidates=64, horizon=H, num_rollouts=2, context=True)
    o, cpo, cpa = rng.standard_normal((2, D)), 0.1 * rng.standard_normal((2, D * Hh)), rng.uniform(-1, 1, (2, A * Hh))
    mean, var = np.zeros((2, H, A)), np.full((2, H, A), 0.25)
    plan, _ = policy.get_actions(o, cpo, cpa, mean, var)
    assert plan.shape == (2, H, A) and np.isfinite(plan).all() and np.abs(plan).max() <= 1.0
    warm = np.concatenate([plan[:, 1:], np.zeros((2, 1, A))], axis=1)          # the samplers' CEM warm start
    plan2, _ = policy.get_actions(o, cpo, cpa, warm, var)
    assert np.isfinite(plan2).all()
    from cadm_amd.caller import DevicePlannerState
    assert DevicePlannerState(model, 2).eng.spec == spec          # the device-resident caller state builds on the same engine
    mu, sd = model.predict(o, plan[:, 0], cpo, cpa, return_std=True)
    assert np.isfinite(mu).all() and np.isfinite(sd).all() and (sd > 0).all()
    cp = model.get_context_pred(cpo, cpa)
    assert np.isfinite(np.asarray(cp)).all()
    path = str(tmp_path / "params")
    model.save(path)
    model2 = MLPEnsembleCEMDynamicsModel("dyn", env, **kw)
    model2.load(path)
    model._call = model2._call = 7
    a1 = model.get_action(o, cpo, cpa, warm, var)
    a2 = model2.get_action(o, cpo, cpa, warm, var)
    np.testing.assert_array_equal(a1, a2)


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
