"""GPU: the context encoder under NON-identity history statistics -- what a model built with the class default state_diff = False
runs with: the history holds raw observations, every column has its own mean and spread (helpers.raw_history_problem), and
x = (cp_obs - cp_obs_mean) / (cp_obs_std + 1e-10) is computed independently at five places: `context_kernel`, `plan_head_kernel`
and `context_batched_kernel<1 / 2>` (csrc/context.hip), the training chain's input assembly (csrc/train_chain.h) and, upstream of
them, the caller's history ring buffer (csrc/caller.hip).  tests/test_context_stats_inputs.py shows on the oracle alone that a
mean or std read from the neighbouring column moves these inputs' context vector by 1.6 - 30 x its rms, six orders above the bars
here, while the float32 oracle stays within 1.8e-6 of the float64 one.

The batched kernel runs with one or two 16-row tiles per workgroup by the launcher's rule (helpers.context_row_tiles, evaluated
for the device's CU count): the tests assert which side of the rule their row counts fall on, so on another CU count they fail
instead of testing one flavour twice."""
import types

import numpy as np
import pytest
import torch

import test_gpu_fit as fit_tests
import test_gpu_horizon as horizon_tests
from cadm_amd import synth
from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as CaDMModel
from cadm_amd.envs import make_env_spec
from helpers import (CWD, RAW_GEOMETRIES, WD, _cfg, _check_gradients, _dev_batch, _dev_engine, _oracle_nets, assert_close,
                     context_row_tiles, floored_rel, make_engine, oracle_problem, raw_histories, raw_history_problem, raw_train_batch,
                     rolled_stats, two_tile_m)
from horizon_ref import check_against_oracle, make_mask
from oracle import nets as onets
from oracle import planner as oplanner
from oracle import train as otrain

pytestmark = pytest.mark.gpu

IDS = ["%s-E%d-Hh%d-%s" % (g[0], g[1], g[2], "x".join(map(str, g[3]))) for g in RAW_GEOMETRIES]
DEFAULT, PENDULUM, ODD = RAW_GEOMETRIES[0], RAW_GEOMETRIES[1], RAW_GEOMETRIES[6]


@pytest.fixture(scope="module")
def n_cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def _row_counts(E, n_cus):
    """(1, 2, 47: the per-row kernel; 48, 65: batched, one row tile; m2: batched, two row tiles, the last tile one row)"""
    m2 = two_tile_m(E, n_cus)
    assert context_row_tiles(E, 48, n_cus) == 1 and context_row_tiles(E, 65, n_cus) == 1, "48 / 65 rows take two row tiles on %d CUs" % n_cus
    assert context_row_tiles(E, m2, n_cus) == 2 and m2 % 32 == 1 and m2 > 65
    return (1, 2, 47, 48, 65, m2)


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------- a
def _check_inference(env, E, Hh, cp_sizes, C, n_cus, seed, zero_std_cols=()):
    ms = _row_counts(E, n_cus)
    prob, cp_obs, cp_act = raw_history_problem(env, E, Hh, cp_sizes, C, ms[-1], seed, zero_std_cols)
    eng = make_engine(prob, p=E)
    o32, o64 = oracle_problem(prob, np.float32), oracle_problem(prob, np.float64)
    ref32 = onets.context_forward(o32["cp"], o32["cp_obs"], o32["cp_act"], o32["st"])
    ref64 = onets.context_forward(o64["cp"], cp_obs, cp_act, o64["st"])
    worst = [0.0, 0.0]
    for m in ms:
        got = _np(eng.context_forward(cp_obs[:m], cp_act[:m]))
        assert got.shape == (E, m, C) and np.isfinite(got).all()
        worst = [max(worst[0], floored_rel(got, ref32[:, :m])), max(worst[1], floored_rel(got, ref64[:, :m]))]
        assert_close(got, ref32[:, :m], 1e-5, "m = %d vs the float32 oracle" % m)
        assert_close(got, ref64[:, :m], 1e-5, "m = %d vs the float64 oracle" % m)
    rng = np.random.default_rng(seed + 7)
    for m in (47, ms[-1]):      # the training graph's layout: [E, m, .] with different rows per member
        bo, ba = raw_histories(prob, (E, m), rng)
        got = _np(eng.context_forward(bo, ba, bs=True))
        for dt, k in ((np.float32, 0), (np.float64, 1)):
            ref = onets.context_forward_bs(onets.cast_params(prob["cp"], dt), bo.astype(dt), ba.astype(dt), onets.cast_stats(prob["stats"], dt))
            worst[k] = max(worst[k], floored_rel(got, ref))
            assert_close(got, ref, 1e-5, "[E,m,.] inputs, m = %d vs the %s oracle" % (m, dt.__name__))
    eng.close()
    print("%s E=%d Hh=%d %r%s, m in %r: worst error %.2e vs the float32 oracle, %.2e vs the float64 oracle (bar 1e-05)" % (
        env, E, Hh, cp_sizes, " zero-std column" if zero_std_cols else "", ms, worst[0], worst[1]))


@pytest.mark.parametrize("env,E,Hh,cp_sizes,C", RAW_GEOMETRIES, ids=IDS)
def test_every_inference_kernel_under_raw_statistics(gpu, n_cus, env, E, Hh, cp_sizes, C):
    """`eng.context_forward` against the float32 and the float64 oracle at 1e-5 (assert_close), per geometry at m = 1, 2, 47 (per-row
    kernel), 48, 65 (batched, one row tile), the smallest m = 1 (mod 32) on the two-tile side (385 / 673 / 289 / 1025 for E = 5 / 3 /
    7 / 2 on 256 CUs; (1024, 512) does not fit two tiles in LDS and runs one there too), and the [E, m, .] layout at m = 47 and the
    two-tile m.
    Measured on an MI355X, worst floored-relative error over all calls of a geometry, vs float32 / float64 oracle: halfcheetah (256, 128, 64)
    1.6e-06 / 1.5e-06; pendulum (8, 6) 6.1e-07 / 8.4e-07; (320, 100, 30) 1.4e-06 / 1.3e-06; ant (64,) 7.9e-07 / 9.0e-07; slim humanoid 3.8e-06 /
    3.1e-06; (1024, 512) 2.9e-06 / 2.7e-06; (70, 50, 30) 1.4e-06 / 1.4e-06 (bar 1e-05; the test prints them)."""
    _check_inference(env, E, Hh, cp_sizes, C, n_cus, seed=5)


@pytest.mark.parametrize("env,E,Hh,cp_sizes,C", [DEFAULT, PENDULUM], ids=[IDS[0], IDS[1]])
def test_a_zero_std_history_column(gpu, n_cus, env, E, Hh, cp_sizes, C):
    """Column 1 has std 0 and sits on its mean (np.std of a constant column): the kernels divide by 1e-10 and get exactly 0.
    Measured on an MI355X: halfcheetah 1.8e-06 / 1.8e-06, pendulum 8.5e-07 / 7.1e-07 vs the float32 / float64 oracle (bar 1e-05)."""
    _check_inference(env, E, Hh, cp_sizes, C, n_cus, seed=6, zero_std_cols=(1,))


# ---------------------------------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("env,E,Hh,cp_sizes,C", [DEFAULT, ODD], ids=[IDS[0], IDS[6]])
def test_a_rows_bits_do_not_depend_on_its_company(gpu, n_cus, env, E, Hh, cp_sizes, C):
    """A batched row is an MFMA chain over k from the bias, the same in both flavours: the first 48 rows of the two-tile call equal
    the one-tile m = 48 call BIT FOR BIT; likewise 40 of 47 rows within the per-row kernel.  Across the two kernels (other summation
    order): 2e-6, test_context_across_the_kernel_dispatch_threshold's pin.  Measured on an MI355X: every bit-equality holds;
    per-row vs batched 1.5e-06 for (256, 128, 64), 8.4e-07 for (70, 50, 30)."""
    ms = _row_counts(E, n_cus)
    prob, cp_obs, cp_act = raw_history_problem(env, E, Hh, cp_sizes, C, ms[-1], seed=11)
    eng = make_engine(prob, p=E)
    call = lambda m: _np(eng.context_forward(cp_obs[:m], cp_act[:m]))
    a2, a65, a48, a47, a40 = call(ms[-1]), call(65), call(48), call(47), call(40)
    np.testing.assert_array_equal(a2[:, :48], a48, err_msg="two row tiles (m = %d) vs one (m = 48)" % ms[-1])
    np.testing.assert_array_equal(a65[:, :48], a48, err_msg="one row tile: m = 65 vs m = 48")
    np.testing.assert_array_equal(a47[:, :40], a40, err_msg="per-row kernel: m = 47 vs m = 40")
    np.testing.assert_array_equal(call(ms[-1]), a2)
    print("%s %r: per-row vs batched kernel on the same 47 rows: %.2e (bar 2e-06)" % (env, cp_sizes, floored_rel(a48[:, :47], a47)))
    assert_close(a48[:, :47], a47, 2e-6, "batched (m = 48) vs per-row (m = 47) kernel")
    assert_close(a2[:, :47], a47, 2e-6, "batched, two row tiles vs per-row (m = 47) kernel")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("Hh,cp_sizes", [(10, (256, 128, 64)), (3, (70, 50, 30))], ids=["Hh10-256x128x64", "Hh3-70x50x30"])
def test_planner_head_reads_the_same_statistics(gpu, Hh, cp_sizes):
    """`cem_plan_host` (plan_head_kernel: the encoder on the histories in the kernel-argument block) and `cem_plan` (context_kernel, then
    separate launches) return the same plan bit for bit under raw statistics, and the plan changes when cp_obs_mean is rolled by one
    column: the context reaches the plan.  tests/test_gpu_icem.py's rollout geometry: hidden (32,) * 4, m = 2, n = 64, H = 5, p = 5.
    Measured on an MI355X: both pairs bit-equal; the rolled mean moves 60 of 60 plan entries (Hh = 10) / 43 of 60 (Hh = 3), by up to 0.17."""
    m, H, n = 2, 5, 64
    prob, cp_obs, cp_act = raw_history_problem("halfcheetah", 5, Hh, cp_sizes, 10, m, seed=3, H=H, hidden_sizes=(32,) * 4)
    assert m * (18 + Hh * 24 + 2 * H * 6) <= 896 and m < 48          # csrc/planner.h CADM_HEAD_INGEST_MAX: the staged call takes the fused head
    eng = make_engine(prob, p=5, num_elites=8, num_cem_iters=3)
    f32 = lambda x: np.asarray(x, np.float32)
    arrays = (f32(prob["obs"]), f32(cp_obs), f32(cp_act), f32(prob["init_mean"]), f32(prob["init_var"]))
    head = eng.cem_plan_host(arrays, n, seed=3, call=9)
    sep = _np(eng.cem_plan(*arrays, n, seed=3, call=9))
    assert head.shape == (m, H, 6) and np.isfinite(head).all() and np.abs(head).max() <= 1.0
    np.testing.assert_array_equal(head, sep)
    eng.set_stats(rolled_stats(prob["stats"], "cp_obs_mean"))
    head2 = eng.cem_plan_host(arrays, n, seed=3, call=9)
    np.testing.assert_array_equal(head2, _np(eng.cem_plan(*arrays, n, seed=3, call=9)))
    assert np.isfinite(head2).all() and not np.array_equal(head, head2), "the plan ignores the history statistics"
    print("Hh=%d %r: rolling cp_obs_mean moves %d of %d plan entries, by up to %.6f" % (Hh, cp_sizes, (head2 != head).sum(), head.size, np.abs(head2 - head).max()))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------- d
TRAIN_CASES = [("halfcheetah", True, 3, 37), ("ant", False, 2, 50)]      # env, with_back, E, B (tests/test_gpu_train.py CASES 2 and 6)


@pytest.mark.parametrize("flavour", [8, 4, 4 + 16 + 64, 8 + 16 + 64])
@pytest.mark.parametrize("env,with_back,E,B", TRAIN_CASES)
def test_gradients_under_raw_statistics(gpu, env, with_back, E, B, flavour):
    """tests/test_gpu_train.py test_gradients_elementwise_vs_fp64_autograd with the batch's cp_obs at raw scale: the chain kernels'
    input assembly normalises the history itself, and the first encoder layer's dW is x^T dz.  Bars: helpers._check_gradients.
    Measured on an MI355X (worst tensor, of its max / pure relative): halfcheetah 5.5e-07 / 7.3e-06 (context_model/cp_hidden_2_weight), ant
    3.5e-07 / 3.1e-06 (ff_model/output_logvar_weight), the same in all four flavours to two digits (bars 1e-05 / 1e-04)."""
    prob, _, _ = raw_history_problem(env, E, 10, (256, 128, 64), 10, 1, seed=22, with_back=with_back)
    eng = _dev_engine(prob, E, deterministic=False)
    eng._check(eng.lib.cadm_dev_set_train_flavour(eng._ctx, flavour), "cadm_dev_set_train_flavour")
    bc = 0.5 if with_back else 0.0
    eng.train_configure(1e-3, WD, CWD, 1.0, bc, max_batch=B, beta1=0.0)
    batch = raw_train_batch(prob, B, seed=3)
    before = {n: {k: v.clone() for k, v in eng.nets[n].items()} for n in eng.net_names()}
    eng.train_step(_dev_batch(eng, batch, True, with_back), train=True)
    ff, back, cp, st = _oracle_nets(prob, torch.float64)
    tb = {k: torch.tensor(v, dtype=torch.float64) for k, v in batch.items()}
    out = otrain.train_losses(env, ff, back, cp, st, tb, _cfg(prob, False, bc))
    grads = otrain.grads_of(out["loss"], {"ff_model": ff, "backward_model": back, "context_model": cp})
    assert _check_gradients(eng, grads, "raw statistics, %s E=%d B=%d flavour %d" % (env, E, B, flavour)) >= 8
    for net in eng.net_names():
        for name, w0 in before[net].items():
            if grads[net][name] is None:
                assert torch.equal(w0, eng.nets[net][name]), "%s/%s moved although it has no gradient" % (net, name)
    eng.close()


@pytest.mark.parametrize("env,with_back,E,B", TRAIN_CASES)
def test_losses_under_raw_statistics(gpu, env, with_back, E, B):
    """The loss triple of an evaluation step against the float32 / float64 oracle at test_losses_match_oracle's 2e-5 / 5e-5.
    Measured on an MI355X: at most 0.4 % of the bar against either oracle, both cases."""
    prob, _, _ = raw_history_problem(env, E, 10, (256, 128, 64), 10, 1, seed=21, with_back=with_back)
    eng = make_engine(prob, p=E)
    bc = 0.5 if with_back else 0.0
    eng.train_configure(1e-3, WD, CWD, 1.0, bc, max_batch=B)
    batch = raw_train_batch(prob, B, seed=2)
    got = _np(eng.train_step(_dev_batch(eng, batch, True, with_back), train=False))
    for dt, tol in ((torch.float32, 2e-5), (torch.float64, 5e-5)):
        ff, back, cp, st = _oracle_nets(prob, dt, False)
        tb = {k: torch.tensor(v, dtype=dt) for k, v in batch.items()}
        ref = otrain.train_losses(env, ff, back, cp, st, tb, _cfg(prob, False, bc))
        want = np.array([float(ref["mse"]), float(ref["back_mse"]), float(ref["recon"])])
        print("%s losses vs %s oracle: worst |diff| / (tol (1 + |want|)) = %.3f (tol %.0e)" % (
            env, dt, (np.abs(got - want) / (tol * (1 + np.abs(want)))).max(), tol))
        np.testing.assert_allclose(got, want, rtol=tol, atol=tol, err_msg="losses vs %s oracle" % dt)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------- e
def test_evaluate_horizon_under_raw_statistics(gpu):
    """`cadm_eval_horizon` forces the batched encoder at any row count: N = 20 windows (fewer than 48) with raw statistics, the composite
    against the oracle trajectory's statistics within tests/horizon_ref.py's propagated bound (its stats64 / check_against_oracle).
    Measured on an MI355X: worst |diff| / bound 0.011 (se), 0.002 (spread), 0.014 (se_member)."""
    th = horizon_tests
    N = 20
    c = types.SimpleNamespace()
    prob, _, _ = raw_history_problem("halfcheetah", th.E, 10, (256, 128, 64), 10, N, seed=41, H=th.H_ENG, trained_like=False)      # (that file's model: the reference's initialiser)
    D, A = prob["D"], prob["A"]
    rng = np.random.default_rng(141)
    acts = rng.uniform(-1, 1, (N, 1, th.F, A)).astype(np.float32)
    eps = rng.standard_normal((th.F, N, 1, th.P_, D)).astype(np.float32)
    c.mask = make_mask(N, th.F)
    assert (c.mask[5] == 0).all() and tuple(c.mask[9]) == (1, 1, 0, 1)
    o = oracle_problem(prob, np.float32)
    T = oplanner.context_table_indexed(onets.context_forward(o["cp"], o["cp_obs"], o["cp_act"], o["st"]), 0)
    _, t_ref = oplanner.rollout_indexed(o["env"], o["ff"], o["st"], o["obs"], T, acts.copy(), eps.copy(), th.E, th.P_, False, return_traj=True)
    c.t_ref = t_ref.reshape(th.F, N, th.P_, D)
    scale = np.sqrt((c.t_ref.astype(np.float64) ** 2).mean(axis=(0, 1, 2)))
    c.truth = (rng.standard_normal((N, th.F, D)) * scale).astype(np.float32)
    obs = rng.standard_normal((N, th.F, D)).astype(np.float32)
    obs[:, 0] = prob["obs"].astype(np.float32)
    ds = dict(obs=obs.reshape(N, th.F * D), act=acts[:, 0].reshape(N, th.F * A).copy(), obs_next=c.truth.reshape(N, th.F * D),
              cp_obs=prob["cp_obs"], cp_act=prob["cp_act"], future_bool=c.mask)
    eng = make_engine(prob, p=th.P_)
    comp = th._np(eng.eval_horizon({k: eng._t(v) for k, v in ds.items()}, N, th.F, eps=eps.copy()))
    check_against_oracle(c, comp, "halfcheetah, raw statistics, 20 windows")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------- f
def _cadm_model(**over):
    kw = dict(name="dyn_model", env=make_env_spec("halfcheetah"), hidden_sizes=(200,) * 4, hidden_nonlinearity="swish", batch_size=64,
              normalize_input=True, n_forwards=8, n_candidates=64, ensemble_size=5, n_particles=10, use_cem=True, cp_hidden_sizes=(256, 128, 64),
              context_out_dim=10, history_length=10, future_length=10, state_diff=0, back_coeff=0.5)
    kw.update(over)
    return CaDMModel(**kw)


def _normalization(st):
    return {"obs": (st["obs_mean"], st["obs_std"]), "delta": (st["delta_mean"], st["delta_std"]), "act": (st["act_mean"], st["act_std"]),
            "cp_obs": (st["cp_obs_mean"], st["cp_obs_std"]), "cp_act": (st["cp_act_mean"], st["cp_act_std"]),
            "back_delta": (st["back_delta_mean"], st["back_delta_std"])}


def test_device_planner_state_with_raw_observation_history(gpu):
    """tests/test_gpu_model.py test_device_planner_state_matches_sampler_bookkeeping with state_diff = 0: the ring buffer stores the
    observation itself (csrc/caller.hip), the model normalises it with the installed cp_obs statistics (a zero-filled history at an
    episode start is -mean / std, not 0), and the plan from the device-resident history is the class API's on the reference's."""
    from cadm_amd.caller import DevicePlannerState
    from oracle.caller import SamplerState
    m, H = 3, 8
    st = raw_history_problem("halfcheetah", 5, 10, (256, 128, 64), 10, m, seed=8)[0]["stats"]
    model = _cadm_model(state_diff=0)
    model.set_normalization(_normalization(st))
    got = model.get_normalization_stats()
    np.testing.assert_array_equal(got[6], st["cp_obs_mean"])
    np.testing.assert_array_equal(got[7], st["cp_obs_std"])
    twin = _cadm_model(state_diff=1)
    twin.set_normalization(_normalization(st))
    np.testing.assert_array_equal(twin.get_normalization_stats()[6], np.zeros(180))
    np.testing.assert_array_equal(twin.get_normalization_stats()[7], np.ones(180))
    dev = DevicePlannerState(model, m)
    ref = SamplerState(m, H, 18, 6, 10, state_diff=0)
    rng = np.random.default_rng(0)
    obs = (st["cp_obs_mean"][:18] + rng.standard_normal((m, 18))).astype(np.float32)
    for step in range(14):
        np.testing.assert_array_equal(_np(dev.hist_obs), ref.history_state.astype(np.float32))
        np.testing.assert_array_equal(_np(dev.hist_act), ref.history_act.astype(np.float32))
        np.testing.assert_array_equal(_np(dev.prev_sol), ref.prev_sol.astype(np.float32))
        call_before = model._call
        plan_ref = model.get_action(obs, ref.history_state, ref.history_act, ref.prev_sol, ref.init_var)
        model._call = call_before
        act_dev = _np(dev.act(obs))
        act_ref = ref.after_plan(plan_ref)
        np.testing.assert_array_equal(act_dev, act_ref.astype(np.float32))
        nxt = (obs + 0.1 * rng.standard_normal((m, 18))).astype(np.float32)
        done = np.array([step == 5, False, step in (3, 11)])
        dev.observe(obs, act_dev, nxt, done)
        ref.after_step(obs, act_ref.astype(np.float32), nxt, done)
        if step == 0:      # raw observations, not differences
            np.testing.assert_array_equal(ref.history_state[:, :18].astype(np.float32), obs)
        obs = nxt
    np.testing.assert_array_equal(_np(dev.counts), np.array(ref.state_counts, dtype=np.int32))


# ---------------------------------------------------------------------------------------------------------------------- g
def test_fit_with_raw_observation_history(gpu):
    """tests/test_gpu_fit.py's fit-against-oracle run with state_diff = 0 on both sides and cp_obs windows at raw scale: `fit` computes the
    cp_obs statistics and installs them; same bars, including the 1e-12 agreement of the twelve statistic vectors.
    Measured on an MI355X: worst per-step loss error 2.8e-07 over 8 steps (bar 2e-03)."""
    data = fit_tests._windows(np.random.default_rng(2), 30)
    rng = np.random.default_rng(12)
    col = synth.norm_stats(rng, 18, 6, 18, 10, state_diff=False)
    data["cp_obs"] = 5.0 * col["cp_obs_mean"] + col["cp_obs_std"] * rng.standard_normal(data["cp_obs"].shape)
    fit_tests.check_fit_against_oracle(0.5, 0, data)
