"""GPU: user-declared envs at the corners of the kernels' envelope (include/cadm_hip.h CADM_SPEC_MAX_*: D <= 48, A <= 24, P <= 64,
32 reward terms), against the oracle.  The corners (tests/helpers.py CORNER_DECLS) reach what the shapes of test_gpu_env_spec.py do
not: pairs 16..23 sharing return slots with pairs 0..7, the ctrl cost and bonus on a shared slot, Philox counter groups 8..11, mask bits
32..47, a four-chunk layer 0 with and without context, a half-filled last pair that is sin / cos and replaced, no reward terms at all,
a first term on the next state -- and the widest spec's rollout modules, which spill registers (tests/test_env_spec.py prints where).

* rollouts (H = 1 with obs_rows, H = 30; stochastic and deterministic models) in every flavour at 1e-5, flavours bit-identical;
* device-drawn Gaussian-head noise against oracle/philox.eps_normals (every flavour, a candidate shard) and the action draws at A = 24;
* the planner at A = 24, H = 30, n = 64 (fused refit-and-sample) and n = 300: one-call plan == per-iteration orchestration bit for bit,
  the orchestration with injected draws against the oracle, random shooting;
* a training step and predict_heads on the widest spec with and without context; the class API on the widest spec."""
import numpy as np
import pytest

from cadm_amd import _lib, synth
from cadm_amd import planner as hplanner
from helpers import (FLAVOURS, _np, assert_close, check_class_api_on_spec, check_spec_training_step, close_but_jumps, corner_spec,
                     flavour, make_engine, run_flavour, spec_oracle, threshold_jump, trunc_z)
from oracle import nets as onets
from oracle import philox as ophilox
from oracle import planner as oplanner

pytestmark = pytest.mark.gpu

ROLLOUT_CASES = [  # corner, context, p, deterministic
    pytest.param("widest", True, 10, False, id="widest_D48_A24_P64_32terms"),
    pytest.param("widest", True, 5, True, id="widest_D48_A24_P64_32terms_deterministic"),
    pytest.param("widest", False, 10, False, id="widest_no_context_K0_88"),
    pytest.param("tiny", True, 5, False, id="tiny_D1_A1_P1_no_terms"),
    pytest.param("tiny_sincos", False, 5, True, id="tiny_D2_drop_sincos_deterministic"),
    pytest.param("odd_tail", True, 10, False, id="odd_tail_D47_sincos_replace_last_dim"),
    pytest.param("first_next", True, 5, True, id="first_term_on_next_obs_deterministic"),
]


@pytest.mark.parametrize("corner,context,p,det", ROLLOUT_CASES)
def test_corner_rollouts_match_oracle(gpu, corner, context, p, det):
    spec = corner_spec(corner)
    E, m, n = 5, 2, 9
    dev = _lib.load_dev()
    rng = np.random.default_rng(21)
    for H in (1, 30):
        prob = synth.make_problem(env=spec, context=context, E=E, m=m, H=H, trained_like=H == 1, seed=22)
        eng = make_engine(prob, p=p, H=H, deterministic=det, lib=dev)
        D, A = prob["D"], prob["A"]
        acts = rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32)
        eps = rng.standard_normal((H, m, n, p, D)).astype(np.float32)
        obs_rows = rng.standard_normal((m, n, p, D)).astype(np.float32) if H == 1 else None
        ctx = eng.context_forward(prob["cp_obs"], prob["cp_act"]) if context else None
        o = spec_oracle(prob, spec)
        T = oplanner.context_table_indexed(onets.context_forward(o["cp"], o["cp_obs"], o["cp_act"], o["st"]), 0) if context else None
        r_ref, t_ref = oplanner.rollout_indexed(spec, o["ff"], o["st"], o["obs"], T, acts, eps, E, p, det, obs_rows=obs_rows, return_traj=True)
        assert np.isfinite(r_ref).all() and np.isfinite(t_ref).all()
        kw = dict(obs_rows=obs_rows) if H == 1 else {}
        if not det:
            kw["eps"] = eps
        first = None
        for fl in FLAVOURS:
            rows, traj = run_flavour(eng, fl, prob["obs"], ctx, acts, **kw)
            assert_close(traj, t_ref, 1e-5, "%s H=%d next obs, flavour %s" % (corner, H, fl))
            assert_close(rows, r_ref, 1e-5, "%s H=%d returns, flavour %s" % (corner, H, fl))
            if first is None:
                first = (rows, traj)
            np.testing.assert_array_equal(rows, first[0], err_msg="returns, flavour %s vs %s" % (fl, FLAVOURS[0]))
            np.testing.assert_array_equal(traj, first[1], err_msg="next obs, flavour %s vs %s" % (fl, FLAVOURS[0]))
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------------
# device-drawn noise: Philox counter groups 0..11 (eps_group), both pairings of the wave-tile kernel's calls
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["widest", "odd_tail", "slim_humanoid"],
                         ids=["widest_D48_groups_0_11", "odd_tail_D47_group_11_half_pair", "slim_humanoid_D45_builtin"])
def test_device_noise_matches_oracle_streams(gpu, env):
    """Device-drawn Gaussian-head noise equals the oracle's stream layout: a rollout with seed / call / it against the same rollout
    given eps = oracle/philox.eps_normals, in every flavour, over all candidates and over a shard (the bar of
    test_gpu_planner.py::test_device_rng_matches_oracle_streams: Box-Muller transcendental ulps)."""
    prob = synth.make_problem(env=env if env == "slim_humanoid" else corner_spec(env), context=True, m=2, H=5, seed=1)
    p, n, D, A = 5, 33, prob["D"], prob["A"]
    eng = make_engine(prob, p=p, H=5, lib=_lib.load_dev())
    ctx = eng.context_forward(prob["cp_obs"], prob["cp_act"])
    a = np.random.default_rng(0).uniform(-1, 1, (2, n, 5, A))
    for lo, hi in ((0, n), (11, 22)):
        eps = ophilox.eps_normals(123, 7, 2, 2, n, p, 5, D, cand_lo=lo, cand_hi=hi)
        shard = dict(cand_offset=lo, n_local=hi - lo)
        for fl in FLAVOURS:
            r_dev, t_dev = run_flavour(eng, fl, prob["obs"], ctx, a, seed=123, call=7, it=2, **shard)
            r_inj, t_inj = run_flavour(eng, fl, prob["obs"], ctx, a, eps=eps, it=2, **shard)
            what = "%s flavour %s candidates [%d,%d)" % (env, fl, lo, hi)
            assert_close(t_dev, t_inj, 1e-4, "device eps vs injected oracle eps, next obs, " + what)
            assert_close(r_dev, r_inj, 1e-4, "device eps vs injected oracle eps, returns, " + what)
    eng.close()


def test_action_draws_match_oracle_at_A24(gpu):
    spec = corner_spec("widest")
    m, n, H, A = 2, 33, 30, 24
    prob = synth.make_problem(env=spec, m=m, H=H, seed=1)
    eng = make_engine(prob, p=5, H=H)
    mean = np.zeros((m, H, A), np.float32)
    var = np.ones((m, H, A), np.float32)   # constrained var = 0.25 -> actions = 0.5 z
    zref = ophilox.truncated_normals(123, 7, 3, m, n, H, A)
    acts = _np(eng.sample_actions(mean, var, n, seed=123, call=7, it=3))
    assert np.abs(acts / 0.5).max() < 2.0
    np.testing.assert_allclose(acts / 0.5, zref, rtol=0, atol=4e-6)
    part = _np(eng.sample_actions(mean, var, n, seed=123, call=7, it=3, cand_offset=11, n_local=11))
    np.testing.assert_allclose(part[:, 11:22] / 0.5, zref[:, 11:22], rtol=0, atol=4e-6)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the planner at A = 24, H = 30: refit over 720 plan elements, the fused refit-and-sample kernel at small n
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 300])
def test_widest_planner_matches_oracle(gpu, n):
    spec = corner_spec("widest")
    E, p, m, H = 5, 5, 2, 30
    prob = synth.make_problem(env=spec, context=True, E=E, m=m, H=H, seed=8)
    eng = make_engine(prob, p=p, lib=_lib.load_dev())
    D, A = prob["D"], prob["A"]
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], n)
    for fl in FLAVOURS:
        with flavour(eng, fl):
            one = _np(eng.cem_plan(*args, seed=4, call=2))
            loop = _np(hplanner.cem_plan(eng, *args, seed=4, call=2))
        np.testing.assert_array_equal(one, loop, err_msg="one-call CEM plan vs orchestration, flavour %s, n=%d" % (fl, n))
        assert one.shape == (m, H, A) and np.isfinite(one).all() and np.abs(one).max() <= 1.0
    rng = np.random.default_rng(12)
    z = trunc_z(rng, (5, m, n, H, A)).astype(np.float32)
    eps = rng.standard_normal((5, H, m, n, p, D)).astype(np.float32)
    o = spec_oracle(prob, spec)
    ref, rinfo, _ = oplanner.cem_plan(spec, o["ff"], o["cp"], o["st"], o["obs"], o["cp_obs"], o["cp_act"], o["init_mean"], o["init_var"],
                                      z, eps, E, p, deterministic=False, return_info=True)
    jump = threshold_jump(spec, H, p)
    for fl in FLAVOURS:
        with flavour(eng, fl):
            plan, info, _ = hplanner.cem_plan(eng, *args, z=eng._t(z), eps=eng._t(eps), return_info=True)
        for it in range(5):
            np.testing.assert_array_equal(np.sort(_np(info[it]["elites"]), axis=1), np.sort(rinfo[it]["elites"], axis=1),
                                          err_msg="elite set differs at CEM iteration %d, flavour %s, n=%d" % (it, fl, n))
            close_but_jumps(_np(info[it]["cand"])[0], rinfo[it]["cand_returns"], jump, "candidate returns it=%d flavour %s" % (it, fl))
        assert_close(_np(plan), oplanner.get_action_clip(ref), 1e-4, "final CEM plan, flavour %s, n=%d" % (fl, n))
    acts = rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32)
    first, cand = hplanner.rs_plan(eng, prob["obs"], prob["cp_obs"], prob["cp_act"], n, actions=acts, eps=eng._t(eps[0]))
    rfirst, rcand = oplanner.rs_plan(spec, o["ff"], o["cp"], o["st"], o["obs"], o["cp_obs"], o["cp_act"], acts, eps[0], E, p)
    close_but_jumps(_np(cand)[0], rcand, jump, "RS candidate returns, n=%d" % n)
    np.testing.assert_array_equal(_np(first), np.clip(rfirst, -1, 1))
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------------
# training: a 64-entry feature table, layer 0 of 98 (88 without context) inputs
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("context", [True, False], ids=["widest_context", "widest_no_context"])
def test_widest_training_step_matches_oracle(gpu, context):
    spec = corner_spec("widest")
    prob = synth.make_problem(env=spec, context=context, E=5, trained_like=True, with_back=True, seed=61)
    check_spec_training_step(spec, prob, 5, False, "widest context=%s" % context, predict=True)


def test_class_api_on_the_widest_spec(gpu, tmp_path):
    check_class_api_on_spec(corner_spec("widest"), tmp_path, epochs=2)
