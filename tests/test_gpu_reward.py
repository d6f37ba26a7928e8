"""GPU: the learned reward of the opt-in planner -- the kernels (`cadm_reward_eval` / `cadm_reward_returns`, csrc/reward.hip) against the
numpy restatement (tests/reward_ref.py), their independence of the batch and of the launcher's row-tile variant, the step sum and the
row update, non-finite inputs and the `first` cut, the fused loop (`cadm_rewarded_plan`) against the stepwise one, the no-ops, the
direction a reward pulls a plan in, the class route, a reward-free declared env and the refusals.

Geometries: the module-scoped engines of tests/test_gpu_tracking.py -- hopper_like (D = 11, A = 3, p = 5, H = 3), halfcheetah (D = 18,
A = 6, p = 20, H = 8 and p = 5, H = 5); synthetic trajectories from tests/behind_rollout.py; the class route on tests/helpers.py's
`plan_model`.

The kernel is held to the float64 restatement at the project's bar for fp32 kernels, `helpers.assert_close` at 1e-5 of the output's
scale.  Measured on an MI355X, worst |err| / (1e-5 x max(|ref|, rms)): relu 0.105, tanh 0.098, swish 0.227; 512 x 2: 0.138; with
statistics: 0.089."""
import ctypes as ct
import math
import os

import numpy as np
import pytest
import torch

import reward_ref as rref
import value_ref as vref
from behind_rollout import synth_traj
from cadm_amd import _lib, jit
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from cadm_amd.env_spec import EnvDecl
from helpers import _np, assert_close, floored_rel, make_engine, plan_act, plan_model, zero_carry
from test_gpu_tracking import engines      # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")
M, N, KE, ITERS = 2, 24, 8, 3
HIDDEN = [(), (48,), (64,), (200,), (64, 48, 200)]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _set(eng, inputs, hidden, act="relu", seed=0, weight=1.0, mean=None, std=None, out_scale=1.0):
    """register a He-initialised net on the engine: (reward_params, its layers)"""
    layers = rref.he_net(rref.input_dims(inputs, eng.D, eng.A), hidden, seed, out_scale)
    prm = HipEngine.reward_params(inputs, hidden, act, weight)
    eng.set_reward_net(prm, layers, in_mean=mean, in_std=std)
    return prm, layers


def _case(eng, m, n, seed):
    return synth_traj(seed, eng.H, m, n, eng.p, eng.D, eng.A)


def _cus(eng):
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


# ---------------------------------------------------------------------------------------------------------------------- 1: the kernel
@pytest.mark.parametrize("act", vref.ACTS)
def test_kernel_against_restatement(engines, act):
    """`cadm_reward_returns`' step_out on hopper_like against the float64 restatement at 1e-5 of scale, for every `inputs` (K = 11, 14
    and 25: none a multiple of 4) and L in {0, 1, 3} with widths 48, 64, 200 and (64, 48, 200): at (m, n) = (3, 11) a step has 165 rows,
    no multiple of 16, so tiles straddle steps, envs and candidates; at (3, 1) a step has fewer rows than one tile.  `cadm_reward_eval`
    on the concatenated inputs gives step_out's bits; the sum and the rows are the restatement's from those bits."""
    _, eng = engines("hopper")
    worst = 0.0
    for ii, inputs in enumerate(rref.INPUTS):
        for gi, hidden in enumerate(HIDDEN):
            prm, layers = _set(eng, inputs, hidden, act, seed=10 + gi, weight=0.5)
            for m, n in ((3, 11), (3, 1)):
                traj, obs, actions = _case(eng, m, n, 30 + gi + 7 * ii)
                rows = np.random.default_rng(gi).standard_normal((m, n, eng.p)).astype(F)
                what = "%s %s %r m=%d n=%d" % (act, inputs, hidden, m, n)
                worst = max(worst, check_kernel_case(eng, prm, layers, act, inputs, traj, obs, actions, rows, 0.5, what)[0])
    print("\n[%s] worst |err| / (1e-5 of scale): %.3f" % (act, worst))


def check_kernel_case(eng, prm, layers, act, inputs, traj, obs, actions, rows, weight, what, mean=None, std=None):
    """`cadm_reward_returns`' step_out against the float64 restatement at 1e-5 of scale; `cadm_reward_eval` on the concatenated inputs
    gives step_out's bits; the sum and the rows are the restatement's from those bits.  Returns (|err| / (1e-5 of scale), step_out,
    the restatement's step rewards)."""
    m, n = traj.shape[1:3]
    x = rref.gather_inputs(traj, obs, actions, inputs)
    ref = rref.reward64(x, layers, act, mean, std)
    out, steps, S = (_np(t) for t in eng.reward_returns(traj, obs, actions, rows, prm, want_steps=True))
    assert steps.shape == (eng.H, m, n, eng.p) and np.isfinite(steps).all(), what
    ratio = floored_rel(steps, ref) / 1e-5
    assert_close(steps, ref, what=what)
    np.testing.assert_array_equal(_bits(_np(eng.reward_eval(x))), _bits(steps), err_msg=what + ": cadm_reward_eval against step_out")
    np.testing.assert_array_equal(_bits(S), _bits(rref.step_sum(steps)), err_msg=what)
    np.testing.assert_array_equal(_bits(out), _bits(rref.update(rows, S, weight)), err_msg=what)
    return ratio, steps, ref


def test_kernel_at_the_widest_net(engines):
    """512 x 2: two activation regions of 16 x 512 floats are 64 KiB, with the per-row words beyond what a kernel gets without raising
    its dynamic-LDS attribute; on halfcheetah (D = 18, A = 6, p = 20, H = 8) at (2, 3): 960 rows, K = 42."""
    _, eng = engines("hc8")
    prm, layers = _set(eng, "obs_act_next_obs", (512, 512), "relu", seed=3)
    traj, obs, actions = _case(eng, 2, 3, 5)
    ref = rref.reward64(rref.gather_inputs(traj, obs, actions, "obs_act_next_obs"), layers, "relu")
    _, steps, _ = eng.reward_returns(traj, obs, actions, np.zeros((2, 3, eng.p), F), prm, want_steps=True)
    print("\n[512 x 2] worst |err| / (1e-5 of scale): %.3f" % (floored_rel(_np(steps), ref) / 1e-5))
    assert_close(_np(steps), ref, what="512 x 2")


def test_kernel_with_statistics(engines):
    """in_mean / in_std that are not 0 / 1, over the concatenated input: the input is (x - mean) * float32(1 / std)."""
    _, eng = engines("hc5")
    rng = np.random.default_rng(8)
    K = rref.input_dims("obs_act_next_obs", eng.D, eng.A)
    mean, std = rng.standard_normal(K).astype(F), rng.uniform(0.3, 4.0, K).astype(F)
    prm, layers = _set(eng, "obs_act_next_obs", (200, 200), "tanh", seed=4, mean=mean, std=std)
    traj, obs, actions = _case(eng, 3, 7, 6)
    x = rref.gather_inputs(traj, obs, actions, "obs_act_next_obs")
    ref = rref.reward64(x, layers, "tanh", mean, std)
    _, steps, _ = eng.reward_returns(traj, obs, actions, np.zeros((3, 7, eng.p), F), prm, want_steps=True)
    print("\n[statistics] worst |err| / (1e-5 of scale): %.3f" % (floored_rel(_np(steps), ref) / 1e-5))
    assert_close(_np(steps), ref, what="with statistics")
    assert floored_rel(_np(steps), rref.reward64(x, layers, "tanh")) > 1e-3, "the statistics must matter"


# ---------------------------------------------------------------------------------------------------------------------- 2: batch independence
BATCH = [("obs_act_next_obs", (64, 48, 200), "swish"), ("obs_act", (128, 128), "relu"), ("obs_act", (192, 100), "tanh"),
         ("obs_act_next_obs", (256, 64), "relu"), ("next_obs", (), "relu")]


@pytest.mark.parametrize("inputs,hidden,act", BATCH, ids=["%s-%s" % (i, "x".join(map(str, h)) or "linear") for i, h, _ in BATCH])
def test_a_step_has_the_same_bits_in_any_batch(engines, inputs, hidden, act):
    """The same (t, q) inputs through `reward_eval` at R = 1, 5, 16, at other row positions, through `reward_returns`' step_out, run to
    run, and inside a batch large enough for the launcher's other row-tile variant -- more than 2 sixteen-row tiles per CU (the CU count
    is the device's): two row tiles, for the nets whose tiles then still fit a CU four times; (256, 64) does not and stays at one, the
    others switch -- where the small batch's candidates recur at other row positions: equal bits.  The nets take every path of a
    layer's work split: 1, 2, 3 and 4 groups of 64 units."""
    _, eng = engines("hopper")
    H, p = eng.H, eng.p
    prm, _ = _set(eng, inputs, hidden, act, seed=21)
    m, n = 3, 11
    traj, obs, actions = _case(eng, m, n, 41)
    x = rref.gather_inputs(traj, obs, actions, inputs)
    flat = x.reshape(-1, x.shape[-1])
    full = _np(eng.reward_eval(flat))
    assert full.shape == (H * 165,)
    np.testing.assert_array_equal(_bits(_np(eng.reward_eval(flat))), _bits(full), err_msg="run to run")
    for R in (1, 5, 16):
        np.testing.assert_array_equal(_bits(_np(eng.reward_eval(flat[:R]))), _bits(full[:R]), err_msg="R = %d" % R)
    np.testing.assert_array_equal(_bits(_np(eng.reward_eval(np.roll(flat, 7, axis=0)))), _bits(np.roll(full, 7)), err_msg="rows moved by 7")
    rows = np.zeros((m, n, p), F)
    _, steps, _ = eng.reward_returns(traj, obs, actions, rows, prm, want_steps=True)
    np.testing.assert_array_equal(_bits(_np(steps)).reshape(-1), _bits(full), err_msg="reward_returns' step_out")
    _, again, _ = eng.reward_returns(traj, obs, actions, rows, prm, want_steps=True)
    np.testing.assert_array_equal(_bits(_np(again)), _bits(_np(steps)), err_msg="reward_returns run to run")
    cus = _cus(eng)
    for tiles_per_cu, name in ((2, "the large batch"),):
        reps = (tiles_per_cu * cus * 16) // (H * m * n * p) + 2
        assert H * m * n * reps * p > tiles_per_cu * cus * 16 + 16
        big = eng.reward_returns(np.tile(traj, (1, 1, reps, 1, 1)), obs, np.tile(actions, (1, reps, 1, 1)), np.zeros((m, n * reps, p), F), prm,
                                 want_steps=True)[1]
        big = _np(big).reshape(H, m, reps, n, p)
        for r in (0, 1, reps - 1):
            np.testing.assert_array_equal(_bits(big[:, :, r]), _bits(_np(steps)), err_msg="%s, copy %d of the candidates" % (name, r))
        ev = _np(eng.reward_eval(np.concatenate([flat[3:]] + [flat] * ((tiles_per_cu * cus * 16) // flat.shape[0] + 2), axis=0)))
        assert ev.shape[0] > tiles_per_cu * cus * 16 + 16
        np.testing.assert_array_equal(_bits(ev[:flat.shape[0] - 3]), _bits(full[3:]), err_msg=name + ": reward_eval, head")
        np.testing.assert_array_equal(_bits(ev[-flat.shape[0]:]), _bits(full), err_msg=name + ": reward_eval, tail")


# ---------------------------------------------------------------------------------------------------------------------- 3: the step sum, the row update
@pytest.mark.parametrize("weight", [1.0, -0.37, 0.0])
def test_step_sum_and_row_update(engines, weight):
    """S and rows_out from the kernel's own step_out, bit for bit: plain float32 adds in ascending t, then float32(rows_in +
    float32(weight * S)); rows_out aliasing rows_in and step_out / sum_out = NULL give the same rows_out; rows_in is not written
    otherwise."""
    _, eng = engines("hc5")
    prm, _ = _set(eng, "obs_act", (64, 64), "swish", seed=5, weight=weight)
    traj, obs, actions = _case(eng, 3, 7, 9)
    rows = (10.0 * np.random.default_rng(2).standard_normal((3, 7, eng.p))).astype(F)
    t_dev, o_dev, a_dev, r_dev = (eng._t(v) for v in (traj, obs, actions, rows))
    out, steps, S = eng.reward_returns(t_dev, o_dev, a_dev, r_dev, prm, want_steps=True)
    np.testing.assert_array_equal(_bits(_np(r_dev)), _bits(rows), err_msg="rows_in was written")
    np.testing.assert_array_equal(_bits(_np(S)), _bits(rref.step_sum(_np(steps))))
    np.testing.assert_array_equal(_bits(_np(out)), _bits(rref.update(rows, _np(S), weight)))
    np.testing.assert_array_equal(_bits(_np(eng.reward_returns(t_dev, o_dev, a_dev, r_dev, prm))), _bits(_np(out)), err_msg="step_out = sum_out = NULL")
    np.testing.assert_array_equal(_bits(_np(r_dev)), _bits(rows), err_msg="rows_in was written")
    alias = r_dev.clone()
    assert eng.reward_returns(t_dev, o_dev, a_dev, alias, prm, out=alias) is alias
    np.testing.assert_array_equal(_bits(_np(alias)), _bits(_np(out)), err_msg="rows_out aliasing rows_in")
    assert weight == 0.0 or not np.array_equal(_bits(_np(out)), _bits(rows))
    if weight == 0.0:
        np.testing.assert_array_equal(_np(out), rows)


# ---------------------------------------------------------------------------------------------------------------------- 4: non-finite inputs, the first cut
@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_non_finite_inputs_and_the_first_cut(engines, act):
    """NaN and +-inf planted in traj at chosen (t, q), in obs of one env and in one action make exactly the steps that read them NaN --
    under relu too --, and exactly the rows that count such a step; no other step's bits move.  With `first` mixing 0, mid-horizon,
    H - 1 and H the steps beyond it read NaN in step_out and are not summed, and NaN planted only in steps that are not counted changes
    no row."""
    _, eng = engines("hopper")
    H, p, D, A = eng.H, eng.p, eng.D, eng.A
    inputs = "obs_act_next_obs"
    prm, _ = _set(eng, inputs, (48, 48), act, seed=6, weight=2.0)
    m, n = 3, 11
    traj, obs, actions = _case(eng, m, n, 12)
    rows = np.random.default_rng(4).standard_normal((m, n, p)).astype(F)
    ref_out, ref_steps, ref_S = (_np(t) for t in eng.reward_returns(traj, obs, actions, rows, prm, want_steps=True))
    assert np.isfinite(ref_steps).all()
    bad_t, bad_o, bad_a = traj.copy(), obs.copy(), actions.copy()
    hit = np.zeros((H, m, n, p), bool)                 # the steps whose input holds a planted value
    bad_t[0, 0, 0, 0, 3] = np.nan                      # s_1 of the first row: s_{t+1} of step 0, s_t of step 1
    hit[0, 0, 0, 0] = hit[1, 0, 0, 0] = True
    bad_t[H - 1, 2, n - 1, p - 1, D - 1] = -np.inf     # s_H of the last row: step H - 1 alone
    hit[H - 1, 2, n - 1, p - 1] = True
    bad_t[1, 1, 4, 2, 0] = np.inf                      # s_2: steps 1 and 2
    hit[1, 1, 4, 2] = hit[2, 1, 4, 2] = True
    bad_o[1, 5] = np.nan                               # obs of env 1: step 0 of every row of env 1
    hit[0, 1] = True
    bad_a[2, 3, 1, A - 1] = np.inf                     # a_1 of candidate (2, 3): step 1 of its p particles
    hit[1, 2, 3] = True
    out, steps, S = (_np(t) for t in eng.reward_returns(bad_t, bad_o, bad_a, rows, prm, want_steps=True))
    assert np.isnan(steps[hit]).all()
    np.testing.assert_array_equal(_bits(steps[~hit]), _bits(ref_steps[~hit]), err_msg="a step met its neighbour's poison")
    dead = hit.any(axis=0)
    assert dead.any() and (~dead).any() and np.isnan(S[dead]).all() and np.isnan(out[dead]).all()
    np.testing.assert_array_equal(_bits(S[~dead]), _bits(ref_S[~dead]))
    np.testing.assert_array_equal(_bits(out[~dead]), _bits(ref_out[~dead]))
    # the first cut: on the clean inputs, then with NaN only where nothing counts
    rng = np.random.default_rng(13)
    first = rng.integers(0, H + 1, (m, n, p)).astype(np.int32)
    first[0, 0, 0], first[0, 0, 1], first[0, 0, 2], first[0, 0, 3] = 0, H, H - 1, 1
    live = rref.counted(H, (m, n, p), first)
    out, steps, S = (_np(t) for t in eng.reward_returns(traj, obs, actions, rows, prm, first=first, want_steps=True))
    assert np.isnan(steps[~live]).all() and (~live).any()
    np.testing.assert_array_equal(_bits(steps[live]), _bits(ref_steps[live]))
    np.testing.assert_array_equal(_bits(S), _bits(rref.step_sum(ref_steps, first)))
    np.testing.assert_array_equal(_bits(out), _bits(rref.update(rows, rref.step_sum(ref_steps, first), 2.0)))
    only = traj.copy()
    only[~live] = np.nan                               # s_{t+1} of every step that is not counted: no counted step reads it
    out2, steps2, S2 = (_np(t) for t in eng.reward_returns(only, obs, actions, rows, prm, first=first, want_steps=True))
    assert np.isnan(only).any()
    np.testing.assert_array_equal(_bits(out2), _bits(out), err_msg="NaN in steps that are not counted reached a row")
    np.testing.assert_array_equal(_bits(S2), _bits(S))
    np.testing.assert_array_equal(_bits(steps2), _bits(steps))


# ---------------------------------------------------------------------------------------------------------------------- 5: fused against stepwise
def _check_iterations(eng, info, prob, prm, inputs, first_used):
    """every stepwise iteration: rows == the row update of reward_rows from the iteration's own step rewards, which are `reward_eval`'s
    of the inputs gathered from the iteration's own trajectories and candidates"""
    for x in info:
        steps, S, before, rows = (_np(x[k]) for k in ("reward_steps", "reward_sum", "reward_rows", "rows" if "value_rows" not in x else "value_rows"))
        first = _np(x["first_violation"]) if first_used else None
        np.testing.assert_array_equal(_bits(S), _bits(rref.step_sum(steps, first)))
        np.testing.assert_array_equal(_bits(rows), _bits(rref.update(before, S, prm.weight)))
        flat = _np(eng.reward_eval(rref.gather_inputs(_np(x["traj"]), _np(eng._t(prob["obs"])), _np(x["actions"]), inputs)))
        keep = rref.counted(eng.H, S.shape, first)
        np.testing.assert_array_equal(_bits(steps[keep]), _bits(flat[keep]))
        assert np.isnan(steps[~keep]).all()


COMBOS = ["alone", "terminate-tracking", "value-cvar", "actuator-uncertainty-mppi-knots"]


@pytest.mark.parametrize("combo", COMBOS)
def test_fused_equals_stepwise(engines, combo):
    """`cadm_rewarded_plan` with device RNG == the same loop one launch at a time (`planner.icem_plan(..., reward=...)`), bit for bit
    over two consecutive calls: the plan, the best return, the carry (and the actuator state); in every stepwise iteration the rows are
    the row update of the rows before it from the kernel's own step rewards.  Under decay the packed candidate count changes per
    iteration."""
    from test_gpu_actuator import _params, _state
    from test_gpu_constraints import binding_bounds, iteration0_traj
    from test_gpu_tracking import _tracking_inputs
    from test_gpu_uncertainty import _prm as unc_prm
    prob, eng = engines("hc5-vanilla" if combo == "alone" else "hc5")
    H, A = eng.H, eng.A
    inputs = {"alone": "obs_act_next_obs", "terminate-tracking": "obs_act", "value-cvar": "next_obs"}.get(combo, "obs_act_next_obs")
    reward, _ = _set(eng, inputs, (64, 48), "tanh", seed=31, weight=1.5)
    mppi = combo == "actuator-uncertainty-mppi-knots"
    K = 0 if combo == "alone" else 2
    icem = dict(noise_beta=1.0 if mppi else 0.0, keep_elites=K, decay=1.25 if K else 1.0, return_best=combo == "terminate-tracking",
                add_mean_last=K > 0)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if mppi else HipEngine.icem_params(**icem)
    score = HipEngine.score_params("cvar", k=2) if combo == "value-cvar" else None
    cons = track = targets = offset = act = unc = value = knots = None
    if combo == "terminate-tracking":
        track, targets, offset, _ = _tracking_inputs(eng, prob, 3, H, 13)
        cons = HipEngine.constraint_params(binding_bounds(iteration0_traj(eng, prob, 0.0, 4, 1), (1, 7), H, "rewarded"), "terminate", 4.0)
    if combo == "value-cvar":
        value = HipEngine.value_params((32,), "relu", 2.0)
        eng.set_value_net(value, vref.he_net(eng.D, (32,), 33))
    (pa, fa), (pb, fb) = (None, None), (None, None)
    if mppi:
        act, unc, knots = _params(eng, 1, 0.4, 2.0), unc_prm(eng, "epistemic", 0.3), HipEngine.knot_params(2, "linear")
        (pa, fa), (pb, fb) = _state(eng, 1, 8), _state(eng, 1, 8)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    (ca, va), (cb, vb) = zero_carry(eng, M, K, H), zero_carry(eng, M, K, H)
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2):
        a, ra = eng.rewarded_plan(reward, value, unc, act, pa, fa, True, track, targets, offset, knots, None, cons, score, prm, *args, mean, var,
                                  N, carry=ca, carry_valid=va, seed=4, call=call, want_best_return=True)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                            update="mppi" if mppi else "cem", temperature=0.5, relative=True, score=score, constraints=cons,
                                            knots=knots, tracking=None if track is None else (track, targets, offset),
                                            actuator=None if act is None else (act, pb, fb), action_advance=True, uncertainty=unc,
                                            value=value, reward=reward, **icem)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        for x, y in ((ca, cb), (pa, pb), (fa, fb)):
            if x is not None:
                np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))
        _check_iterations(eng, info, prob, reward, inputs, cons is not None)
        if K:
            assert len({int(x["rows"].shape[1]) for x in info}) > 1, "decay must change the packed candidate count"
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)
    if cons is not None:
        share = float((_np(info[0]["first_violation"]) < H).mean())
        assert 0.1 <= share <= 0.9, "%.2f of the rows are cut" % share
    # the term matters: without it, another plan
    other = _np(eng.rewarded_plan(None, value, unc, act, pb, fb, False, track, targets, offset, knots, None, cons, score, prm, *args, mean, var, N,
                                  *zero_carry(eng, M, K, H), seed=4, call=2))
    assert not np.array_equal(_bits(other), _bits(a))
    assert (mppi, "rew", cons is not None, act is not None, unc is not None) in eng._loop_ws


# ---------------------------------------------------------------------------------------------------------------------- 6: the no-ops
@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_no_reward_is_the_loop_underneath(engines, update):
    """reward = NULL: the plan, the best return and the carry of `cadm_valued_plan` on the same inputs (here with a value net), bit for
    bit, through the C entry itself with that loop's workspace; and the workspace with a reward is the valued loop's plus the step
    rewards [H, m, n, p]."""
    prob, eng = engines("hc5")
    H, A = eng.H, eng.A
    value = HipEngine.value_params((32,), "relu", 2.0)
    eng.set_value_net(value, vref.he_net(eng.D, (32,), 33))
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    mppi, full = eng._as_mppi_params(prm)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    carry, valid = zero_carry(eng, M, 2, H)
    plan, best = eng.valued_plan(value, None, None, None, None, True, None, None, None, None, None, None, None, prm, *args, carry=carry,
                                 carry_valid=valid, seed=5, call=2, want_best_return=True)
    carry2, valid2 = zero_carry(eng, M, 2, H)
    t = [eng._t(x) for x in args[:5]]
    ws = eng._loop_workspace(mppi, M, N, 2, val=(False, False, False))
    out = torch.empty((M, H, A), dtype=torch.float32, device=eng.device)
    best2 = torch.empty((M,), dtype=torch.float32, device=eng.device)
    P = lambda x: ct.c_void_p(x.data_ptr())
    rc = eng.lib.cadm_rewarded_plan(eng._ctx, None, ct.byref(value), None, None, None, None, 1, None, None, 0, None, None, None, None, None,
                                    int(mppi), ct.byref(full), *[P(x) for x in t], P(carry2), P(valid2), M, N, 5, 2, P(ws), P(out), P(best2),
                                    eng.stream)
    assert rc == 0, eng.lib.cadm_last_error().decode()
    for x, y in ((plan, out), (best, best2), (carry, carry2)):
        np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))
    lib = eng.lib
    for terminate in (0, 1):
        for act in (0, 1):
            for unc in (0, 1):
                assert lib.cadm_rewarded_workspace_bytes(eng._ctx, M, N, 2, int(mppi), terminate, act, unc) >= \
                    lib.cadm_valued_workspace_bytes(eng._ctx, M, N, 2, int(mppi), terminate, act, unc) + 4 * H * M * N * eng.p
    assert lib.cadm_reward_workspace_bytes(eng._ctx, M, N) == 4 * H * M * N * eng.p
    assert lib.cadm_rewarded_workspace_bytes(eng._ctx, 0, N, 2, 0, 0, 0, 0) == 0


@pytest.mark.parametrize("how", ["zero-output-layer", "zero-weight"])
def test_a_zero_reward_changes_no_plan(engines, how):
    """A net whose output layer is all zeros has R = +0.0 and S = +0.0; weight = 0 multiplies a finite S to +-0.0: every row keeps its
    value (x + 0.0 == x), so the elite sets of every iteration, the plan and the carry are those of the loop without the term."""
    prob, eng = engines("hc5")
    inputs = "obs_act_next_obs"
    layers = rref.he_net(rref.input_dims(inputs, eng.D, eng.A), (64, 64), 7)
    if how == "zero-output-layer":
        layers[-1] = (np.zeros_like(layers[-1][0]), np.zeros_like(layers[-1][1]))
    reward = HipEngine.reward_params(inputs, (64, 64), "relu", 5.0 if how == "zero-output-layer" else 0.0)
    eng.set_reward_net(reward, layers)
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.0, return_best=False, add_mean_last=True)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    (ca, va), (cb, vb) = zero_carry(eng, M, 2, eng.H), zero_carry(eng, M, 2, eng.H)
    a, ia, _ = hplanner.icem_plan(eng, *args, carry=ca, carry_valid=va, seed=3, call=1, return_info=True, reward=reward, **icem)
    b, ib, _ = hplanner.icem_plan(eng, *args, carry=cb, carry_valid=vb, seed=3, call=1, return_info=True, **icem)
    for x, y in zip(ia, ib):
        assert how == "zero-weight" or (_np(x["reward_sum"]) == 0).all()
        assert np.isfinite(_np(x["reward_sum"])).all()
        np.testing.assert_array_equal(_np(x["elites"]), _np(y["elites"]))
        assert (_np(x["rows"]) == _np(y["rows"])).all()
    np.testing.assert_array_equal(_bits(_np(a)), _bits(_np(b)))
    np.testing.assert_array_equal(_bits(_np(ca)), _bits(_np(cb)))
    fused = eng.rewarded_plan(reward, None, None, None, None, None, True, None, None, None, None, None, None, None, HipEngine.icem_params(**icem),
                              *args, *zero_carry(eng, M, 2, eng.H), seed=3, call=1)
    np.testing.assert_array_equal(_bits(_np(fused)), _bits(_np(b)))


# ---------------------------------------------------------------------------------------------------------------------- 7: the direction
def test_a_linear_reward_on_the_action_pulls_the_plan(engines):
    """A linear net (L = 0) on "obs_act" with R = +c a[0] gives a plan whose first-step a[0] exceeds that of R = -c a[0], in every env of
    the batch; c = 100 per step is far above the scale of the synthetic halfcheetah's own reward.  Cannot pass without the term."""
    prob, eng = engines("hc5")
    c, plans = 100.0, {}
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    for name, sign in (("up", 1.0), ("down", -1.0)):
        W = np.zeros((eng.D + eng.A, 1), F)
        W[eng.D, 0] = sign * c
        reward = HipEngine.reward_params("obs_act", (), "relu", 1.0)
        eng.set_reward_net(reward, [(W, np.zeros((1,), F))])
        plans[name] = _np(eng.rewarded_plan(reward, None, None, None, None, None, True, None, None, None, None, None, None, None,
                                            HipEngine.icem_params(), *args, seed=6, call=1))
        assert np.isfinite(plans[name]).all()
    print("\n[direction] first-step a[0]: down %s  up %s" % (plans["down"][:, 0, 0], plans["up"][:, 0, 0]))
    assert (plans["up"][:, 0, 0] > plans["down"][:, 0, 0]).all()


# ---------------------------------------------------------------------------------------------------------------------- 8: the class route
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_class_route(gpu, context):
    """`get_action` with a Sequential-set net agrees with the engine call and with the list form of the same net; `reward_net` and
    `plan_rewards` with the restatement; no net raises RuntimeError; a replaced net takes effect on the next call and builds nothing."""
    H, A, D = 5, 6, 18
    hidden, act, inputs = (64, 32), "swish", "obs_act_next_obs"
    K = rref.input_dims(inputs, D, A)
    rn = dict(inputs=inputs, hidden_sizes=hidden, activation=act, weight=0.8)
    model, prob = plan_model(context, H, cem_reward_net=rn, cem_keep_elites=2)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    rng = np.random.default_rng(5)
    so, sa, sn = ((2.0 * rng.standard_normal((4, 7, d))).astype(F) for d in (D, A, D))
    with pytest.raises(RuntimeError, match="no reward net"):
        plan_act(model, prob, context, mean, var)
    with pytest.raises(RuntimeError, match="no reward net"):
        model.reward_net(so, sa, sn)
    assert model._call == 0
    stats = (rng.standard_normal(K).astype(F), rng.uniform(0.5, 2.0, K).astype(F))
    layers = rref.he_net(K, hidden, 17)
    model.set_reward_net(vref.sequential(layers, act), *stats)
    plan = plan_act(model, prob, context, mean, var)
    assert np.isfinite(plan).all() and model._call == 1
    eng, opt = model.engine, model._opt
    hist = (prob["cp_obs"], prob["cp_act"]) if context else (None, None)
    carry, valid = zero_carry(eng, M, 2, H)
    direct = eng.rewarded_plan(opt.reward_params, None, None, None, None, None, True, None, None, None, None, None, None, None, opt.params,
                               prob["obs"], *hist, mean, var, model.n_candidates, carry=carry, carry_valid=valid, seed=model.seed, call=1)
    np.testing.assert_array_equal(_bits(plan), _bits(_np(direct)))
    np.testing.assert_array_equal(_bits(_np(model._plan_carry)), _bits(_np(carry)))
    twin, _ = plan_model(context, H, cem_reward_net=rn, cem_keep_elites=2)
    twin.set_reward_net(layers, *stats)                          # the list form of the same net
    np.testing.assert_array_equal(_bits(plan_act(twin, prob, context, mean, var)), _bits(plan))
    # R through the class, against the restatement
    r = model.reward_net(so, sa, sn)
    assert r.shape == (4, 7)
    assert_close(r, rref.reward64(np.concatenate([so, sa, sn], axis=-1), layers, act, *stats), what="reward_net")
    with pytest.raises(ValueError, match="need act"):
        model.reward_net(so, None, sn)
    res = model.plan_rewards(prob["obs"], plan, *(hist if context else ()))
    assert res["reward"].shape == (M, 5, H) and res["total"].shape == (M, 5) and res["first"] is None and model._call == 1
    many = model.plan_rewards(prob["obs"], np.repeat(plan[:, None], 3, axis=1), *(hist if context else ()))
    assert many["reward"].shape == (M, 3, 5, H) and np.isfinite(many["reward"]).all()
    np.testing.assert_array_equal(_bits(many["reward"][0, 0]), _bits(res["reward"][0]))      # (the noise is drawn per row: env 0's rows are where they were)
    np.testing.assert_array_equal(_bits(res["total"]), _bits(rref.step_sum(np.moveaxis(res["reward"], -1, 0)[:, :, None])[:, 0]))
    # ... and against the restatement on the trajectories the same rollout records
    ctx_vec = eng.context_forward(*hist) if context else None
    acts = eng._t(plan)[:, None].contiguous()
    _, traj = eng.rollout_returns(eng._t(prob["obs"]), ctx_vec, acts, seed=model.seed, call=1, it=hplanner.FORECAST_IT, want_traj=True)
    x = rref.gather_inputs(_np(traj), np.asarray(prob["obs"], F), _np(acts), inputs)
    assert_close(np.moveaxis(res["reward"], -1, 0), rref.reward64(x, layers, act, *stats)[:, :, 0], what="plan_rewards")
    # a replaced net: the next call plans with it, and nothing is built
    before = sorted((f, os.path.getmtime(os.path.join(jit.cache_dir(), f))) for f in os.listdir(jit.cache_dir()))
    ws = dict(eng._loop_ws)
    other = rref.he_net(K, hidden, 18, out_scale=30.0)
    model.set_reward_net(other, *stats)
    assert_close(model.reward_net(so, sa, sn), rref.reward64(np.concatenate([so, sa, sn], axis=-1), other, act, *stats), what="the replaced net")
    plan2 = plan_act(model, prob, context, mean, var)      # call 2, from call 1's carry: what `carry` / `valid` hold since the direct call above
    direct2 = eng.rewarded_plan(opt.reward_params, None, None, None, None, None, True, None, None, None, None, None, None, None, opt.params,
                                prob["obs"], *hist, mean, var, model.n_candidates, carry=carry, carry_valid=valid, seed=model.seed, call=2)
    np.testing.assert_array_equal(_bits(plan2), _bits(_np(direct2)))
    assert not np.array_equal(_bits(plan2), _bits(plan))
    assert sorted((f, os.path.getmtime(os.path.join(jit.cache_dir(), f))) for f in os.listdir(jit.cache_dir())) == before
    assert all(eng._loop_ws[k][1] is ws[k][1] for k in ws)
    # fit-free housekeeping leaves the net alone; clearing it brings the RuntimeError back
    model.reset_plan_carry()
    assert_close(model.reward_net(so, sa, sn), rref.reward64(np.concatenate([so, sa, sn], axis=-1), other, act, *stats), what="after reset_plan_carry")
    model.clear_reward_net()
    with pytest.raises(RuntimeError, match="no reward net"):
        plan_act(model, prob, context, mean, var)
    plain, _ = plan_model(context, H, cem_noise_beta=1.0)
    for fn in (lambda: plain.set_reward_net(layers), lambda: plain.reward_net(so, sa, sn), lambda: plain.clear_reward_net()):
        with pytest.raises(ValueError, match="no cem_reward_net"):
            fn()


# ---------------------------------------------------------------------------------------------------------------------- 9: a reward-free env
def test_a_reward_free_declared_env(gpu):
    """An env declared with no reward terms, no control cost and no bonus builds and rolls out rows of exact zeros; with a reward net its
    rows are weight * S bit for bit, and the planner plans on the learned reward alone."""
    spec = EnvDecl(7, 1, reward=(), ctrl_cost=0)
    prob = synth.make_problem(env=spec, context=False, E=5, m=M, H=4, seed=3, hidden_sizes=(32,) * 4)
    eng = make_engine(prob, p=5, num_elites=KE, num_cem_iters=ITERS)
    try:
        actions = np.random.default_rng(1).uniform(-1, 1, (M, 6, eng.H, eng.A)).astype(F)
        rows, traj = eng.rollout_returns(prob["obs"], None, actions, seed=2, call=1, it=0, want_traj=True)
        assert np.isfinite(_np(traj)).all()
        np.testing.assert_array_equal(_bits(_np(rows)), np.zeros(rows.shape, np.uint32), err_msg="a reward-free env's returns must be +0.0")
        prm, layers = _set(eng, "obs_act_next_obs", (24,), "tanh", seed=2, weight=-0.75)
        out, steps, S = (_np(t) for t in eng.reward_returns(traj, prob["obs"], actions, rows, prm, want_steps=True))
        assert np.abs(S).min() > 0
        np.testing.assert_array_equal(_bits(out), _bits(F(-0.75) * S))
        np.testing.assert_array_equal(_bits(S), _bits(rref.step_sum(steps)))
        assert_close(steps, rref.reward64(rref.gather_inputs(_np(traj), np.asarray(prob["obs"], F), actions, "obs_act_next_obs"), layers, "tanh"),
                     what="reward-free env")
        plan = _np(eng.rewarded_plan(prm, None, None, None, None, None, True, None, None, None, None, None, None, None, HipEngine.icem_params(),
                                     prob["obs"], None, None, prob["init_mean"], prob["init_var"], N, seed=1, call=1))
        assert np.isfinite(plan).all() and np.abs(plan).max() > 0
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------- 10: refusals
def test_argument_checks_return_einval(engines):
    """The C entries refuse bad arguments with CADM_EINVAL (no net: CADM_ESTATE) and a message that names them and the argument, before
    any HIP call (the dummy pointers next to the bad argument are never touched); the engine plans normally afterwards."""
    prob, eng = engines("hc5")
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(8192, dtype=torch.float32, device=eng.device)
    P = ct.c_void_p(buf.data_ptr())
    mp = HipEngine.mppi_params()
    _set(eng, "obs_act", (32, 16), "relu", seed=1)
    two = (ct.c_void_p * 5)(*([buf.data_ptr()] * 5))

    def V(n_hidden=2, hidden=(32, 16), activation=0, inputs=1, weight=1.0):
        v = _lib.RewardParams()
        v.n_hidden, v.activation, v.inputs, v.weight = n_hidden, activation, inputs, weight
        for l, h in enumerate(hidden):
            v.hidden[l] = h
        return ct.byref(v)

    def setnet(v, c=ctx, W=two, b=two, mean=P, inv=P):
        return lib.cadm_set_reward_net(c, v, W, b, mean, inv, None)

    def returns(v, c=ctx, traj=P, obs=P, actions=P, rows_out=P, step=P, ws=None):
        return lib.cadm_reward_returns(c, v, traj, obs, actions, None, M, 4, P, rows_out, step, None, ws, None)

    def plan(v, c=ctx, update=0, prm=ct.byref(mp)):
        return lib.cadm_rewarded_plan(c, v, None, None, None, None, None, 1, None, None, 0, None, None, None, None, None, update, prm, P, P, P, P,
                                      P, None, None, M, N, 0, 1, P, P, None, None)

    def refused(rc, name, frag, code=-1):
        msg = lib.cadm_last_error().decode()
        assert rc == code, "%s: expected %d, got %d (%s)" % (name, code, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    for name, fn in (("cadm_set_reward_net", setnet), ("cadm_reward_returns", returns), ("cadm_rewarded_plan", plan)):
        refused(fn(V(n_hidden=5)), name, "hidden layers")
        refused(fn(V(n_hidden=-1)), name, "hidden layers")
        refused(fn(V(hidden=(32, 0))), name, "width")
        refused(fn(V(hidden=(513, 16))), name, "width")
        refused(fn(V(activation=3)), name, "activation")
        refused(fn(V(activation=-1)), name, "activation")
        refused(fn(V(inputs=3)), name, "inputs")
        refused(fn(V(inputs=-1)), name, "inputs")
        for bad in (NAN, math.inf, -math.inf):
            refused(fn(V(weight=bad)), name, "weight")
    for name, fn in (("cadm_reward_returns", returns), ("cadm_rewarded_plan", plan)):
        refused(fn(V(hidden=(32, 17))), name, "registered net")
        refused(fn(V(n_hidden=1)), name, "registered net")
        refused(fn(V(activation=1)), name, "registered net")
        refused(fn(V(inputs=2)), name, "registered net")
    refused(returns(None), "cadm_reward_returns", "null")
    for kw in (dict(traj=None), dict(obs=None), dict(actions=None), dict(rows_out=None)):
        refused(returns(V(), **kw), "cadm_reward_returns", "null")
    refused(returns(V(), step=None, ws=None), "cadm_reward_returns", "workspace")
    refused(lib.cadm_reward_eval(ctx, None, 4, P, None), "cadm_reward_eval", "null")
    refused(lib.cadm_reward_eval(ctx, P, 0, P, None), "cadm_reward_eval", "R must be")
    refused(setnet(V(), W=None), "cadm_set_reward_net", "null")
    refused(setnet(V(), mean=None), "cadm_set_reward_net", "null")
    holes = (ct.c_void_p * 5)(buf.data_ptr(), None, buf.data_ptr(), None, None)
    refused(setnet(V(), b=holes), "cadm_set_reward_net", "layer 1")
    refused(plan(V(), update=2), "cadm_rewarded_plan", "update")
    refused(plan(V(), prm=None), "cadm_rewarded_plan", "bad arguments")
    # no registered net
    assert lib.cadm_set_reward_net(ctx, None, None, None, None, None, None) == 0
    refused(returns(V()), "cadm_reward_returns", "no reward net", code=-4)
    refused(plan(V()), "cadm_rewarded_plan", "no reward net", code=-4)
    refused(lib.cadm_reward_eval(ctx, P, 4, P, None), "cadm_reward_eval", "no reward net", code=-4)
    # K beyond CADM_MAX_REWARD_DIMS cannot be reached with the rollout's own limits on D and A: the check is the host's (test_reward_ref)
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=M, H=5, seed=1)
    deng = make_engine(dprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    refused(setnet(V(), c=deng._ctx), "cadm_set_reward_net", "continuous-action")
    refused(plan(V(), c=deng._ctx), "cadm_rewarded_plan", "continuous actions only")
    deng.close()
    sprob = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=5, seed=3, trained_like=True)
    seng = make_engine(sprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(seng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    refused(setnet(V(), c=seng._ctx), "cadm_set_reward_net", "sharded")
    refused(plan(V(), c=seng._ctx), "cadm_rewarded_plan", "sharded")
    assert lib.cadm_dist_destroy(seng._ctx) == 0
    seng.close()
    assert (_np(buf) == 0).all()
    # python: shapes that do not fit the engine or the declared net
    prm, layers = _set(eng, "obs_act", (32, 16), "relu", seed=1)
    z = lambda *s: np.zeros(s, F)
    good = (z(eng.H, M, 4, eng.p, eng.D), z(M, eng.D), z(M, 4, eng.H, eng.A), z(M, 4, eng.p))
    with pytest.raises(ValueError, match="reward_returns: traj"):
        eng.reward_returns(z(eng.H, M, 4, eng.p, eng.D + 1), *good[1:], prm)
    with pytest.raises(ValueError, match="reward_returns: obs"):
        eng.reward_returns(good[0], z(M + 1, eng.D), *good[2:], prm)
    with pytest.raises(ValueError, match="reward_returns: actions"):
        eng.reward_returns(*good[:2], z(M, 4, eng.H + 1, eng.A), good[3], prm)
    with pytest.raises(ValueError, match="reward_returns: first"):
        eng.reward_returns(*good, prm, first=np.zeros((M, 4), np.int32))
    with pytest.raises(ValueError, match="reward_eval: x"):
        eng.reward_eval(z(4, eng.D))
    with pytest.raises(ValueError, match="layer 1 is"):
        eng.set_reward_net(prm, rref.he_net(eng.D + eng.A, (32, 17), 0))
    args = (None, None, None, None, None, None, None, None, None, None, None, None, None, HipEngine.icem_params(), prob["obs"], prob["cp_obs"],
            prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    out = _np(eng.rewarded_plan(prm, *args, seed=1, call=1))
    assert np.isfinite(out).all() and np.abs(out).max() <= 1.0


def test_refusals_at_construction(gpu, monkeypatch):
    """`cem_reward_net` is refused where the other `cem_*` options are: use_cem=False, a discrete env, a process group of more than one
    rank; a Sequential of other sizes or another activation than the declared one is refused when it is set."""
    from cadm_amd.envs import make_env_spec
    rn = dict(inputs="obs_act", hidden_sizes=(16,), activation="tanh")
    with pytest.raises(ValueError, match="need use_cem=True"):
        plan_model(True, 5, use_cem=False, cem_reward_net=rn)
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        plan_model(True, 5, env=make_env_spec("cartpole"), cem_reward_net=rn)
    with pytest.raises(ValueError, match="hidden widths"):
        plan_model(True, 5, cem_reward_net=dict(hidden_sizes=(0,)))
    with pytest.raises(ValueError, match="reward inputs"):
        plan_model(True, 5, cem_reward_net=dict(inputs="act"))
    model, _ = plan_model(False, 5, cem_reward_net=rn)
    with pytest.raises(ValueError, match="activation"):
        model.set_reward_net(vref.sequential(rref.he_net(24, (16,), 0), "relu"))
    with pytest.raises(ValueError, match="layer 0 is"):
        model.set_reward_net(vref.sequential(rref.he_net(18, (16,), 0), "tanh"))
    with pytest.raises(ValueError, match="in_std"):
        model.set_reward_net(rref.he_net(24, (16,), 0), in_std=np.zeros(24))
    assert not model._reward_set
    import torch.distributed as dist
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        plan_model(True, 5, process_group=object(), cem_reward_net=rn)
