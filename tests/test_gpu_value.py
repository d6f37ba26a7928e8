"""GPU: the terminal value of the opt-in planner -- the kernel (`cadm_value_eval` / `cadm_value_returns`, csrc/value.hip) against the
numpy restatement (tests/value_ref.py), its independence of the batch, the row update, non-finite terminal states and the `first` cut,
the fused loop (`cadm_valued_plan`) against the stepwise one, the no-ops, the direction a value pulls a plan in, the class route and
the refusals.

Geometries: the module-scoped engines of tests/test_gpu_tracking.py -- hopper_like (D = 11, p = 5, H = 3), halfcheetah (D = 18, p = 20,
H = 8 and p = 5, H = 5); synthetic trajectories from tests/behind_rollout.py; the class route on tests/helpers.py's `plan_model`.

The kernel is held to the float64 restatement at the project's bar for fp32 kernels, `helpers.assert_close` at 1e-5 of the output's
scale.  Measured on an MI355X, worst |err| / (1e-5 x max(|ref|, rms)): relu 0.112, tanh 0.108, swish 0.190; 512 x 2: 0.074; with
statistics: 0.073."""
import ctypes as ct
import math
import os

import numpy as np
import pytest
import torch

import value_ref as vref
from behind_rollout import synth_traj
from cadm_amd import _lib, jit
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.caller import DevicePlannerState
from cadm_amd.engine import HipEngine
from helpers import _np, assert_close, floored_rel, make_engine, plan_act, plan_model, zero_carry
from test_gpu_tracking import engines      # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")
M, N, KE, ITERS = 2, 24, 8, 3
GEOMETRIES = [(), (48,), (64,), (200,), (48,) * 3, (64,) * 3, (200,) * 3, (64, 48, 200)]      # L in {0, 1, 3}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _set(eng, hidden, act="relu", seed=0, weight=1.0, mean=None, std=None, out_scale=1.0):
    """register a He-initialised net on the engine: (value_params, its layers)"""
    layers = vref.he_net(eng.D, hidden, seed, out_scale)
    prm = HipEngine.value_params(hidden, act, weight)
    eng.set_value_net(prm, layers, obs_mean=mean, obs_std=std)
    return prm, layers


def _traj(eng, m, n, seed):
    return synth_traj(seed, eng.H, m, n, eng.p, eng.D, eng.A)[0]


# ---------------------------------------------------------------------------------------------------------------------- 1: the kernel
@pytest.mark.parametrize("act", vref.ACTS)
def test_kernel_against_restatement(engines, act):
    """`cadm_value_eval` and `cadm_value_returns`' v_out on hopper_like (D = 11: a K that is no multiple of 4) against the float64
    restatement at 1e-5 of scale, for L in {0, 1, 3} and widths 48, 64, 200 and (64, 48, 200): 3 x 11 x 5 = 165 rows are ten full 16-row
    tiles and a tail of 5, n = 1 gives 15 rows, fewer than one tile."""
    _, eng = engines("hopper")
    worst = 0.0
    for gi, hidden in enumerate(GEOMETRIES):
        prm, layers = _set(eng, hidden, act, seed=10 + gi, weight=0.5)
        for m, n in ((3, 11), (3, 1)):
            traj = _traj(eng, m, n, 30 + gi)
            rows = np.random.default_rng(gi).standard_normal((m, n, eng.p)).astype(F)
            worst = max(worst, check_kernel_case(eng, prm, layers, act, traj, rows, 0.5, "%s %r %d rows" % (act, hidden, m * n * eng.p))[0])
    print("\n[%s] worst |err| / (1e-5 of scale): %.3f" % (act, worst))


def check_kernel_case(eng, prm, layers, act, traj, rows, weight, what, mean=None, std=None):
    """`cadm_value_eval` of traj's last states against the float64 restatement at 1e-5 of scale; `cadm_value_returns`' v_out has its bits,
    and the rows are the row update from them.  Returns (|err| / (1e-5 of scale), V float32, the restatement's V)."""
    m, n = traj.shape[1:3]
    states = traj[-1].reshape(-1, eng.D)
    ref = vref.value(states, layers, act, mean, std)
    got = _np(eng.value_eval(states))
    assert got.shape == (m * n * eng.p,) and np.isfinite(got).all(), what
    ratio = floored_rel(got, ref) / 1e-5
    assert_close(got, ref, what=what)
    out, v = eng.value_returns(traj, rows, prm, want_v=True)
    np.testing.assert_array_equal(_bits(_np(v)).reshape(-1), _bits(got), err_msg=what + ": v_out against cadm_value_eval")
    np.testing.assert_array_equal(_bits(_np(out)), _bits(vref.update(rows, _np(v), weight)), err_msg=what)
    return ratio, got, ref


def test_kernel_at_the_widest_net(engines):
    """512 x 2: two activation regions of 16 x 512 floats are 64 KiB, with the flags beyond what a kernel gets without raising its
    dynamic-LDS attribute; on halfcheetah (D = 18, p = 20), 2 x 3 x 20 = 120 rows."""
    _, eng = engines("hc8")
    prm, layers = _set(eng, (512, 512), "relu", seed=3)
    traj = _traj(eng, 2, 3, 5)
    states = traj[-1].reshape(-1, eng.D)
    ref = vref.value(states, layers, "relu")
    got = _np(eng.value_eval(states))
    print("\n[512 x 2] worst |err| / (1e-5 of scale): %.3f" % (floored_rel(got, ref) / 1e-5))
    assert_close(got, ref, what="512 x 2")


def test_kernel_with_statistics(engines):
    """obs_mean / obs_std that are not 0 / 1: the input is (x - mean) * float32(1 / std)."""
    _, eng = engines("hc5")
    rng = np.random.default_rng(8)
    mean, std = rng.standard_normal(eng.D).astype(F), rng.uniform(0.3, 4.0, eng.D).astype(F)
    prm, layers = _set(eng, (200, 200), "tanh", seed=4, mean=mean, std=std)
    states = _traj(eng, 3, 7, 6)[-1].reshape(-1, eng.D)
    ref = vref.value(states, layers, "tanh", mean, std)
    got = _np(eng.value_eval(states))
    print("\n[statistics] worst |err| / (1e-5 of scale): %.3f" % (floored_rel(got, ref) / 1e-5))
    assert_close(got, ref, what="with statistics")
    assert floored_rel(got, vref.value(states, layers, "tanh")) > 1e-3, "the statistics must matter"


# ---------------------------------------------------------------------------------------------------------------------- 2: batch independence
@pytest.mark.parametrize("hidden,act", [((64, 48, 200), "swish"), ((200, 200), "relu"), ((), "relu")], ids=["unequal-swish", "200x2-relu", "linear"])
def test_a_state_has_the_same_bits_in_any_batch(engines, hidden, act):
    """The same states through `value_eval` at R = 1, 5, 16, 165, at other row positions, inside a batch large enough for two row tiles
    per workgroup (more than 2 x 16 x the CU count rows), through `value_returns`' v_out, and run to run: equal bits."""
    _, eng = engines("hopper")
    prm, _ = _set(eng, hidden, act, seed=21)
    traj = _traj(eng, 3, 11, 41)
    states = traj[-1].reshape(-1, eng.D)
    full = _np(eng.value_eval(states))
    assert full.shape == (165,)
    np.testing.assert_array_equal(_bits(_np(eng.value_eval(states))), _bits(full), err_msg="run to run")
    for R in (1, 5, 16):
        np.testing.assert_array_equal(_bits(_np(eng.value_eval(states[:R]))), _bits(full[:R]), err_msg="R = %d" % R)
    rolled = _np(eng.value_eval(np.roll(states, 7, axis=0)))
    np.testing.assert_array_equal(_bits(rolled), _bits(np.roll(full, 7)), err_msg="rows moved by 7")
    reps = 2 * 16 * 256 // 165 + 8
    big = _np(eng.value_eval(np.concatenate([states[3:]] + [states] * reps, axis=0)))
    assert big.shape[0] > 2 * 16 * 256
    np.testing.assert_array_equal(_bits(big[:162]), _bits(full[3:]), err_msg="the two-row-tile launch, head")
    np.testing.assert_array_equal(_bits(big[-165:]), _bits(full), err_msg="the two-row-tile launch, tail")
    _, v = eng.value_returns(traj, np.zeros((3, 11, eng.p), F), prm, want_v=True)
    np.testing.assert_array_equal(_bits(_np(v)).reshape(-1), _bits(full), err_msg="value_returns' v_out")
    lead = eng.value_eval(states.reshape(3, 11, eng.p, eng.D))
    assert tuple(lead.shape) == (3, 11, eng.p)
    np.testing.assert_array_equal(_bits(_np(lead)).reshape(-1), _bits(full))


# ---------------------------------------------------------------------------------------------------------------------- 3: the row update
@pytest.mark.parametrize("weight", [1.0, -0.37, 0.0])
def test_row_update(engines, weight):
    """rows_out == float32(rows_in + float32(weight * v)) bit for bit from the kernel's own v_out; rows_out aliasing rows_in and
    v_out = NULL give the same rows_out; rows_in is not written otherwise."""
    _, eng = engines("hc5")
    prm, _ = _set(eng, (64, 64), "swish", seed=5, weight=weight)
    traj = _traj(eng, 3, 7, 9)
    rows = (10.0 * np.random.default_rng(2).standard_normal((3, 7, eng.p))).astype(F)
    t_dev, r_dev = eng._t(traj), eng._t(rows)
    out, v = eng.value_returns(t_dev, r_dev, prm, want_v=True)
    np.testing.assert_array_equal(_bits(_np(r_dev)), _bits(rows), err_msg="rows_in was written")
    np.testing.assert_array_equal(_bits(_np(out)), _bits(vref.update(rows, _np(v), weight)))
    np.testing.assert_array_equal(_bits(_np(eng.value_returns(t_dev, r_dev, prm))), _bits(_np(out)), err_msg="v_out = NULL")
    alias = r_dev.clone()
    assert eng.value_returns(t_dev, alias, prm, out=alias) is alias
    np.testing.assert_array_equal(_bits(_np(alias)), _bits(_np(out)), err_msg="rows_out aliasing rows_in")
    assert weight == 0.0 or not np.array_equal(_bits(_np(out)), _bits(rows))


# ---------------------------------------------------------------------------------------------------------------------- 4: non-finite states, the first cut
@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_non_finite_terminal_states_and_the_first_cut(engines, act):
    """NaN and +-inf in single dims of traj[H-1] make those rows' V and return NaN -- under relu too, whose max(NaN, 0) would hide them --,
    garbage in earlier steps reaches nothing, and every other row has the bits it has without its neighbours' poison.  With `first`,
    rows with first < H keep their input bits, terminal NaN or not, and read NaN in v_out; rows with first == H are valued."""
    _, eng = engines("hopper")
    H, p, D = eng.H, eng.p, eng.D
    prm, _ = _set(eng, (48, 48), act, seed=6, weight=2.0)
    m, n = 3, 11
    clean = _traj(eng, m, n, 12)
    rows = np.random.default_rng(4).standard_normal((m, n, p)).astype(F)
    ref_out, ref_v = (_np(x) for x in eng.value_returns(clean, rows, prm, want_v=True))
    assert np.isfinite(ref_v).all()
    rng = np.random.default_rng(13)
    bad = clean.copy()
    bad[:-1][rng.uniform(size=bad[:-1].shape) < 0.2] = np.nan             # earlier steps: never read
    bad[0, 0, 0, 0, :] = np.inf
    hit = rng.uniform(size=(m, n, p)) < 0.2
    hit[0, 0, 0], hit[0, 0, 1], hit[m - 1, n - 1, p - 1] = True, False, True      # the first row, its neighbour, the tail tile's last row
    mi, ni, j = np.nonzero(hit)
    poison = np.array([np.nan, np.inf, -np.inf], F)[rng.integers(0, 3, mi.size)]
    bad[H - 1, mi, ni, j, rng.integers(0, D, mi.size)] = poison
    out, v = (_np(x) for x in eng.value_returns(bad, rows, prm, want_v=True))
    assert np.isnan(v[hit]).all() and np.isnan(out[hit]).all()
    np.testing.assert_array_equal(_bits(v[~hit]), _bits(ref_v[~hit]), err_msg="a row met its neighbour's poison")
    np.testing.assert_array_equal(_bits(out[~hit]), _bits(ref_out[~hit]))
    flat = _np(eng.value_eval(bad[-1]))
    assert np.isnan(flat[hit]).all()
    np.testing.assert_array_equal(_bits(flat[~hit]), _bits(ref_v[~hit]))
    # the first cut
    first = rng.integers(0, H + 1, (m, n, p)).astype(np.int32)
    first[0, 0, 0], first[0, 0, 1], first[0, 0, 2] = 0, H, H - 1
    hit[0, 0, 2] = True
    bad[H - 1, 0, 0, 2, 3] = np.nan
    cut = first < H
    assert cut[hit].any() and (~cut)[hit].any() and cut[~hit].any() and (~cut)[~hit].any()
    out, v = (_np(x) for x in eng.value_returns(bad, rows, prm, first=first, want_v=True))
    np.testing.assert_array_equal(_bits(out[cut]), _bits(rows[cut]), err_msg="a row with first < H must keep its input bits")
    assert np.isnan(v[cut]).all()
    live = ~cut & ~hit
    np.testing.assert_array_equal(_bits(out[live]), _bits(ref_out[live]))
    np.testing.assert_array_equal(_bits(v[live]), _bits(ref_v[live]))
    assert np.isnan(out[~cut & hit]).all() and np.isnan(v[~cut & hit]).all()


# ---------------------------------------------------------------------------------------------------------------------- 5: fused against stepwise
def _check_iterations(eng, info, prm, first_used):
    """every stepwise iteration: rows == the row update of value_rows from the iteration's own V, and V == `value_eval` of traj[H-1]"""
    for x in info:
        v, before, rows = _np(x["value"]), _np(x["value_rows"]), _np(x["rows"])
        first = _np(x["first_violation"]) if first_used else None
        np.testing.assert_array_equal(_bits(rows), _bits(vref.update(before, v, prm.weight, first, eng.H)))
        flat = _np(eng.value_eval(x["traj"][-1]))
        keep = np.ones(v.shape, bool) if first is None else first >= eng.H
        np.testing.assert_array_equal(_bits(v[keep]), _bits(flat[keep]))
        assert np.isnan(v[~keep]).all()


COMBOS = ["alone", "mppi-cvar", "terminate-tracking", "actuator-uncertainty"]


@pytest.mark.parametrize("combo", COMBOS)
def test_fused_equals_stepwise(engines, combo):
    """`cadm_valued_plan` with device RNG == the same loop one launch at a time (`planner.icem_plan(..., value=...)`), bit for bit over
    two consecutive calls: the plan, the best return, the carry (and the actuator state); in every stepwise iteration the rows are the
    row update of the rows before it from the kernel's own V."""
    from test_gpu_actuator import _params, _state
    from test_gpu_constraints import binding_bounds, iteration0_traj
    from test_gpu_tracking import _tracking_inputs
    from test_gpu_uncertainty import _prm as unc_prm
    prob, eng = engines("hc5-vanilla" if combo == "alone" else "hc5")
    H, A = eng.H, eng.A
    value, _ = _set(eng, (64, 48), "tanh", seed=31, weight=3.0)
    mppi = combo == "mppi-cvar"
    K = 0 if combo == "alone" else 2
    icem = dict(noise_beta=1.0 if mppi else 0.0, keep_elites=K, decay=1.25 if K else 1.0, return_best=combo == "terminate-tracking",
                add_mean_last=K > 0)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if mppi else HipEngine.icem_params(**icem)
    score = HipEngine.score_params("cvar", k=2) if mppi else None
    cons = track = targets = offset = act = unc = None
    if combo == "terminate-tracking":
        track, targets, offset, _ = _tracking_inputs(eng, prob, 3, H, 13)
        cons = HipEngine.constraint_params(binding_bounds(iteration0_traj(eng, prob, 0.0, 4, 1), (1, 7), H, "valued"), "terminate", 4.0)
    (pa, fa), (pb, fb) = (None, None), (None, None)
    if combo == "actuator-uncertainty":
        act, unc = _params(eng, 1, 0.4, 2.0), unc_prm(eng, "epistemic", 0.3)
        (pa, fa), (pb, fb) = _state(eng, 1, 8), _state(eng, 1, 8)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    (ca, va), (cb, vb) = zero_carry(eng, M, K, H), zero_carry(eng, M, K, H)
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2):
        a, ra = eng.valued_plan(value, unc, act, pa, fa, True, track, targets, offset, None, None, cons, score, prm, *args, mean, var, N,
                                carry=ca, carry_valid=va, seed=4, call=call, want_best_return=True)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                            update="mppi" if mppi else "cem", temperature=0.5, relative=True, score=score, constraints=cons,
                                            tracking=None if track is None else (track, targets, offset),
                                            actuator=None if act is None else (act, pb, fb), action_advance=True, uncertainty=unc,
                                            value=value, **icem)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        for x, y in ((ca, cb), (pa, pb), (fa, fb)):
            if x is not None:
                np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))
        _check_iterations(eng, info, value, cons is not None)
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)
    if cons is not None:
        share = float((_np(info[0]["first_violation"]) < H).mean())
        assert 0.1 <= share <= 0.9, "%.2f of the rows are cut" % share
    # the term matters: without it, another plan
    other = _np(eng.valued_plan(None, unc, act, pb, fb, False, track, targets, offset, None, None, cons, score, prm, *args, mean, var, N,
                                *zero_carry(eng, M, K, H), seed=4, call=2))
    assert not np.array_equal(_bits(other), _bits(a))
    assert (mppi, "val", cons is not None, act is not None, unc is not None) in eng._loop_ws


# ---------------------------------------------------------------------------------------------------------------------- 6: the no-ops
@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_no_value_is_the_loop_underneath(engines, update):
    """value = NULL: the plan, the best return and the carry of `cadm_uncertain_plan` on the same inputs, bit for bit, through the C entry
    itself with that loop's workspace; and the workspace with a value is the loop underneath's with the trajectory view (under TERMINATE
    with the first-violation view), nothing more."""
    prob, eng = engines("hc5")
    H, A = eng.H, eng.A
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    mppi, full = eng._as_mppi_params(prm)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    carry, valid = zero_carry(eng, M, 2, H)
    plan, best = eng.uncertain_plan(None, None, None, None, True, None, None, None, None, None, None, None, prm, *args, carry=carry,
                                    carry_valid=valid, seed=5, call=2, want_best_return=True)
    carry2, valid2 = zero_carry(eng, M, 2, H)
    t = [eng._t(x) for x in args[:5]]
    ws = eng._loop_workspace(mppi, M, N, 2)
    out = torch.empty((M, H, A), dtype=torch.float32, device=eng.device)
    best2 = torch.empty((M,), dtype=torch.float32, device=eng.device)
    P = lambda x: ct.c_void_p(x.data_ptr())
    rc = eng.lib.cadm_valued_plan(eng._ctx, None, None, None, None, None, 1, None, None, 0, None, None, None, None, None, int(mppi),
                                  ct.byref(full), *[P(x) for x in t], P(carry2), P(valid2), M, N, 5, 2, P(ws), P(out), P(best2), eng.stream)
    assert rc == 0, eng.lib.cadm_last_error().decode()
    for x, y in ((plan, out), (best, best2), (carry, carry2)):
        np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))
    lib = eng.lib
    for terminate in (0, 1):
        for act in (0, 1):
            assert lib.cadm_valued_workspace_bytes(eng._ctx, M, N, 2, int(mppi), terminate, act, 1) == \
                lib.cadm_uncertain_workspace_bytes(eng._ctx, M, N, 2, int(mppi), terminate, act)
            assert lib.cadm_valued_workspace_bytes(eng._ctx, M, N, 2, int(mppi), terminate, act, 0) == (
                lib.cadm_actuated_workspace_bytes(eng._ctx, M, N, 2, int(mppi), 1, terminate) if act
                else lib.cadm_tracking_workspace_bytes(eng._ctx, M, N, 2, int(mppi), terminate))
    assert lib.cadm_valued_workspace_bytes(eng._ctx, 0, N, 2, 0, 0, 0, 0) == 0


def test_a_zero_output_layer_changes_no_plan(engines):
    """A net whose output layer is all zeros has V = +0.0: every row keeps its value (x + 0.0 == x), so the elite sets of every iteration,
    the plan and the carry are those of the loop without the term."""
    prob, eng = engines("hc5")
    layers = vref.he_net(eng.D, (64, 64), 7)
    layers[-1] = (np.zeros_like(layers[-1][0]), np.zeros_like(layers[-1][1]))
    value = HipEngine.value_params((64, 64), "relu", 5.0)
    eng.set_value_net(value, layers)
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.0, return_best=False, add_mean_last=True)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    (ca, va), (cb, vb) = zero_carry(eng, M, 2, eng.H), zero_carry(eng, M, 2, eng.H)
    a, ia, _ = hplanner.icem_plan(eng, *args, carry=ca, carry_valid=va, seed=3, call=1, return_info=True, value=value, **icem)
    b, ib, _ = hplanner.icem_plan(eng, *args, carry=cb, carry_valid=vb, seed=3, call=1, return_info=True, **icem)
    for x, y in zip(ia, ib):
        assert (_np(x["value"]) == 0).all()
        np.testing.assert_array_equal(_np(x["elites"]), _np(y["elites"]))
        assert (_np(x["rows"]) == _np(y["rows"])).all()
    np.testing.assert_array_equal(_bits(_np(a)), _bits(_np(b)))
    np.testing.assert_array_equal(_bits(_np(ca)), _bits(_np(cb)))
    fused = eng.valued_plan(value, None, None, None, None, True, None, None, None, None, None, None, None, HipEngine.icem_params(**icem), *args,
                            *zero_carry(eng, M, 2, eng.H), seed=3, call=1)
    np.testing.assert_array_equal(_bits(_np(fused)), _bits(_np(b)))


# ---------------------------------------------------------------------------------------------------------------------- 7: the direction
def test_a_linear_value_pulls_the_plan(gpu):
    """halfcheetah, a linear V = c x_d: against the plain plan, the planned trajectory's terminal mean of x_d (from `forecast`) moves up
    with +c and down with -c, in every env, on a deterministic model (the members' mean predictions).  d is the dim whose terminal mean the ACTIONS move most, measured on random plans through the
    plain model's forecast in units of the particles' own spread there (the synthetic model's property, not the planner's), and c is 100
    times the spread of those plans' returns over the spread of their terminal x_d: far above the reward's scale.  Cannot pass without
    the term."""
    H, A, D = 5, 6, 18
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    other = dict(cem_return="best", deterministic=True)      # no particle noise: a plan's effect is not drowned in the draw of its row
    plain, prob = plan_model(False, H, **other)
    probe = np.random.default_rng(1).uniform(-1, 1, (M, 16, H, A)).astype(F)
    fc = plain.forecast(prob["obs"], probe, seed=11)
    end = fc["mean"][:, :, -1].astype(np.float64)                                    # [M,16,D]
    moved = end.std(axis=1).min(axis=0)                                               # what the plan moves, the weaker env
    d = int(np.argmax(moved / fc["std_total"][:, :, -1].astype(np.float64).mean(axis=(0, 1))))
    c = 100.0 * float(fc["rollout_returns"].astype(np.float64).mean(axis=2).std(axis=1).max()) / float(moved[d])
    term = {"plain": plain.forecast(prob["obs"], plan_act(plain, prob, False, mean, var), seed=11)["mean"][:, -1, d].astype(np.float64)}
    for name, sign in (("up", 1.0), ("down", -1.0)):
        model, _ = plan_model(False, H, cem_terminal_value=dict(hidden_sizes=(), weight=1.0), **other)
        W = np.zeros((D, 1), F)
        W[d, 0] = sign * c
        model.set_terminal_value([(W, np.zeros((1,), F))])
        plan = plan_act(model, prob, False, mean, var)
        assert np.isfinite(plan).all()
        term[name] = model.forecast(prob["obs"], plan, seed=11)["mean"][:, -1, d].astype(np.float64)
    print("\n[direction] d = %d, c = %.3g, random plans move it by %.3g; terminal mean: down %s  plain %s  up %s"
          % (d, c, moved[d], term["down"], term["plain"], term["up"]))
    assert (term["up"] > term["plain"]).all() and (term["down"] < term["plain"]).all()


# ---------------------------------------------------------------------------------------------------------------------- 8: the class route
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_class_route(gpu, context):
    """`get_action` and `DevicePlannerState` with a Sequential-set net agree with the engine call; `terminal_value` and
    `plan_terminal_value` with the restatement; no net raises RuntimeError; a replaced net takes effect on the next call and builds nothing."""
    H, A, D = 5, 6, 18
    hidden, act = (64, 32), "swish"
    tv = dict(hidden_sizes=hidden, activation=act, weight=0.8)
    model, prob = plan_model(context, H, cem_terminal_value=tv, cem_keep_elites=2)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    with pytest.raises(RuntimeError, match="no value net"):
        plan_act(model, prob, context, mean, var)
    with pytest.raises(RuntimeError, match="no value net"):
        model.terminal_value(np.zeros((3, D), F))
    assert model._call == 0
    rng = np.random.default_rng(5)
    stats = (rng.standard_normal(D).astype(F), rng.uniform(0.5, 2.0, D).astype(F))
    layers = vref.he_net(D, hidden, 17)
    model.set_terminal_value(vref.sequential(layers, act), *stats)
    plan = plan_act(model, prob, context, mean, var)
    assert np.isfinite(plan).all() and model._call == 1
    eng, opt = model.engine, model._opt
    hist = (prob["cp_obs"], prob["cp_act"]) if context else (None, None)
    carry, valid = zero_carry(eng, M, 2, H)
    direct = eng.valued_plan(opt.value_params, None, None, None, None, True, None, None, None, None, None, None, None, opt.params, prob["obs"],
                             *hist, mean, var, model.n_candidates, carry=carry, carry_valid=valid, seed=model.seed, call=1)
    np.testing.assert_array_equal(_bits(plan), _bits(_np(direct)))
    np.testing.assert_array_equal(_bits(_np(model._plan_carry)), _bits(_np(carry)))
    # the device-resident caller state takes the same route
    twin, _ = plan_model(context, H, cem_terminal_value=tv, cem_keep_elites=2)
    twin.set_terminal_value(layers, *stats)                      # the list form of the same net
    state = DevicePlannerState(twin, M)
    if context:
        state.hist_obs.copy_(eng._t(prob["cp_obs"]).reshape(state.hist_obs.shape))
        state.hist_act.copy_(eng._t(prob["cp_act"]).reshape(state.hist_act.shape))
    first_action = _np(state.act(prob["obs"]))
    np.testing.assert_array_equal(_bits(first_action), _bits(plan[:, 0]))
    # V through the class, against the restatement
    states = (2.0 * rng.standard_normal((4, 7, D))).astype(F)
    v = model.terminal_value(states)
    assert v.shape == (4, 7)
    assert_close(v, vref.value(states, layers, act, *stats), what="terminal_value")
    res = model.plan_terminal_value(prob["obs"], plan, *(hist if context else ()))
    assert res["value"].shape == (M, 5) and res["first"] is None and model._call == 1
    fc = model.forecast(prob["obs"], plan, *(hist if context else ()))
    many = model.plan_terminal_value(prob["obs"], np.repeat(plan[:, None], 3, axis=1), *(hist if context else ()))
    assert many["value"].shape == (M, 3, 5) and np.isfinite(many["value"]).all()
    np.testing.assert_array_equal(_bits(many["value"][0, 0]), _bits(res["value"][0]))      # (the noise is drawn per row: env 0's rows are where they were)
    assert np.isfinite(fc["rollout_returns"]).all()
    # a replaced net: the next call plans with it, and nothing is built
    before = sorted((f, os.path.getmtime(os.path.join(jit.cache_dir(), f))) for f in os.listdir(jit.cache_dir()))
    ws = dict(eng._loop_ws)
    other = vref.he_net(D, hidden, 18, out_scale=30.0)
    model.set_terminal_value(other, *stats)
    assert_close(model.terminal_value(states), vref.value(states, other, act, *stats), what="the replaced net")
    plan2 = plan_act(model, prob, context, mean, var)      # call 2, from call 1's carry: what `carry` / `valid` hold since the direct call above
    direct2 = eng.valued_plan(opt.value_params, None, None, None, None, True, None, None, None, None, None, None, None, opt.params, prob["obs"],
                              *hist, mean, var, model.n_candidates, carry=carry, carry_valid=valid, seed=model.seed, call=2)
    np.testing.assert_array_equal(_bits(plan2), _bits(_np(direct2)))
    assert not np.array_equal(_bits(plan2), _bits(plan))
    assert sorted((f, os.path.getmtime(os.path.join(jit.cache_dir(), f))) for f in os.listdir(jit.cache_dir())) == before
    assert all(eng._loop_ws[k][1] is ws[k][1] for k in ws)
    # fit-free housekeeping leaves the net alone; clearing it brings the RuntimeError back
    model.reset_plan_carry()
    assert_close(model.terminal_value(states), vref.value(states, other, act, *stats), what="after reset_plan_carry")
    model.clear_terminal_value()
    with pytest.raises(RuntimeError, match="no value net"):
        plan_act(model, prob, context, mean, var)
    plain, _ = plan_model(context, H, cem_noise_beta=1.0)
    for fn in (lambda: plain.set_terminal_value(layers), lambda: plain.terminal_value(states), lambda: plain.clear_terminal_value()):
        with pytest.raises(ValueError, match="no cem_terminal_value"):
            fn()


def test_class_route_under_terminate_constraints(gpu):
    """`plan_terminal_value` of a model with TERMINATE constraints reports their first violations and values only the particles that
    reach the horizon."""
    H, A, D = 5, 6, 18
    tv = dict(hidden_sizes=(32,), activation="relu")
    base, prob = plan_model(True, H, cem_terminal_value=tv)
    layers = vref.he_net(D, (32,), 3)
    base.set_terminal_value(layers)
    plan = np.random.default_rng(3).uniform(-1, 1, (M, 4, H, A)).astype(F)
    hist = (prob["cp_obs"], prob["cp_act"])
    free = base.plan_terminal_value(prob["obs"], plan, *hist)
    fc = base.forecast(prob["obs"], plan, *hist)
    lo = float(np.quantile(fc["mean"][..., 1], 0.3))
    model, _ = plan_model(True, H, cem_terminal_value=tv, cem_constraints=[dict(dim=1, lo=lo)], cem_constraint_mode="terminate",
                          cem_constraint_weight=1.0)
    model.set_terminal_value(layers)
    res = model.plan_terminal_value(prob["obs"], plan, *hist)
    cut = res["first"] < H
    assert cut.any() and (~cut).any() and free["first"] is None
    assert np.isnan(res["value"][cut]).all()
    np.testing.assert_array_equal(_bits(res["value"][~cut]), _bits(free["value"][~cut]))


# ---------------------------------------------------------------------------------------------------------------------- 9: refusals
def test_argument_checks_return_einval(engines):
    """The C entries refuse bad arguments with CADM_EINVAL (no net: CADM_ESTATE) and a message that names them and the argument, before
    any HIP call (the dummy pointers next to the bad argument are never touched); the engine plans normally afterwards."""
    prob, eng = engines("hc5")
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(8192, dtype=torch.float32, device=eng.device)
    P = ct.c_void_p(buf.data_ptr())
    mp = HipEngine.mppi_params()
    _set(eng, (32, 16), "relu", seed=1)
    two = (ct.c_void_p * 5)(*([buf.data_ptr()] * 5))

    def V(n_hidden=2, hidden=(32, 16), activation=0, weight=1.0):
        v = _lib.ValueParams()
        v.n_hidden, v.activation, v.weight = n_hidden, activation, weight
        for l, h in enumerate(hidden):
            v.hidden[l] = h
        return ct.byref(v)

    def setnet(v, c=ctx, W=two, b=two, mean=P, inv=P):
        return lib.cadm_set_value_net(c, v, W, b, mean, inv, None)

    def returns(v, c=ctx):
        return lib.cadm_value_returns(c, v, P, None, M, 4, P, P, None, None)

    def plan(v, c=ctx, update=0, prm=ct.byref(mp)):
        return lib.cadm_valued_plan(c, v, None, None, None, None, 1, None, None, 0, None, None, None, None, None, update, prm, P, P, P, P, P, None,
                                    None, M, N, 0, 1, P, P, None, None)

    def refused(rc, name, frag, code=-1):
        msg = lib.cadm_last_error().decode()
        assert rc == code, "%s: expected %d, got %d (%s)" % (name, code, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    for name, fn in (("cadm_set_value_net", setnet), ("cadm_value_returns", returns), ("cadm_valued_plan", plan)):
        refused(fn(V(n_hidden=5)), name, "hidden layers")
        refused(fn(V(n_hidden=-1)), name, "hidden layers")
        refused(fn(V(hidden=(32, 0))), name, "width")
        refused(fn(V(hidden=(513, 16))), name, "width")
        refused(fn(V(activation=3)), name, "activation")
        refused(fn(V(activation=-1)), name, "activation")
        for bad in (NAN, math.inf, -math.inf):
            refused(fn(V(weight=bad)), name, "weight")
    for name, fn in (("cadm_value_returns", returns), ("cadm_valued_plan", plan)):
        refused(fn(V(hidden=(32, 17))), name, "registered net")
        refused(fn(V(n_hidden=1)), name, "registered net")
        refused(fn(V(activation=1)), name, "registered net")
    refused(returns(None), "cadm_value_returns", "null")
    refused(lib.cadm_value_returns(ctx, V(), P, None, M, 4, P, None, None, None), "cadm_value_returns", "null")
    refused(lib.cadm_value_eval(ctx, None, 4, P, None), "cadm_value_eval", "null")
    refused(lib.cadm_value_eval(ctx, P, 0, P, None), "cadm_value_eval", "R must be")
    refused(setnet(V(), W=None), "cadm_set_value_net", "null")
    refused(setnet(V(), mean=None), "cadm_set_value_net", "null")
    holes = (ct.c_void_p * 5)(buf.data_ptr(), None, buf.data_ptr(), None, None)
    refused(setnet(V(), b=holes), "cadm_set_value_net", "layer 1")
    refused(plan(V(), update=2), "cadm_valued_plan", "update")
    refused(plan(V(), prm=None), "cadm_valued_plan", "bad arguments")
    # no registered net
    assert lib.cadm_set_value_net(ctx, None, None, None, None, None, None) == 0
    refused(returns(V()), "cadm_value_returns", "no value net", code=-4)
    refused(plan(V()), "cadm_valued_plan", "no value net", code=-4)
    refused(lib.cadm_value_eval(ctx, P, 4, P, None), "cadm_value_eval", "no value net", code=-4)
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=M, H=5, seed=1)
    deng = make_engine(dprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    refused(setnet(V(), c=deng._ctx), "cadm_set_value_net", "continuous-action")
    refused(plan(V(), c=deng._ctx), "cadm_valued_plan", "continuous actions only")
    deng.close()
    sprob = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=5, seed=3, trained_like=True)
    seng = make_engine(sprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(seng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    refused(setnet(V(), c=seng._ctx), "cadm_set_value_net", "sharded")
    refused(plan(V(), c=seng._ctx), "cadm_valued_plan", "sharded")
    assert lib.cadm_dist_destroy(seng._ctx) == 0
    seng.close()
    assert (_np(buf) == 0).all()
    # python: shapes that do not fit the engine or the declared net
    prm, layers = _set(eng, (32, 16), "relu", seed=1)
    with pytest.raises(ValueError, match="value_returns: traj"):
        eng.value_returns(np.zeros((eng.H, M, 4, eng.p, eng.D + 1), F), np.zeros((M, 4, eng.p), F), prm)
    with pytest.raises(ValueError, match="value_returns: first"):
        eng.value_returns(np.zeros((eng.H, M, 4, eng.p, eng.D), F), np.zeros((M, 4, eng.p), F), prm, first=np.zeros((M, 4), np.int32))
    with pytest.raises(ValueError, match="value_eval: states"):
        eng.value_eval(np.zeros((4, eng.D + 1), F))
    with pytest.raises(ValueError, match="layer 1 is"):
        eng.set_value_net(prm, vref.he_net(eng.D, (32, 17), 0))
    args = (None, None, None, None, None, None, None, None, None, None, None, None, HipEngine.icem_params(), prob["obs"], prob["cp_obs"],
            prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    out = _np(eng.valued_plan(prm, *args, seed=1, call=1))
    assert np.isfinite(out).all() and np.abs(out).max() <= 1.0


def test_refusals_at_construction(gpu, monkeypatch):
    """`cem_terminal_value` is refused where the other `cem_*` options are: use_cem=False, a discrete env, a process group of more than
    one rank; a Sequential of other sizes or another activation than the declared one is refused when it is set."""
    from cadm_amd.envs import make_env_spec
    tv = dict(hidden_sizes=(16,), activation="tanh")
    with pytest.raises(ValueError, match="need use_cem=True"):
        plan_model(True, 5, use_cem=False, cem_terminal_value=tv)
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        plan_model(True, 5, env=make_env_spec("cartpole"), cem_terminal_value=tv)
    with pytest.raises(ValueError, match="hidden widths"):
        plan_model(True, 5, cem_terminal_value=dict(hidden_sizes=(0,)))
    model, _ = plan_model(False, 5, cem_terminal_value=tv)
    with pytest.raises(ValueError, match="activation"):
        model.set_terminal_value(vref.sequential(vref.he_net(18, (16,), 0), "relu"))
    with pytest.raises(ValueError, match="layer 0 is"):
        model.set_terminal_value(vref.sequential(vref.he_net(18, (24,), 0), "tanh"))
    with pytest.raises(ValueError, match="obs_std"):
        model.set_terminal_value(vref.he_net(18, (16,), 0), obs_std=np.zeros(18))
    assert not model._value_set
    import torch.distributed as dist
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        plan_model(True, 5, process_group=object(), cem_terminal_value=tv)
