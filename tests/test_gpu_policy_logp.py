"""GPU: the actor's log-density of given actions -- the kernel (`cadm_policy_logp` / `cadm_policy_logp_returns`, csrc/policy_logp.hip)
against the restatement (tests/policy_logp_ref.py) under its `bars()`, its independence of the batch and of the launcher's row-tile
variant, the step sum and the row update, non-finite inputs and the `first` cut, the fused loop (`cadm_anchored_plan`) against the
stepwise one, the no-ops, the direction the term pulls a plan in, the class route and the refusals.

Geometries: kernel level on pendulum (A = 1) and halfcheetah (A = 6; once with the action bounds [-0.5, 2]), never rolled out; the stage
and the loops on the module-scoped engines of tests/test_gpu_tracking.py -- hopper_like (D = 11, A = 3, p = 5, H = 3), halfcheetah
(p = 5, H = 5); synthetic trajectories from tests/behind_rollout.py; the class route on tests/helpers.py's `plan_model`.

Every test prints its worst |err| / bar; the figures of one run on an MI355X stand in profiles/policy_logp.md."""
import ctypes as ct
import math

import numpy as np
import pytest
import torch

import gauss_policy_ref as gref
import policy_logp_ref as lref
import policy_ref as pref
import reward_ref as rref
import test_gpu_gauss_policy as gp
import value_ref as vref
from behind_rollout import synth_traj
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import _np, make_engine, plan_act, plan_model, zero_carry
from test_gpu_tracking import engines      # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")
M, N, KE, ITERS = 2, 24, 8, 3
LO, HI = gp.LO, gp.HI
NETS = [(), (50, 33)]
SIZES = (1, 15, 17, 33)
CASES = [(sq, bd) for sq in ("tanh", "none") for bd in gref.BOUNDS]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


@pytest.fixture(scope="module")
def kengines(gpu):
    """name -> engine, kernel level, never rolled out: "pend" (D = 3, A = 1), "hc" (D = 18, A = 6), "hc-bounds" (bounds [-0.5, 2])"""
    built = {}

    def get(name):
        if name not in built:
            prob = synth.make_problem(env="pendulum" if name == "pend" else "halfcheetah", context=False, E=5, m=2, H=3, seed=52)
            built[name] = make_engine(prob, p=5, **(dict(lower_bound=-0.5, upper_bound=2.0) if name == "hc-bounds" else {}))
        return built[name]
    yield get
    for eng in built.values():
        eng.close()


def _actions(rng, R, A, lb, ub):
    """interior actions, with elements exactly on lb / ub and beyond them planted (these hit the clamp)"""
    mid, half = 0.5 * (ub + lb), 0.5 * (ub - lb)
    a = (mid + half * rng.uniform(-0.98, 0.98, (R, A))).astype(F)
    a[0::5, 0] = ub
    a[1::5, A - 1] = lb
    a[2::7, 0] = ub + 0.75
    a[3::7, A - 1] = lb - 0.25
    return a


def _gather(traj, obs, actions):
    """(states [H,m,n,p,D], actions [H,m,n,p,A]) of every (step, row): s_t = obs[mi] at t = 0, else traj[t-1]; a_t = actions[mi,ni,t]"""
    traj, obs, actions = (np.asarray(_np(v) if isinstance(v, torch.Tensor) else v, F) for v in (traj, obs, actions))
    H, m, n, p, D = traj.shape
    s = np.concatenate([np.broadcast_to(obs[None, :, None, None, :], (1, m, n, p, D)), traj[:-1]], axis=0)
    a = np.broadcast_to(np.moveaxis(actions, 2, 0)[:, :, :, None, :], (H, m, n, p, actions.shape[-1]))
    return np.ascontiguousarray(s), np.ascontiguousarray(a)


def _ratio(eng, layers, act, squash, bound, x, a, space, lb=-1.0, ub=1.0, lo=LO, hi=HI, got=None):
    """worst |kernel - float64 restatement| / bar over the rows"""
    z = gref.z64(x, layers, act)
    ref = lref.logp64(z, a, squash, bound, lo, hi, lb, ub, space=space, y=lref.y32(a, lb, ub) if squash == "tanh" else None)
    bar = lref.bars(z, ref, squash, bound, lo, hi, lb, ub, space=space)
    got = _np(eng.policy_log_prob(x, a, space)) if got is None else got
    assert got.shape == ref["logp"].shape and np.isfinite(got).all() and np.isfinite(ref["logp"]).all()
    return float((np.abs(got.astype(np.float64) - ref["logp"]) / bar).max())


# ---------------------------------------------------------------------------------------------------------------------- 1: the kernel
@pytest.mark.parametrize("squash,bound", CASES)
def test_kernel_against_restatement(kengines, squash, bound):
    """`cadm_policy_logp` against the float64 restatement (continued from the kernel's own float32 y) under `lref.bars`: A = 1 and A = 6,
    the linear policy and (50, 33) -- no multiples of 4 or 64 --, both spaces, R in {1, 15, 17, 33} (below, at and above one and two
    16-row tiles), actions inside the bounds, exactly on them and beyond them; once with bounds that are not symmetric."""
    worst = 0.0
    for name in ("pend", "hc", "hc-bounds"):
        eng = kengines(name)
        lb, ub = (-0.5, 2.0) if name == "hc-bounds" else (-1.0, 1.0)
        rng = np.random.default_rng(7 + eng.A)
        x = gp._states(eng.D, max(SIZES), eng.A)
        a = _actions(rng, max(SIZES), eng.A, lb, ub)
        for hidden in NETS if name != "hc-bounds" else NETS[1:]:
            act = "tanh" if hidden else "relu"
            layers = gp._set(eng, hidden, act, squash, bound, x, seed=len(hidden))
            for space in lref.SPACES:
                full = _np(eng.policy_log_prob(x, a, space))
                for R in SIZES:
                    got = _np(eng.policy_log_prob(x[:R], a[:R], space))
                    _same(got, full[:R], "R = %d" % R)
                    worst = max(worst, _ratio(eng, layers, act, squash, bound, x[:R], a[:R], space, lb, ub, got=got))
            if squash == "none":
                _same(_np(eng.policy_log_prob(x, a, "pre_squash")), _np(eng.policy_log_prob(x, a, "action")), "no squash: the two spaces agree")
            else:
                assert not np.array_equal(_np(eng.policy_log_prob(x, a, "pre_squash")), _np(eng.policy_log_prob(x, a, "action")))
    print("\n[%s %s] worst |err| / bar: %.3f" % (squash, bound, worst))
    assert worst <= 1.0


def test_kernel_at_the_widest_net(kengines):
    """(512, 512): the activation regions alone are 64 KiB, the kernel's dynamic-LDS attribute is raised"""
    eng = kengines("hc")
    x, a = gp._states(eng.D, 33, 1), _actions(np.random.default_rng(2), 33, eng.A, -1.0, 1.0)
    layers = gp._set(eng, (512, 512), "relu", "tanh", "clamp", x, seed=3)
    worst = max(_ratio(eng, layers, "relu", "tanh", "clamp", x, a, space) for space in lref.SPACES)
    print("\n[512 x 2] worst |err| / bar: %.3f" % worst)
    assert worst <= 1.0


def _mild_actor(D, hidden, A, seed):
    """a SAC actor whose means are of order 0.5 and whose raw log-std lies around -1: most draws stay inside |u| <= 2"""
    layers = pref.he_policy(D, hidden, 2 * A, seed, 0.5)
    W, b = layers[-1]
    b = b.copy()
    b[A:] -= F(1.0)
    return list(layers[:-1]) + [(W, b)]


@pytest.mark.parametrize("bound", gref.BOUNDS)
def test_round_trip_through_the_sampler_per_element(kengines, bound):
    """On A = 1 a row is an element: `policy_log_prob(s, policy_sample(s)["act"])` is `policy_sample`'s logp under `lref.roundtrip_bars`
    on every element with |u| <= 2, and at most 10 % of the elements fall outside (u from the restatement on the sampler's own draws)."""
    eng = kengines("pend")
    R, seed, call, lo, hi = 257, 5, 9, -5.0, 2.0
    x = gp._states(eng.D, R, 4)
    layers = _mild_actor(eng.D, (50, 33), eng.A, 8)
    mean_layers, W_ls, b_ls = gref.split(layers, eng.A)
    eng.set_policy_net(HipEngine.policy_params((50, 33), "tanh", "tanh", 1, 0.0), mean_layers)
    eng.set_policy_head(gp._head(bound, lo, hi), W_ls, b_ls)
    smp = {k: _np(v) for k, v in eng.policy_sample(x, seed=seed, call=call).items()}
    z = gref.z64(x, layers, "tanh")
    s64 = gref.sample64(z, gref.xi(seed, call, np.arange(R), 0, eng.A), "tanh", bound, lo, hi)
    keep = np.abs(s64["u"][:, 0]) <= 2.0
    assert keep.mean() >= 0.9, "more than 10 %% of the elements fall outside |u| <= 2 (%.3f kept)" % keep.mean()
    back = _np(eng.policy_log_prob(x, smp["act"]))
    r64 = lref.logp64(z, smp["act"], "tanh", bound, lo, hi, y=lref.y32(smp["act"]))
    bar = lref.roundtrip_bars(z, r64, smp["act"], "tanh", bound, lo, hi)[:, 0]
    gap = np.abs(back.astype(np.float64) - smp["logp"].astype(np.float64))
    print("\n[round trip, A = 1, %s] kept %.3f of the elements, worst gap %.3g, worst gap / bar %.3f" % (bound, keep.mean(), gap[keep].max(),
                                                                                                      (gap / bar)[keep].max()))
    assert (gap[keep] <= bar[keep]).all()


# ---------------------------------------------------------------------------------------------------------------------- 2: batch independence
@pytest.mark.parametrize("hidden,act", [((50, 33), "swish"), ((), "relu"), ((128, 128), "relu")], ids=["50x33", "linear", "128x128"])
def test_a_row_has_the_same_bits_in_any_batch(engines, hidden, act):
    """`policy_log_prob(x[5:], a[5:])` is `policy_log_prob(x, a)[5:]`; the stage's step output is `policy_log_prob` of the inputs gathered
    from traj, obs and actions, bit for bit, at m n p = 30 rows per step (no multiple of 16: tiles straddle steps, envs and candidates);
    and inside a launch with more than 2 sixteen-row tiles per CU -- two row tiles per workgroup, these nets' tiles fit a CU four times
    -- where the candidates recur at other row positions: equal bits, and equal rows."""
    _, eng = engines("hopper")
    H, p, m, n = eng.H, eng.p, 2, 3
    layers = gp._set(eng, hidden, act, "tanh", "clamp", gp._states(eng.D, 64, 3), seed=21)
    traj, obs, actions = synth_traj(41, H, m, n, p, eng.D, eng.A)
    prm = HipEngine.policy_logp_params(0.5, "action")
    s, a = _gather(traj, obs, actions)
    flat_s, flat_a = s.reshape(-1, eng.D), a.reshape(-1, eng.A)
    full = _np(eng.policy_log_prob(flat_s, flat_a))
    assert full.shape == (H * 30,) and np.isfinite(full).all()
    _same(_np(eng.policy_log_prob(flat_s, flat_a)), full, "run to run")
    _same(_np(eng.policy_log_prob(flat_s[5:], flat_a[5:])), full[5:], "the batch cut by 5")
    rows = np.random.default_rng(1).standard_normal((m, n, p)).astype(F)
    out, steps, S = (_np(t) for t in eng.policy_logp_returns(traj, obs, actions, rows, prm, want_steps=True))
    _same(steps.reshape(-1), full, "the stage's step output")
    print("\n[stage %r] worst |err| / bar: %.3f" % (hidden, _ratio(eng, layers, act, "tanh", "clamp", flat_s, flat_a, "action", got=steps.reshape(-1))))
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    reps = (2 * cus * 16) // (H * m * n * p) + 2
    assert H * m * n * reps * p > 2 * cus * 16 + 16
    big_out, big, _ = eng.policy_logp_returns(np.tile(traj, (1, 1, reps, 1, 1)), obs, np.tile(actions, (1, reps, 1, 1)),
                                              np.tile(rows, (1, reps, 1)), prm, want_steps=True)
    big, big_out = _np(big).reshape(H, m, reps, n, p), _np(big_out).reshape(m, reps, n, p)
    for r in (0, 1, reps - 1):
        _same(big[:, :, r], steps, "two row tiles, copy %d of the candidates" % r)
        _same(big_out[:, r], out, "two row tiles, the rows of copy %d" % r)


# ---------------------------------------------------------------------------------------------------------------------- 3: the step sum, the row update
@pytest.mark.parametrize("weight", [1.0, -0.37, 0.0])
def test_step_sum_and_row_update(engines, weight):
    """S and rows_out from the kernel's own step output, replayed in numpy float32 bit for bit: without and with `first`, and under a
    discount over the horizon; rows_out aliasing rows_in and step_out / sum_out = NULL give the same rows; rows_in is not written."""
    _, eng = engines("hc5")
    gp._set(eng, (50, 33), "tanh", "tanh", "tanh", gp._states(eng.D, 64, 5), seed=5)
    prm = HipEngine.policy_logp_params(weight, "action")
    m, n = 3, 7
    traj, obs, actions = synth_traj(9, eng.H, m, n, eng.p, eng.D, eng.A)
    rows = (10.0 * np.random.default_rng(2).standard_normal((m, n, eng.p))).astype(F)
    first = np.random.default_rng(3).integers(0, eng.H + 1, (m, n, eng.p)).astype(np.int32)
    t_dev, o_dev, a_dev, r_dev = (eng._t(v) for v in (traj, obs, actions, rows))
    try:
        for gamma in (1.0, 0.9):
            eng.set_discount(gamma)
            disc = eng.discount_weights()
            assert (disc is None) == (gamma == 1.0)
            for f in (None, first):
                what = "gamma %g, first %s" % (gamma, f is not None)
                out, steps, S = (_np(t) for t in eng.policy_logp_returns(t_dev, o_dev, a_dev, r_dev, prm, first=f, want_steps=True))
                live = rref.counted(eng.H, (m, n, eng.p), f)
                assert np.isfinite(steps[live]).all() and np.isnan(steps[~live]).all(), what
                S_ref, out_ref = lref.step_sum32(steps, f, weight, rows, disc)
                _same(S, S_ref, what)
                _same(out, out_ref, what)
                _same(_np(r_dev), rows, "rows_in was written")
                _same(_np(eng.policy_logp_returns(t_dev, o_dev, a_dev, r_dev, prm, first=f)), out, what + ": step_out = sum_out = NULL")
                alias = r_dev.clone()
                assert eng.policy_logp_returns(t_dev, o_dev, a_dev, alias, prm, first=f, out=alias) is alias
                _same(_np(alias), out, what + ": rows_out aliasing rows_in")
                if weight == 0.0:
                    np.testing.assert_array_equal(out, rows)
                else:
                    assert not np.array_equal(_bits(out), _bits(rows))
    finally:
        eng.set_discount(1.0)


# ---------------------------------------------------------------------------------------------------------------------- 4: non-finite inputs, the first cut
def test_non_finite_inputs_and_the_first_cut(engines):
    """NaN and +-inf planted in traj, in obs of one env and in actions make exactly the steps that read them NaN (an infinite action too:
    the clamp would hide it), and exactly the rows that count such a step; no other step's bits move.  Steps behind `first` read NaN, are
    not summed, and NaN planted only there changes no row."""
    _, eng = engines("hopper")
    H, p, D, A = eng.H, eng.p, eng.D, eng.A
    gp._set(eng, (50, 33), "relu", "tanh", "clamp", gp._states(eng.D, 64, 6), seed=6)
    prm = HipEngine.policy_logp_params(2.0, "action")
    m, n = 3, 11
    traj, obs, actions = synth_traj(12, H, m, n, p, D, A)
    rows = np.random.default_rng(4).standard_normal((m, n, p)).astype(F)
    ref_out, ref_steps, ref_S = (_np(t) for t in eng.policy_logp_returns(traj, obs, actions, rows, prm, want_steps=True))
    assert np.isfinite(ref_steps).all()
    bad_t, bad_o, bad_a = traj.copy(), obs.copy(), actions.copy()
    hit = np.zeros((H, m, n, p), bool)
    bad_t[0, 0, 0, 0, 3] = np.nan                      # s_1 of the first row: the state of step 1 alone
    hit[1, 0, 0, 0] = True
    bad_t[H - 1, 2, n - 1, p - 1, D - 1] = -np.inf     # s_H: no step reads it
    bad_t[1, 1, 4, 2, 0] = np.inf                      # s_2: step 2
    hit[2, 1, 4, 2] = True
    bad_o[1, 5] = np.nan                               # obs of env 1: step 0 of every row of env 1
    hit[0, 1] = True
    bad_a[2, 3, 1, A - 1] = np.inf                     # a_1 of candidate (2, 3): step 1 of its p particles
    hit[1, 2, 3] = True
    bad_a[0, 5, 2, 0] = np.nan                         # a_2 of candidate (0, 5)
    hit[2, 0, 5] = True
    out, steps, S = (_np(t) for t in eng.policy_logp_returns(bad_t, bad_o, bad_a, rows, prm, want_steps=True))
    assert np.isnan(steps[hit]).all()
    _same(steps[~hit], ref_steps[~hit], "a step met its neighbour's poison")
    dead = hit.any(axis=0)
    assert dead.any() and (~dead).any() and np.isnan(S[dead]).all() and np.isnan(out[dead]).all()
    _same(S[~dead], ref_S[~dead])
    _same(out[~dead], ref_out[~dead])
    # the same through cadm_policy_logp
    s, a = _gather(bad_t, bad_o, bad_a)
    _same(_np(eng.policy_log_prob(s.reshape(-1, D), a.reshape(-1, A))), steps.reshape(-1), "cadm_policy_logp on the poisoned rows")
    # the first cut
    first = np.random.default_rng(13).integers(0, H + 1, (m, n, p)).astype(np.int32)
    first[0, 0, 0], first[0, 0, 1], first[0, 0, 2], first[0, 0, 3] = 0, H, H - 1, 1
    live = rref.counted(H, (m, n, p), first)
    out, steps, S = (_np(t) for t in eng.policy_logp_returns(traj, obs, actions, rows, prm, first=first, want_steps=True))
    assert np.isnan(steps[~live]).all() and (~live).any()
    _same(steps[live], ref_steps[live])
    _same(S, rref.step_sum(ref_steps, first))
    _same(out, rref.update(rows, rref.step_sum(ref_steps, first), 2.0))
    only = traj.copy()
    only[:-1][~live[1:]] = np.nan                      # s_t of every step that is not counted: no counted step reads it
    out2, steps2, S2 = (_np(t) for t in eng.policy_logp_returns(only, obs, actions, rows, prm, first=first, want_steps=True))
    assert np.isnan(only).any()
    _same(out2, out, "NaN in steps that are not counted reached a row")
    _same(steps2, steps)


# ---------------------------------------------------------------------------------------------------------------------- 5: fused against stepwise
def _check_iterations(eng, info, prob, prm, first_used):
    """every stepwise iteration: the rows behind the stage are the row update of the rows before it from the iteration's own step
    log-densities, which are `policy_log_prob`'s of the inputs gathered from the iteration's own trajectories and candidates"""
    for x in info:
        after = x["value_rows"] if "value_rows" in x else x["q_rows"] if "q_rows" in x else x["rows"]
        steps, S, before, rows = (_np(v) for v in (x["logp_steps"], x["logp_sum"], x["logp_rows"], after))
        first = _np(x["first_violation"]) if first_used else None
        _same(S, rref.step_sum(steps, first))
        _same(rows, rref.update(before, S, prm.weight))
        s, a = _gather(x["traj"], eng._t(prob["obs"]), x["actions"])
        flat = _np(eng.policy_log_prob(s, a, int(prm.space)))
        keep = rref.counted(eng.H, S.shape, first)
        _same(steps[keep], flat[keep])
        assert np.isnan(steps[~keep]).all()


COMBOS = ["alone", "terminate-tracking", "value-cvar", "actuator-uncertainty-mppi-knots"]


@pytest.mark.parametrize("combo", COMBOS)
def test_fused_equals_stepwise(engines, combo):
    """`cadm_anchored_plan` with device RNG == the same loop one launch at a time (`planner.icem_plan(..., policy_logp=)`), bit for bit
    over two consecutive calls: the plan, the best return, the carry (and the actuator state).  Under decay the packed candidate count
    changes per iteration."""
    from test_gpu_actuator import _params, _state
    from test_gpu_constraints import binding_bounds, iteration0_traj
    from test_gpu_tracking import _tracking_inputs
    from test_gpu_uncertainty import _prm as unc_prm
    prob, eng = engines("hc5-vanilla" if combo == "alone" else "hc5")
    H, A = eng.H, eng.A
    gp._set(eng, (50, 33), "tanh", "tanh", "clamp", np.asarray(prob["obs"], F), seed=31)
    logp = HipEngine.policy_logp_params(0.05, "pre_squash" if combo == "value-cvar" else "action")
    mppi = combo == "actuator-uncertainty-mppi-knots"
    K = 0 if combo == "alone" else 2
    icem = dict(noise_beta=1.0 if mppi else 0.0, keep_elites=K, decay=1.25 if K else 1.0, return_best=combo == "terminate-tracking",
                add_mean_last=K > 0)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if mppi else HipEngine.icem_params(**icem)
    score = HipEngine.score_params("cvar", k=2) if combo == "value-cvar" else None
    cons = track = targets = offset = act = unc = value = knots = None
    if combo == "terminate-tracking":
        track, targets, offset, _ = _tracking_inputs(eng, prob, 3, H, 13)
        cons = HipEngine.constraint_params(binding_bounds(iteration0_traj(eng, prob, 0.0, 4, 1), (1, 7), H, "anchored"), "terminate", 4.0)
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
        a, ra = eng.anchored_plan(logp, None, None, None, value, unc, act, pa, fa, True, track, targets, offset, knots, None, cons, score, prm,
                                  *args, mean, var, N, carry=ca, carry_valid=va, seed=4, call=call, want_best_return=True)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                            update="mppi" if mppi else "cem", temperature=0.5, relative=True, score=score, constraints=cons,
                                            knots=knots, tracking=None if track is None else (track, targets, offset),
                                            actuator=None if act is None else (act, pb, fb), action_advance=True, uncertainty=unc,
                                            value=value, policy_logp=logp, **icem)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
        _same(a, _np(b), "plan of call %d" % call)
        _same(_np(ra), _np(extra["best_ret"]), "best return of call %d" % call)
        for x, y in ((ca, cb), (pa, pb), (fa, fb)):
            if x is not None:
                _same(_np(x), _np(y))
        _check_iterations(eng, info, prob, logp, cons is not None)
        if K:
            assert len({int(x["rows"].shape[1]) for x in info}) > 1, "decay must change the packed candidate count"
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)
    # the term matters: without it, another plan
    other = _np(eng.anchored_plan(None, None, None, None, value, unc, act, pb, fb, False, track, targets, offset, knots, None, cons, score, prm,
                                  *args, mean, var, N, *zero_carry(eng, M, K, H), seed=4, call=2))
    assert not np.array_equal(_bits(other), _bits(a))
    assert (mppi, "anc", cons is not None, act is not None, unc is not None, 0) in eng._loop_ws


# ---------------------------------------------------------------------------------------------------------------------- 6: the no-ops
@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_no_term_is_the_loop_underneath(engines, update):
    """logp = NULL: the plan, the best return and the carry of `cadm_critic_plan` on the same inputs (here with a value net), bit for
    bit, through the C entry itself with that loop's workspace; and the workspace with the term is the critic loop's plus the step
    log-densities [H, m, n, p]."""
    prob, eng = engines("hc5")
    H, A = eng.H, eng.A
    value = HipEngine.value_params((32,), "relu", 2.0)
    eng.set_value_net(value, vref.he_net(eng.D, (32,), 33))
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    mppi, full = eng._as_mppi_params(prm)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    carry, valid = zero_carry(eng, M, 2, H)
    plan, best = eng.critic_plan(None, None, None, value, None, None, None, None, True, None, None, None, None, None, None, None, prm, *args,
                                 carry=carry, carry_valid=valid, seed=5, call=2, want_best_return=True)
    carry2, valid2 = zero_carry(eng, M, 2, H)
    t = [eng._t(x) for x in args[:5]]
    ws = eng._loop_workspace(mppi, M, N, 2, crt=(False, False, False, 0))
    out = torch.empty((M, H, A), dtype=torch.float32, device=eng.device)
    best2 = torch.empty((M,), dtype=torch.float32, device=eng.device)
    P = lambda x: ct.c_void_p(x.data_ptr())
    rc = eng.lib.cadm_anchored_plan(eng._ctx, None, None, None, None, ct.byref(value), None, None, None, None, 1, None, None, 0, None, None, None,
                                    None, None, int(mppi), ct.byref(full), *[P(x) for x in t], P(carry2), P(valid2), M, N, 5, 2, P(ws), P(out),
                                    P(best2), eng.stream)
    assert rc == 0, eng.lib.cadm_last_error().decode()
    for x, y in ((plan, out), (best, best2), (carry, carry2)):
        _same(_np(x), _np(y))
    lib = eng.lib
    step_bytes = (4 * H * M * N * eng.p + 255) & ~255
    for terminate in (0, 1):
        for act in (0, 1):
            for unc in (0, 1):
                for P_ in (0, 3):
                    flags = (eng._ctx, M, N, 2, int(mppi), terminate, act, unc, P_)
                    assert lib.cadm_anchored_workspace_bytes(*flags) == lib.cadm_critic_workspace_bytes(*flags) + step_bytes
    assert lib.cadm_policy_logp_workspace_bytes(eng._ctx, M, N) == 4 * H * M * N * eng.p
    assert lib.cadm_anchored_workspace_bytes(eng._ctx, 0, N, 2, 0, 0, 0, 0, 0) == 0


def test_a_zero_weight_changes_no_plan(engines):
    """weight = 0 multiplies a finite S to +-0.0: every row keeps its value, so the elite sets of every iteration, the plan and the
    carry are those of the loop without the term."""
    prob, eng = engines("hc5")
    gp._set(eng, (50, 33), "tanh", "tanh", "clamp", np.asarray(prob["obs"], F), seed=7)
    logp = HipEngine.policy_logp_params(0.0, "action")
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.0, return_best=False, add_mean_last=True)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    (ca, va), (cb, vb) = zero_carry(eng, M, 2, eng.H), zero_carry(eng, M, 2, eng.H)
    a, ia, _ = hplanner.icem_plan(eng, *args, carry=ca, carry_valid=va, seed=3, call=1, return_info=True, policy_logp=logp, **icem)
    b, ib, _ = hplanner.icem_plan(eng, *args, carry=cb, carry_valid=vb, seed=3, call=1, return_info=True, **icem)
    for x, y in zip(ia, ib):
        assert np.isfinite(_np(x["logp_sum"])).all()
        np.testing.assert_array_equal(_np(x["elites"]), _np(y["elites"]))
        assert (_np(x["rows"]) == _np(y["rows"])).all()
    _same(_np(a), _np(b))
    _same(_np(ca), _np(cb))
    fused = eng.anchored_plan(logp, None, None, None, None, None, None, None, None, True, None, None, None, None, None, None, None,
                              HipEngine.icem_params(**icem), *args, *zero_carry(eng, M, 2, eng.H), seed=3, call=1)
    _same(_np(fused), _np(b))


def test_the_default_model_is_untouched(gpu):
    """A model with cem_policy_logp=None gives `get_action` bit-identical to one without the kwarg, and launches no new entry point"""
    H, A = 5, 6
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    plans = []
    for kw in (dict(), dict(cem_policy_logp=None)):
        model, prob = plan_model(True, H, cem_keep_elites=2, **kw)
        plans.append(plan_act(model, prob, True, mean, var))
        assert model._opt.logp_params is None and not any("anc" in k for k in model.engine._loop_ws)
    _same(plans[0], plans[1])


# ---------------------------------------------------------------------------------------------------------------------- 7: the direction
def test_the_term_pulls_the_plan_towards_the_actor(engines):
    """A linear actor with a zero output layer and bias b has the constant mode c = tanh(b) and, from a zero log-std layer with bias
    log 0.2, sigma = 0.2.  With weight 100 the first-step a[0] of the plan under c = +0.5 exceeds that under c = -0.5 in every env.
    Cannot pass without the term."""
    prob, eng = engines("hc5")
    D, A = eng.D, eng.A
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    logp = HipEngine.policy_logp_params(100.0, "action")
    plans = {}
    for name, c in (("up", 0.5), ("down", -0.5)):
        b = np.full((A,), math.atanh(c), F)
        eng.set_policy_net(HipEngine.policy_params((), "relu", "tanh", 1, 0.0), [(np.zeros((D, A), F), b)])
        eng.set_policy_head(gp._head("clamp"), np.zeros((D, A), F), np.full((A,), math.log(0.2), F))
        np.testing.assert_allclose(_np(eng.policy_eval(np.asarray(prob["obs"], F))), c, atol=1e-6)
        plans[name] = _np(eng.anchored_plan(logp, None, None, None, None, None, None, None, None, True, None, None, None, None, None, None,
                                            None, HipEngine.icem_params(), *args, seed=6, call=1))
        assert np.isfinite(plans[name]).all()
    print("\n[direction] first-step a[0]: down %s  up %s" % (plans["down"][:, 0, 0], plans["up"][:, 0, 0]))
    assert (plans["up"][:, 0, 0] > plans["down"][:, 0, 0]).all()


# ---------------------------------------------------------------------------------------------------------------------- 8: the class route
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_class_route(gpu, context):
    """`get_action`, `policy_log_prob` and `plan_policy_log_prob` agree with the engine calls; the density of `policy_sample`'s own actions
    is its `logp` under the round-trip bar; without the actor or its head the calls are refused."""
    H, A, D = 5, 6, 18
    hidden, act = (50, 33), "tanh"
    actor = dict(hidden_sizes=hidden, activation=act, squash="tanh")
    head = dict(kind="gaussian", log_std_bounds=(LO, HI))
    model, prob = plan_model(context, H, cem_policy_logp=dict(weight=0.05, policy=actor), policy_head=head, cem_keep_elites=2)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    with pytest.raises(RuntimeError, match="no policy net"):
        plan_act(model, prob, context, mean, var)
    assert model._call == 0
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4, 7, D)).astype(F)
    stats = (rng.standard_normal(D).astype(F), rng.uniform(0.5, 2.0, D).astype(F))
    layers = gref.actor(D, hidden, A, act, x.reshape(-1, D), LO, HI, seed=17, mean=stats[0], std=stats[1])
    model.set_policy(layers, *stats)
    plan = plan_act(model, prob, context, mean, var)
    assert np.isfinite(plan).all() and model._call == 1
    eng, opt = model.engine, model._opt
    hist = (prob["cp_obs"], prob["cp_act"]) if context else (None, None)
    carry, valid = zero_carry(eng, M, 2, H)
    direct = eng.anchored_plan(opt.logp_params, None, None, None, None, None, None, None, None, True, None, None, None, None, None, None, None,
                               opt.params, prob["obs"], *hist, mean, var, model.n_candidates, carry=carry, carry_valid=valid, seed=model.seed,
                               call=1)
    _same(plan, _np(direct))
    _same(_np(model._plan_carry), _np(carry))
    # the density of given actions, through the class
    a = _actions(rng, 28, A, -1.0, 1.0).reshape(4, 7, A)
    lp = model.policy_log_prob(x, a)
    assert lp.shape == (4, 7)
    _same(lp, _np(eng.policy_log_prob(x, a)))
    z = gref.z64(x.reshape(-1, D), layers, act, *stats)
    ref = lref.logp64(z, a.reshape(-1, A), "tanh", "clamp", LO, HI, y=lref.y32(a.reshape(-1, A)))
    worst = float((np.abs(lp.reshape(-1).astype(np.float64) - ref["logp"]) / lref.bars(z, ref, "tanh", "clamp", LO, HI)).max())
    assert worst <= 1.0
    assert not np.array_equal(model.policy_log_prob(x, a, space="pre_squash"), lp)
    # the round trip: log pi of the sampler's own actions is the sampler's logp, on the rows whose elements all have |u| <= 2
    xs = rng.standard_normal((257, D)).astype(F)
    smp = model.policy_sample(xs, seed=3)
    zs = gref.z64(xs, layers, act, *stats)
    e = gref.xi(3, 0, np.arange(257), 0, A)
    s64 = gref.sample64(zs, e, "tanh", "clamp", LO, HI)
    back = model.policy_log_prob(xs, smp["act"])
    r64 = lref.logp64(zs, smp["act"], "tanh", "clamp", LO, HI, y=lref.y32(smp["act"]))
    keep = (np.abs(s64["u"]) <= 2.0).all(axis=-1)
    bar = lref.roundtrip_bars(zs, r64, smp["act"], "tanh", "clamp", LO, HI).sum(axis=-1) + 2e-5 * np.maximum(1.0, np.abs(smp["logp"]))
    gap = np.abs(back.astype(np.float64) - smp["logp"].astype(np.float64))
    print("\n[round trip] kept %d of 257 rows, worst gap %.3g, worst gap / bar %.3f (class route worst |err| / bar %.3f)"
          % (keep.sum(), gap[keep].max(), (gap / bar)[keep].max(), worst))
    assert keep.sum() >= 64 and (gap[keep] <= bar[keep]).all()
    # the companion, against the engine's stage on the trajectories the same rollout records
    res = model.plan_policy_log_prob(prob["obs"], plan, *(hist if context else ()))
    assert res["logp"].shape == (M, 5, H) and res["total"].shape == (M, 5) and res["first"] is None and model._call == 1
    ctx_vec = eng.context_forward(*hist) if context else None
    acts = eng._t(plan)[:, None].contiguous()
    rows, traj = eng.rollout_returns(eng._t(prob["obs"]), ctx_vec, acts, seed=model.seed, call=1, it=hplanner.FORECAST_IT, want_traj=True)
    _, steps, S = eng.policy_logp_returns(traj, eng._t(prob["obs"]), acts, rows, opt.logp_params, want_steps=True)
    _same(np.moveaxis(res["logp"], -1, 0), _np(steps)[:, :, 0])
    _same(res["total"], _np(S)[:, 0])
    # the lifecycle: the library drops the head with every set_policy_net; set_policy brings both back; clear_policy refuses
    mean_layers, _, _ = gref.split(layers, A)
    eng.set_policy_net(opt.actor_params(), mean_layers, *stats)
    with pytest.raises(_lib.CadmError, match=r"code -4.*no Gaussian head"):
        eng.policy_log_prob(x, a)
    with pytest.raises(_lib.CadmError, match=r"code -4.*no Gaussian head"):
        eng.policy_logp_returns(traj, eng._t(prob["obs"]), acts, rows, opt.logp_params)
    model.set_policy(layers, *stats)
    _same(model.policy_log_prob(x, a), lp)
    model.clear_policy()
    with pytest.raises(RuntimeError, match="no policy net"):
        model.policy_log_prob(x, a)
    with pytest.raises(RuntimeError, match="no policy net"):
        plan_act(model, prob, context, mean, var)
    with pytest.raises(_lib.CadmError, match=r"code -4.*no policy net"):
        eng.policy_log_prob(x, a)
    # a model with a head and no term evaluates densities too; one without an actor refuses
    other, _ = plan_model(context, H, imagine_policy=actor, policy_head=head)
    other.set_policy(layers, *stats)
    _same(other.policy_log_prob(x, a), lp)
    with pytest.raises(ValueError, match="no cem_policy_logp"):
        other.plan_policy_log_prob(prob["obs"], plan, *(hist if context else ()))
    plain, _ = plan_model(context, H, cem_noise_beta=1.0)
    with pytest.raises(ValueError, match="no cem_policy_prior"):
        plain.policy_log_prob(x, a)
    with pytest.raises(ValueError, match="declare policy_head"):
        plan_model(context, H, cem_policy_logp=dict(policy=actor))
    with pytest.raises(ValueError, match="below -10"):
        plan_model(context, H, cem_policy_logp=dict(policy=actor), policy_head=dict(log_std_bounds=(-11.0, 2.0)))


def test_argument_checks_return_einval(engines):
    """The C entries refuse bad arguments with CADM_EINVAL (no net, no head: CADM_ESTATE) and a message that names them, before any HIP
    call (the dummy pointers are never touched); the engine evaluates normally afterwards."""
    prob, eng = engines("hc5")
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(8192, dtype=torch.float32, device=eng.device)
    P = ct.c_void_p(buf.data_ptr())
    mp = HipEngine.mppi_params()
    x = gp._states(eng.D, 33, 1)
    layers = gp._set(eng, (50, 33), "tanh", "tanh", "clamp", x, seed=1)

    def V(weight=1.0, space=0):
        v = _lib.PolicyLogpParams()
        v.weight, v.space = weight, space
        return ct.byref(v)

    def returns(v, c=ctx, traj=P, obs=P, actions=P, rows_out=P, step=P, ws=None, m=M):
        return lib.cadm_policy_logp_returns(c, v, traj, obs, actions, None, m, 4, P, rows_out, step, None, ws, None)

    def plan(v, c=ctx, update=0, prm=ct.byref(mp)):
        return lib.cadm_anchored_plan(c, v, None, None, None, None, None, None, None, None, 1, None, None, 0, None, None, None, None, None, update,
                                      prm, P, P, P, P, P, None, None, M, N, 0, 1, P, P, None, None)

    def refused(rc, name, frag, code=-1):
        msg = lib.cadm_last_error().decode()
        assert rc == code, "%s: expected %d, got %d (%s)" % (name, code, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    for name, fn in (("cadm_policy_logp_returns", returns), ("cadm_anchored_plan", plan)):
        refused(fn(V(space=2)), name, "space")
        refused(fn(V(space=-1)), name, "space")
        for bad in (NAN, math.inf, -math.inf):
            refused(fn(V(weight=bad)), name, "weight")
    refused(returns(None), "cadm_policy_logp_returns", "null")
    for kw in (dict(traj=None), dict(obs=None), dict(actions=None), dict(rows_out=None)):
        refused(returns(V(), **kw), "cadm_policy_logp_returns", "null")
    refused(returns(V(), step=None, ws=None), "cadm_policy_logp_returns", "workspace")
    refused(returns(V(), m=0), "cadm_policy_logp_returns", "m, n must be")
    refused(lib.cadm_policy_logp(ctx, None, P, 4, 0, P, None), "cadm_policy_logp", "null")
    refused(lib.cadm_policy_logp(ctx, P, None, 4, 0, P, None), "cadm_policy_logp", "null")
    refused(lib.cadm_policy_logp(ctx, P, P, 4, 0, None, None), "cadm_policy_logp", "null")
    refused(lib.cadm_policy_logp(ctx, P, P, 0, 0, P, None), "cadm_policy_logp", "R must be")
    refused(lib.cadm_policy_logp(ctx, P, P, 4, 2, P, None), "cadm_policy_logp", "space")
    refused(plan(V(), update=2), "cadm_anchored_plan", "update")
    refused(plan(V(), prm=None), "cadm_anchored_plan", "bad arguments")
    # a head whose log-std reaches below -10: exp(-ls) would leave the margin
    mean_layers, W_ls, b_ls = gref.split(layers, eng.A)
    eng.set_policy_head(gp._head("clamp", -11.0, 0.5), W_ls, b_ls)
    refused(lib.cadm_policy_logp(ctx, P, P, 4, 0, P, None), "cadm_policy_logp", "below -10")
    refused(returns(V()), "cadm_policy_logp_returns", "below -10")
    refused(plan(V()), "cadm_anchored_plan", "below -10")
    eng.set_policy_head(gp._head("clamp", -10.0, 0.5), W_ls, b_ls)
    assert np.isfinite(_np(eng.policy_log_prob(x, np.zeros((33, eng.A), F)))).all()
    # no head, then no net
    calls = ((lambda: lib.cadm_policy_logp(ctx, P, P, 4, 0, P, None), "cadm_policy_logp"), (lambda: returns(V()), "cadm_policy_logp_returns"),
             (lambda: plan(V()), "cadm_anchored_plan"))
    eng.set_policy_head(None)
    for fn, name in calls:      # (one at a time: the message is the last refusal's)
        refused(fn(), name, "no Gaussian head", code=-4)
    eng.set_policy_net(None)
    for fn, name in calls:      # (one at a time: the message is the last refusal's)
        refused(fn(), name, "no policy net", code=-4)
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=M, H=5, seed=1)
    deng = make_engine(dprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    refused(plan(V(), c=deng._ctx), "cadm_anchored_plan", "continuous actions only")
    deng.close()
    assert (_np(buf) == 0).all()
    # python: shapes that do not fit the engine
    layers = gp._set(eng, (50, 33), "tanh", "tanh", "clamp", x, seed=1)
    z = lambda *s: np.zeros(s, F)
    prm = HipEngine.policy_logp_params()
    good = (z(eng.H, M, 4, eng.p, eng.D), z(M, eng.D), z(M, 4, eng.H, eng.A), z(M, 4, eng.p))
    with pytest.raises(ValueError, match="policy_logp_returns: traj"):
        eng.policy_logp_returns(z(eng.H, M, 4, eng.p, eng.D + 1), *good[1:], prm)
    with pytest.raises(ValueError, match="policy_logp_returns: obs"):
        eng.policy_logp_returns(good[0], z(M + 1, eng.D), *good[2:], prm)
    with pytest.raises(ValueError, match="policy_logp_returns: actions"):
        eng.policy_logp_returns(*good[:2], z(M, 4, eng.H + 1, eng.A), good[3], prm)
    with pytest.raises(ValueError, match="policy_log_prob: actions"):
        eng.policy_log_prob(z(4, eng.D), z(5, eng.A))
    with pytest.raises(ValueError, match="space must be"):
        eng.policy_log_prob(z(4, eng.D), z(4, eng.A), "latent")
    out = _np(eng.anchored_plan(prm, None, None, None, None, None, None, None, None, True, None, None, None, None, None, None, None,
                                HipEngine.icem_params(), prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N,
                                seed=1, call=1))
    assert np.isfinite(out).all() and np.abs(out).max() <= 1.0
