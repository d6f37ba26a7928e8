"""GPU: the actuator model of the opt-in planner -- the kernel (`cadm_actuate_actions`, csrc/actuator.hip) against the numpy restatement
(tests/actuator_ref.py), the fused loop (`cadm_actuated_plan`) against the stepwise one, pins and rate limits on every returned plan
through the class route, episode time, `action_cost`, and the refusals.

Geometries: those tests/test_gpu_tracking.py builds -- the compiled-in halfcheetah kernel (H = 5, p = 5, A = 6) with and without context
and hopper_like (H = 3, A = 3); the class route on tests/helpers.py's `plan_model`.

The actuated sequences are compared bit for bit.  Bound of the cost against the float64 restatement, derived, not measured
(`actuator_ref.bound`): |cost - ref| <= 2 (H + A + 2) 2^-24 ref -- one rounding each for the difference, the square and the product of a
term, one per add of a dim's chain (H) and of the dims (A - 1); doubled for slack.  tests/test_actuator_ref.py holds a float32 emulation
of the chain to it on the CPU.
Measured on an MI355X, worst |err| / bound of the cost: 0.12 at A = 6, H = 5; 0.18 at A = 3, H = 3."""
import ctypes as ct
import math

import numpy as np
import pytest
import torch

import actuator_ref as aref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import _np, make_engine, plan_act, plan_model, zero_carry
from test_gpu_tracking import ITERS, KE, M, N, engines  # noqa: F401  (the module-scoped engine fixture)

pytestmark = pytest.mark.gpu
F = np.float32
NAN = float("nan")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _params(eng, d, dl, w):
    return HipEngine.actuator_params(d, dl, w, action_dim=eng.A, horizon=eng.H)


# ---------------------------------------------------------------------------------------------------------------------- 1: the kernel
KERNEL = [(e, m, n) for e in ("hc5", "hopper") for (m, n) in ((2, 24), (4, 7), (4, 1), (3, 100))]


@pytest.mark.parametrize("name,m,n", KERNEL, ids=["%s-m%d-n%d" % c for c in KERNEL])
def test_kernel_against_restatement(engines, name, m, n):
    """`cadm_actuate_actions` against tests/actuator_ref.py for d in {0, 1, H - 1}: the sequences bit for bit, the cost within the
    derived bound.  Limits finite on even dims and +inf on odd ones, weights zero on every third dim, a prefix with scattered NaNs, the
    last env's prev all NaN, env 0's prev outside the box (the box wins).  2 x 24 x 6 = 288 chains end in a partial workgroup (42
    candidates each at A = 6), 3 x 100 candidates span workgroups and envs inside one, n = 1 is the plan's own pass.  A second pass
    changes no bit; inert parameters copy their input and cost 0; the [m,H,A] form is the n = 1 form."""
    _, eng = engines(name)
    check_kernel(eng, name, m, n)


def check_kernel(eng, name, m, n, make_case=aref.make_case):
    """The body of `test_kernel_against_restatement` on any engine; `make_case`: `actuator_ref.make_case`, or a function of its
    arguments (where its weights would all be zero).  Returns the worst |err| / bound of the cost."""
    H, A = eng.H, eng.A
    worst = 0.0
    for d in (0, 1, H - 1):
        seqs, dl, w, prev, prefix = make_case(m, n, H, A, d, seed=10 * m + n + d, nan_env=m - 1, outside=True)
        ref, cost_ref, S = aref.actuate(seqs, d, dl, w, prev, prefix, eng.cfg.lower_bound, eng.cfg.upper_bound)
        prm = _params(eng, d, dl, w)
        dev = eng._t(seqs).clone()
        out, cost = eng.actuate_actions(dev, prm, prev=prev, prefix=prefix if d else None, want_cost=True)
        assert out is dev and tuple(cost.shape) == (m, n)
        what = "%s m=%d n=%d d=%d" % (name, m, n, d)
        np.testing.assert_array_equal(_bits(_np(out)), _bits(ref), err_msg=what + ": sequences")
        assert (np.abs(ref[0][:, :, np.isfinite(dl)]) <= 1.0).all() or d > 0      # env 0: prev outside the box, the box wins
        err, lim = np.abs(_np(cost).astype(np.float64) - cost_ref), aref.bound(S, H, A)
        assert np.isfinite(_np(cost)).all() and (cost_ref > 0).all()
        assert (err <= lim).all(), "%s: cost, worst |err| / bound %.3f" % (what, (err / lim).max())
        worst = max(worst, float((err / lim).max()))
        again, cost2 = eng.actuate_actions(dev.clone(), prm, prev=prev, prefix=prefix if d else None, want_cost=True)
        np.testing.assert_array_equal(_bits(_np(again)), _bits(ref), err_msg=what + ": a second pass")
        np.testing.assert_array_equal(_bits(_np(cost2)), _bits(_np(cost)), err_msg=what + ": the cost of feasible sequences")
        nocost = eng.actuate_actions(eng._t(seqs).clone(), prm, prev=prev, prefix=prefix if d else None)
        np.testing.assert_array_equal(_bits(_np(nocost)), _bits(ref), err_msg=what + ": without cost_out")
        # prev / prefix None: nothing known, nothing committed -- step 0 is free, the rest is limited against it
        free, cfree = eng.actuate_actions(eng._t(seqs).clone(), prm, want_cost=True)
        rfree, rcost, rS = aref.actuate(seqs, d, dl, w, None, None)
        np.testing.assert_array_equal(_bits(_np(free)), _bits(rfree), err_msg=what + ": prev / prefix None")
        assert (np.abs(_np(cfree) - rcost) <= aref.bound(rS, H, A)).all()
    print("\n[%s m=%d n=%d] cost: worst |err| / bound %.3f" % (name, m, n, worst))
    seqs[0, 0, 0, 0] = -0.0
    inert = HipEngine.actuator_params(0, None, None)
    out, cost = eng.actuate_actions(eng._t(seqs).clone(), inert, prev=prev, want_cost=True)
    np.testing.assert_array_equal(_bits(_np(out)), _bits(seqs), err_msg="inert parameters")
    assert (_np(cost) == 0).all()
    if n == 1:
        flat, c1 = eng.actuate_actions(eng._t(seqs[:, 0]).clone(), prm, prev=prev, prefix=prefix, want_cost=True)
        assert tuple(flat.shape) == (m, H, A) and tuple(c1.shape) == (m,)
        np.testing.assert_array_equal(_bits(_np(flat)), _bits(ref[:, 0]))
    return worst


# ---------------------------------------------------------------------------------------------------------------------- 2: the loop
def _state(eng, d, seed):
    """(prev [M,A], prefix [M,d,A]) on the device: env 0 known with one free committed element, env 1's prev unknown"""
    rng = np.random.default_rng(seed)
    prev = rng.uniform(-0.8, 0.8, (M, eng.A)).astype(F)
    prev[1] = np.nan
    prefix = rng.uniform(-1, 1, (M, d, eng.A)).astype(F)
    if d:
        prefix[0, 0, 1] = np.nan
    return eng._t(prev).clone(), eng._t(prefix).clone()


def _check_iterations(eng, info, d, dl, w, before):
    """every stepwise iteration: the score behind the actuator's subtraction (`cand`, or `unc_score` where an uncertainty term follows)
    is float32(score - cost) bit for bit, the candidates are feasible against the state `before` = (prev, prefix) the call started
    from (a second pass changes nothing), and the cost is the restatement's within the bound"""
    for x in info:
        acts, cost, score, cand = _np(x["actions"]), _np(x["action_cost"]), _np(x["score"]), _np(x["unc_score" if "unc_score" in x else "cand"])
        np.testing.assert_array_equal(_bits(cand), _bits((score - cost).astype(F)))
        ref, cost_ref, S = aref.actuate(acts, d, dl, w, before[0], before[1], eng.cfg.lower_bound, eng.cfg.upper_bound)
        np.testing.assert_array_equal(_bits(ref), _bits(acts), err_msg="an iteration's candidates are not feasible")
        assert (np.abs(cost - cost_ref) <= aref.bound(S, eng.H, eng.A)).all() and (cost_ref[0] > 0).all()


LOOP = [("hc5-vanilla", "cem", False, 0, 1, 1), ("hc5", "cem", True, 2, 1, 2), ("hc5", "mppi", False, 2, 2, 4), ("hc5-vanilla", "mppi", True, 0, 1, 0),
        ("hopper", "cem", False, 2, 1, 2), ("hopper", "mppi", True, 2, 2, 1)]


@pytest.mark.parametrize("name,update,best,K,r,d", LOOP, ids=["%s-%s-%s-K%d-r%d-d%d" % (e, u, "best" if b else "mean", K, r, d) for e, u, b, K, r, d in LOOP])
def test_fused_equals_stepwise(engines, name, update, best, K, r, d):
    """`cadm_actuated_plan` with device RNG == the same loop one launch at a time (`planner.icem_plan(..., actuator=...)`), bit for bit
    over two consecutive calls: the plan, the best return, the carry and the actuator state it leaves.  In every stepwise iteration
    `cand` is float32(score - cost) bit for bit, the candidates are feasible (a second pass changes nothing), and the cost is the
    restatement's within the bound.  The plan obeys pins and windows exactly."""
    prob, eng = engines(name)
    H, A = eng.H, eng.A
    d = min(d, H - 1)
    rng = np.random.default_rng(3)
    dl = np.where(np.arange(A) % 2 == 0, 0.3, np.inf).astype(F)
    w = np.where(np.arange(A) % 3 == 0, 0.0, rng.uniform(0.5, 4.0, A)).astype(F)
    act = _params(eng, d, dl, w)
    knots = HipEngine.knot_params(r, "hold") if r > 1 else None
    phase = torch.tensor([0, 1], dtype=torch.int32, device=eng.device) if r > 1 else None
    icem = dict(noise_beta=1.0 if update == "mppi" else 0.0, keep_elites=K, decay=1.0, return_best=best, add_mean_last=K > 0)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    (ca, va), (cb, vb) = zero_carry(eng, M, K, H), zero_carry(eng, M, K, H)
    (pa, fa), (pb, fb) = _state(eng, d, 5), _state(eng, d, 5)
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2):
        before = (_np(pa).copy(), _np(fa).copy())
        a, ra = eng.actuated_plan(act, pa, fa, True, None, None, None, knots, phase, None, None, prm, *args, mean, var, N, carry=ca, carry_valid=va,
                                  seed=4, call=call, want_best_return=True)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                            update=update, temperature=0.5, relative=True, knots=knots, phase=phase, actuator=(act, pb, fb),
                                            action_advance=True, **icem)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max()
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        if K:
            np.testing.assert_array_equal(_bits(_np(ca)), _bits(_np(cb)), err_msg="carry after call %d" % call)
        np.testing.assert_array_equal(_bits(_np(pa)), _bits(_np(pb)), err_msg="prev after call %d" % call)
        np.testing.assert_array_equal(_bits(_np(fa)), _bits(_np(fb)), err_msg="prefix after call %d" % call)
        np.testing.assert_array_equal(_bits(_np(pa)), _bits(a[:, 0]))
        np.testing.assert_array_equal(_bits(_np(fa)), _bits(a[:, 1:1 + d]))
        # the plan against the state it was planned from
        pinned = np.zeros((M, H, A), bool)
        pinned[:, :d] = ~np.isnan(before[1])
        np.testing.assert_array_equal(_bits(a[:, :d][pinned[:, :d]]), _bits(before[1][pinned[:, :d]]), err_msg="pins of call %d" % call)
        assert aref.window_ok(a, dl, before[0], eng.cfg.lower_bound, eng.cfg.upper_bound, free=~pinned).all(), "windows of call %d" % call
        if best:      # the last pass over the best sequence is a bitwise no-op
            np.testing.assert_array_equal(_bits(a), _bits(_np(extra["best_seq"])))
        _check_iterations(eng, info, d, dl, w, before)
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)      # the samplers' warm start
    # the model matters: without it, another plan
    other = _np(eng.tracking_plan(None, None, None, knots, phase, None, None, prm, *args, mean, var, N, *zero_carry(eng, M, K, H), seed=4, call=2))
    assert not np.array_equal(_bits(other), _bits(a))
    assert (update == "mppi", False, "act") in eng._loop_ws      # the actuated slot: no trajectory view without constraints or terms


@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_no_params_is_the_loop_underneath(engines, update):
    """params = NULL: the plan, the best return and the carry of `cadm_tracking_plan` on the same inputs, bit for bit, through the C
    entry itself with that loop's workspace; and the actuated workspace is the loop underneath's plus the cost and the plan copy."""
    prob, eng = engines("hc5")
    H, A = eng.H, eng.A
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    mppi, full = eng._as_mppi_params(prm)
    knots, phase = HipEngine.knot_params(2, "hold"), torch.tensor([1, 0], dtype=torch.int32, device=eng.device)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    carry, valid = zero_carry(eng, M, 2, H)
    plan, best = eng.tracking_plan(None, None, None, knots, phase, None, None, prm, *args, carry=carry, carry_valid=valid, seed=5, call=2,
                                   want_best_return=True)
    carry2, valid2 = zero_carry(eng, M, 2, H)
    t = [eng._t(x) for x in args[:5]]
    ws = eng._loop_workspace(mppi, M, N, 2)
    out = torch.empty((M, H, A), dtype=torch.float32, device=eng.device)
    best2 = torch.empty((M,), dtype=torch.float32, device=eng.device)
    P = lambda x: ct.c_void_p(x.data_ptr())
    rc = eng.lib.cadm_actuated_plan(eng._ctx, None, None, None, 1, None, None, 0, None, ct.byref(knots), P(phase), None, None, int(mppi),
                                    ct.byref(full), *[P(x) for x in t], P(carry2), P(valid2), M, N, 5, 2, P(ws), P(out), P(best2), eng.stream)
    assert rc == 0, eng.lib.cadm_last_error().decode()
    for x, y in ((plan, out), (best, best2), (carry, carry2)):
        np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))
    same = _np(eng.actuated_plan(None, None, None, True, None, None, None, knots, phase, None, None, prm, *args, *zero_carry(eng, M, 2, H), seed=5, call=2))
    np.testing.assert_array_equal(_bits(same), _bits(_np(plan)))
    pad = lambda nbytes: (nbytes + 255) & ~255
    more = pad(M * N * 4) + pad(M * H * A * 4)
    lib = eng.lib
    assert lib.cadm_actuated_workspace_bytes(eng._ctx, M, N, 2, int(mppi), 0, 0) == \
        (lib.cadm_mppi_workspace_bytes if mppi else lib.cadm_icem_workspace_bytes)(eng._ctx, M, N, 2) + more
    assert lib.cadm_actuated_workspace_bytes(eng._ctx, M, N, 2, int(mppi), 1, 0) == lib.cadm_constrained_workspace_bytes(eng._ctx, M, N, 2, int(mppi)) + more
    assert lib.cadm_actuated_workspace_bytes(eng._ctx, M, N, 2, int(mppi), 1, 1) == lib.cadm_tracking_workspace_bytes(eng._ctx, M, N, 2, int(mppi), 1) + more
    assert lib.cadm_actuated_workspace_bytes(eng._ctx, 0, N, 2, 0, 0, 0) == 0


def test_with_tracking_and_constraints_on(engines):
    """The actuator model under TERMINATE constraints, tracking terms, a CVaR score, knots and kept elites: fused == stepwise bit for bit,
    and the cost comes off the candidate score, not off the particle rows (the rows are the tracked rows)."""
    from test_gpu_constraints import binding_bounds, iteration0_traj
    from test_gpu_tracking import _tracking_inputs
    prob, eng = engines("hc5")
    H, A, d = eng.H, eng.A, 1
    track, targets, offset, _ = _tracking_inputs(eng, prob, 3, H, 13)
    cp = HipEngine.constraint_params(binding_bounds(iteration0_traj(eng, prob, 1.0, 4, 1), (1, 7), H, "actuated"), "terminate", 4.0)
    score, knots = HipEngine.score_params("cvar", k=2), HipEngine.knot_params(2, "linear")
    phase = torch.tensor([0, 1], dtype=torch.int32, device=eng.device)
    act = _params(eng, d, 0.4, 2.0)
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, return_best=False, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    (ca, va), (cb, vb) = zero_carry(eng, M, 2, H), zero_carry(eng, M, 2, H)
    (pa, fa), (pb, fb) = _state(eng, d, 8), _state(eng, d, 8)
    a, ra = eng.actuated_plan(act, pa, fa, True, track, targets, offset, knots, phase, cp, score, prm, *args, carry=ca, carry_valid=va, seed=4, call=1,
                              want_best_return=True)
    b, info, extra = hplanner.icem_plan(eng, *args, carry=cb, carry_valid=vb, seed=4, call=1, return_info=True, update="mppi", temperature=0.5,
                                        relative=True, score=score, constraints=cp, knots=knots, phase=phase, tracking=(track, targets, offset),
                                        actuator=(act, pb, fb), action_advance=True, **icem)
    for x, y in ((a, b), (ra, extra["best_ret"]), (ca, cb), (pa, pb), (fa, fb)):
        np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))
    for x in info:
        np.testing.assert_array_equal(_bits(_np(x["rows"])), _bits(_np(x["rows_untracked"]) - _np(x["track_cost"])))
        np.testing.assert_array_equal(_bits(_np(x["score"])), _bits(_np(eng.particle_score(x["rows"], score))))
        np.testing.assert_array_equal(_bits(_np(x["cand"])), _bits(_np(x["score"]) - _np(x["action_cost"])))
    assert (True, "track", True, "act") in eng._loop_ws


# ---------------------------------------------------------------------------------------------------------------------- 3: the class route
ROUTES = [(False, dict()), (True, dict(cem_update="mppi", cem_temperature=0.5, cem_temperature_relative=True, cem_noise_beta=1.0)),
          (True, dict(cem_return="best", cem_keep_elites=2)), (False, dict(cem_knots=2, cem_keep_elites=2, cem_add_mean=True))]


@pytest.mark.parametrize("context,other", ROUTES, ids=["elite", "mppi", "best", "knots"])
def test_returned_plans_obey_pins_and_limits(gpu, context, other):
    """Every plan `get_action` returns (a pinned host buffer: the last pass runs on the device copy) carries the committed values bit for
    bit and passes the float32 window check at every step, step 0 against `prev` included -- under the elite refit, MPPI and
    cem_return="best" -- over three calls, the state moving on in between."""
    H, A, d = 5, 6, 2
    dl = [0.15, 0.3, math.inf, 0.05, 0.6, 0.2]
    model, prob = plan_model(context, H, cem_action_delay=d, cem_action_rate_limit=dl, cem_action_rate_cost=0.05, **other)
    assert model._opt.actuator_params.delay == d and model.actuator_state() is None
    rng = np.random.default_rng(12)
    prev = rng.uniform(-0.9, 0.9, (M, A)).astype(F)
    committed = rng.uniform(-1, 1, (M, d, A)).astype(F)
    committed[1, 1, 2:4] = np.nan
    model.set_applied_actions(prev=prev, committed=committed)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    for call in range(3):
        st = model.actuator_state()
        plan = plan_act(model, prob, context, mean, var)
        assert plan.shape == (M, H, A) and np.isfinite(plan).all()
        pinned = np.zeros((M, H, A), bool)
        pinned[:, :d] = ~np.isnan(st["committed"])
        assert pinned[0, :d].all()
        np.testing.assert_array_equal(_bits(plan[:, :d][pinned[:, :d]]), _bits(st["committed"][pinned[:, :d]]), err_msg="pins of call %d" % call)
        ok = aref.window_ok(plan, dl, st["prev"], free=~pinned)
        assert ok.all(), "call %d: %d steps outside their float32 window" % (call, (~ok).sum())
        assert (np.abs(plan[~pinned]) <= 1.0).all()
        after = model.actuator_state()
        np.testing.assert_array_equal(_bits(after["prev"]), _bits(plan[:, 0]))
        np.testing.assert_array_equal(_bits(after["committed"]), _bits(plan[:, 1:1 + d]))
        mean = np.concatenate([plan[:, 1:], np.zeros((M, 1, A))], axis=1)
    assert model._call == 3


@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_a_limit_that_cannot_bind_changes_no_plan(gpu, context):
    """delta = 2 (ub - lb) with prev inside the box and no cost: what the same model without the kwargs plans, bit for bit, call after
    call (both on the opt-in route via cem_noise_beta=1.0), the kept elites included."""
    H, A = 5, 6
    other = dict(cem_noise_beta=1.0, cem_keep_elites=2)
    plain, prob = plan_model(context, H, **other)
    loose, _ = plan_model(context, H, cem_action_rate_limit=4.0, **other)
    assert plain._opt.actuator_params is None and loose._opt.actuator_params is not None
    loose.set_applied_actions(prev=np.random.default_rng(1).uniform(-1, 1, (M, A)))
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    for call in range(3):
        pa, pb = plan_act(plain, prob, context, mean, var), plan_act(loose, prob, context, mean, var)
        assert np.isfinite(pa).all() and 0 < np.abs(pa).max() <= 1.0
        np.testing.assert_array_equal(_bits(pa), _bits(pb), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(plain._plan_carry)), _bits(_np(loose._plan_carry)))
        mean = np.concatenate([pa[:, 1:], np.zeros((M, 1, A))], axis=1)
    assert not [s for s in plain.engine._loop_ws if s[-1] == "act"], "a model without the kwargs allocates no actuated workspace"
    # and one that binds plans something else
    tight, _ = plan_model(context, H, cem_action_rate_limit=0.05, **other)
    tight.set_applied_actions(prev=np.zeros((M, A)))
    assert not np.array_equal(_bits(plan_act(tight, prob, context, np.zeros((M, H, A)), var)), _bits(plan_act(plain, prob, context, np.zeros((M, H, A)), var)))


# ---------------------------------------------------------------------------------------------------------------------- 4: episode time
def test_commitments_follow_the_episode(gpu):
    """d = 2, three consecutive calls: call k's plan[:,0] is call k-1's plan[:,1] and call k-2's plan[:,2], bit for bit (what is decided
    stays decided).  `reset_plan_carry(mask)` frees only the masked envs (NaN, not zero); another number of envs starts from NaN;
    `set_applied_actions` is honoured, masked or not; `action_cost` in between moves nothing."""
    H, A, d = 5, 6, 2
    model, prob = plan_model(True, H, cem_action_delay=d, cem_action_rate_limit=0.25, cem_action_rate_cost=[0.1] * A, cem_keep_elites=2)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    plans = []
    for k in range(3):
        plans.append(plan_act(model, prob, True, mean, var))
        model.action_cost(plans[-1])
        mean = np.concatenate([plans[-1][:, 1:], np.zeros((M, 1, A))], axis=1)
    for k in (1, 2):
        np.testing.assert_array_equal(_bits(plans[k][:, 0]), _bits(plans[k - 1][:, 1]))
        np.testing.assert_array_equal(_bits(plans[k][:, 1]), _bits(plans[k - 1][:, 2]))
    np.testing.assert_array_equal(_bits(plans[2][:, 0]), _bits(plans[0][:, 2]))
    assert not np.array_equal(_bits(plans[1][:, 2]), _bits(plans[0][:, 3])), "the first free step was never re-decided"
    st = model.actuator_state()
    model.reset_plan_carry([True, False])
    st2 = model.actuator_state()
    assert np.isnan(st2["prev"][0]).all() and np.isnan(st2["committed"][0]).all() and _np(model._plan_carry_valid).tolist() == [0, 1]
    np.testing.assert_array_equal(_bits(st2["prev"][1]), _bits(st["prev"][1]))
    np.testing.assert_array_equal(_bits(st2["committed"][1]), _bits(st["committed"][1]))
    plan = plan_act(model, prob, True, mean, var)
    np.testing.assert_array_equal(_bits(plan[1, :d]), _bits(st["committed"][1]))
    assert not np.array_equal(_bits(plan[0, :d]), _bits(st["committed"][0]))
    with pytest.raises(ValueError, match="mask has 3 entries"):
        model.reset_plan_carry([True, False, True])
    model.reset_plan_carry()
    st = model.actuator_state()
    assert np.isnan(st["prev"]).all() and np.isnan(st["committed"]).all()
    # set_applied_actions: the caller's word against the plan's
    prev = np.full((M, A), 0.5, F)
    model.set_applied_actions(prev=prev, mask=[False, True])
    st = model.actuator_state()
    assert np.isnan(st["prev"][0]).all() and (st["prev"][1] == 0.5).all() and np.isnan(st["committed"]).all()
    committed = np.full((M, d, A), -0.25, F)
    model.set_applied_actions(committed=committed)
    plan = plan_act(model, prob, True, mean, var)
    np.testing.assert_array_equal(_bits(plan[:, :d]), _bits(committed))
    assert (np.abs(plan[:, d] - F(-0.25)) <= F(0.25)).all()
    # another number of envs starts from NaN
    model.set_applied_actions(prev=np.zeros((3, A)))
    assert model.actuator_state()["prev"].shape == (3, A) and np.isnan(model.actuator_state()["committed"]).all()


def test_advance_off_leaves_the_state_alone(gpu):
    H, A, d = 5, 6, 1
    model, prob = plan_model(False, H, cem_action_delay=d, cem_action_rate_limit=0.25, cem_action_advance=False)
    rng = np.random.default_rng(2)
    prev, committed = rng.uniform(-1, 1, (M, A)).astype(F), rng.uniform(-1, 1, (M, d, A)).astype(F)
    model.set_applied_actions(prev, committed)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    for _ in range(2):
        plan = plan_act(model, prob, False, mean, var)
        st = model.actuator_state()
        np.testing.assert_array_equal(_bits(st["prev"]), _bits(prev))
        np.testing.assert_array_equal(_bits(st["committed"]), _bits(committed))
        np.testing.assert_array_equal(_bits(plan[:, :d]), _bits(committed))


def test_device_planner_state_gives_the_same_plans(gpu):
    """`DevicePlannerState.act` == `get_action` with the samplers' warm start, call after call: the executed action is plan[:,0], the one
    committed d calls ago; `observe(done=)` and `reset` forget the masked / all envs' commitments with no code of their own."""
    from cadm_amd.caller import DevicePlannerState
    H, A, d = 5, 6, 2
    kw = dict(cem_action_delay=d, cem_action_rate_limit=0.3, cem_action_rate_cost=0.2, cem_keep_elites=2)
    a, prob = plan_model(False, H, **kw)
    b, _ = plan_model(False, H, **kw)
    state = DevicePlannerState(b, M)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    for call in range(3):
        plan = plan_act(a, prob, False, mean, var)
        act = _np(state.act(prob["obs"]))
        np.testing.assert_array_equal(_bits(act), _bits(plan[:, 0]), err_msg="call %d" % call)
        for k in ("prev", "committed"):
            np.testing.assert_array_equal(_bits(a.actuator_state()[k]), _bits(b.actuator_state()[k]))
        mean = np.concatenate([plan[:, 1:], np.zeros((M, 1, A))], axis=1)
    state.observe(prob["obs"], act, prob["obs"], done=np.array([0, 1]))
    st = b.actuator_state()
    assert np.isnan(st["prev"][1]).all() and np.isnan(st["committed"][1]).all() and np.isfinite(st["prev"][0]).all()
    state.reset()
    assert np.isnan(b.actuator_state()["prev"]).all()


# ---------------------------------------------------------------------------------------------------------------------- 5: action_cost
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_action_cost_against_restatement(gpu, context):
    H, A, d = 5, 6, 2
    dl, w = [0.2, math.inf, 0.4, 0.1, math.inf, 0.3], [1.0, 0.5, 0.0, 2.0, 0.25, 3.0]
    model, prob = plan_model(context, H, cem_action_delay=d, cem_action_rate_limit=dl, cem_action_rate_cost=w)
    seqs, _, _, prev, committed = aref.make_case(M, 9, H, A, d, seed=4)
    # before anything is known: step 0 is free
    res = model.action_cost(seqs)
    ref, cost_ref, S = aref.actuate(seqs, d, dl, w)
    np.testing.assert_array_equal(_bits(res["actions"]), _bits(ref))
    assert res["cost"].shape == (M, 9) and (np.abs(res["cost"] - cost_ref) <= aref.bound(S, H, A)).all()
    assert model.actuator_state() is None and model._call == 0
    model.set_applied_actions(prev, committed)
    keep = seqs.copy()
    res = model.action_cost(seqs)
    ref, cost_ref, S = aref.actuate(seqs, d, dl, w, prev, committed)
    np.testing.assert_array_equal(_bits(seqs), _bits(keep))
    np.testing.assert_array_equal(_bits(res["actions"]), _bits(ref))
    assert (np.abs(res["cost"] - cost_ref) <= aref.bound(S, H, A)).all() and (cost_ref > 0).all()
    one = model.action_cost(seqs[:, 3])                                   # [m,H,A]: the n axis is dropped
    assert one["cost"].shape == (M,) and one["actions"].shape == (M, H, A)
    np.testing.assert_array_equal(_bits(one["cost"]), _bits(res["cost"][:, 3]))
    st = model.actuator_state()
    np.testing.assert_array_equal(_bits(st["prev"]), _bits(prev))
    np.testing.assert_array_equal(_bits(st["committed"]), _bits(committed))
    assert model._call == 0
    with pytest.raises(ValueError, match="action_cost: actions"):
        model.action_cost(np.zeros((M, H + 1, A)))
    with pytest.raises(ValueError, match="actuator state holds 2"):
        model.action_cost(np.zeros((3, H, A)))
    plain, _ = plan_model(context, H, cem_noise_beta=1.0)
    with pytest.raises(ValueError, match="no actuator model"):
        plain.action_cost(seqs)


# ---------------------------------------------------------------------------------------------------------------------- 6: refusals
def test_argument_checks_return_einval(engines):
    """Both exports refuse bad arguments with CADM_EINVAL and a message that names them and the argument, before any HIP call (the dummy
    pointers next to the bad argument are never touched); the engine plans normally afterwards."""
    prob, eng = engines("hc5")
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(4096, dtype=torch.float32, device=eng.device)
    P = ct.c_void_p(buf.data_ptr())
    mp = HipEngine.mppi_params()

    def A_(delay=0, n_dims=0, limit=math.inf, w=0.0, at=0):
        a = HipEngine.actuator_params(0, None, None)
        a.delay, a.n_dims, a.rate_limit[at], a.rate_w[at] = delay, n_dims, limit, w
        return ct.byref(a)

    def actuate(a, c=ctx):
        return lib.cadm_actuate_actions(c, a, P, P, M, 4, P, None, None)

    def plan(a, c=ctx, prev=P, prefix=P, update=0, prm=ct.byref(mp)):
        return lib.cadm_actuated_plan(c, a, prev, prefix, 1, None, None, 0, None, None, None, None, None, update, prm, P, P, P, P, P, None, None, M, N,
                                      0, 1, P, P, None, None)

    def einval(rc, name, frag):
        msg = lib.cadm_last_error().decode()
        assert rc == -1, "%s: expected CADM_EINVAL, got %d (%s)" % (name, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    for name, fn in (("cadm_actuate_actions", actuate), ("cadm_actuated_plan", plan)):
        einval(fn(A_(delay=-1)), name, "action delay")
        einval(fn(A_(delay=eng.H)), name, "action delay")
        einval(fn(A_(n_dims=eng.A - 1)), name, "action dims")
        einval(fn(A_(n_dims=eng.A + 1)), name, "action dims")
        for at in (0, eng.A - 1):
            einval(fn(A_(limit=0.0, at=at)), name, "rate limit")
            einval(fn(A_(limit=-1.0, at=at)), name, "rate limit")
            einval(fn(A_(limit=NAN, at=at)), name, "rate limit")
            einval(fn(A_(w=-1.0, at=at)), name, "rate cost")
            einval(fn(A_(w=NAN, at=at)), name, "rate cost")
            einval(fn(A_(w=math.inf, at=at)), name, "rate cost")
        assert eng.A < _lib.MAX_ACT_DIMS      # entries beyond A are not looked at
    einval(actuate(None), "cadm_actuate_actions", "bad arguments")
    einval(plan(A_(), prev=None), "cadm_actuated_plan", "needs prev")
    einval(plan(A_(delay=1), prefix=None), "cadm_actuated_plan", "needs prev")
    einval(plan(A_(), update=2), "cadm_actuated_plan", "update")
    einval(plan(A_(), prm=None), "cadm_actuated_plan", "bad arguments")
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=M, H=5, seed=1)
    deng = make_engine(dprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    einval(actuate(A_(), c=deng._ctx), "cadm_actuate_actions", "continuous-action")
    einval(plan(A_(), c=deng._ctx), "cadm_actuated_plan", "continuous actions only")
    deng.close()
    sprob = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=5, seed=3, trained_like=True)
    seng = make_engine(sprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(seng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    einval(actuate(A_(), c=seng._ctx), "cadm_actuate_actions", "sharded")
    einval(plan(A_(), c=seng._ctx), "cadm_actuated_plan", "sharded")
    assert lib.cadm_dist_destroy(seng._ctx) == 0
    seng.close()
    assert (_np(buf) == 0).all()
    # python: shapes that do not fit the engine
    seqs = torch.zeros((M, 4, eng.H, eng.A), dtype=torch.float32, device=eng.device)
    ok = HipEngine.actuator_params(1, 0.5, None)
    for kw in (dict(prev=np.zeros((M + 1, eng.A))), dict(prev=np.zeros((M, eng.A + 1))), dict(prefix=np.zeros((M, 2, eng.A))), dict(prefix=np.zeros((M, eng.A)))):
        with pytest.raises(ValueError, match="actuate_actions"):
            eng.actuate_actions(seqs, ok, **kw)
    with pytest.raises(ValueError, match="actuate_actions: expected"):
        eng.actuate_actions(np.zeros((M, 4, eng.H, eng.A), F), ok)
    args = (None, None, None, None, None, None, None, HipEngine.icem_params(), prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    with pytest.raises(ValueError, match="needs prev"):
        eng.actuated_plan(ok, None, None, True, *args)
    with pytest.raises(ValueError, match="float32 device tensor"):
        eng.actuated_plan(ok, np.zeros((M, eng.A), F), None, True, *args)
    with pytest.raises(ValueError, match="action delay"):
        plan_model(True, 5, cem_action_delay=5)
    with pytest.raises(ValueError, match="entries"):
        plan_model(True, 5, cem_action_rate_limit=[0.1] * 5)
    nan = torch.full((M, eng.A), NAN, dtype=torch.float32, device=eng.device)
    out = _np(eng.actuated_plan(HipEngine.actuator_params(0, 0.5, 1.0), nan, None, True, *args, seed=1, call=1))
    assert np.isfinite(out).all() and np.abs(out).max() <= 1.0
    np.testing.assert_array_equal(_bits(_np(nan)), _bits(out[:, 0]))
