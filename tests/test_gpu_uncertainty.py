"""GPU: the uncertainty cost of the opt-in planner -- the kernels (`cadm_uncertainty_cost`, csrc/uncertainty.hip) against the numpy
restatement (tests/uncertainty_ref.py) and, bit for bit, against `cadm_forecast_stats`; the cap, non-finite values and the `first` cut;
the fused loop (`cadm_uncertain_plan`) against the stepwise one; the no-ops; the sign of lambda; the class route; the refusals.

Geometries: those tests/test_gpu_tracking.py builds -- hopper_like with context (D = 11, E = 5, p = 5, H = 3: one particle per member, an
odd D, unaligned spans) and the compiled-in halfcheetah 200 x 4 kernel (p = 20, H = 8: four particles per member; p = 5, H = 5) --, small
halfcheetah engines for H = 1, E = 1, p = 1 and the LDS limit, and the class route on tests/helpers.py's `plan_model`.

Bound against the float64 restatement, derived, not measured, and NOT doubled (`uncertainty_ref`): per variance 4 (p + 4) 2^-24 R^2 with
R = max_j |x_j - x_0|; per step (var) B_t = sum_d w_d bv_d + (n_w + 1) 2^-24 u_t; (std) min(B_t / sqrt u_t, sqrt B_t) + 2^-24 sqrt u_t;
cost sum_t B_t + H 2^-24 sum_t u_t over the counted steps.  tests/test_uncertainty_ref.py holds a float32 emulation of the chain to it
on the CPU (worst |err| / bound there: below 0.1).
Measured on an MI355X, worst |err| / bound over steps and cost (`test_kernel_against_restatement`, m = 3): hopper_like 0.014 (n = 1),
0.023 (n = 11); halfcheetah p = 20 0.007, 0.009; halfcheetah p = 5 0.013, 0.027."""
import ctypes as ct
import math

import numpy as np
import pytest
import torch

import uncertainty_ref as uref
from behind_rollout import synth_traj
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


def _prm(eng, kind, lam=1.0, w=None, form="var", cap=None):
    return HipEngine.uncertainty_params(kind, lam, w, form, cap, obs_dim=eng.D)


@pytest.fixture(scope="module")
def small(gpu):
    """name -> vanilla halfcheetah engine (E, p, H), built when first asked for"""
    built = {}

    def get(E, p, H):
        if (E, p, H) not in built:
            prob = synth.make_problem(env="halfcheetah", context=False, E=E, m=M, H=H, seed=3, trained_like=True)
            built[(E, p, H)] = (prob, make_engine(prob, p=p, num_elites=KE, num_cem_iters=ITERS))
        return built[(E, p, H)]
    yield get
    for _, eng in built.values():
        eng.close()


def _check(eng, traj, kind, w, form, cap, first, what):
    """steps and cost within the bound; step_out = NULL gives the same cost bits.  Returns the worst |err| / bound."""
    step_ref, cost_ref, B, S = uref.cost(traj, eng.E, kind, w, form, cap, first)
    prm = _prm(eng, kind, 1.0, w, form, cap)
    dev = eng._t(traj)
    step, cost = eng.uncertainty_cost(dev, prm, first=first, want_steps=True)
    only = eng.uncertainty_cost(dev, prm, first=first)
    step, cost = _np(step), _np(cost)
    H, m, n = traj.shape[:3]
    assert step.shape == (m, n, H) and cost.shape == (m, n)
    np.testing.assert_array_equal(_bits(_np(only)), _bits(cost), err_msg=what + ": cost without step_out")
    lim = uref.bound(B, S, H, first)
    es, ec = np.abs(step - step_ref), np.abs(cost - cost_ref)
    assert np.isfinite(step).all() and np.isfinite(cost).all(), what
    assert (es <= B).all(), "%s: steps, worst |err| / bound %.3f" % (what, (es[B > 0] / B[B > 0]).max())
    assert (ec <= lim).all(), "%s: cost, worst |err| / bound %.3f" % (what, (ec[lim > 0] / lim[lim > 0]).max())
    worst = [float((e[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0 for e, b in ((es, B), (ec, lim))]
    return max(worst), step, cost


# ---------------------------------------------------------------------------------------------------------------------- 1: the kernel
@pytest.mark.parametrize("name", ["hopper", "hc8", "hc5"])
@pytest.mark.parametrize("n", [1, 11])
def test_kernel_against_restatement(engines, name, n):
    """`cadm_uncertainty_cost` on `synth_traj` against tests/uncertainty_ref.py within the undoubled bound: both kinds x both forms x
    (broadcast, per-dim with zeros, one-hot) weights, m = 3 -- 33 candidates are four full groups of 8 and one of 1, groups span envs;
    3 candidates are one partial group.  hopper's odd D leaves the spans of odd steps off 16-byte alignment."""
    _, eng = engines(name)
    m, worst = 3, 0.0
    traj, _, _ = synth_traj(7 + n, eng.H, m, n, eng.p, eng.D, eng.A)
    if name == "hopper":
        assert (m * n * eng.p * eng.D * 4) % 16 != 0
    for kind in uref.KINDS:
        for form in uref.FORMS:
            for style in ("broadcast", "per-dim", "one-hot-%d" % (eng.D - 1)):
                w = uref.make_w(style, eng.D, seed=n)
                r, step, cost = _check(eng, traj, kind, w, form, None, None, "%s n=%d %s %s %s" % (name, n, kind, form, style))
                assert (cost > 0).all()
                worst = max(worst, r)
    print("\n[%s m=3 n=%d] worst |err| / bound %.3f" % (name, n, worst))
    assert worst > 0


def test_kernel_one_step_one_member_one_particle(small):
    """H = 1; E = 1: the epistemic variance is exactly 0, the total one is not; p = 1: both are exactly 0."""
    _, eng = small(1, 4, 1)
    traj, _, _ = synth_traj(3, 1, 3, 11, 4, eng.D, eng.A)
    for form in uref.FORMS:
        _, step, cost = _check(eng, traj, "epistemic", None, form, None, None, "E=1 epistemic " + form)
        assert (step == 0).all() and (cost == 0).all()
        _, step, cost = _check(eng, traj, "total", uref.make_w("per-dim", eng.D), form, None, None, "E=1 total " + form)
        assert (cost > 0).all()
        np.testing.assert_array_equal(_bits(step[:, :, 0]), _bits(cost))
    _, eng = small(1, 1, 3)
    traj, _, _ = synth_traj(4, 3, 3, 11, 1, eng.D, eng.A)
    for kind in uref.KINDS:
        for form in uref.FORMS:
            _, step, cost = _check(eng, traj, kind, None, form, None, None, "p=1 %s %s" % (kind, form))
            assert (step == 0).all() and (cost == 0).all()


# ---------------------------------------------------------------------------------------------------------------------- 2: the forecast's bits
@pytest.mark.parametrize("name", ["hopper", "hc8"])
def test_one_hot_weights_give_the_forecast_bits(engines, name):
    """For every dim d: w = e_d, form var, no cap -> step_out[mi,c,t] == cadm_forecast_stats' var_epistemic / var_total [mi,c,t,d] on the
    same traj, bit for bit: the chain is the forecast's, whatever numpy says."""
    _, eng = engines(name)
    m, n = 3, 5
    traj, obs, acts = synth_traj(31, eng.H, m, n, eng.p, eng.D, eng.A)
    dev = eng._t(traj)
    fc = {k: _np(v) for k, v in eng.forecast_stats(dev, obs, acts).items() if k in ("var_epistemic", "var_total")}
    assert fc["var_total"].shape == (m, n, eng.H, eng.D) and (fc["var_epistemic"] > 0).all()
    for kind in uref.KINDS:
        for d in range(eng.D):
            w = np.zeros((eng.D,), F)
            w[d] = 1.0
            step, cost = eng.uncertainty_cost(dev, _prm(eng, kind, 1.0, w), want_steps=True)
            np.testing.assert_array_equal(_bits(_np(step)), _bits(fc["var_" + kind][..., d]), err_msg="%s %s dim %d" % (name, kind, d))


# ---------------------------------------------------------------------------------------------------------------------- 3: cap, non-finite values
def test_cap_and_non_finite_values(engines):
    _, eng = engines("hc8")
    H, D, m, n = eng.H, eng.D, 3, 11
    traj, _, _ = synth_traj(5, H, m, n, eng.p, D, eng.A)
    w = uref.make_w("per-dim", D, seed=2)
    assert w[0] == 0 and w[1] > 0
    for kind in uref.KINDS:
        for form in uref.FORMS:
            free = uref.cost(traj, eng.E, kind, w, form)[0]
            cap = float(F(np.median(free)))
            r, step, cost = _check(eng, traj, kind, w, form, cap, None, "capped %s %s" % (kind, form))
            hit = free > cap * (1 + 1e-5)
            assert 0.2 < hit.mean() < 0.8
            np.testing.assert_array_equal(_bits(step[hit]), _bits(np.full(int(hit.sum()), cap, F)), err_msg="a capped step holds the cap's bits")
            assert (step <= F(cap)).all()
    prm = _prm(eng, "total", 1.0, w)
    base_step, base = [_np(x) for x in eng.uncertainty_cost(eng._t(traj), prm, want_steps=True)]
    for val in (NAN, math.inf, -math.inf):
        bad = traj.copy()
        bad[4, 1, 7, 3, 1] = val                          # a weighted dim of candidate (1, 7)
        bad[:, :, :, :, 0] = NAN                          # a zero-weight dim, everywhere
        cost = _np(eng.uncertainty_cost(eng._t(bad), prm))
        assert not np.isfinite(cost[1, 7])
        keep = np.ones((m, n), bool)
        keep[1, 7] = False
        np.testing.assert_array_equal(_bits(cost[keep]), _bits(base[keep]), err_msg="another candidate's cost moved")
    only0 = traj.copy()
    only0[:, :, :, :, 0] = NAN
    step, cost = [_np(x) for x in eng.uncertainty_cost(eng._t(only0), prm, want_steps=True)]
    np.testing.assert_array_equal(_bits(step), _bits(base_step), err_msg="a NaN in a zero-weight dim")
    np.testing.assert_array_equal(_bits(cost), _bits(base))
    # a cap is a comparison: a NaN step stays NaN under it; a square that overflows is capped like any other value
    big = traj.copy()
    big[2, 0, 0, 0, 1] = 1e30
    big[3, 0, 1, 0, 1] = NAN
    step = _np(eng.uncertainty_cost(eng._t(big), _prm(eng, "total", 1.0, w, cap=2.0), want_steps=True)[0])
    assert _bits(step[0, 0, 2]) == _bits(F(2.0)) and np.isnan(step[0, 1, 3])
    assert np.isinf(_np(eng.uncertainty_cost(eng._t(big), prm, want_steps=True)[0])[0, 0, 2])


# ---------------------------------------------------------------------------------------------------------------------- 4: the first cut
@pytest.mark.parametrize("name", ["hopper", "hc8"])
def test_first_cut(engines, name):
    """`first` drawn over 0 .. H with 0 and H planted: NaNs behind min_j first never reach the cost, and the result is the
    restatement's with the same cut; step_out = NULL the same bits; a NaN at the cut itself does reach it."""
    _, eng = engines(name)
    H, D, p, m, n = eng.H, eng.D, eng.p, 3, 11
    traj, _, _ = synth_traj(9, H, m, n, p, D, eng.A)
    rng = np.random.default_rng(17)
    first = rng.integers(0, H + 1, (m, n, p)).astype(np.int32)
    first[0, 0], first[2, 10], first[1, 3] = 0, H, H
    first[1, 3, 2] = 1
    cut = first.min(axis=2)
    assert (cut == 0).any() and (cut == H).any() and (cut[1, 3] == 1)
    dirty = traj.copy()
    behind = np.arange(H)[:, None, None] > cut[None]
    assert behind.any()
    dirty[behind] = NAN
    for kind in uref.KINDS:
        for form in uref.FORMS:
            w = uref.make_w("per-dim", D, seed=4)
            _, step, cost = _check(eng, traj, kind, w, form, None, first, "%s cut %s %s" % (name, kind, form))
            prm = _prm(eng, kind, 1.0, w, form)
            got = _np(eng.uncertainty_cost(eng._t(dirty), prm, first=first))
            np.testing.assert_array_equal(_bits(got), _bits(cost), err_msg="NaNs behind the cut reached the cost")
            s2, c2 = eng.uncertainty_cost(eng._t(dirty), prm, first=first, want_steps=True)
            np.testing.assert_array_equal(_bits(_np(c2)), _bits(cost))
            assert np.isnan(_np(s2)[np.transpose(behind, (1, 2, 0))]).all()
            uncut = _np(eng.uncertainty_cost(eng._t(traj), prm))
            assert (uncut[cut < H - 1] > cost[cut < H - 1]).all() and np.array_equal(_bits(uncut[cut >= H - 1]), _bits(cost[cut >= H - 1]))
    dirty[1, 1, 3, 0, 1] = NAN                            # step 1 of candidate (1, 3): its cut
    assert np.isnan(_np(eng.uncertainty_cost(eng._t(dirty), prm, first=first))[1, 3])


# ---------------------------------------------------------------------------------------------------------------------- 5: the loop
def _lam_cand(score, cost, lam):
    return (score - (F(lam) * cost).astype(F)).astype(F)


def _check_iterations(eng, info, unc, kind, w, form, cap, terminate=False):
    for x in info:
        score, cost, cand, steps = _np(x["unc_score"]), _np(x["unc_cost"]), _np(x["cand"]), _np(x["unc_steps"])
        assert np.isfinite(cand).all() and (cost > 0).all()
        np.testing.assert_array_equal(_bits(cand), _bits(_lam_cand(score, cost, unc.weight)), err_msg="cand is not float32(score - lambda cost)")
        order = np.argsort(-cand.astype(np.float64), axis=1, kind="stable")[:, :KE]
        np.testing.assert_array_equal(_np(x["elites"]).reshape(order.shape), order, err_msg="the elites are not the top num_elites of the final score")
        first = _np(x["first_violation"]) if terminate else None
        step_ref, cost_ref, B, S = uref.cost(_np(x["traj"]), eng.E, kind, w, form, cap, first)
        assert (np.abs(cost - cost_ref) <= uref.bound(B, S, eng.H, first)).all() and (np.abs(steps - step_ref) <= B).all()


LOOP = [("hc5-vanilla", "cem", False, 0, "epistemic", "var", 0.7), ("hc5", "mppi", True, 2, "total", "std", -0.4),
        ("hopper", "cem", True, 2, "total", "var", 0.05), ("hopper", "mppi", False, 2, "epistemic", "std", 1.5)]


@pytest.mark.parametrize("name,update,best,K,kind,form,lam", LOOP, ids=["%s-%s-%s-%s" % (c[0], c[1], c[4], c[5]) for c in LOOP])
def test_fused_equals_stepwise(engines, name, update, best, K, kind, form, lam):
    """`cadm_uncertain_plan` with device RNG == the same loop one launch at a time (`planner.icem_plan(..., uncertainty=...)`), bit for
    bit over two consecutive calls: the plan, the best return, the carry.  In every stepwise iteration `cand` is
    float32(score - float32(lambda cost)) bit for bit, the elites are the top num_elites of it, and the cost is the restatement's."""
    prob, eng = engines(name)
    H, A = eng.H, eng.A
    w = uref.make_w("per-dim", eng.D, seed=6)
    cap = 50.0 if lam < 0 else None
    unc = _prm(eng, kind, lam, w, form, cap)
    icem = dict(noise_beta=1.0 if update == "mppi" else 0.0, keep_elites=K, decay=1.25 if K else 1.0, return_best=best, add_mean_last=K > 0)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    (ca, va), (cb, vb) = zero_carry(eng, M, K, H), zero_carry(eng, M, K, H)
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2):
        a, ra = eng.uncertain_plan(unc, None, None, None, True, None, None, None, None, None, None, None, prm, *args, mean, var, N, carry=ca,
                                   carry_valid=va, seed=4, call=call, want_best_return=True)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                            update=update, temperature=0.5, relative=True, uncertainty=unc, **icem)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        if K:
            np.testing.assert_array_equal(_bits(_np(ca)), _bits(_np(cb)), err_msg="carry after call %d" % call)
        _check_iterations(eng, info, unc, kind, w, form, cap)
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)      # the samplers' warm start
    # the term matters: without it, another plan
    other = _np(eng.actuated_plan(None, None, None, True, None, None, None, None, None, None, None, prm, *args, mean, var, N,
                                  *zero_carry(eng, M, K, H), seed=4, call=2))
    assert not np.array_equal(_bits(other), _bits(a))
    assert (update == "mppi", "unc", False, False) in eng._loop_ws


def test_with_everything_on(engines):
    """Under TERMINATE constraints, tracking terms, a CVaR score, knots, kept elites and an actuator model: fused == stepwise bit for bit;
    the cost stops at the smallest first violation of a candidate's particles and comes off the candidate score behind the actuator's."""
    from test_gpu_actuator import _params, _state
    from test_gpu_constraints import binding_bounds, iteration0_traj
    from test_gpu_tracking import _tracking_inputs
    prob, eng = engines("hc5")
    H, A, d = eng.H, eng.A, 1
    track, targets, offset, _ = _tracking_inputs(eng, prob, 3, H, 13)
    cp = HipEngine.constraint_params(binding_bounds(iteration0_traj(eng, prob, 1.0, 4, 1), (1, 7), H, "uncertain"), "terminate", 4.0)
    score, knots = HipEngine.score_params("cvar", k=2), HipEngine.knot_params(2, "linear")
    phase = torch.tensor([0, 1], dtype=torch.int32, device=eng.device)
    act = _params(eng, d, 0.4, 2.0)
    w = uref.make_w("per-dim", eng.D, seed=8)
    unc = _prm(eng, "total", 0.3, w, "std", 7.5)
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, return_best=False, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    (ca, va), (cb, vb) = zero_carry(eng, M, 2, H), zero_carry(eng, M, 2, H)
    (pa, fa), (pb, fb) = _state(eng, d, 8), _state(eng, d, 8)
    a, ra = eng.uncertain_plan(unc, act, pa, fa, True, track, targets, offset, knots, phase, cp, score, prm, *args, carry=ca, carry_valid=va, seed=4,
                               call=1, want_best_return=True)
    b, info, extra = hplanner.icem_plan(eng, *args, carry=cb, carry_valid=vb, seed=4, call=1, return_info=True, update="mppi", temperature=0.5,
                                        relative=True, score=score, constraints=cp, knots=knots, phase=phase, tracking=(track, targets, offset),
                                        actuator=(act, pb, fb), action_advance=True, uncertainty=unc, **icem)
    for x, y in ((a, b), (ra, extra["best_ret"]), (ca, cb), (pa, pb), (fa, fb)):
        np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))
    _check_iterations(eng, info, unc, "total", w, "std", 7.5, terminate=True)
    share = float((_np(info[0]["first_violation"]).min(axis=2) < H - 1).mean())
    assert 0.1 <= share, "%.2f of the candidates are cut" % share
    for x in info:
        np.testing.assert_array_equal(_bits(_np(x["score"])), _bits(_np(eng.particle_score(x["rows"], score))))
        np.testing.assert_array_equal(_bits(_np(x["unc_score"])), _bits(_np(x["score"]) - _np(x["action_cost"])))
    assert (True, "unc", True, True) in eng._loop_ws


# ---------------------------------------------------------------------------------------------------------------------- 6: the no-ops
@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_no_params_is_the_loop_underneath(engines, update):
    """params = NULL: the plan, the best return and the carry of `cadm_actuated_plan` on the same inputs, bit for bit, through the C entry
    itself with that loop's workspace; and the workspace with the term is the loop underneath's, with the trajectory (and first-violation)
    view, plus u [m,n,H] and the cost [m,n]."""
    prob, eng = engines("hc5")
    H, A = eng.H, eng.A
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    mppi, full = eng._as_mppi_params(prm)
    knots, phase = HipEngine.knot_params(2, "hold"), torch.tensor([1, 0], dtype=torch.int32, device=eng.device)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    carry, valid = zero_carry(eng, M, 2, H)
    plan, best = eng.actuated_plan(None, None, None, True, None, None, None, knots, phase, None, None, prm, *args, carry=carry, carry_valid=valid,
                                   seed=5, call=2, want_best_return=True)
    carry2, valid2 = zero_carry(eng, M, 2, H)
    t = [eng._t(x) for x in args[:5]]
    ws = eng._loop_workspace(mppi, M, N, 2)
    out = torch.empty((M, H, A), dtype=torch.float32, device=eng.device)
    best2 = torch.empty((M,), dtype=torch.float32, device=eng.device)
    P = lambda x: ct.c_void_p(x.data_ptr())
    rc = eng.lib.cadm_uncertain_plan(eng._ctx, None, None, None, None, 1, None, None, 0, None, ct.byref(knots), P(phase), None, None, int(mppi),
                                     ct.byref(full), *[P(x) for x in t], P(carry2), P(valid2), M, N, 5, 2, P(ws), P(out), P(best2), eng.stream)
    assert rc == 0, eng.lib.cadm_last_error().decode()
    for x, y in ((plan, out), (best, best2), (carry, carry2)):
        np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))
    same = _np(eng.uncertain_plan(None, None, None, None, True, None, None, None, knots, phase, None, None, prm, *args, *zero_carry(eng, M, 2, H),
                                  seed=5, call=2))
    np.testing.assert_array_equal(_bits(same), _bits(_np(plan)))
    pad = lambda nbytes: (nbytes + 255) & ~255
    more = pad(M * N * H * 4) + pad(M * N * 4)
    lib = eng.lib
    for terminate in (0, 1):
        for act in (0, 1):
            assert lib.cadm_uncertain_workspace_bytes(eng._ctx, M, N, 2, int(mppi), terminate, act) == more + (
                lib.cadm_actuated_workspace_bytes(eng._ctx, M, N, 2, int(mppi), 1, terminate) if act
                else lib.cadm_tracking_workspace_bytes(eng._ctx, M, N, 2, int(mppi), terminate))
    assert lib.cadm_uncertain_workspace_bytes(eng._ctx, 0, N, 2, 0, 0, 0) == 0


@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_lambda_zero_changes_no_plan(gpu, context):
    """lambda = 0 on finite trajectories: what the same model without `cem_uncertainty` plans, bit for bit, call after call, the kept
    elites included (both on the opt-in route via cem_noise_beta=1.0): it records trajectories, and nothing else differs."""
    H, A = 5, 6
    other = dict(cem_noise_beta=1.0, cem_keep_elites=2)
    plain, prob = plan_model(context, H, **other)
    zero, _ = plan_model(context, H, cem_uncertainty=dict(kind="total", weight=0.0, w="delta_std", form="std"), **other)
    assert plain._opt.uncertainty_params is None and zero._opt.uncertainty_params is not None
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    for call in range(3):
        pa, pb = plan_act(plain, prob, context, mean, var), plan_act(zero, prob, context, mean, var)
        assert np.isfinite(pa).all() and 0 < np.abs(pa).max() <= 1.0
        np.testing.assert_array_equal(_bits(pa), _bits(pb), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(plain._plan_carry)), _bits(_np(zero._plan_carry)))
        mean = np.concatenate([pa[:, 1:], np.zeros((M, 1, A))], axis=1)
    assert not [s for s in plain.engine._loop_ws if "unc" in s], "a model without the kwarg allocates no such workspace"
    assert [s for s in zero.engine._loop_ws if "unc" in s]
    # and a lambda that is not 0 plans something else
    heavy, _ = plan_model(context, H, cem_uncertainty=dict(kind="total", weight=50.0, w="delta_std"), **other)
    z = np.zeros((M, H, A))
    assert not np.array_equal(_bits(plan_act(heavy, prob, context, z, var)), _bits(plan_act(plan_model(context, H, **other)[0], prob, context, z, var)))


def test_epistemic_with_one_member_changes_no_plan(small):
    """E = 1: the epistemic cost is exactly 0, so any lambda reproduces the loop without the term, bit for bit."""
    prob, eng = small(1, 5, 5)
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.0, return_best=False, add_mean_last=True)
    prm = HipEngine.icem_params(**icem)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    for call in (1, 2):
        (ca, va), (cb, vb) = zero_carry(eng, M, 2, eng.H), zero_carry(eng, M, 2, eng.H)
        a, ra = eng.uncertain_plan(_prm(eng, "epistemic", 123.0), None, None, None, True, None, None, None, None, None, None, None, prm, *args,
                                   carry=ca, carry_valid=va, seed=2, call=call, want_best_return=True)
        b, rb = eng.actuated_plan(None, None, None, True, None, None, None, None, None, None, None, prm, *args, carry=cb, carry_valid=vb, seed=2,
                                  call=call, want_best_return=True)
        for x, y in ((a, b), (ra, rb), (ca, cb)):
            np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))
        assert np.isfinite(_np(a)).all()


# ---------------------------------------------------------------------------------------------------------------------- 7: the sign
def test_sign_of_lambda(engines):
    """One seed, the same iteration-0 candidates: with |lambda| x (spread of the cost) above 10 x the spread of the scores -- and
    |lambda| x (the smallest gap between two costs) above the spread of the scores, so that the order is the cost's alone -- the
    iteration-0 elites under +lambda are the lowest-cost candidates, under -lambda the highest-cost ones."""
    prob, eng = engines("hc5")
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    run = lambda lam: hplanner.icem_plan(eng, *args, seed=6, call=1, return_info=True, uncertainty=_prm(eng, "epistemic", lam))[1][0]
    x = run(1.0)
    score, cost = _np(x["unc_score"]).astype(np.float64), _np(x["unc_cost"]).astype(np.float64)
    spread = lambda v: float((v.max(axis=1) - v.min(axis=1)).max())
    gap = float(np.diff(np.sort(cost, axis=1), axis=1).min())
    assert gap > 0
    lam = max(10.0 * spread(score) / float((cost.max(axis=1) - cost.min(axis=1)).min()), 2.0 * spread(score) / gap)
    by_cost = np.argsort(cost, axis=1, kind="stable")
    for sign, want in ((1.0, by_cost[:, :KE]), (-1.0, by_cost[:, ::-1][:, :KE])):
        y = run(sign * lam)
        np.testing.assert_array_equal(_bits(_np(y["actions"])), _bits(_np(x["actions"])), err_msg="iteration 0's candidates moved")
        np.testing.assert_array_equal(_bits(_np(y["unc_cost"])), _bits(_np(x["unc_cost"])))
        assert abs(sign * lam) * spread(_np(y["unc_cost"]).astype(np.float64)) > 10.0 * spread(_np(y["unc_score"]).astype(np.float64))
        np.testing.assert_array_equal(np.sort(_np(y["elites"]).reshape(M, KE), axis=1), np.sort(want, axis=1),
                                      err_msg="lambda %+g: the elites are not the %s-cost candidates" % (sign * lam, "lowest" if sign > 0 else "highest"))


# ---------------------------------------------------------------------------------------------------------------------- 8: the class route
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_class_route(gpu, context):
    H, A, D, d = 5, 6, 18, 4
    onehot = [0.0] * D
    onehot[d] = 1.0
    model, prob = plan_model(context, H, cem_uncertainty=dict(kind="epistemic", weight=0.5, w=onehot))
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    plan = plan_act(model, prob, context, mean, var)
    assert np.isfinite(plan).all() and model._call == 1
    hist = (prob["cp_obs"], prob["cp_act"]) if context else ()
    res = model.uncertainty_cost(prob["obs"], plan, *hist)
    fc = model.forecast(prob["obs"], plan, *hist)
    assert res["step"].shape == (M, H) and res["cost"].shape == (M,) and res["returns"].shape == (M, 5) and model._call == 1
    sq = fc["std_epistemic"][..., d].astype(np.float64) ** 2
    assert (res["step"] > 0).all() and (np.abs(res["step"] - sq) <= 3 * 2.0 ** -24 * sq).all()      # (the float32 rounding of the forecast's sqrt, squared)
    np.testing.assert_array_equal(_bits(res["returns"]), _bits(fc["rollout_returns"]))
    assert (np.abs(res["cost"] - res["step"].astype(np.float64).sum(axis=1)) <= H * 2.0 ** -24 * res["cost"]).all()
    many = model.uncertainty_cost(prob["obs"], np.repeat(plan[:, None], 3, axis=1), *hist)
    assert many["step"].shape == (M, 3, H) and many["cost"].shape == (M, 3)
    # w = "delta_std" follows the statistics the model holds
    st = prob["stats"]
    follow, _ = plan_model(context, H, cem_uncertainty=dict(kind="total", weight=1.0, w="delta_std"))
    a = follow.uncertainty_cost(prob["obs"], plan, *hist)
    want = (1.0 / (np.asarray(st["delta_std"], np.float64) + 1e-10) ** 2).astype(F)
    np.testing.assert_array_equal(_bits(np.array(follow._opt.uncertainty_params.w[:D], F)), _bits(want))
    nz = dict(follow.normalization)
    nz["delta"] = (nz["delta"][0], 2.0 * np.asarray(nz["delta"][1]))
    follow.set_normalization(nz)
    b = follow.uncertainty_cost(prob["obs"], plan, *hist)
    np.testing.assert_array_equal(_bits(np.array(follow._opt.uncertainty_params.w[:D], F)),
                                  _bits((1.0 / (2.0 * np.asarray(st["delta_std"], np.float64) + 1e-10) ** 2).astype(F)))
    fixed, _ = plan_model(context, H, cem_uncertainty=dict(kind="total", weight=1.0, w=list(follow._opt.uncertainty_params.w[:D])))
    fixed.set_normalization(nz)
    np.testing.assert_array_equal(_bits(fixed.uncertainty_cost(prob["obs"], plan, *hist)["step"]), _bits(b["step"]))
    assert not np.array_equal(_bits(a["step"]), _bits(b["step"]))
    # set_uncertainty_weights takes effect on the next call, and stops the following
    follow.set_uncertainty_weights(onehot)
    c = follow.uncertainty_cost(prob["obs"], plan, *hist)
    fc = follow.forecast(prob["obs"], plan, *hist)
    sq = fc["std_total"][..., d].astype(np.float64) ** 2
    assert (np.abs(c["step"] - sq) <= 3 * 2.0 ** -24 * sq).all()
    follow.set_normalization(nz)
    follow.uncertainty_cost(prob["obs"], plan, *hist)
    assert list(follow._opt.uncertainty_params.w[:D]) == onehot
    plain, _ = plan_model(context, H, cem_noise_beta=1.0)
    for fn in (lambda: plain.uncertainty_cost(prob["obs"], plan, *hist), lambda: plain.set_uncertainty_weights(1.0)):
        with pytest.raises(ValueError, match="no cem_uncertainty"):
            fn()


def test_class_route_under_terminate_constraints(gpu):
    """`uncertainty_cost` of a model with TERMINATE constraints applies their first violations, as the loop does."""
    H, A, D = 5, 6, 18
    base, prob = plan_model(True, H, cem_uncertainty=dict(kind="total", weight=1.0))
    plan = np.random.default_rng(3).uniform(-1, 1, (M, 4, H, A)).astype(F)
    hist = (prob["cp_obs"], prob["cp_act"])
    free = base.uncertainty_cost(prob["obs"], plan, *hist)
    fc = base.forecast(prob["obs"], plan, *hist)
    lo = float(np.quantile(fc["mean"][..., 1], 0.3))
    model, _ = plan_model(True, H, cem_uncertainty=dict(kind="total", weight=1.0), cem_constraints=[dict(dim=1, lo=lo)],
                          cem_constraint_mode="terminate", cem_constraint_weight=1.0)
    cut = model.constraint_check(prob["obs"], plan, *hist)["first_violation"].min(axis=2)
    res = model.uncertainty_cost(prob["obs"], plan, *hist)
    assert (cut < H - 1).any()
    np.testing.assert_array_equal(_bits(res["step"]), _bits(free["step"]))
    want = np.where(np.arange(H)[None, None] <= cut[..., None], free["step"].astype(np.float64), 0.0).sum(axis=2)
    assert (np.abs(res["cost"] - want) <= H * 2.0 ** -24 * want).all() and (res["cost"][cut < H - 1] < free["cost"][cut < H - 1]).all()


# ---------------------------------------------------------------------------------------------------------------------- 9: refusals
def test_argument_checks_return_einval(engines, small):
    """Both exports refuse bad arguments with CADM_EINVAL and a message that names them and the argument, before any HIP call (the dummy
    pointers next to the bad argument are never touched); the engine plans normally afterwards."""
    prob, eng = engines("hc5")
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(8192, dtype=torch.float32, device=eng.device)
    P = ct.c_void_p(buf.data_ptr())
    mp = HipEngine.mppi_params()

    def U(kind=0, form=0, weight=1.0, cap=math.inf, n_dims=0, w=1.0, at=0):
        u = HipEngine.uncertainty_params("epistemic", 1.0)
        u.kind, u.form, u.weight, u.cap, u.n_dims, u.w[at] = kind, form, weight, cap, n_dims, w
        return ct.byref(u)

    def cost(u, c=ctx):
        return lib.cadm_uncertainty_cost(c, u, P, None, M, 4, P, P, None)

    def plan(u, c=ctx, update=0, prm=ct.byref(mp)):
        return lib.cadm_uncertain_plan(c, u, None, None, None, 1, None, None, 0, None, None, None, None, None, update, prm, P, P, P, P, P, None, None,
                                       M, N, 0, 1, P, P, None, None)

    def einval(rc, name, frag):
        msg = lib.cadm_last_error().decode()
        assert rc == -1, "%s: expected CADM_EINVAL, got %d (%s)" % (name, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    for name, fn in (("cadm_uncertainty_cost", cost), ("cadm_uncertain_plan", plan)):
        einval(fn(U(kind=2)), name, "kind")
        einval(fn(U(kind=-1)), name, "kind")
        einval(fn(U(form=2)), name, "form")
        for bad in (NAN, math.inf, -math.inf):
            einval(fn(U(weight=bad)), name, "lambda")
        for bad in (NAN, 0.0, -1.0):
            einval(fn(U(cap=bad)), name, "cap")
        einval(fn(U(n_dims=eng.D - 1)), name, "observation dims")
        einval(fn(U(n_dims=eng.D + 1)), name, "observation dims")
        for bad in (-1.0, NAN, math.inf):
            einval(fn(U(w=bad)), name, "w[0]")
            einval(fn(U(n_dims=eng.D, w=bad, at=eng.D - 1)), name, "w[%d]" % (eng.D - 1))
        einval(fn(U(w=0.0)), name, "weight w is 0")
        zeros = HipEngine.uncertainty_params("total", 1.0, [1.0] * eng.D)
        for k in range(eng.D):
            zeros.w[k] = 0.0
        zeros.w[eng.D] = 1.0                                  # (entries beyond D are not looked at)
        einval(fn(ct.byref(zeros)), name, "weight w is 0")
    einval(cost(None), "cadm_uncertainty_cost", "null")
    einval(lib.cadm_uncertainty_cost(ctx, U(), P, None, M, 4, P, None, None), "cadm_uncertainty_cost", "null")
    einval(plan(U(), update=2), "cadm_uncertain_plan", "update")
    einval(plan(U(), prm=None), "cadm_uncertain_plan", "bad arguments")
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=M, H=5, seed=1)
    deng = make_engine(dprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    einval(cost(U(), c=deng._ctx), "cadm_uncertainty_cost", "continuous-action")
    einval(plan(U(), c=deng._ctx), "cadm_uncertain_plan", "continuous actions only")
    deng.close()
    sprob = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=5, seed=3, trained_like=True)
    seng = make_engine(sprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(seng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    einval(cost(U(), c=seng._ctx), "cadm_uncertainty_cost", "sharded")
    einval(plan(U(), c=seng._ctx), "cadm_uncertain_plan", "sharded")
    assert lib.cadm_dist_destroy(seng._ctx) == 0
    seng.close()
    assert (_np(buf) == 0).all()
    # python: shapes that do not fit the engine
    with pytest.raises(ValueError, match="uncertainty_cost: traj"):
        eng.uncertainty_cost(np.zeros((eng.H, M, 4, eng.p, eng.D + 1), F), _prm(eng, "total"))
    with pytest.raises(ValueError, match="uncertainty_cost: first"):
        eng.uncertainty_cost(np.zeros((eng.H, M, 4, eng.p, eng.D), F), _prm(eng, "total"), first=np.zeros((M, 4), np.int32))
    args = (None, None, None, None, None, None, None, None, None, None, None, HipEngine.icem_params(), prob["obs"], prob["cp_obs"], prob["cp_act"],
            prob["init_mean"], prob["init_var"], N)
    out = _np(eng.uncertain_plan(_prm(eng, "total", 0.5), *args, seed=1, call=1))
    assert np.isfinite(out).all() and np.abs(out).max() <= 1.0


def test_lds_limit(small):
    """D = 18: p = 680 is the largest tile the LDS check accepts (pad4(p D) + 2 pad4(D) floats <= 48 KiB) -- it runs, one candidate per
    workgroup, and matches the restatement; p = 681 is refused, before any launch."""
    _, eng = small(1, 680, 2)
    assert 4 * (((680 * 18 + 3) & ~3) + 2 * 20) <= 48 * 1024 < 4 * (((681 * 18 + 3) & ~3) + 2 * 20)
    traj, _, _ = synth_traj(12, 2, 1, 3, 680, eng.D, eng.A)
    for kind in uref.KINDS:
        r, step, cost = _check(eng, traj, kind, uref.make_w("per-dim", eng.D), "var", None, None, "p=680 " + kind)
        assert (cost > 0).all() or kind == "epistemic"
    _, big = small(1, 681, 2)
    buf = torch.zeros(64, dtype=torch.float32, device=big.device)
    P = ct.c_void_p(buf.data_ptr())
    u = _prm(big, "total")
    rc = big.lib.cadm_uncertainty_cost(big._ctx, ct.byref(u), P, None, 1, 1, P, P, None)
    msg = big.lib.cadm_last_error().decode()
    assert rc == -1 and "LDS" in msg and "49152" in msg and (_np(buf) == 0).all(), (rc, msg)


def test_refusals_at_construction(gpu, monkeypatch):
    """`cem_uncertainty` is refused where the other `cem_*` options are: use_cem=False, a discrete env, a process group of more than one
    rank; a list `w` is checked against the env's observation dims."""
    from cadm_amd.envs import make_env_spec
    u = dict(kind="epistemic", weight=1.0)
    with pytest.raises(ValueError, match="need use_cem=True"):
        plan_model(True, 5, use_cem=False, cem_uncertainty=u)
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        plan_model(True, 5, env=make_env_spec("cartpole"), cem_uncertainty=u)
    with pytest.raises(ValueError, match="17 entries, expected 18"):
        plan_model(True, 5, cem_uncertainty=dict(kind="total", weight=1.0, w=[1.0] * 17))
    import torch.distributed as dist
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        plan_model(True, 5, process_group=object(), cem_uncertainty=u)
