"""GPU: plans on knots in the opt-in planner (csrc/knots.hip `cadm_shape_actions`, csrc/icem.hip `cadm_knot_plan`): action repeat and linear
interpolation between knot steps, per-env grid phases.

Geometry of every test: that of tests/test_gpu_icem.py -- halfcheetah, vanilla and CaDM, hidden (32,) * 4 (nothing is built on demand),
ensemble 5, particles 5, n = 64, num_elites = 8, 3 CEM iterations.  Numpy restatement of the grid: tests/knot_ref.py."""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

import knot_ref as kref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import _np, make_engine, zero_carry
from helpers import plan_act as _act
from helpers import plan_model as _model

pytestmark = pytest.mark.gpu

HID = (32,) * 4
M, N, KE, ITERS, A = 2, 64, 8, 3, 6


@functools.lru_cache(maxsize=None)
def _engine(H, context=False, m=M):
    prob = synth.make_problem(env="halfcheetah", context=context, E=5, m=m, H=H, seed=3, hidden_sizes=HID, trained_like=True)
    return prob, make_engine(prob, p=5, num_elites=KE, num_cem_iters=ITERS)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _phase(eng, values):
    return torch.tensor(list(values), dtype=torch.int32, device=eng.device)


def _mean_var(eng, H, seed, m=M):
    """(mean, var) device tensors: a mean off the grid (shaping it matters), a variance wide enough for distinct candidates"""
    rng = np.random.default_rng(seed)
    return eng._t(rng.uniform(-0.7, 0.7, (m, H, A))), eng._t(rng.uniform(0.05, 0.25, (m, H, A)))


def _bps(plans):
    return [kref.breakpoints(p) for p in np.asarray(plans)]


# ---------------------------------------------------------------------------------------------------------------------- 1: the primitive
PRIM = [(5, 2), (6, 3), (7, 3), (7, 4), (5, 5), (5, 8), (1, 2)]


@pytest.mark.parametrize("interp", ["hold", "linear"])
@pytest.mark.parametrize("H,r", PRIM, ids=["H%d-r%d" % hr for hr in PRIM])
def test_shape_actions_against_numpy(gpu, H, r, interp):
    """`cadm_shape_actions` on m = 3 envs with phases (0, 1, r - 1), with phases outside [0, r) (the modulo), and without phases, for
    n in {1, 37, 64} packed candidates at the head of a LARGER buffer: HOLD bit-equal to the numpy restatement everywhere; LINEAR bit-equal
    at the knot steps and in held tails, elsewhere within 2^-22 absolute (the reference rounds the float64 expression once; the kernel
    rounds the difference, the weight and the fused multiply-add: 2^-24 + 2^-25 + 2^-25 on values in [-1, 1], plus the reference's 2^-25);
    nothing leaves [-1, 1]; the floats behind the m n sequences are untouched."""
    _, eng = _engine(H, False, 3)
    check_shape_actions(eng, r, interp)


def check_shape_actions(eng, r, interp, ns=(1, 37, 64)):
    """The body of `test_shape_actions_against_numpy` on any engine (its H and A), for n in `ns`.  Returns the largest error of an
    interpolated step against float64."""
    m, H, A = 3, eng.H, eng.A
    knots, code = HipEngine.knot_params(r, interp), _lib.KNOT_INTERPS[interp]
    rng = np.random.default_rng(100 * H + r)
    worst = 0.0
    for phases in ((0, 1, r - 1), (-1, r, 2 * r + 1), None):
        for n in ns:
            used = m * n * H * A
            host = rng.uniform(-1, 1, (used + 5 * H * A + 3,)).astype(np.float32)
            host[rng.integers(0, host.size, 40)] = 1.0
            host[rng.integers(0, host.size, 40)] = -1.0
            buf = eng._t(host)
            view = buf[:used].view(m, n, H, A)
            assert eng.shape_actions(view, knots, None if phases is None else _phase(eng, phases)) is view
            got = _np(buf)
            np.testing.assert_array_equal(_bits(got[used:]), _bits(host[used:]), err_msg="floats behind [m, n] sequences (n = %d)" % n)
            got, src = got[:used].reshape(m, n, H, A), host[:used].reshape(m, n, H, A)
            ref = kref.shape(src, r, code, phases)
            assert got.min() >= -1.0 and got.max() <= 1.0
            for mi in range(m):
                phi = 0 if phases is None else phases[mi]
                exact = kref.exact_steps(H, r, code, phi)
                ks = kref.knot_steps(H, r, phi)
                np.testing.assert_array_equal(_bits(got[mi][:, ks]), _bits(src[mi][:, ks]), err_msg="knot steps, env %d" % mi)
                np.testing.assert_array_equal(_bits(got[mi][:, exact]), _bits(ref[mi][:, exact]), err_msg="copied steps, env %d, n = %d" % (mi, n))
                if not exact.all():
                    assert interp == "linear"
                    err = np.abs(got[mi][:, ~exact].astype(np.float64) - ref[mi][:, ~exact]).max()
                    worst = max(worst, float(err))
                    assert err <= 2.0 ** -22, "interpolated steps, env %d, n = %d: %.3e" % (mi, n, err)
    print("\n[H=%d r=%d %s] interpolated steps vs float64: max abs %.2e (bound %.2e)" % (H, r, interp, worst, 2.0 ** -22))
    # the [m, H, A] form is the [m, 1, H, A] form
    x = eng._t(rng.uniform(-1, 1, (m, H, A)))
    ph = _phase(eng, (1, 0, r - 1))
    a, b = eng.shape_actions(x.clone(), knots, ph), eng.shape_actions(x.clone()[:, None].contiguous(), knots, ph)
    np.testing.assert_array_equal(_bits(_np(a)), _bits(_np(b)[:, 0]))
    # spacing 1: the identity
    np.testing.assert_array_equal(_bits(_np(eng.shape_actions(x.clone(), HipEngine.knot_params(1, interp), ph))), _bits(_np(x)))
    return worst


def test_argument_checks_return_einval(gpu):
    """The two exports refuse bad arguments with CADM_EINVAL and a message naming themselves, before any HIP call (the null and dummy
    pointers next to the bad argument are never touched), and the engine plans normally afterwards."""
    prob, eng = _engine(6, True)
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(4096, dtype=torch.float32, device=eng.device)
    ibuf = torch.zeros(64, dtype=torch.int32, device=eng.device)
    P, I = ct.c_void_p(buf.data_ptr()), ct.c_void_p(ibuf.data_ptr())
    K = lambda s, i: ct.byref(_lib.KnotParams(s, i))
    mp = HipEngine.mppi_params()

    def einval(rc, name, frag):
        msg = lib.cadm_last_error().decode()
        assert rc == -1, "%s: expected CADM_EINVAL, got %d (%s)" % (name, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    einval(lib.cadm_shape_actions(ctx, K(0, 0), None, M, 4, P, None), "cadm_shape_actions", "spacing")
    einval(lib.cadm_shape_actions(ctx, K(-3, 1), I, M, 4, P, None), "cadm_shape_actions", "spacing")
    einval(lib.cadm_shape_actions(ctx, K(3, 2), None, M, 4, P, None), "cadm_shape_actions", "interp")
    einval(lib.cadm_shape_actions(ctx, K(3, -1), None, M, 4, P, None), "cadm_shape_actions", "interp")
    einval(lib.cadm_shape_actions(ctx, None, None, M, 4, P, None), "cadm_shape_actions", "bad arguments")
    einval(lib.cadm_shape_actions(ctx, K(3, 0), None, 0, 4, P, None), "cadm_shape_actions", "bad arguments")
    einval(lib.cadm_shape_actions(ctx, K(3, 0), None, M, 0, P, None), "cadm_shape_actions", "bad arguments")
    einval(lib.cadm_shape_actions(ctx, K(3, 0), None, M, 4, None, None), "cadm_shape_actions", "bad arguments")

    def plan(k, c=ctx, update=0, prm=ct.byref(mp)):
        return lib.cadm_knot_plan(c, k, None, None, None, update, prm, P, P, P, P, P, None, None, M, N, 0, 1, P, P, None, None)
    einval(plan(K(0, 0)), "cadm_knot_plan", "spacing")
    einval(plan(K(2, 7)), "cadm_knot_plan", "interp")
    einval(plan(K(1, 7)), "cadm_knot_plan", "interp")            # (an unknown interp is refused at spacing 1 too)
    einval(plan(K(3, 0), update=2), "cadm_knot_plan", "update")
    einval(plan(K(3, 0), prm=None), "cadm_knot_plan", "bad arguments")
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=M, H=5, seed=1, hidden_sizes=HID)
    deng = make_engine(dprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    einval(plan(K(3, 0), c=deng._ctx), "cadm_knot_plan", "continuous actions only")
    sprob = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=6, seed=3, hidden_sizes=HID, trained_like=True)
    seng = make_engine(sprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(seng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    einval(plan(K(3, 0), c=seng._ctx), "cadm_knot_plan", "sharded")
    assert lib.cadm_dist_destroy(seng._ctx) == 0
    with pytest.raises(ValueError, match="shape_actions"):
        eng.shape_actions(torch.zeros((M, 4, 5, A), dtype=torch.float32, device=eng.device), HipEngine.knot_params(3))
    with pytest.raises(ValueError, match="phase"):
        eng.shape_actions(torch.zeros((M, 4, 6, A), dtype=torch.float32, device=eng.device), HipEngine.knot_params(3), _phase(eng, (0, 1, 2)))
    # a spacing far beyond the horizon is legal: one knot, or two with a phase
    x = eng._t(np.random.default_rng(0).uniform(-1, 1, (M, 4, 6, A)))
    big = 2 ** 31 - 1
    got = _np(eng.shape_actions(x.clone(), HipEngine.knot_params(big), _phase(eng, (0, big - 2))))
    np.testing.assert_array_equal(_bits(got), _bits(kref.shape(_np(x), big, kref.HOLD, (0, big - 2))))
    assert _bps(got[0]) == [[]] * 4 and _bps(got[1]) == [[2]] * 4
    mean, var = _mean_var(eng, 6, 0)
    out = _np(eng.knot_plan(HipEngine.knot_params(3), None, None, None, HipEngine.icem_params(), prob["obs"], prob["cp_obs"], prob["cp_act"], mean, var, N,
                            seed=1, call=1))
    assert np.isfinite(out).all() and np.abs(out).max() <= 1.0


# ---------------------------------------------------------------------------------------------------------------------- 2: the loop
VARIANTS = [(6, 3, "hold", False), (7, 3, "linear", True)]
VARIANT_IDS = ["H%d-r%d-%s-%s" % (v[0], v[1], v[2], "cadm" if v[3] else "vanilla") for v in VARIANTS]
CASES = {
    "cem-white": dict(),
    "mppi-colored": dict(update="mppi", noise_beta=1.0),
    "keep3-one-valid-carry": dict(keep_elites=3, noise_beta=1.0),
    "decay": dict(decay=1.25, keep_elites=3),
    "add-mean": dict(add_mean_last=True, keep_elites=3),
    "best": dict(return_best=True, noise_beta=1.0),
    "score": dict(score=("mean_std", 1.0)),
    "constraint": dict(constraint=True, update="mppi", keep_elites=3),
}
PHASE = (0, 2)


def _binding_constraint(eng, prob, mean, var, knots, phase):
    """Bounds on observation dim 1 between the 20 % and 80 % quantiles of what shaped candidates around `mean` reach: they bind."""
    ctxv = eng.context_forward(prob["cp_obs"], prob["cp_act"]) if eng.C > 0 else None
    acts = eng.shape_actions(eng.sample_actions(mean, var, N, seed=4, call=1, it=0), knots, phase)
    _, traj = eng.rollout_returns(prob["obs"], ctxv, acts, seed=4, call=1, it=0, want_traj=True)
    x = _np(traj)[..., 1]
    return HipEngine.constraint_params([dict(dim=1, lo=float(np.quantile(x, 0.2)), hi=float(np.quantile(x, 0.8)))], "penalty", 4.0)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("H,r,interp,context", VARIANTS, ids=VARIANT_IDS)
def test_fused_equals_stepwise(gpu, H, r, interp, context, case):
    """`cadm_knot_plan` with device RNG == `planner.icem_plan(knots=, phase=)`, the same launches one at a time, bit for bit over two
    consecutive calls (the second consumes the first's carry): the plan, the best return, the carry and carry_valid.  Env 0 plans on
    phase 0, env 1 on phase 2; with kept elites only env 1 starts from a valid carry.  Every iteration's rolled-out candidates equal
    their own re-shaping -- they are on the grid, the kept-elite slots [0, K) and the mean slot included -- and there are n_it of them."""
    c = CASES[case]
    prob, eng = _engine(H, context)
    knots, phase = HipEngine.knot_params(r, interp), _phase(eng, PHASE)
    update, K, decay = c.get("update", "cem"), c.get("keep_elites", 0), c.get("decay", 1.0)
    icem = dict(noise_beta=c.get("noise_beta", 0.0), keep_elites=K, decay=decay, return_best=c.get("return_best", False),
                add_mean_last=c.get("add_mean_last", False))
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    score = HipEngine.score_params(*c["score"]) if "score" in c else None
    mean, var = _mean_var(eng, H, 7)
    cons = _binding_constraint(eng, prob, mean, var, knots, phase) if c.get("constraint") else None
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    ca = va = cb = vb = None
    if K > 0:
        carry0 = np.random.default_rng(5).uniform(-1, 1, (M, K, H, A)).astype(np.float32)
        ca, cb = eng._t(carry0), eng._t(carry0)
        va, vb = _phase(eng, (0, 1)), _phase(eng, (0, 1))
    for call in (1, 2):
        keep = mean.clone()
        a, ra = eng.knot_plan(knots, phase, cons, score, prm, *args, mean, var, N, carry=ca, carry_valid=va, seed=4, call=call,
                              want_best_return=True)
        np.testing.assert_array_equal(_bits(_np(mean)), _bits(_np(keep)), err_msg="the caller's init_mean after call %d" % call)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True, update=update,
                                            temperature=0.5, relative=True, score=score, constraints=cons, knots=knots, phase=phase, **icem)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        if K > 0:
            np.testing.assert_array_equal(_bits(_np(ca)), _bits(_np(cb)), err_msg="carry after call %d" % call)
            np.testing.assert_array_equal(_np(va), _np(vb))
            np.testing.assert_array_equal(_np(va), [1, 1])
        assert len(info) == ITERS
        for it in range(ITERS):
            acts = info[it]["actions"]
            assert acts.shape[1] == eng.icem_candidates(N, decay, it, K)
            again = eng.shape_actions(acts.clone(), knots, phase)
            np.testing.assert_array_equal(_bits(_np(again)), _bits(_np(acts)), err_msg="candidates of iteration %d are on the grid" % it)
        if decay > 1.0:
            assert info[1]["actions"].shape[1] < N
        acts0 = _np(info[0]["actions"])
        if K > 0 and call == 1:      # env 1 starts from its carry, moved one step on and shaped: its knot steps before H - 1 hold the carry's next step
            ks = [k for k in kref.knot_steps(H, r, PHASE[1]) if k < H - 1]
            np.testing.assert_array_equal(_bits(acts0[1, :K][:, ks]), _bits(carry0[1][:, [k + 1 for k in ks]]))
        if icem["add_mean_last"]:    # the mean slot of the last iteration: the clipped mean going into it, shaped
            want = eng.shape_actions(info[-2]["mean"].clamp(-1.0, 1.0), knots, phase)
            np.testing.assert_array_equal(_bits(_np(info[-1]["actions"])[:, K]), _bits(_np(want)))
        if cons is not None:
            v = _np(info[0]["violations"])
            assert (v > 0).any() and (v == 0).any(), "the constraint does not bind"
        mean = torch.cat([eng._t(a)[:, 1:], torch.zeros((M, 1, A), dtype=torch.float32, device=eng.device)], dim=1)      # the samplers' warm start


@pytest.mark.parametrize("beta", [0.0, 1.0], ids=["white", "colored"])
@pytest.mark.parametrize("H,r,interp,context", VARIANTS, ids=VARIANT_IDS)
def test_knots_leave_the_draws_alone(gpu, H, r, interp, context, beta):
    """Same (seed, call), no carry: iteration 0's candidates at each env's knot steps are bit-equal to the un-knotted loop's at those steps
    (the noise is keyed by element, the shaped mean keeps its knot steps), and differ elsewhere."""
    prob, eng = _engine(H, context)
    knots, phase = HipEngine.knot_params(r, interp), _phase(eng, PHASE)
    mean, var = _mean_var(eng, H, 11)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], mean, var, N)
    _, ik, _ = hplanner.icem_plan(eng, *args, noise_beta=beta, seed=9, call=3, return_info=True, knots=knots, phase=phase)
    _, i0, _ = hplanner.icem_plan(eng, *args, noise_beta=beta, seed=9, call=3, return_info=True)
    ak, a0 = _np(ik[0]["actions"]), _np(i0[0]["actions"])
    for mi, phi in enumerate(PHASE):
        ks = kref.knot_steps(H, r, phi)
        np.testing.assert_array_equal(_bits(ak[mi][:, ks]), _bits(a0[mi][:, ks]), err_msg="env %d" % mi)
        assert not np.array_equal(ak[mi], a0[mi])


@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_knots_off_is_the_loop_underneath(gpu, update):
    """spacing = 1 (whatever the interp and the phases) and knots = NULL: the plan, the best return and the carry of `constrained_plan`,
    `scored_plan` and `icem_plan` / `mppi_plan` on the same inputs, bit for bit."""
    H, K = 6, 3
    prob, eng = _engine(H, True)
    icem = dict(noise_beta=1.0, keep_elites=K, decay=1.25, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    mean, var = _mean_var(eng, H, 13)
    score = HipEngine.score_params("cvar", k=2)
    cons = _binding_constraint(eng, prob, mean, var, HipEngine.knot_params(1), None)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], mean, var, N)
    kw = dict(seed=5, call=2, want_best_return=True)
    plain = eng.mppi_plan if update == "mppi" else eng.icem_plan
    for cs, sc, under in ((cons, score, lambda **k: eng.constrained_plan(cons, score, prm, *args, **k)),
                          (None, score, lambda **k: eng.scored_plan(score, prm, *args, **k)),
                          (None, None, lambda **k: plain(prm, *args, **k))):
        runs = []
        for how in ((None, None), (HipEngine.knot_params(1, "linear"), _phase(eng, (1, -4))), (None, _phase(eng, (2, 1))), None):
            carry, valid = zero_carry(eng, M, K, H)
            if how is None:
                plan, best = under(carry=carry, carry_valid=valid, **kw)
            else:
                plan, best = eng.knot_plan(how[0], how[1], cs, sc, prm, *args, carry=carry, carry_valid=valid, **kw)
            runs.append((_bits(_np(plan)), _bits(_np(best)), _bits(_np(carry)), _np(valid)))
        for got in runs[:-1]:
            for x, y in zip(got, runs[-1]):
                np.testing.assert_array_equal(x, y)
    # and a grid does change the plan
    other = _np(eng.knot_plan(HipEngine.knot_params(3), None, None, None, prm, *args, *zero_carry(eng, M, K, H), seed=5, call=2))
    assert not np.array_equal(_bits(other), runs[-1][0])


@pytest.mark.parametrize("ret", ["mean", "best"])
@pytest.mark.parametrize("update", ["cem", "mppi"])
@pytest.mark.parametrize("H,r,interp,context", VARIANTS, ids=VARIANT_IDS)
def test_plan_structure(gpu, H, r, interp, context, update, ret):
    """HOLD: the returned plan is exactly piecewise constant on each env's grid -- the refitted mean (equal inputs at every step of a
    segment give equal reductions) and the best sequence alike -- with a breakpoint at every knot.  LINEAR: the plan is within 1e-6 of its
    own re-shaping (a mean of interpolants against the interpolant of the means: the rounding of an 8-term fp32 sum of values in
    [-1, 1], 2^-22 per partial sum before the division by 8, and three roundings of 2^-25 per interpolant); the best sequence, a
    candidate, exactly."""
    prob, eng = _engine(H, context)
    knots, phase = HipEngine.knot_params(r, interp), _phase(eng, PHASE)
    icem = dict(noise_beta=1.0, return_best=ret == "best")
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    mean, var = _mean_var(eng, H, 17)
    plan = eng.knot_plan(knots, phase, None, None, prm, prob["obs"], prob["cp_obs"], prob["cp_act"], mean, var, N, seed=2, call=1)
    again = _np(eng.shape_actions(plan.clone(), knots, phase))
    plan = _np(plan)
    assert np.isfinite(plan).all() and 0 < np.abs(plan).max() <= 1.0
    err = np.abs(plan.astype(np.float64) - again).max()
    print("\n[%s %s %s] plan against its own re-shaping: max abs %.2e" % (interp, update, ret, err))
    if interp == "hold" or ret == "best":
        np.testing.assert_array_equal(_bits(plan), _bits(again))
    else:
        assert err <= 1e-6
    for mi, phi in enumerate(PHASE):
        if interp == "hold":
            assert kref.breakpoints(plan[mi]) == kref.knot_steps(H, r, phi)[1:]
            np.testing.assert_array_equal(_bits(plan[mi]), _bits(kref.shape_one(plan[mi], r, kref.HOLD, phi)))


# ---------------------------------------------------------------------------------------------------------------------- 3: the models
GRIDS = {0: [3, 6], 1: [2, 5], 2: [1, 4]}      # H = 7, r = 3: the breakpoints of a HOLD plan by phase


def _shift(plan):
    return np.concatenate([plan[:, 1:], np.zeros((plan.shape[0], 1, A))], axis=1)


@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_model_call_anchor(gpu, context):
    """cem_knots = 3 alone takes the opt-in route; anchored on the call, every get_action plan breaks at steps {3, 6} and the model keeps
    no phase.  A model with default kwargs still takes today's route."""
    H = 7
    model, prob = _model(context, H, cem_knots=3)
    assert model._opt is not None and model._opt.knots == (3, "hold", "call") and model._opt.keep_elites == 0
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    for _ in range(3):
        plan = _act(model, prob, context, mean, var)
        assert plan.shape == (M, H, A) and np.isfinite(plan).all() and np.abs(plan).max() <= 1.0
        assert _bps(plan) == [GRIDS[0]] * M
        mean = _shift(plan)
    assert model._plan_phase is None and model._plan_carry is None
    model.reset_plan_carry()
    lin, _ = _model(context, H, cem_knots=3, cem_knot_interp="linear", cem_return="best")
    plan = _act(lin, prob, context, np.zeros((M, H, A)), var)
    np.testing.assert_array_equal(_bits(plan), _bits(_np(lin.engine.shape_actions(lin.engine._t(plan), lin._opt.knot_params))))
    assert _bps(plan) != [GRIDS[0]] * M
    default, _ = _model(context, H)
    spelled, _ = _model(context, H, cem_knots=1, cem_knot_interp="hold", cem_knot_anchor="call")
    assert default._opt is None and spelled._opt is None and default._plan_phase is None


@pytest.mark.parametrize("K", [0, 3], ids=["keep0", "keep3"])
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_model_episode_anchor(gpu, context, K):
    """cem_knot_anchor = "episode": the model's device phase advances by one modulo 3 per call -- the breakpoints of successive plans
    follow phases 0, 1, 2, 0 --, reset_plan_carry(mask) puts the masked envs back on phase 0 (and forgets their elites), reset_plan_carry()
    all of them, and another number of envs starts from zeros; with and without kept elites."""
    H = 7
    model, prob = _model(context, H, cem_knots=3, cem_knot_anchor="episode", cem_keep_elites=K)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)

    def step(want_phases):
        nonlocal mean
        plan = _act(model, prob, context, mean, var)
        assert np.isfinite(plan).all() and _bps(plan) == [GRIDS[p] for p in want_phases]
        mean = _shift(plan)
    assert model._plan_phase is None
    for ph in (0, 1, 2, 0):
        step([ph] * M)
    assert model._plan_phase.dtype == torch.int32 and _np(model._plan_phase).tolist() == [1, 1]
    model.reset_plan_carry([True, False])
    assert _np(model._plan_phase).tolist() == [0, 1]
    if K > 0:
        assert _np(model._plan_carry_valid).tolist() == [0, 1]
    step([0, 1])
    assert _np(model._plan_phase).tolist() == [1, 2]
    model.reset_plan_carry()
    assert _np(model._plan_phase).tolist() == [0, 0]
    step([0, 0])
    step([1, 1])
    with pytest.raises(ValueError, match="mask has 3 entries"):
        model.reset_plan_carry([True, False, True])
    one = {k: (v[:1] if isinstance(v, np.ndarray) and v.shape[0] == M else v) for k, v in prob.items()}
    plan = _act(model, one, context, mean[:1], var[:1])
    assert _bps(plan) == [GRIDS[0]] and _np(model._plan_phase).tolist() == [1]


def test_device_planner_state_follows_the_phase(gpu):
    """DevicePlannerState.act plans through the model's phase (its warm start is the plan moved one step on: breakpoints one step earlier),
    observe(done=) puts finished envs back on phase 0, reset() all of them."""
    from cadm_amd.caller import DevicePlannerState
    H = 7
    model, prob = _model(True, H, cem_knots=3, cem_knot_anchor="episode")
    state = DevicePlannerState(model, M)
    obs = prob["obs"]
    a = state.act(obs)
    assert tuple(a.shape) == (M, A) and np.isfinite(_np(a)).all()
    assert _np(model._plan_phase).tolist() == [1, 1]
    assert _bps(_np(state.prev_sol)[:, :H - 1]) == [[2, 5]] * M
    state.observe(obs, a, obs, done=np.array([1, 0]))
    assert _np(model._plan_phase).tolist() == [0, 1]
    state.act(obs)
    assert _np(model._plan_phase).tolist() == [1, 2]
    assert _bps(_np(state.prev_sol)[:, :H - 1]) == [[2, 5], [1, 4]]
    state.reset()
    assert _np(model._plan_phase).tolist() == [0, 0]
