"""GPU: the risk-aware candidate scores (csrc/score.hip: `cadm_particle_score`) and the opt-in planner loop that uses them
(`cadm_scored_plan`, csrc/icem.hip).

Geometry as tests/test_gpu_icem.py and tests/test_gpu_mppi.py: halfcheetah, vanilla and CaDM, hidden (32,) * 4, ensemble 5, m = 2,
num_elites = 8, 3 CEM iterations, H = 5 / 6.  Numpy restatement: tests/risk_ref.py, used at float64 on the float32 inputs.

The bar against float64 is the project's: 1e-5 of the env's largest |particle return| R.  What the kernel can owe: mu carries at most
p 2^-24 R (a chain of p additions and one division), each deviation r_j - mu (p + 1) 2^-24 R, and the root-mean-square of the deviations
no more than its largest term's error plus its own roundings: |S - S64| <= (1 + |kappa|) (p + 4) 2^-24 R; for cvar, k - 1 additions of
terms within R and one division: (k + 1) 2^-24 R.  Both sit under the bar for every case below (asserted where the cases are made)."""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

import risk_ref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import _np, make_engine, plan_model, zero_carry
from helpers import plan_act as _act
from helpers import planner_engine as _engine

pytestmark = pytest.mark.gpu

HID = (32,) * 4
M, N, KE, K, ITERS, A, E = 2, 64, 8, 3, 3, 6, 5
BAR = 1e-5
EPS = 2.0 ** -24
_model = functools.partial(plan_model, n_particles=10)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _rows(p, n, seed):
    """Particle returns in [-30, 30], both ends present in every env; some candidates constant across their particles."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-30.0, 30.0, (M, n, p)).astype(np.float32)
    rows[:, 0, 0], rows[:, -1, p - 1] = 30.0, -30.0
    const = [c for c in (1, 5, 62, 63, 64, 129) if c < n - 1]
    for c in const:
        rows[:, c, :] = rows[:, c, :1]
    if n == 1:
        rows[1, 0, :] = np.float32(-17.3)
    return rows, const


def _cases(p):
    """(mode, kappa, k): kappa in {-1, 0.5, 2}, k in {1, 2, p - 1, p}; the long rows (p >= 125) take the kappas their bound admits"""
    kappas = (-1.0, 0.5, 2.0) if p <= 20 else (-0.2, 0.2)
    ks = sorted({1, 2, p - 1, p})
    for kappa in kappas:
        assert (1.0 + abs(kappa)) * (p + 4) * EPS < BAR
    assert (p + 1) * EPS < BAR
    return ([("mean", 0.0, None)] + [(mode, kappa, None) for mode in ("mean_std", "member_std") for kappa in kappas]
            + [("cvar", 0.0, k) for k in ks])


def _ref(rows, mode, kappa, k):
    return risk_ref.score(rows.astype(np.float64), mode, kappa=float(np.float32(kappa)), k=k, E=E)


def _score(eng, rows, mode, kappa=0.0, k=None):
    return _np(eng.particle_score(eng._t(rows), mode, kappa=kappa, k=k))


# ---------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("p", [5, 10, 20, 125, 130])
def test_particle_score_against_float64(gpu, p):
    """`cadm_particle_score` on injected rows against the float64 restatement, every mode: p = 5 (q = 1), 10, 20, and the ends of the
    kernel's two load paths (p = 125: the longest rows staged in LDS; p = 130: read from global memory); n_local = 1 (one thread), 63 and
    64 (a ragged and a full wave), 130 (three workgroups, the last ragged); kappa in {-1, 0.5, 2} and k in {1, 2, p - 1, p}.
    Measured on an MI355X, worst |S - S64| / R over all cases of a p (the test prints it):
    p = 5: 1.8e-07; p = 10: 3.3e-07; p = 20: 2.0e-07; p = 125: 1.7e-06; p = 130: 1.7e-06 (bar 1e-05; the long rows' figure is the mean's
    own chain of p additions on the constant candidates)."""
    prob, eng = _engine(5, False, p)
    worst = 0.0
    for n in (1, 63, 64, 130):
        rows, const = _rows(p, n, 1000 * p + n)
        R = np.abs(rows).reshape(M, -1).max(axis=1)
        assert n == 1 or (R == 30.0).all()
        mean = _score(eng, rows, "mean")
        for mode, kappa, k in _cases(p):
            got = _score(eng, rows, mode, kappa, k)
            ref = _ref(rows, mode, kappa, k)
            assert got.shape == (M, n) and np.isfinite(got).all()
            err = (np.abs(got - ref).max(axis=1) / R).max()
            worst = max(worst, err)
            assert err <= BAR, "p=%d n=%d %s kappa=%g k=%s: %.2e of R" % (p, n, mode, kappa, k, err)
            if const:                                    # no spread, no tail: a constant candidate scores its constant
                assert np.abs(got[:, const] - rows[:, const, 0]).max() <= BAR * 30.0
            if n > 1 and mode in ("mean_std", "member_std"):      # ... and the others move by kappa times a spread of several units
                moved = np.delete(got - mean, const, axis=1)
                assert (np.sign(moved) == -np.sign(kappa)).all() and np.abs(moved).min() > 0.1 * abs(kappa)
            if mode == "cvar" and k == 1:
                np.testing.assert_array_equal(got, rows.min(axis=-1))
    print("\n[p=%d] worst |S - S64| / R = %.2e (bar %.0e)" % (p, worst, BAR), end="")


# ---------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("p", [5, 20, 130])
def test_mean_and_kappa_zero_are_the_particle_means_bits(gpu, p):
    """Mode MEAN is `cadm_particle_mean`; kappa = 0 in both std modes gives the same bits (mu - 0 sigma).  A candidate's score does
    not depend on where it sits in the call: a slice of the rows scores the same bits."""
    prob, eng = _engine(5, False, p)
    rows, _ = _rows(p, 130, 77 + p)
    want = _bits(_np(eng.particle_mean(eng._t(rows))))
    np.testing.assert_array_equal(_bits(_score(eng, rows, "mean")), want)
    np.testing.assert_array_equal(_bits(_score(eng, rows, 0, kappa=float("nan"), k=-3)), want)      # (MEAN reads neither)
    for mode in ("mean_std", "member_std"):
        np.testing.assert_array_equal(_bits(_score(eng, rows, mode, 0.0)), want)
    for mode, kappa, k in (("mean_std", 2.0, None), ("member_std", -1.0, None), ("cvar", 0.0, 2)):
        full = _score(eng, rows, mode, kappa, k)
        np.testing.assert_array_equal(_bits(_score(eng, rows, mode, kappa, k)), _bits(full))      # run to run
        part = _score(eng, np.ascontiguousarray(rows[1:, 37:101]), mode, kappa, k)
        np.testing.assert_array_equal(_bits(part), _bits(full[1:, 37:101]))


# ---------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("p", [10, 130])
def test_non_finite_rows_score_the_particle_mean(gpu, p):
    """Candidates with a NaN, +inf, -inf or both infinities among their particle returns: in every mode the bits of
    `cadm_particle_mean` come out for them, and their finite neighbours score what they score without them."""
    prob, eng = _engine(5, False, p)
    n = 130
    clean, _ = _rows(p, n, 300 + p)
    bad = clean.copy()
    bad[0, 2, 3] = np.nan
    bad[0, 63, 0] = np.inf
    bad[0, 64, p - 1] = -np.inf
    bad[1, 0, 1], bad[1, 0, p - 2] = np.inf, -np.inf
    bad[1, 129, 0], bad[1, 129, 4] = np.nan, np.inf
    bad[1, 70, :] = np.inf
    hit = np.zeros((M, n), bool)
    hit[0, [2, 63, 64]] = True
    hit[1, [0, 129, 70]] = True
    plain = _np(eng.particle_mean(eng._t(bad)))
    assert np.isnan(plain[0, 2]) and plain[0, 63] == np.inf and plain[0, 64] == -np.inf and np.isnan(plain[1, 0]) and plain[1, 70] == np.inf
    for mode, kappa, k in _cases(p):
        got, ok = _score(eng, bad, mode, kappa, k), _score(eng, clean, mode, kappa, k)
        np.testing.assert_array_equal(_bits(got)[hit], _bits(plain)[hit], err_msg="%s %g %s" % (mode, kappa, k))
        np.testing.assert_array_equal(_bits(got)[~hit], _bits(ok)[~hit], err_msg="%s %g %s" % (mode, kappa, k))
        assert np.isfinite(got[~hit]).all()


# ---------------------------------------------------------------------------------------------------------------------- 4
LOOP = [      # mode, kappa, k, update, context, H, beta, decay, K, return_best, add_mean_last
    ("mean_std", 2.0, None, "cem", False, 5, 0.0, 1.0, 0, False, False),
    ("mean_std", 0.5, None, "mppi", True, 6, 1.0, 1.25, 3, True, True),
    ("member_std", 2.0, None, "cem", True, 5, 1.0, 1.25, 3, True, True),
    ("member_std", -1.0, None, "mppi", False, 6, 0.0, 1.0, 0, False, False),
    ("cvar", 0.0, 2, "cem", True, 6, 0.0, 1.5, 3, False, False),
    ("cvar", 0.0, 3, "mppi", False, 5, 1.0, 1.25, 3, True, True),
]


def _params(update, **icem):
    return HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)


@pytest.mark.parametrize("mode,kappa,k,update,context,H,beta,decay,keep,best,addmean", LOOP,
                         ids=["%s-%s-%s-H%d-beta%g-decay%g-K%d-%s%s" % (r[0], r[3], "cadm" if r[4] else "vanilla", r[5], r[6], r[7], r[8],
                                                                       "best" if r[9] else "mean", "-addmean" if r[10] else "") for r in LOOP])
def test_fused_equals_stepwise(gpu, mode, kappa, k, update, context, H, beta, decay, keep, best, addmean):
    """`cadm_scored_plan` with device RNG == the same loop one launch at a time (`planner.icem_plan(..., score=...)`), bit for bit: the
    plan, the best return, the carried elites and their valid flags over two consecutive calls.  Every stepwise score is held to the
    float64 restatement on the device's own rows, the elites are the top num_elites by SCORE and the best return is the best score."""
    p = 10
    prob, eng = _engine(H, context, p)
    score = HipEngine.score_params(mode, kappa, k)
    icem = dict(noise_beta=beta, keep_elites=keep, decay=decay, return_best=best, add_mean_last=addmean)
    prm = _params(update, **icem)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    (ca, va), (cb, vb) = zero_carry(eng, M, keep, H), zero_carry(eng, M, keep, H)
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2):
        a, ra = eng.scored_plan(score, prm, *args, mean, var, N, carry=ca, carry_valid=va, seed=4, call=call, want_best_return=True)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                            update=update, temperature=0.5, relative=True, score=score, **icem)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
        np.testing.assert_array_equal(a, _np(b), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        if keep:
            np.testing.assert_array_equal(_np(ca), _np(cb), err_msg="carry after call %d" % call)
            np.testing.assert_array_equal(_np(va), [1, 1])
            np.testing.assert_array_equal(_np(vb), [1, 1])
        assert [x["actions"].shape[1] for x in info] == [eng.icem_candidates(N, decay, it, keep) for it in range(ITERS)]
        best_score = np.full((M,), -np.inf)
        for it, x in enumerate(info):
            rows, cand = _np(x["rows"]), _np(x["cand"])
            assert np.isfinite(rows).all()
            ref = _ref(rows, mode, kappa, k)
            R = np.abs(rows).reshape(M, -1).max(axis=1)
            assert (np.abs(cand - ref).max(axis=1) <= BAR * R).all(), "call %d iteration %d" % (call, it)
            np.testing.assert_array_equal(_np(x["elites"]), risk_ref.top_elites(cand, KE))
            best_score = np.maximum(best_score, cand.max(axis=1))
        np.testing.assert_array_equal(_np(ra), best_score.astype(np.float32))
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), np.float32)], axis=1)      # the samplers' warm start


# ---------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_mean_score_is_the_existing_entry(gpu, update):
    """`cadm_scored_plan` with score NULL or CADM_SCORE_MEAN == `cadm_icem_plan` / `cadm_mppi_plan`, bit for bit: plan, best return and
    carried elites of two consecutive calls."""
    H, p = 6, 10
    prob, eng = _engine(H, True, p)
    prm = _params(update, noise_beta=1.0, keep_elites=K, decay=1.25, return_best=True, add_mean_last=True)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    existing = eng.mppi_plan if update == "mppi" else eng.icem_plan
    carries = [zero_carry(eng, M, K, H) for _ in range(3)]
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2):
        want, wr = existing(prm, *args, mean, var, N, carry=carries[0][0], carry_valid=carries[0][1], seed=9, call=call, want_best_return=True)
        for score, (c, v) in ((None, carries[1]), (HipEngine.score_params("mean", kappa=float("nan"), k=99), carries[2])):
            got, gr = eng.scored_plan(score, prm, *args, mean, var, N, carry=c, carry_valid=v, seed=9, call=call, want_best_return=True)
            np.testing.assert_array_equal(_bits(_np(got)), _bits(_np(want)))
            np.testing.assert_array_equal(_bits(_np(gr)), _bits(_np(wr)))
            np.testing.assert_array_equal(_np(c), _np(carries[0][0]))
            np.testing.assert_array_equal(_np(v), [1, 1])
        mean = np.concatenate([_np(want)[:, 1:], np.zeros((M, 1, A), np.float32)], axis=1)


@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_get_action_with_kappa_zero_is_get_action_with_the_mean(gpu, context):
    """cem_score="mean_std", cem_risk=0.0 plans through `cadm_scored_plan`, cem_score="mean" with the same other kwargs through
    `cadm_icem_plan` / `cadm_mppi_plan`: the same plans over two calls, bit for bit.  A model built with the new kwargs spelled out
    at their defaults holds no opt-in state at all."""
    H = 5
    plain, prob = _model(context, H, cem_score="mean", cem_risk=None)
    assert plain._opt is None
    for other in (dict(cem_keep_elites=K, cem_noise_beta=1.0), dict(cem_update="mppi", cem_temperature=0.3, cem_keep_elites=K)):
        a, _ = _model(context, H, cem_score="mean", **other)
        b, _ = _model(context, H, cem_score="mean_std", cem_risk=0.0, **other)
        assert a._opt.score_params is None and b._opt.score_params is not None and b._opt.score_params.mode == 1
        mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
        for _ in range(2):
            pa, pb = _act(a, prob, context, mean, var), _act(b, prob, context, mean, var)
            assert np.isfinite(pa).all() and 0 < np.abs(pa).max() <= 1.0
            np.testing.assert_array_equal(pa, pb)
            np.testing.assert_array_equal(_np(a._plan_carry), _np(b._plan_carry))
            mean = np.concatenate([pa[:, 1:], np.zeros((M, 1, A))], axis=1)


# ---------------------------------------------------------------------------------------------------------------------- 6
def test_the_score_changes_the_plan_and_the_elites_are_the_top_scores(gpu):
    """A stochastic model (Philox head noise, five different members), kappa = 2 against kappa = 0: another plan.  The rows of the
    last iteration, scored with the float64 restatement: the refit's elites are the top 8 of those scores."""
    H, p = 5, 20
    prob, eng = _engine(H, True, p)
    assert not eng.deterministic
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    plans = {}
    for kappa in (0.0, 2.0):
        score = HipEngine.score_params("mean_std", kappa)
        plans[kappa] = _np(eng.scored_plan(score, HipEngine.icem_params(), *args, seed=5, call=1))
    assert np.abs(plans[2.0] - plans[0.0]).max() > 1e-3
    score = HipEngine.score_params("mean_std", 2.0)
    plan, info, _ = hplanner.icem_plan(eng, *args, seed=5, call=1, return_info=True, score=score)
    np.testing.assert_array_equal(_np(plan), plans[2.0])
    rows = _np(info[-1]["rows"])
    assert rows.shape == (M, N, p) and np.isfinite(rows).all() and rows.std(axis=-1).min() > 0
    np.testing.assert_array_equal(_np(info[-1]["elites"]), risk_ref.top_elites(_ref(rows, "mean_std", 2.0, None), KE))


# ---------------------------------------------------------------------------------------------------------------------- 7
def test_argument_checks_return_einval(gpu):
    """The new exports refuse bad arguments with CADM_EINVAL and a message naming themselves.  The checks run before any HIP call: the
    null pointers next to the bad argument are never touched and the output keeps its sentinel; the engine plans normally afterwards."""
    p = 10
    prob, eng = _engine(5, True, p)
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(8192, dtype=torch.float32, device=eng.device)
    out = torch.full((M * N,), 123.0, dtype=torch.float32, device=eng.device)
    ibuf = torch.zeros(64, dtype=torch.int32, device=eng.device)
    P, O, I = ct.c_void_p(buf.data_ptr()), ct.c_void_p(out.data_ptr()), ct.c_void_p(ibuf.data_ptr())

    def einval(rc, name, frag):
        msg = lib.cadm_last_error().decode()
        assert rc == -1, "%s: expected CADM_EINVAL, got %d (%s)" % (name, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    def sc(mode, kappa=0.0, k=0):
        return ct.byref(HipEngine.score_params(mode, kappa, k))

    def score(s, c=ctx, rows=P, m=M, n=N, dst=O):
        return lib.cadm_particle_score(c, rows, m, n, s, dst, None)

    def plan(s, update=0, prm=None, c=ctx, n=N, carry=P, valid=I, cp=P, dst=O):
        prm = HipEngine.mppi_params() if prm is None else prm
        return lib.cadm_scored_plan(c, s, update, ct.byref(prm), P, cp, cp, P, P, carry, valid, M, n, 0, 1, P, dst, None, None)
    bad_scores = [(sc(4), "unknown score mode"), (sc(-1), "unknown score mode"), (sc(1, float("nan")), "kappa"), (sc(1, float("inf")), "kappa"),
                  (sc(2, float("-inf")), "kappa"), (sc(2, float("nan")), "kappa"), (sc(3, 0.0, 0), "cvar k"), (sc(3, 0.0, -1), "cvar k"),
                  (sc(3, 0.0, p + 1), "cvar k")]
    for s, frag in bad_scores:
        einval(score(s), "cadm_particle_score", frag)
        einval(score(s, rows=None, dst=None), "cadm_particle_score", "bad arguments")
        for update in (0, 1):
            einval(plan(s, update), "cadm_scored_plan", frag)
    einval(score(sc(1), m=0), "cadm_particle_score", "bad arguments")
    einval(score(sc(1), n=0), "cadm_particle_score", "bad arguments")
    einval(score(sc(1), c=None), "cadm_particle_score", "bad arguments")
    # the loop's own refusals, under a legal score
    ok = sc("cvar", 0.0, 2)
    einval(plan(ok, update=2), "cadm_scored_plan", "update 2")
    einval(plan(ok, update=-1), "cadm_scored_plan", "update -1")
    einval(lib.cadm_scored_plan(ctx, ok, 0, None, P, P, P, P, P, P, I, M, N, 0, 1, P, O, None, None), "cadm_scored_plan", "bad arguments")
    einval(plan(ok, prm=HipEngine.mppi_params(keep_elites=KE + 1)), "cadm_scored_plan", "keep_elites")
    einval(plan(ok, prm=HipEngine.mppi_params(decay=0.9)), "cadm_scored_plan", "decay")
    einval(plan(ok, prm=HipEngine.mppi_params(noise_beta=-1.0)), "cadm_scored_plan", "noise_beta")
    einval(plan(ok, prm=HipEngine.mppi_params(keep_elites=K), carry=None), "cadm_scored_plan", "carry")
    einval(plan(ok, n=KE - 1), "cadm_scored_plan", "num_elites")
    einval(plan(ok, cp=None), "cadm_scored_plan", "cp_obs/cp_act")
    einval(plan(ok, dst=None), "cadm_scored_plan", "bad arguments")
    einval(plan(ok, update=1, prm=HipEngine.mppi_params(temperature=0.0)), "cadm_scored_plan", "temperature")
    dprob, deng = _engine(5, True, p, env="cartpole")
    einval(plan(ok, c=deng._ctx), "cadm_scored_plan", "continuous actions only")
    # a candidate-sharded ctx (a host-supplied all-gather registered for two ranks; it is never called): the loop refuses, the score works
    sprob = synth.make_problem(env="halfcheetah", context=True, E=E, m=M, H=5, seed=3, hidden_sizes=HID, trained_like=True)
    seng = make_engine(sprob, p=p, num_elites=KE, num_cem_iters=ITERS)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(seng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    einval(plan(ok, c=seng._ctx), "cadm_scored_plan", "sharded")
    rows, _ = _rows(p, 63, 5)
    np.testing.assert_array_equal(_bits(_score(seng, rows, "cvar", k=2)), _bits(_score(eng, rows, "cvar", k=2)))
    assert lib.cadm_dist_destroy(seng._ctx) == 0
    torch.cuda.synchronize()
    assert (_np(out) == 123.0).all()                     # no refused call wrote a score or a plan
    # the Python layer: unknown mode names, rows of another particle count
    with pytest.raises(KeyError):
        HipEngine.score_params("variance")
    with pytest.raises(ValueError, match="particle_score: rows"):
        eng.particle_score(torch.zeros((M, N, p + 1), dtype=torch.float32, device=eng.device), "mean_std", 1.0)
    res = _np(eng.scored_plan(HipEngine.score_params("cvar", k=2), HipEngine.icem_params(noise_beta=1.0), prob["obs"], prob["cp_obs"], prob["cp_act"],
                              prob["init_mean"], prob["init_var"], N, seed=1, call=1))
    assert np.isfinite(res).all() and np.abs(res).max() <= 1.0
    # update 0 reads params->icem only: a temperature no MPPI call would take changes nothing (a real workspace: this call runs)
    dev = [eng._t(prob[key]) for key in ("obs", "cp_obs", "cp_act", "init_mean", "init_var")]
    ws, dst = eng._loop_workspace(False, M, N, 0), torch.empty((M, 5, A), dtype=torch.float32, device=eng.device)
    rc = lib.cadm_scored_plan(ctx, ok, 0, ct.byref(HipEngine.mppi_params(temperature=0.0, noise_beta=1.0)), *[_lib.ptr(t) for t in dev], None, None,
                              M, N, 1, 1, _lib.ptr(ws), _lib.ptr(dst), None, eng.stream)
    assert rc == 0, lib.cadm_last_error().decode()
    np.testing.assert_array_equal(_np(dst), res)


def test_refusals_at_construction(gpu, monkeypatch):
    from cadm_amd.envs import make_env_spec
    for bad, msg in ((dict(cem_score="variance", cem_risk=1.0), "cem_score must be"), (dict(cem_score="mean", cem_risk=0.5), "cem_risk configures"),
                     (dict(cem_risk=2.0, cem_keep_elites=2), "cem_risk configures"), (dict(cem_score="mean_std"), "needs a finite cem_risk"),
                     (dict(cem_score="member_std", cem_risk=float("nan")), "needs a finite cem_risk"), (dict(cem_score="cvar", cem_risk=float("inf")), "needs a finite cem_risk"),
                     (dict(cem_score="cvar", cem_risk=0.0), "tail fraction"), (dict(cem_score="cvar", cem_risk=1.01), "tail fraction"),
                     (dict(use_cem=False, cem_score="cvar", cem_risk=0.1), "need use_cem=True"),
                     (dict(cem_score="mean_std", cem_risk=1.0, cem_keep_elites=51), "exceeds the planner's 50 elites")):
        for context in (False, True):
            with pytest.raises(ValueError, match=msg):
                _model(context, 5, **bad)
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        _model(True, 5, env=make_env_spec("cartpole"), cem_score="mean_std", cem_risk=1.0)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        _model(True, 5, process_group=object(), cem_score="cvar", cem_risk=0.5)


# ---------------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_class_route_under_cvar(gpu, context):
    """cem_score="cvar", cem_risk=0.1 with 20 particles (k = 2) and carried elites: two get_action calls equal the direct
    `scored_plan` calls with the model's seed and call counter, carry included; reset_plan_carry makes the next plan a fresh model's;
    DevicePlannerState.act (caller.py) takes the same entry point."""
    from cadm_amd.caller import DevicePlannerState
    H, p = 6, 20
    kw = dict(cem_score="cvar", cem_risk=0.1, cem_keep_elites=K, cem_noise_beta=1.0)
    model, prob = _model(context, H, n_particles=p, **kw)
    eng = model.engine
    assert model._opt is not None and model._opt.score == ("cvar", 0.0, 2) and model._opt.score_params.k == 2 and model._opt.score_params.mode == 3
    cp = (prob["cp_obs"], prob["cp_act"]) if context else (None, None)
    score, prm = HipEngine.score_params("cvar", k=2), HipEngine.icem_params(noise_beta=1.0, keep_elites=K)
    carry, valid = zero_carry(eng, M, K, H)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    plans = []
    for call in (1, 2):
        got = _act(model, prob, context, mean, var)
        assert model._call == call and got.shape == (M, H, A) and np.isfinite(got).all() and 0 < np.abs(got).max() <= 1.0
        want = _np(eng.scored_plan(score, prm, prob["obs"], cp[0], cp[1], mean, var, N, carry=carry, carry_valid=valid, seed=model.seed, call=call))
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(_np(model._plan_carry), _np(carry))
        np.testing.assert_array_equal(_np(model._plan_carry_valid), [1, 1])
        plans.append(got)
        mean = np.concatenate([got[:, 1:], np.zeros((M, 1, A))], axis=1)
    # the score is in the loop: the plain-mean planner with the same switches, seed and call plans something else
    plain = _np(eng.icem_plan(prm, prob["obs"], cp[0], cp[1], np.zeros((M, H, A)), var, N, carry=torch.zeros_like(carry),
                              carry_valid=torch.zeros_like(valid), seed=model.seed, call=1))
    assert np.abs(plans[0] - plain).max() > 1e-3
    fresh, _ = _model(context, H, n_particles=p, **kw)
    fresh._call = model._call
    model.reset_plan_carry()
    np.testing.assert_array_equal(_np(model._plan_carry_valid), [0, 0])
    np.testing.assert_array_equal(_act(model, prob, context, mean, var), _act(fresh, prob, context, mean, var))
    if not context:
        return
    # caller.py: its state starts from a zero warm start and a zero history; the model's carry is valid from the call above
    state = DevicePlannerState(model, M)
    c2, v2 = model._plan_carry.clone(), model._plan_carry_valid.clone()
    act = state.act(prob["obs"])
    zero = torch.zeros((M, H, A), dtype=torch.float32, device=eng.device)
    want = eng.scored_plan(score, prm, prob["obs"], torch.zeros_like(state.hist_obs), torch.zeros_like(state.hist_act), zero, state.init_var, N,
                           carry=c2, carry_valid=v2, seed=model.seed, call=model._call)
    assert tuple(act.shape) == (M, A)
    np.testing.assert_array_equal(_np(act), _np(want)[:, 0])
    np.testing.assert_array_equal(_np(model._plan_carry), _np(c2))
    state.observe(prob["obs"], act, prob["obs"], done=np.array([1, 0]))
    np.testing.assert_array_equal(_np(model._plan_carry_valid), [0, 1])


# ---------------------------------------------------------------------------------------------------------------------- 9
def test_the_dispatcher_calls_the_public_method(gpu):
    """`HipEngine.opt_in_plan` under a `PlanOptions` for each update, with and without a score == the public method those options stand
    for, given structs built by hand, on the same (seed, call) and a valid carry: plan, best return and the carry it leaves, bit for bit."""
    from cadm_amd.planner import PlanOptions
    H, p = 5, 10
    prob, eng = _engine(H, True, p)
    icem, mppi = dict(noise_beta=1.0, keep_elites=K), dict(cem_update="mppi", cem_temperature=0.5, cem_temperature_relative=True)
    lam, cvar = HipEngine.mppi_params(temperature=0.5, relative=True, **icem), HipEngine.score_params("cvar", k=2)
    routes = [(dict(), eng.icem_plan, (HipEngine.icem_params(**icem),)), (mppi, eng.mppi_plan, (lam,)),
              (dict(cem_score="cvar", cem_risk=0.2), eng.scored_plan, (cvar, HipEngine.icem_params(**icem))),
              (dict(mppi, cem_score="cvar", cem_risk=0.2), eng.scored_plan, (cvar, lam))]
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    carry = eng._t(np.random.default_rng(1).uniform(-1, 1, (M, K, H, A)).astype(np.float32))
    plans = []
    for kw, method, head in routes:
        opt = PlanOptions.from_kwargs(cem_noise_beta=1.0, cem_keep_elites=K, use_cem=True, n_particles=p, **kw)
        (ca, va), (cb, vb) = [(carry.clone(), torch.ones((M,), dtype=torch.int32, device=eng.device)) for _ in range(2)]
        got, gr = eng.opt_in_plan(opt, *args, carry=ca, carry_valid=va, seed=6, call=3, want_best_return=True)
        want, wr = method(*head, *args, carry=cb, carry_valid=vb, seed=6, call=3, want_best_return=True)
        assert np.isfinite(_np(got)).all() and 0 < np.abs(_np(got)).max() <= 1.0
        np.testing.assert_array_equal(_bits(_np(got)), _bits(_np(want)))
        np.testing.assert_array_equal(_bits(_np(gr)), _bits(_np(wr)))
        np.testing.assert_array_equal(_np(ca), _np(cb))
        assert not np.array_equal(_np(ca), _np(carry))
        plans.append(_np(got))
    assert not any(np.array_equal(plans[i], plans[j]) for i in range(4) for j in range(i))      # four routes, four plans


def test_each_update_keeps_its_workspace(gpu):
    """icem_plan, mppi_plan, icem_plan on one engine: neither workspace is reallocated (the tensors are held here, so a new allocation
    could not land on an old address)."""
    prob, eng = _engine(5, True, 10)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    eng.icem_plan(HipEngine.icem_params(), *args, seed=1, call=1)
    wi = eng._loop_workspace(False, M, N, 0)
    eng.mppi_plan(HipEngine.mppi_params(), *args, seed=1, call=1)
    wm = eng._loop_workspace(True, M, N, 0)
    ptrs = wi.data_ptr(), wm.data_ptr()
    assert ptrs[0] != ptrs[1] and wm.numel() > wi.numel()
    eng.icem_plan(HipEngine.icem_params(), *args, seed=1, call=2)
    assert (eng._loop_workspace(False, M, N, 0).data_ptr(), eng._loop_workspace(True, M, N, 0).data_ptr()) == ptrs
