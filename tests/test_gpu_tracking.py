"""GPU: run-time tracking targets of the opt-in planner -- the kernel (`cadm_tracking_returns`, csrc/tracking.hip) on synthetic
trajectories and at its edges, the `first` cut, the fused loop (`cadm_tracking_plan`) against the stepwise one, targets that bind and
targets that are all NaN, episode time through the class route, and the refusals.

Geometries: those tests/test_gpu_constraints.py builds -- its hopper_like declaration (D = 11, H = 3, p = 5: the same JIT module) and the
compiled-in halfcheetah 200 x 4 kernel (H = 8, p = 20 and H = 5, p = 5); the class route on tests/helpers.py's `plan_model`.  Numpy
restatement: tests/tracking_ref.py.

Bound of the kernel against the float64 restatement, derived, not measured: |out - ref| <= (H K + 4) 2^-23 S + 2^-24 |ref| per row, S the
row's sum of |w c| over the counted (step, term) pairs -- one rounding each for e, c and w c, one per add of the chain, the final
subtraction; doubled for slack (tests/test_tracking_ref.py holds a float32 emulation of the chain to it on the CPU).  `cost_out`: the
same without the last term.  Rows with nothing counted are compared bit for bit with `rows_in`.
Measured on an MI355X, worst |err| / bound: rows 0.78 (K = 1, 45 rows), 0.06 at K = 16; cost 0.23; behind a `first` cut 0.14."""
import ctypes as ct

import numpy as np
import pytest
import torch

import tracking_ref as tref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import _np, make_engine, plan_act, plan_model, zero_carry
from test_gpu_constraints import binding_bounds, hopper_like, iteration0_traj

pytestmark = pytest.mark.gpu

M, N, KE, ITERS = 2, 24, 8, 3


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def engines(gpu):
    """name -> (problem, engine), built when first asked for: "hopper" (hopper_like with context, p = 5, H = 3), "hc8" (halfcheetah
    with context, p = 20, H = 8), "hc5" / "hc5-vanilla" (halfcheetah, p = 5, H = 5); 8 elites, 3 CEM iterations but hc8."""
    built = {}

    def get(name):
        if name not in built:
            if name == "hopper":
                prob = synth.make_problem(env=hopper_like(), context=True, E=5, m=M, H=3, seed=52)
                built[name] = (prob, make_engine(prob, p=5, num_elites=KE, num_cem_iters=ITERS))
            elif name == "hc8":
                prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=8, seed=51)
                built[name] = (prob, make_engine(prob, p=20))
            else:
                prob = synth.make_problem(env="halfcheetah", context=name == "hc5", E=5, m=M, H=5, seed=3, trained_like=True)
                built[name] = (prob, make_engine(prob, p=5, num_elites=KE, num_cem_iters=ITERS))
        return built[name]
    yield get
    for _, eng in built.values():
        eng.close()


ENGINE_OF = {"hopper-240": "hopper", "hopper-45": "hopper", "halfcheetah-320": "hc8"}


# ---------------------------------------------------------------------------------------------------------------------- 1: the kernel
def check_kernel_case(eng, H, K, case, what, all_nan_env=None):
    """One (traj, rows, terms, targets, offset) case of `cadm_tracking_returns` against tests/tracking_ref.py within the derived bound: the
    rows and `cost_out`, `rows_in` left alone, rows with nothing counted bit for bit, `rows_out` aliasing `rows_in`.  Returns (worst
    |err| / bound of the rows, of the cost, the number of rows with nothing counted, the kernel's rows)."""
    traj, rows, terms, targets, offset = case
    ref, cost_ref, S, counted = tref.tracking(traj, rows, terms, targets, offset)
    t_dev, r_dev = eng._t(traj), eng._t(rows)
    out, cost = eng.tracking_returns(t_dev, r_dev, terms, targets, offset=offset, want_cost=True)
    out, cost = _np(out), _np(cost)
    np.testing.assert_array_equal(_bits(_np(r_dev)), _bits(rows), err_msg=what + ": rows_in was written")
    none = counted == 0
    np.testing.assert_array_equal(_bits(out[none]), _bits(rows[none]), err_msg=what + ": rows with nothing counted")
    assert (cost[none] == 0).all()
    lim, lim_cost = tref.bound(S, ref, H, K), tref.bound(S, None, H, K)
    err, err_cost = np.abs(out - ref), np.abs(cost - cost_ref)
    assert np.isfinite(out).all()
    assert (err[~none] <= lim[~none]).all(), "%s: rows, worst |err| / bound %.3f" % (what, (err[~none] / lim[~none]).max())
    assert (err_cost[~none] <= lim_cost[~none]).all(), "%s: cost, worst |err| / bound %.3f" % (what, (err_cost[~none] / lim_cost[~none]).max())
    worst = worst_cost = 0.0
    if (~none).any():
        worst = float((err[~none] / lim[~none]).max())
        worst_cost = float((err_cost[~none] / np.maximum(lim_cost[~none], 1e-300)).max())
    if all_nan_env is not None:
        assert none[all_nan_env].all()
    alias = r_dev.clone()
    assert eng.tracking_returns(t_dev, alias, terms, targets, offset=offset, out=alias) is alias
    np.testing.assert_array_equal(_bits(_np(alias)), _bits(out), err_msg=what + ": rows_out aliasing rows_in")
    return worst, worst_cost, int(none.sum()), out


@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("shape", list(ENGINE_OF))
def test_kernel_against_restatement(engines, shape, K):
    """`cadm_tracking_returns` on `synth_traj` against tests/tracking_ref.py within the derived bound, for T in {1, H, H - 1, H + 3} --
    K = 1: each kind alone; K = 16: the three kinds in turn -- with offsets that are negative, in range and beyond T, a fifth of every
    env's targets NaN and (m = 4) one env whose targets are all NaN; rows with nothing counted keep their bits; `rows_out` aliasing
    `rows_in` gives the same bits.  240 and 320 rows end in a partial workgroup and their workgroups span envs; 45 rows are fewer than one
    workgroup and their odd steps' spans are not 16-byte aligned (the scalar-load path)."""
    _, eng = engines(ENGINE_OF[shape])
    H, m, n, p, D = tref.SHAPES[shape][:5]
    assert (eng.H, eng.p, eng.D) == (H, p, D)
    if shape == "hopper-45":
        assert (m * n * p * D * 4) % 16 != 0
    worst = worst_cost = 0.0
    skipped_rows = 0
    for T in (1, H, H - 1, H + 3):
        for kinds in ([(k,) for k in tref.KINDS] if K == 1 else [tref.KINDS]):
            case = tref.make_case(shape, K, T, kinds=kinds, seed=len(kinds[0]))
            what = "%s K=%d T=%d %s" % (shape, K, T, "/".join(kinds))
            r, rc, skipped, _ = check_kernel_case(eng, H, K, case, what, tref.ALL_NAN_ENV if m == 4 else None)
            worst, worst_cost, skipped_rows = max(worst, r), max(worst_cost, rc), skipped_rows + skipped
    assert m != 4 or skipped_rows > 0
    print("\n[%s K=%d] worst |err| / bound: rows %.3f, cost %.3f" % (shape, K, worst, worst_cost))


# ---------------------------------------------------------------------------------------------------------------------- 2: the first cut
def test_first_cut(engines):
    """`first` drawn over 0 .. H with 0 and H planted: steps behind it are not counted -- a NaN planted there in a tracked dim does not reach
    the row, the result is the restatement's with the same cut --, a NaN at or before it makes the row non-finite, a NaN in an untracked
    dim never does."""
    shape = "halfcheetah-320"
    _, eng = engines("hc8")
    H, m, n, p, D = tref.SHAPES[shape][:5]
    K = 3
    traj, rows, terms, _, _ = tref.make_case(shape, K, 1)
    tracked = sorted({c["dim"] for c in terms})
    free = next(d for d in range(D) if d not in tracked)
    targets = np.full((m, 1, K), 0.5, np.float32)
    rng = np.random.default_rng(77)
    first = rng.integers(0, H + 1, (m, n, p)).astype(np.int32)
    first[0, 0, 0], first[0, 0, 1] = 0, H
    ref, _, S, counted = tref.tracking(traj, rows, terms, targets, None, first)
    assert (counted == K * np.minimum(first + 1, H)).all()
    bad = traj.copy()
    behind = np.arange(H)[:, None, None, None] > first[None]
    for d in tracked:
        bad[..., d][behind] = np.nan                       # everything behind the cut
    bad[..., free] = np.where(rng.uniform(size=bad.shape[:-1]) < 0.3, np.nan, bad[..., free])      # an untracked dim, anywhere
    hit = rng.uniform(size=(m, n, p)) < 0.25                # rows that take a NaN at or before the cut
    hit[0, 0, 0], hit[0, 0, 1] = True, False
    at = np.minimum(rng.integers(0, H, (m, n, p)), np.minimum(first, H - 1))
    at[0, 0, 0] = 0
    mi, ni, j = np.nonzero(hit)
    bad[at[hit], mi, ni, j, tracked[0]] = np.nan
    out, cost = eng.tracking_returns(bad, rows, terms, targets, first=first, want_cost=True)
    out, cost = _np(out), _np(cost)
    assert np.isnan(out[hit]).all() and np.isnan(cost[hit]).all(), "a NaN at or before the cut must reach the row"
    ok = ~hit
    assert np.isfinite(out[ok]).all(), "a NaN behind the cut, or in an untracked dim, reached a row"
    lim = tref.bound(S, ref, H, K)
    err = np.abs(out - ref)
    assert (err[ok] <= lim[ok]).all(), "worst |err| / bound %.3f" % (err[ok] / lim[ok]).max()
    print("\nfirst cut: %d rows, %d with a NaN at or before the cut; worst |err| / bound %.3f" % (hit.size, int(hit.sum()), (err[ok] / lim[ok]).max()))
    # first = H for every row is no cut at all
    full = _np(eng.tracking_returns(traj, rows, terms, targets, first=np.full((m, n, p), H, np.int32)))
    np.testing.assert_array_equal(_bits(full), _bits(_np(eng.tracking_returns(traj, rows, terms, targets))))


# ---------------------------------------------------------------------------------------------------------------------- 3: the loop
def _tracking_inputs(eng, prob, K, T, seed):
    """(track_params, targets [M,T,K] on the device, offset [M] int32): terms on random dims around what iteration 0 reaches, some NaN"""
    traj0 = iteration0_traj(eng, prob, 0.0, 4, 1)
    rng = np.random.default_rng(seed)
    dims = rng.integers(0, eng.D, K)
    terms = [dict(dim=int(d), kind=tref.KINDS[k % 3], w=float(rng.uniform(0.5, 2.0)), **(dict(delta=0.75) if k % 3 == 2 else {}))
             for k, d in enumerate(dims)]
    mu, sd = traj0.reshape(-1, eng.D).mean(axis=0)[dims], traj0.reshape(-1, eng.D).std(axis=0)[dims]
    targets = (mu + sd * rng.standard_normal((M, T, K))).astype(np.float32)
    targets[rng.uniform(size=targets.shape) < 0.2] = np.nan
    return HipEngine.track_params(terms), eng._t(targets), torch.tensor([1, -1], dtype=torch.int32, device=eng.device), terms


LOOP = [(e, u) for e in ("hc5-vanilla", "hc5", "hopper") for u in ("cem", "mppi")]


@pytest.mark.parametrize("name,update", LOOP, ids=["%s-%s" % c for c in LOOP])
def test_fused_equals_stepwise(engines, name, update):
    """`cadm_tracking_plan` with device RNG == the same loop one launch at a time (`planner.icem_plan(..., tracking=...)`), bit for bit
    over two consecutive calls: the plan, the best return, the carry.  Every stepwise iteration's tracked rows are its untracked rows
    minus its cost, and the cost is the restatement's within the kernel's bound."""
    prob, eng = engines(name)
    H, A, K = eng.H, eng.A, 4
    track, targets, offset, terms = _tracking_inputs(eng, prob, K, H + 1, 11)
    icem = dict(noise_beta=1.0 if update == "mppi" else 0.0, keep_elites=2, decay=1.0, return_best=update == "mppi", add_mean_last=False)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    (ca, va), (cb, vb) = zero_carry(eng, M, 2, H), zero_carry(eng, M, 2, H)
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2):
        a, ra = eng.tracking_plan(track, targets, offset, None, None, None, None, prm, *args, mean, var, N, carry=ca, carry_valid=va, seed=4,
                                  call=call, want_best_return=True)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                            update=update, temperature=0.5, relative=True, tracking=(track, targets, offset), **icem)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ca)), _bits(_np(cb)), err_msg="carry after call %d" % call)
        np.testing.assert_array_equal(_np(va), [1, 1])
        for x in info:
            traj, raw, rows, cost = _np(x["traj"]), _np(x["rows_untracked"]), _np(x["rows"]), _np(x["track_cost"])
            ref, cost_ref, S, counted = tref.tracking(traj, raw, terms, _np(targets), _np(offset))
            assert (counted > 0).all()
            np.testing.assert_array_equal(_bits(rows), _bits(raw - cost))
            assert (np.abs(cost - cost_ref) <= tref.bound(S, None, H, K)).all()
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), np.float32)], axis=1)      # the samplers' warm start
    # the targets matter: other targets, another plan
    other = _np(eng.tracking_plan(track, torch.nan_to_num(targets, nan=0.0) + 1.0, offset, None, None, None, None, prm, *args, mean, var, N,
                                  *zero_carry(eng, M, 2, H), seed=4, call=2))
    assert not np.array_equal(_bits(other), _bits(a))


def test_fused_equals_stepwise_with_everything_on(engines):
    """TERMINATE constraints with about half the rows violating (the tracking kernel reads their first violations), a CVaR score, knots
    r = 2 linear with phases, two kept elites, the best plan: fused == stepwise bit for bit over two calls; and in every stepwise
    iteration the tracked rows are the constrained rows minus a cost that stops at the first violation."""
    prob, eng = engines("hc5")
    H, A, K = eng.H, eng.A, 4
    track, targets, offset, terms = _tracking_inputs(eng, prob, K, H, 13)
    cons = binding_bounds(iteration0_traj(eng, prob, 1.0, 4, 1), (1, 7), H, "everything on")
    cp = HipEngine.constraint_params(cons, "terminate", 4.0)
    score, knots = HipEngine.score_params("cvar", k=2), HipEngine.knot_params(2, "linear")
    phase = torch.tensor([0, 1], dtype=torch.int32, device=eng.device)
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, return_best=True, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    (ca, va), (cb, vb) = zero_carry(eng, M, 2, H), zero_carry(eng, M, 2, H)
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2):
        a, ra = eng.tracking_plan(track, targets, offset, knots, phase, cp, score, prm, *args, mean, var, N, carry=ca, carry_valid=va, seed=4,
                                  call=call, want_best_return=True)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                            update="mppi", temperature=0.5, relative=True, score=score, constraints=cp, knots=knots, phase=phase,
                                            tracking=(track, targets, offset), **icem)
        a = _np(a)
        assert np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ca)), _bits(_np(cb)), err_msg="carry after call %d" % call)
        for it, x in enumerate(info):
            first, traj = _np(x["first_violation"]), _np(x["traj"])
            if call == 1 and it == 0:
                share = float((first < H).mean())
                assert 0.2 <= share <= 0.8, "%.2f of the rows violate" % share
            _, cost_ref, S, _ = tref.tracking(traj, _np(x["rows_untracked"]), terms, _np(targets), _np(offset), first)
            cost = _np(x["track_cost"])
            assert (np.abs(cost - cost_ref) <= tref.bound(S, None, H, K)).all(), "the cost does not stop at the first violation"
            np.testing.assert_array_equal(_bits(_np(x["rows"])), _bits(_np(x["rows_untracked"]) - cost))
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), np.float32)], axis=1)
    assert (True, "track", True) in eng._loop_ws      # the tracking slot under TERMINATE constraints: with the first-violation view
    sizes = [eng.lib.cadm_tracking_workspace_bytes(eng._ctx, M, N, 2, 1, t) for t in (0, 1)]
    assert sizes[0] == eng.lib.cadm_constrained_workspace_bytes(eng._ctx, M, N, 2, 1) and sizes[1] == sizes[0] + ((M * N * eng.p * 4 + 255) & ~255)


@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_no_terms_is_the_loop_underneath(engines, update):
    """track = NULL: the plan, the best return and the carry of `cadm_knot_plan` on the same inputs, bit for bit -- with knots and
    constraints and without --, from the workspace of the loop underneath (no tracking slot is allocated)."""
    prob, eng = engines("hc5")
    H = eng.H
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    cons = HipEngine.constraint_params(binding_bounds(iteration0_traj(eng, prob, 1.0, 5, 2), (1, 7), H, "no terms"), "penalty", 4.0)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    slots = {s for s in eng._loop_ws if s[1] == "track"}
    for knots, phase, cs, sc in ((HipEngine.knot_params(2, "hold"), torch.tensor([1, 0], dtype=torch.int32, device=eng.device), cons,
                                  HipEngine.score_params("mean_std", 1.0)), (None, None, None, None)):
        runs = []
        for fn in (lambda **k: eng.tracking_plan(None, None, None, knots, phase, cs, sc, prm, *args, **k),
                   lambda **k: eng.knot_plan(knots, phase, cs, sc, prm, *args, **k)):
            carry, valid = zero_carry(eng, M, 2, H)
            plan, best = fn(carry=carry, carry_valid=valid, seed=5, call=2, want_best_return=True)
            runs.append((_bits(_np(plan)), _bits(_np(best)), _bits(_np(carry)), _np(valid)))
        for x, y in zip(*runs):
            np.testing.assert_array_equal(x, y)
    assert {s for s in eng._loop_ws if s[1] == "track"} == slots


@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_all_nan_targets_change_no_plan(gpu, context):
    """A model with `cem_tracking` whose targets are all NaN plans, call after call, what the same model without `cem_tracking` plans,
    bit for bit, the kept elites included."""
    H, A = 5, 6
    other = dict(cem_noise_beta=1.0, cem_keep_elites=2)
    plain, prob = plan_model(context, H, **other)
    blind, _ = plan_model(context, H, cem_tracking=[dict(dim=0, w=1e6), dict(dim=9, kind="huber", w=3.0, delta=0.1)], **other)
    assert plain._opt.track_params is None and blind._opt.track_params.n == 2
    blind.set_targets(np.full((M, 4, 2), np.nan))
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    for call in range(3):
        pa, pb = plan_act(plain, prob, context, mean, var), plan_act(blind, prob, context, mean, var)
        assert np.isfinite(pa).all() and 0 < np.abs(pa).max() <= 1.0
        np.testing.assert_array_equal(_bits(pa), _bits(pb), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(plain._plan_carry)), _bits(_np(blind._plan_carry)))
        mean = np.concatenate([pa[:, 1:], np.zeros((M, 1, A))], axis=1)
    assert not [s for s in plain.engine._loop_ws if s[1]], "a model without cem_tracking allocates no trajectory view"
    assert (False, "track", False) in blind.engine._loop_ws


# ---------------------------------------------------------------------------------------------------------------------- 4: it binds
def _far_goal(last, mine):
    """per (env, dim): of the lowest and the highest value in `last` [m,n,D], the one farther from `mine` [m,D]"""
    lo, hi = last.min(axis=1), last.max(axis=1)
    return np.where(mine - lo > hi - mine, lo, hi).astype(np.float32)


def bind_case(context, H=5, A=6):
    """A deterministic model (no noise inside a member: a plan's cost is a function of its actions alone; measured on an MI355X, with
    the noise on, the terminal cost of 64 sampled sequences under two noise draws agrees in rank by 0.0 to 0.2 on these random
    networks, so nothing could be told from it).  The untracked model's plan first.  Then, on rollouts of 64 sampled sequences and of
    that plan: the dim whose particle mean at the LAST step differs most between the sequences, and as its goal there (a terminal cost:
    every other row of the targets is NaN), of the lowest and the highest value any sampled sequence reaches, the one farther from
    where the untracked plan ends.  w: 10^3 times the env's return range over the spread of that cost at w = 1, so the tracking cost
    decides the ranking.  -> (tracked model, plain model, problem, targets [M,H,1], untracked plan, dim, w)"""
    plain, prob = plan_model(context, H, deterministic=True)
    eng = plain.engine
    cpa = (prob["cp_obs"], prob["cp_act"]) if context else ()
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    pu = plan_act(plain, prob, context, mean, var)
    ctxv = eng.context_forward(*cpa) if context else None
    acts = torch.cat([eng.sample_actions(mean, var, 64, seed=3, call=1, it=0), eng._t(pu)[:, None]], dim=1)
    raw, traj = eng.rollout_returns(prob["obs"], ctxv, acts, seed=3, call=1, it=0, want_traj=True)
    last = _np(traj)[-1].astype(np.float64)                               # [m, n + 1, p, D]
    reach = last.mean(axis=2)
    d = int(np.argmax(reach[:, :64].std(axis=1).min(axis=0)))
    goal = _far_goal(reach[:, :64], reach[:, 64])[:, d]                   # [m]
    cost1 = ((last[:, :64, :, d] - goal[:, None, None]) ** 2).mean(axis=2)                # [m, n] at w = 1
    ret = _np(raw).mean(axis=-1)[:, :64]
    w = float(1e3 * (ret.max(axis=1) - ret.min(axis=1)).max() / (cost1.max(axis=1) - cost1.min(axis=1)).min())
    assert np.isfinite(w) and w > 0
    tracked, _ = plan_model(context, H, deterministic=True, cem_tracking=[dict(dim=d, kind="square", w=w)], cem_target_advance=False)
    targets = np.full((M, H, 1), np.nan, np.float32)
    targets[:, -1, 0] = goal
    return tracked, plain, prob, targets, pu, d, w


@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_targets_that_bind_change_the_plan(gpu, context):
    """Class route, same seed, a terminal goal that the untracked plan does not go to (`bind_case`), w such that the tracking cost
    dwarfs the env's return range by 10^3.  The plan differs from the untracked model's, and its particle-mean `tracking_cost` is
    lower than the untracked plan's, for every env."""
    H, A = 5, 6
    tracked, plain, prob, targets, pu, d, w = bind_case(context)
    cpa = (prob["cp_obs"], prob["cp_act"]) if context else ()
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    with pytest.raises(RuntimeError, match="set_targets"):
        plan_act(tracked, prob, context, mean, var)
    assert tracked._call == 0
    tracked.set_targets(targets)
    pt = plan_act(tracked, prob, context, mean, var)
    assert np.isfinite(pt).all() and np.abs(pt).max() <= 1.0
    assert not np.array_equal(_bits(pt), _bits(pu)), "the targets do not change the plan"
    both = np.stack([pt, pu], axis=1)
    res = tracked.tracking_cost(prob["obs"], both, *cpa)
    assert res["cost"].shape == (M, 2, 5) and tracked._call == 1 and _np(tracked._target_offset).tolist() == [0, 0]
    np.testing.assert_array_equal(_bits(res["returns"]), _bits(res["returns_untracked"] - res["cost"]))
    cost = res["cost"].mean(axis=-1)
    print("\nparticle-mean tracking cost per env: tracked plan %s, untracked plan %s (w = %.3g, dim %d)" % (cost[:, 0], cost[:, 1], w, d))
    assert (cost[:, 0] < cost[:, 1]).all()
    one = tracked.tracking_cost(prob["obs"], pt, *cpa)                    # [m,H,A]: the n axis is dropped
    np.testing.assert_array_equal(_bits(one["cost"]), _bits(res["cost"][:, 0]))
    with pytest.raises(ValueError, match="no cem_tracking"):
        plain.tracking_cost(prob["obs"], pu, *cpa)


# ---------------------------------------------------------------------------------------------------------------------- 5: episode time
def test_offsets_follow_the_episode(gpu):
    """The per-env offsets advance by one per get_action, stay put under cem_target_advance=False, are zeroed for the masked envs by
    `reset_plan_carry(mask)` and by `DevicePlannerState.observe(done=)`; `fit`-free calls in between (tracking_cost) leave them alone;
    targets whose m or K do not fit are refused."""
    from cadm_amd.caller import DevicePlannerState
    H, A, T = 5, 6, 9
    terms = [dict(dim=2, w=5.0), dict(dim=8, kind="abs", w=2.0)]
    model, prob = plan_model(True, H, cem_tracking=terms, cem_keep_elites=2)
    ref = np.random.default_rng(5).standard_normal((M, T, 2)).astype(np.float32)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    model.set_targets(ref)
    assert model._target_offset.dtype == torch.int32 and _np(model._target_offset).tolist() == [0, 0]
    for k in (1, 2, 3):
        plan = plan_act(model, prob, True, mean, var)
        assert np.isfinite(plan).all() and _np(model._target_offset).tolist() == [k, k]
    model.tracking_cost(prob["obs"], plan, prob["cp_obs"], prob["cp_act"])
    assert _np(model._target_offset).tolist() == [3, 3]
    model.reset_plan_carry([True, False])
    assert _np(model._target_offset).tolist() == [0, 3] and _np(model._plan_carry_valid).tolist() == [0, 1]
    plan_act(model, prob, True, mean, var)
    assert _np(model._target_offset).tolist() == [1, 4]
    model.reset_plan_carry()
    assert _np(model._target_offset).tolist() == [0, 0]
    model.set_targets(ref, offset=[4, -1])
    assert _np(model._target_offset).tolist() == [4, -1]
    np.testing.assert_array_equal(_bits(_np(model._targets)), _bits(ref))
    with pytest.raises(ValueError, match="mask has 3 entries"):
        model.reset_plan_carry([True, False, True])
    with pytest.raises(ValueError, match="set_targets: targets"):
        model.set_targets(np.zeros((M, T, 3)))
    model.set_targets(np.zeros((M + 1, 2)))
    call = model._call
    with pytest.raises(ValueError, match="expected \\[2,T,2\\]"):
        plan_act(model, prob, True, mean, var)
    assert model._call == call
    model.clear_targets()
    with pytest.raises(RuntimeError, match="set_targets"):
        plan_act(model, prob, True, mean, var)
    # the device-resident caller: observe(done=) and reset() restart the reference
    model.set_targets(ref)
    state = DevicePlannerState(model, M)
    obs = prob["obs"]
    a = state.act(obs)
    assert tuple(a.shape) == (M, A) and np.isfinite(_np(a)).all() and _np(model._target_offset).tolist() == [1, 1]
    state.observe(obs, a, obs, done=np.array([0, 1]))
    assert _np(model._target_offset).tolist() == [1, 0]
    state.act(obs)
    assert _np(model._target_offset).tolist() == [2, 1]
    state.reset()
    assert _np(model._target_offset).tolist() == [0, 0]
    # cem_target_advance=False: the offsets are the caller's
    still, _ = plan_model(True, H, cem_tracking=terms, cem_target_advance=False)
    still.set_targets(ref, offset=[2, 5])
    for _ in range(2):
        plan_act(still, prob, True, mean, var)
    assert _np(still._target_offset).tolist() == [2, 5]


@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_second_call_is_the_window_moved_on(gpu, context):
    """Call 2 against a [m,T,K] reference == a fresh model's call with the same call counter against the reference without its first row
    at offset 0, bit for bit: the offset is the only thing a call leaves behind (no elites are kept here)."""
    H, A, T = 5, 6, 7
    terms = [dict(dim=1, w=50.0), dict(dim=4, kind="huber", w=20.0, delta=0.3)]
    ref = np.random.default_rng(6).standard_normal((M, T, 2)).astype(np.float32)
    ref[0, 3, 1] = np.nan
    a, prob = plan_model(context, H, cem_tracking=terms)
    b, _ = plan_model(context, H, cem_tracking=terms)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    a.set_targets(ref)
    p1 = plan_act(a, prob, context, mean, var)
    mean2 = np.concatenate([p1[:, 1:], np.zeros((M, 1, A))], axis=1)
    p2 = plan_act(a, prob, context, mean2, var)
    b.set_targets(ref[:, 1:])
    b._call = 1                                                           # the next call draws under call number 2, as a's second did
    q2 = plan_act(b, prob, context, mean2, var)
    np.testing.assert_array_equal(_bits(p2), _bits(q2))
    b.set_targets(ref)
    b._call = 1
    assert not np.array_equal(_bits(plan_act(b, prob, context, mean2, var)), _bits(p2)), "the window does not matter"


# ---------------------------------------------------------------------------------------------------------------------- 6: refusals
def test_argument_checks_return_einval(engines):
    """Both exports refuse bad arguments with CADM_EINVAL and a message that names them and the argument, before any HIP call (the dummy
    pointers next to the bad argument are never touched); the engine plans normally afterwards."""
    prob, eng = engines("hc5")
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(4096, dtype=torch.float32, device=eng.device)
    P = ct.c_void_p(buf.data_ptr())
    mp = HipEngine.mppi_params()

    def T_(n=1, dim=0, kind=0, w=1.0, delta=0.0):
        t = _lib.TrackParams()
        t.n, t.dim[0], t.kind[0], t.w[0], t.delta[0] = n, dim, kind, w, delta
        return ct.byref(t)

    def returns(t, c=ctx, targets=P, T=1):
        return lib.cadm_tracking_returns(c, t, P, targets, T, None, None, P, M, 4, P, None, None)

    def plan(t, c=ctx, targets=P, T=1, update=0, prm=ct.byref(mp)):
        return lib.cadm_tracking_plan(c, t, targets, T, None, None, None, None, None, update, prm, P, P, P, P, P, None, None, M, N, 0, 1, P, P,
                                      None, None)

    def einval(rc, name, frag):
        msg = lib.cadm_last_error().decode()
        assert rc == -1, "%s: expected CADM_EINVAL, got %d (%s)" % (name, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    for name, fn in (("cadm_tracking_returns", returns), ("cadm_tracking_plan", plan)):
        einval(fn(T_(n=0)), name, "tracking terms")
        einval(fn(T_(n=17)), name, "tracking terms")
        einval(fn(T_(dim=-1)), name, "dim")
        einval(fn(T_(dim=eng.D)), name, "dim")
        einval(fn(T_(kind=3)), name, "kind")
        einval(fn(T_(kind=-1)), name, "kind")
        einval(fn(T_(w=-1.0)), name, ": w ")
        einval(fn(T_(w=float("nan"))), name, ": w ")
        einval(fn(T_(w=float("inf"))), name, ": w ")
        einval(fn(T_(kind=2, delta=0.0)), name, "delta")
        einval(fn(T_(kind=2, delta=float("inf"))), name, "delta")
        einval(fn(T_(kind=2, delta=float("nan"))), name, "delta")
        einval(fn(T_(), T=0), name, "T = 0")
        einval(fn(T_(), targets=None), name, "targets")
    einval(returns(None), "cadm_tracking_returns", "null")
    einval(plan(T_(), update=2), "cadm_tracking_plan", "update")
    einval(plan(T_(), prm=None), "cadm_tracking_plan", "bad arguments")
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=M, H=5, seed=1)
    deng = make_engine(dprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    einval(returns(T_(), c=deng._ctx), "cadm_tracking_returns", "continuous-action")
    einval(plan(T_(), c=deng._ctx), "cadm_tracking_plan", "continuous actions only")
    deng.close()
    sprob = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=5, seed=3, trained_like=True)
    seng = make_engine(sprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(seng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    einval(returns(T_(), c=seng._ctx), "cadm_tracking_returns", "sharded")
    einval(plan(T_(), c=seng._ctx), "cadm_tracking_plan", "sharded")
    assert lib.cadm_dist_destroy(seng._ctx) == 0
    seng.close()
    # python: shapes that do not fit the engine
    traj = torch.zeros((eng.H, M, 4, eng.p, eng.D), dtype=torch.float32, device=eng.device)
    rows = torch.zeros((M, 4, eng.p), dtype=torch.float32, device=eng.device)
    for kw in (dict(targets=np.zeros((M + 1, 1))), dict(targets=np.zeros((M, 2))), dict(targets=np.zeros((M, 0, 1))),
               dict(targets=np.zeros((M, 1)), offset=np.zeros(3, np.int32)), dict(targets=np.zeros((M, 1)), first=np.zeros((M, 4), np.int32))):
        with pytest.raises(ValueError, match="tracking_returns"):
            eng.tracking_returns(traj, rows, [dict(dim=0)], **kw)
    with pytest.raises(ValueError, match="need targets"):
        eng.tracking_plan(HipEngine.track_params([dict(dim=0)]), None, None, None, None, None, None, HipEngine.icem_params(), prob["obs"],
                          prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    with pytest.raises(ValueError, match="reads observation dim 18"):
        plan_model(True, 5, cem_tracking=[dict(dim=18)])
    out = _np(eng.tracking_plan(HipEngine.track_params([dict(dim=0)]), np.zeros((M, 1)), None, None, None, None, None, HipEngine.icem_params(),
                                prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N, seed=1, call=1))
    assert np.isfinite(out).all() and np.abs(out).max() <= 1.0
