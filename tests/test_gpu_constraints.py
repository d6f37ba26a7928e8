"""GPU: state constraints and early termination of the opt-in planner -- the kernel (`cadm_constrain_returns`, csrc/constrain.hip) on
synthetic trajectories and at its edges, the fused loop (`cadm_constrained_plan`) against the stepwise one, a constraint that never
binds and one that does, the class route with `constraint_check`, and the refusals.

Geometries: the compiled-in halfcheetah 200 x 4 kernel and tests/test_gpu_horizon.py's hopper_like declaration (the JIT module that
file and tests/test_gpu_forecast.py build); the fused loop in terminate mode also on ant, slim_humanoid and pendulum (the isolated
kernel on those: tests/test_gpu_behind_rollout_envs.py).  Numpy restatement: tests/constraint_ref.py.

Bounds.  Counters and `penalty` rows (w = 4: a power of two, the product is exact) are compared bit for bit.  A `terminate` row that
first violates at tau is a chain of tau + 1 step rewards; each is held to b_t = (T + 3) 2^-23 S_t of the env's closure (the bound
tests/test_gpu_forecast.py uses for a step reward: T additive terms, S_t the sum of their absolute values), so the row lies within
(tau + 1) max_{t <= tau} b_t of the float64 reference.  That bound has no term for the last operation, the float32 subtraction of w,
which rounds by up to 2^-24 |sum - w|: on the synthetic trajectories of test 1 and test 2 the rewards are of order 1 to 10 and the
bound is kept as it is; on a model's own rollouts (test 3) a halfcheetah step reward can be of order 1e-2 while |sum - w| is 4, so
there the subtraction's rounding, 2^-24 |reference|, is added to the bound."""
import ctypes as ct

import numpy as np
import pytest
import torch

import constraint_ref as cref
import risk_ref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd._lib import ptr
from cadm_amd.engine import HipEngine
from cadm_amd.env_spec import EnvDecl
from behind_rollout import band, synth_traj
from forecast_ref import reward_bound
from helpers import _np, make_engine, plan_model, zero_carry
from oracle import envs as oenvs

pytestmark = pytest.mark.gpu

M, N, KE, ITERS = 2, 24, 8, 3
NEVER = [dict(dim=0, lo=-3e38, hi=3e38), dict(dim=5, lo=-3e38, hi=3e38)]


def hopper_like():          # tests/test_gpu_horizon.py's declaration (same geometry: one JIT module serves the three files)
    return EnvDecl(11, 3, preproc=["drop", "sincos", "id", "id", "sincos", "id", "id", "id", "id", "id", "id"],
                   postproc=["add"] * 5 + ["replace"] + ["add"] * 5,
                   reward=[dict(kind="linear", dim=5), dict(kind="square", dim=3, w=-0.5, when="next_obs"),
                           dict(kind="abs", dim=10, w=-0.1), dict(kind="inside", dim=0, w=1.0, lo=-0.5, hi=0.5, when="next_obs"),
                           dict(kind="outside", dim=2, w=-1.0, lo=-0.2, hi=0.2), dict(kind="linear", dim=4, w=0.3, when="next_obs"),
                           dict(kind="square", dim=7, w=-0.05), dict(kind="abs", dim=6, w=0.2, when="next_obs"),
                           dict(kind="outside", dim=9, w=-0.5, lo=-1.0, hi=1.0, when="next_obs"),
                           dict(kind="inside", dim=8, w=0.25, lo=-0.3, hi=0.8)],
                   ctrl_cost=0.001, bonus=1.0)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def coverage(first, H, what):
    """The condition under which a comparison shows something: 20 % .. 80 % of the rows violate, one first at step 0, one at H - 1."""
    share = float((first < H).mean())
    print("%s: %.0f %% of %d rows violate; first violations at steps %s" % (what, 100 * share, first.size, sorted(set(first[first < H].tolist()))))
    assert 0.2 <= share <= 0.8, "%s: %.2f of the rows violate" % (what, share)
    assert (first == 0).any() and (first == H - 1).any(), "%s: no first violation at step 0 / at step H - 1" % what


def plant_ends(traj, cons, what):
    """Where no row first violates at step 0 or at step H - 1, set one healthy row's constrained value exactly to its bound there."""
    H = traj.shape[0]
    d, lo = cons[0]["dim"], np.float32(cons[0]["lo"])
    for t in (0, H - 1):
        first = cref.counters(traj, cons)[0]
        if not (first == t).any():
            mi, ni, j = [int(v[0]) for v in np.nonzero(first == H)]
            traj[t, mi, ni, j, d] = lo
            print("%s: row (%d, %d, %d) set to its lower bound at step %d" % (what, mi, ni, j, t))
    return traj


@pytest.fixture(scope="module")
def hop(gpu):
    """hopper_like with context, E = 5, p = 5, H = 3, 8 elites, 3 CEM iterations"""
    spec = hopper_like()
    prob = synth.make_problem(env=spec, context=True, E=5, m=M, H=3, seed=52)
    eng = make_engine(prob, p=5, num_elites=KE, num_cem_iters=ITERS)
    yield spec, prob, eng
    eng.close()


@pytest.fixture(scope="module")
def hc8(gpu):
    """halfcheetah with context, E = 5, p = 20, H = 8: shape (b)"""
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=8, seed=51)
    eng = make_engine(prob, p=20)
    yield prob, eng
    eng.close()


@pytest.fixture(scope="module")
def hc5(gpu):
    """halfcheetah, H = 5, p = 5, 8 elites, 3 CEM iterations: {context: (problem, engine)}"""
    out = {}
    for context in (False, True):
        prob = synth.make_problem(env="halfcheetah", context=context, E=5, m=M, H=5, seed=3, trained_like=True)
        out[context] = (prob, make_engine(prob, p=5, num_elites=KE, num_cem_iters=ITERS))
    yield out
    for _, eng in out.values():
        eng.close()


OTHER_KINDS = dict(ant=(5, (0, 27)), slim_humanoid=(3, (1, 44)), pendulum=(5, (2, 0)))      # kind: (H, constrained dims)


@pytest.fixture(scope="module")
def others(gpu):
    """ant, slim_humanoid and pendulum as hc5[True]: context, trained-like, p = 5, 8 elites, 3 CEM iterations, H = 5, 3, 5.
    kind -> (problem, engine), built when first asked for."""
    built = {}

    def get(kind):
        if kind not in built:
            prob = synth.make_problem(env=kind, context=True, E=5, m=M, H=OTHER_KINDS[kind][0], seed=3, trained_like=True)
            built[kind] = (prob, make_engine(prob, p=5, num_elites=KE, num_cem_iters=ITERS))
        return built[kind]
    yield get
    for _, eng in built.values():
        eng.close()


def run(eng, traj, rows, cons, mode, w, obs, acts, out=None):
    r, f, v = eng.constrain_returns(traj, rows, cons, mode, w, obs=obs, actions=acts, out=out)
    torch.cuda.synchronize()
    return _np(r), _np(f), _np(v)


def terminate_bound(terms_env, traj, obs, acts, first, ref=None):
    """(tau + 1) max_{t <= tau} b_t per row [m,n,p], b = `reward_bound` ((T + 3) 2^-23 S; pendulum: plus its angle's rounding); 0 where
    nothing violates.  ref: the float64 reference, to add
    the rounding of the final subtraction of w, 2^-24 |ref| (see the module docstring)"""
    H = traj.shape[0]
    with np.errstate(all="ignore"):
        b = np.moveaxis(reward_bound(terms_env, traj, obs, acts), 2, 0)              # [H,m,n,p]
    tau = np.minimum(first, H - 1)
    upto = np.where(np.arange(H)[:, None, None, None] <= tau[None], b, 0.0)          # steps after tau are not read: their b may be NaN
    return (tau + 1) * upto.max(axis=0) + (0.0 if ref is None else 2.0 ** -24 * np.abs(ref))


# ---------------------------------------------------------------------------------------------------------------------- 1
def check_kernel(eng, env, terms_env, traj, obs, acts, cons, seed, what):
    H, m, n, p, D = traj.shape
    rows = np.random.default_rng(seed).uniform(-30, 30, (m, n, p)).astype(np.float32)
    first, viol = cref.counters(traj, cons)
    coverage(first, H, what)
    print("%s: up to %d violations per row" % (what, viol.max()))
    # penalty, w = 4
    want = cref.penalty_rows(rows, viol, 4.0)
    pen, f, v = run(eng, traj, rows, cons, "penalty", 4.0, None, None)
    np.testing.assert_array_equal(f, first, err_msg=what + ": first_violation")
    np.testing.assert_array_equal(v, viol, err_msg=what + ": violations")
    np.testing.assert_array_equal(_bits(pen), _bits(want), err_msg=what + ": penalty rows")
    # terminate, w = 4
    ref = cref.terminate_rows(env, traj, obs, acts, rows, first, 4.0)
    lim = terminate_bound(terms_env, traj, obs, acts, first)
    ter, f, v = run(eng, traj, rows, cons, "terminate", 4.0, obs, acts)
    np.testing.assert_array_equal(f, first, err_msg=what + ": first_violation (terminate)")
    np.testing.assert_array_equal(v, viol, err_msg=what + ": violations (terminate)")
    alive = first == H
    np.testing.assert_array_equal(_bits(ter[alive]), _bits(rows[alive]), err_msg=what + ": rows without a violation")
    err = np.abs(ter.astype(np.float64) - ref)[~alive]
    print("%s terminate: worst |err| / bound %.3f over %d rows" % (what, (err / lim[~alive]).max(), err.size))
    assert (err <= lim[~alive]).all(), "%s terminate: worst |err| / bound %.3f" % (what, (err / lim[~alive]).max())
    # run to run, inside a sub-batch, in place
    for mode, got, o, a in (("penalty", pen, None, None), ("terminate", ter, obs, acts)):
        again, f2, v2 = run(eng, traj, rows, cons, mode, 4.0, o, a)
        np.testing.assert_array_equal(_bits(again), _bits(got), err_msg="%s %s: run to run" % (what, mode))
        cuts = [(slice(m - 1, m), slice(None))] + ([(slice(None), slice(n - 1, n))] if n > 1 else []) + ([(slice(1, m), slice(None))] if m > 2 else [])
        for ms, ns in cuts:
            part = np.ascontiguousarray(traj[:, ms, ns])
            sub, fs, vs = run(eng, part, np.ascontiguousarray(rows[ms, ns]), cons, mode, 4.0, None if o is None else o[ms],
                              None if a is None else np.ascontiguousarray(a[ms, ns]))
            np.testing.assert_array_equal(_bits(sub), _bits(got[ms, ns]), err_msg="%s %s: sub-batch %r" % (what, mode, (ms, ns)))
            np.testing.assert_array_equal(fs, first[ms, ns])
            np.testing.assert_array_equal(vs, viol[ms, ns])
        io = eng._t(rows.copy())
        same, _, _ = run(eng, traj, io, cons, mode, 4.0, o, a, out=io)
        np.testing.assert_array_equal(_bits(_np(io)), _bits(got), err_msg="%s %s: rows_out aliasing rows_in" % (what, mode))


def test_kernel_shape_a_declared_env(hop):
    spec, prob, eng = hop
    traj, obs, acts = synth_traj(1, 3, 3, 2, 5, 11, 3)
    traj = (traj * np.float32(0.4)).astype(np.float32)
    cons = [band(traj, 0, 1.5), band(traj, 10, 1.5, lower_only=True)]
    check_kernel(eng, spec, spec, traj, obs, acts, cons, 11, "(a) D=11 p=5 H=3")


def test_kernel_shape_b_halfcheetah(hc8):
    prob, eng = hc8
    traj, obs, acts = synth_traj(2, 8, 2, 1, 20, 18, 6)
    cons = [band(traj, 1, 2.0), band(traj, 7, 2.0)]
    traj = plant_ends(traj, cons, "(b)")
    check_kernel(eng, oenvs.make_env("halfcheetah"), "halfcheetah", traj, obs, acts, cons, 12, "(b) D=18 p=20 H=8")


def test_kernel_shape_c_one_particle_three_workgroups(gpu):
    """p = 1 and 135 rows: two full workgroups and one of 7 rows; step spans that start 8 bytes off a 16-byte boundary at odd steps"""
    prob = synth.make_problem(env="halfcheetah", context=True, E=1, m=1, H=3, seed=54)
    eng = make_engine(prob, p=1)
    traj, obs, acts = synth_traj(3, 3, 5, 27, 1, 18, 6)
    cons = [band(traj, 1, 1.5), band(traj, 7, 1.5)]
    check_kernel(eng, oenvs.make_env("halfcheetah"), "halfcheetah", traj, obs, acts, cons, 13, "(c) D=18 p=1 H=3, 135 rows")
    eng.close()


def test_kernel_shape_d_declared_env_three_workgroups(hop):
    """hopper_like with 165 rows: an odd D over several workgroups, the last one partial"""
    spec, prob, eng = hop
    traj, obs, acts = synth_traj(4, 3, 3, 11, 5, 11, 3)
    traj = (traj * np.float32(0.4)).astype(np.float32)
    cons = [band(traj, 0, 1.5), band(traj, 10, 1.5, lower_only=True)]
    check_kernel(eng, spec, spec, traj, obs, acts, cons, 14, "(d) D=11 p=5 H=3, 165 rows")


# ---------------------------------------------------------------------------------------------------------------------- 2
def test_edges(hop):
    spec, prob, eng = hop
    H = 3
    traj, obs, acts = synth_traj(1, H, 3, 2, 5, 11, 3)
    traj = (traj * np.float32(0.4)).astype(np.float32)
    cons = [band(traj, 0, 10.0), band(traj, 10, 10.0, lower_only=True)]              # wide: nothing violates until it is planted
    lo0, hi0, lo10 = np.float32(cons[0]["lo"]), np.float32(cons[0]["hi"]), np.float32(cons[1]["lo"])
    rows = np.random.default_rng(5).uniform(-30, 30, (3, 2, 5)).astype(np.float32)
    assert (cref.counters(traj, cons)[1] == 0).all()
    base, f, v = run(eng, traj, rows, cons, "terminate", 4.0, obs, acts)
    assert (f == H).all() and (v == 0).all()
    np.testing.assert_array_equal(_bits(base), _bits(rows))
    t = traj.copy()
    t[1, 0, 0, 0, 0] = lo0                      # exactly lo
    t[2, 0, 0, 1, 0] = hi0                      # exactly hi
    t[0, 0, 0, 2, 10] = lo10                    # exactly the one-sided bound
    t[1, 0, 1, 0, 0] = np.nan                   # NaN in a constrained dim
    t[2, 0, 1, 1, 10] = np.inf                  # +inf under a missing upper side
    t[0, 0, 1, 2, 0] = -np.inf
    t[1, 1, 0, 0, 3] = np.nan                   # NaN in an unconstrained dim: not looked at
    t[0, 1, 0, 1, 9] = np.inf
    t[0, 2, 1, 4, 0] = hi0                      # violates at tau = 0 ...
    t[1:, 2, 1, 4, :] = np.nan                  # ... and the model blows up after it
    want_first = np.full((3, 2, 5), H, np.int32)
    for (mi, ni, j), tau in {(0, 0, 0): 1, (0, 0, 1): 2, (0, 0, 2): 0, (0, 1, 0): 1, (0, 1, 1): 2, (0, 1, 2): 0, (2, 1, 4): 0}.items():
        want_first[mi, ni, j] = tau
    first, viol = cref.counters(t, cons)
    np.testing.assert_array_equal(first, want_first)
    assert viol[2, 1, 4] == 3 and viol[1, 0, 0] == 0 and viol[1, 0, 1] == 0
    nan_rows = rows.copy()
    nan_rows[0, 0, 0] = nan_rows[1, 1, 1] = np.nan                                   # one violating row, one healthy row
    pen, f, v = run(eng, t, nan_rows, cons, "penalty", 4.0, None, None)
    np.testing.assert_array_equal(f, want_first)
    np.testing.assert_array_equal(v, viol)
    assert np.isnan(pen[0, 0, 0]) and np.isnan(pen[1, 1, 1])
    np.testing.assert_array_equal(_bits(pen), _bits(cref.penalty_rows(nan_rows, viol, 4.0)))
    ter, f, v = run(eng, t, rows, cons, "terminate", 4.0, obs, acts)
    np.testing.assert_array_equal(f, want_first)
    np.testing.assert_array_equal(v, viol)
    alive = want_first == H
    np.testing.assert_array_equal(_bits(ter[alive]), _bits(rows[alive]))
    assert np.isfinite(ter[~alive]).all(), "a terminated row's return must not read the trajectory behind its first violation"
    ref = cref.terminate_rows(spec, t, obs, acts, rows, first, 4.0)
    lim = terminate_bound(spec, t, obs, acts, first)
    assert np.isfinite(ref[~alive]).all() and (np.abs(ter - ref)[~alive] <= lim[~alive]).all()
    # the blown-up row: the same bits as without the blow-up
    calm = t.copy()
    calm[1:, 2, 1, 4, :] = traj[1:, 2, 1, 4, :]
    ter2, f2, _ = run(eng, calm, rows, cons, "terminate", 4.0, obs, acts)
    assert f2[2, 1, 4] == 0 and _bits(ter2)[2, 1, 4] == _bits(ter)[2, 1, 4]
    # weight 0 in terminate mode: the partial sum itself
    ter0, _, _ = run(eng, t, rows, cons, "terminate", 0.0, obs, acts)
    np.testing.assert_array_equal(_bits(ter0[~alive] - np.float32(4.0)), _bits(ter[~alive]))


def test_early_exit_without_counts(hc5):
    """TERMINATE with both int outputs null, through the C ABI: a workgroup whose rows have all terminated stops loading.  160 rows,
    three workgroups: every row of the first violates at step 0 and holds NaN behind it, the second is synthetic noise, every row of
    the third violates at step 2.  The same bits as the call that asks for the counts (which never leaves early)."""
    prob, eng = hc5[True]
    H, m, n, p, D, A = 5, 2, 16, 5, 18, 6
    traj, obs, acts = synth_traj(6, H, m, n, p, D, A)
    cons = [band(traj, 1, 2.0), band(traj, 7, 2.0)]
    flat = traj.reshape(H, m * n * p, D)
    flat[0, :64, 1] = np.float32(cons[0]["hi"])
    flat[1:, :64, :] = np.nan
    for d, c in ((1, cons[0]), (7, cons[1])):
        flat[:2, 128:, d] = np.float32(0.5 * (c["lo"] + c["hi"]))
    flat[2, 128:, 7] = np.float32(cons[1]["lo"])
    first = cref.counters(traj, cons)[0].reshape(-1)
    assert (first[:64] == 0).all() and (first[128:] == 2).all() and (first[64:128] == H).any() and (first[64:128] < H).any()
    rows = np.random.default_rng(7).uniform(-30, 30, (m, n, p)).astype(np.float32)
    want, f, v = run(eng, traj, rows, cons, "terminate", 4.0, obs, acts)
    np.testing.assert_array_equal(f.reshape(-1), first)
    assert np.isfinite(want).all()
    prm = HipEngine.constraint_params(cons, "terminate", 4.0)
    t, o, a, r = eng._t(traj), eng._t(obs), eng._t(acts), eng._t(rows)
    for only_first in (False, True):
        out = torch.full((m, n, p), 123.0, dtype=torch.float32, device=eng.device)
        fo = torch.full((m, n, p), -1, dtype=torch.int32, device=eng.device) if only_first else None
        rc = eng.lib.cadm_constrain_returns(eng._ctx, ct.byref(prm), ptr(t), ptr(o), ptr(a), ptr(r), m, n, ptr(out), ptr(fo), None, eng.stream)
        assert rc == 0, eng.lib.cadm_last_error().decode()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(_np(out)), _bits(want), err_msg="rows without the counts (first_violation_out %s)" % only_first)
        if only_first:
            np.testing.assert_array_equal(_np(fo).reshape(-1), first)


# ---------------------------------------------------------------------------------------------------------------------- 3
def binding_bounds(traj0, dims, H, what):
    """Bounds for `dims` from iteration 0's recorded trajectory (which no constraint can change): the first quantile pair, from the
    widest down, under which the coverage condition holds."""
    for q in (0.02, 0.05, 0.08, 0.12, 0.16, 0.2, 0.25, 0.3):
        cons = [dict(dim=d, lo=float(np.quantile(traj0[..., d], q)), hi=float(np.quantile(traj0[..., d], 1.0 - q))) for d in dims]
        first = cref.counters(traj0, cons)[0]
        if 0.25 <= (first < H).mean() <= 0.75 and (first == 0).any() and (first == H - 1).any():
            return cons
    raise AssertionError("%s: no quantile band of dims %r gives the coverage condition" % (what, dims))


def iteration0_traj(eng, prob, beta, seed, call):
    """What iteration 0 of a call without carried elites rolls out: its own candidates, its own trajectories"""
    mean, var = eng._t(prob["init_mean"]), eng._t(prob["init_var"])
    ctxv = eng.context_forward(prob["cp_obs"], prob["cp_act"]) if eng.C > 0 else None
    acts = (eng.sample_actions_colored(mean, var, N, beta, seed=seed, call=call, it=0) if beta > 0
            else eng.sample_actions(mean, var, N, seed=seed, call=call, it=0))
    _, traj = eng.rollout_returns(prob["obs"], ctxv, acts, seed=seed, call=call, it=0, want_traj=True)
    return _np(traj)


LOOP = [      # mode, env, context
    ("penalty", "hopper", True), ("penalty", "halfcheetah", False), ("terminate", "halfcheetah", True), ("terminate", "halfcheetah", False),
    ("terminate", "hopper", True), ("terminate", "ant", True), ("terminate", "slim_humanoid", True), ("terminate", "pendulum", True),
]


@pytest.mark.parametrize("mode,env,context", LOOP, ids=["%s-%s-%s" % (r[0], r[1], "cadm" if r[2] else "vanilla") for r in LOOP])
def test_fused_equals_stepwise(hop, hc5, others, mode, env, context):
    """`cadm_constrained_plan` with device RNG == the same loop one launch at a time (`planner.icem_plan(..., constraints=...)`), bit for
    bit over three consecutive calls: plan, best return, carry, carry-valid.  penalty: the elite refit, the mean, white noise, K = 0;
    terminate: MPPI, cvar, coloured noise, two kept elites, decay 1.25, the best plan.  Every stepwise iteration is held to the numpy
    restatement on its own recorded trajectory.  terminate: a row that first violates at the LAST step has paid every step, so its
    partial sum is the rollout's own return -- rows + w is held to rows_raw within the row's bound plus the rounding of the rollout's
    sum, 2^-24 |raw|: the step reward of step_reward.h against the rollout kernels', for every env kind.

    Measured on an MI355X, worst |err| / bound over the iterations of call 1 -- terminated rows: halfcheetah cadm 0.569, vanilla 0.148,
    hopper 0.023, ant 0.413, slim_humanoid 0.056, pendulum 0.104; rows + w against rows_raw: halfcheetah cadm 0.087, vanilla 0.021,
    hopper 0.047, ant 0.000 (the same bits), slim_humanoid 0.019, pendulum 0.048."""
    if env == "hopper":
        spec, prob, eng = hop
        closure, H, dims = spec, 3, (0, 3)
    elif env in OTHER_KINDS:
        prob, eng = others(env)
        closure, spec, (H, dims) = oenvs.make_env(env), env, OTHER_KINDS[env]
    else:
        prob, eng = hc5[context]
        closure, spec, H, dims = oenvs.make_env("halfcheetah"), "halfcheetah", 5, (1, 7)
    A, p = eng.A, eng.p
    if mode == "penalty":
        update, score, icem = "cem", None, dict(noise_beta=0.0, keep_elites=0, decay=1.0, return_best=False, add_mean_last=False)
    else:
        update, score = "mppi", HipEngine.score_params("cvar", k=2)
        icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, return_best=True, add_mean_last=True)
    keep = icem["keep_elites"]
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    what = "%s %s %s" % (mode, env, "cadm" if context else "vanilla")
    cons = binding_bounds(iteration0_traj(eng, prob, icem["noise_beta"], 4, 1), dims, H, what)
    cp = HipEngine.constraint_params(cons, mode, 4.0)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    (ca, va), (cb, vb) = zero_carry(eng, M, keep, H), zero_carry(eng, M, keep, H)
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2, 3):
        a, ra = eng.constrained_plan(cp, score, prm, *args, mean, var, N, carry=ca, carry_valid=va, seed=4, call=call, want_best_return=True)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                            update=update, temperature=0.5, relative=True, score=score, constraints=cp, **icem)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="%s: plan of call %d" % (what, call))
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="%s: best return of call %d" % (what, call))
        if keep:
            np.testing.assert_array_equal(_bits(_np(ca)), _bits(_np(cb)), err_msg="%s: carry after call %d" % (what, call))
            np.testing.assert_array_equal(_np(va), [1, 1])
            np.testing.assert_array_equal(_np(vb), [1, 1])
        assert [x["actions"].shape[1] for x in info] == [eng.icem_candidates(N, icem["decay"], it, keep) for it in range(ITERS)]
        for it, x in enumerate(info):
            traj, raw, rows, acts = _np(x["traj"]), _np(x["rows_raw"]), _np(x["rows"]), _np(x["actions"])
            first, viol = cref.counters(traj, cons)
            if call == 1 and it == 0:
                coverage(first, H, what + ", iteration 0")
            np.testing.assert_array_equal(_np(x["first_violation"]), first)
            np.testing.assert_array_equal(_np(x["violations"]), viol)
            if mode == "penalty":
                want = cref.penalty_rows(raw, viol, 4.0)
                np.testing.assert_array_equal(_bits(rows), _bits(want), err_msg="%s: rows of call %d iteration %d" % (what, call, it))
            else:
                alive = first == H
                np.testing.assert_array_equal(_bits(rows[alive]), _bits(raw[alive]))
                ref = cref.terminate_rows(closure, traj, prob["obs"].astype(np.float32), acts, raw, first, 4.0)
                lim = terminate_bound(spec, traj, prob["obs"].astype(np.float32), acts, first, ref=ref)
                err = np.abs(rows - ref)[~alive]
                if call == 1:
                    print("%s iteration %d: terminated rows, worst |err| / bound %.3f over %d rows" % (what, it, (err / lim[~alive]).max(), err.size))
                assert (err <= lim[~alive]).all(), "%s: terminated rows of call %d iteration %d, worst |err| / bound %.3f" % (
                    what, call, it, (err / lim[~alive]).max())
                last = first == H - 1                                                  # a full-length partial sum: the rollout's return
                if call == 1 and it == 0:
                    assert last.any()
                if last.any():
                    full = np.abs(rows.astype(np.float64) + float(np.float32(4.0)) - raw)[last]
                    lim_full = (lim + 2.0 ** -24 * np.abs(raw))[last]
                    if call == 1:
                        print("%s iteration %d: rows + w vs rows_raw where the first violation is at step H - 1, worst |err| / bound %.3f over "
                              "%d rows" % (what, it, (full / lim_full).max(), full.size))
                    assert (full <= lim_full).all(), "%s: rows + w vs rows_raw of call %d iteration %d, worst |err| / bound %.3f" % (
                        what, call, it, (full / lim_full).max())
                want = rows
                # the score step against the float64 reference: cvar is 1-Lipschitz in the largest row error, plus its own k + 1 roundings
                ref_rows = np.where(alive, raw.astype(np.float64), ref)
                cand_ref = risk_ref.score(ref_rows, "cvar", k=2, E=5)
                tol = np.where(alive, 0.0, lim).max(axis=-1) + 3 * 2.0 ** -24 * np.abs(ref_rows).max(axis=-1)
                assert (np.abs(_np(x["cand"]) - cand_ref) <= tol).all(), "%s: cand of call %d iteration %d against float64" % (what, call, it)
            cand = _np(x["cand"])
            again = _np(eng.particle_mean(eng._t(want)) if score is None else eng.particle_score(eng._t(want), score))
            np.testing.assert_array_equal(_bits(cand), _bits(again), err_msg="%s: cand of call %d iteration %d" % (what, call, it))
            np.testing.assert_array_equal(_np(x["elites"]), risk_ref.top_elites(cand, KE))
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), np.float32)], axis=1)      # the samplers' warm start


# ---------------------------------------------------------------------------------------------------------------------- 4
MODEL = dict(hidden=(200,) * 4, n_candidates=64, n_particles=5)


@pytest.mark.parametrize("mode", ["penalty", "terminate"])
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_a_constraint_that_never_binds_changes_nothing(gpu, context, mode):
    H, A = 5, 6
    other = dict(cem_noise_beta=1.0, cem_keep_elites=2)
    plain, prob = plan_model(context, H, **MODEL, **other)
    bound, _ = plan_model(context, H, cem_constraints=NEVER, cem_constraint_mode=mode, cem_constraint_weight=7.0, **MODEL, **other)
    assert plain._opt.constraint_params is None and bound._opt.constraint_params.n == 2 and bound._opt.constraint_params.mode == (mode == "terminate")
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    cpa = (prob["cp_obs"], prob["cp_act"]) if context else ()
    for call in range(3):
        pa = plain.get_action(prob["obs"], *cpa, mean, var)
        pb = bound.get_action(prob["obs"], *cpa, mean, var)
        assert np.isfinite(pa).all() and 0 < np.abs(pa).max() <= 1.0
        np.testing.assert_array_equal(_bits(pa), _bits(pb), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(plain._plan_carry)), _bits(_np(bound._plan_carry)))
        chk = bound.constraint_check(prob["obs"], pb, *cpa)
        assert (chk["violations"] == 0).all() and (chk["first_violation"] == H).all() and (chk["violation_fraction"] == 0).all()
        mean = np.concatenate([pa[:, 1:], np.zeros((M, 1, A))], axis=1)
    assert (False, False) in plain.engine._loop_ws and (False, True) not in plain.engine._loop_ws      # no trajectory view without constraints
    assert (False, True) in bound.engine._loop_ws
    assert bound.engine._loop_ws[(False, True)][1].numel() > plain.engine._loop_ws[(False, False)][1].numel()


# ---------------------------------------------------------------------------------------------------------------------- 5
def test_a_constraint_that_binds_changes_the_plan(hc5):
    """penalty with w = 2^20: one more violating step costs 2^20 / p of a candidate's mean, far beyond any return, so the elites of the
    last iteration are the candidates with the fewest violations available in it."""
    prob, eng = hc5[True]
    H, p = 5, eng.p
    cons = binding_bounds(iteration0_traj(eng, prob, 0.0, 6, 1), (1, 7), H, "binding")
    cp = HipEngine.constraint_params(cons, "penalty", 2.0 ** 20)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    free = _np(eng.scored_plan(None, HipEngine.icem_params(), *args, seed=6, call=1))
    tied = _np(eng.constrained_plan(cp, None, HipEngine.icem_params(), *args, seed=6, call=1))
    assert np.isfinite(tied).all() and np.abs(tied - free).max() > 1e-3
    plan, info, _ = hplanner.icem_plan(eng, *args, seed=6, call=1, return_info=True, constraints=cp)
    np.testing.assert_array_equal(_bits(_np(plan)), _bits(tied))
    last = info[-1]
    total = _np(last["violations"]).sum(axis=-1)                                      # [m, n]
    np.testing.assert_array_equal(_np(last["violations"]), cref.counters(_np(last["traj"]), cons)[1])
    assert np.abs(_np(last["rows_raw"])).max() < 2.0 ** 20 / p / 8
    elites = _np(last["elites"])
    for mi in range(M):
        rest = np.setdiff1d(np.arange(total.shape[1]), elites[mi])
        print("env %d: violation totals of the elites %s, of the others min %d" % (mi, total[mi, elites[mi]].tolist(), total[mi, rest].min()))
        assert total[mi, elites[mi]].max() <= total[mi, rest].min(), "env %d: an elite violates more than a candidate left out" % mi
        assert total[mi].max() > total[mi].min()


# ---------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_class_route_and_companions(gpu, context):
    from cadm_amd.caller import DevicePlannerState
    H, A, K, p = 5, 6, 2, 5
    cons = [dict(dim=1, lo=-0.3, hi=0.6), dict(dim=7, hi=2.0)]
    kw = dict(cem_constraints=cons, cem_constraint_mode="terminate", cem_constraint_weight=3.0, cem_keep_elites=K, cem_noise_beta=1.0)
    model, prob = plan_model(context, H, **MODEL, **kw)
    eng, n = model.engine, MODEL["n_candidates"]
    cp_ = (prob["cp_obs"], prob["cp_act"]) if context else (None, None)
    cpa = cp_ if context else ()
    opt = hplanner.PlanOptions.from_kwargs(use_cem=True, n_particles=p, **kw)
    assert model._opt.constraints == opt.constraints and model._opt.constraint_params.mode == 1
    carry, valid = zero_carry(eng, M, K, H)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    for call in (1, 2):
        got = model.get_action(prob["obs"], *cpa, mean, var)
        assert model._call == call and got.shape == (M, H, A) and np.isfinite(got).all() and 0 < np.abs(got).max() <= 1.0
        want = _np(eng.opt_in_plan(opt, prob["obs"], cp_[0], cp_[1], mean, var, n, carry=carry, carry_valid=valid, seed=model.seed, call=call))
        np.testing.assert_array_equal(_bits(got), _bits(want))
        np.testing.assert_array_equal(_bits(_np(model._plan_carry)), _bits(_np(carry)))
        mean = np.concatenate([got[:, 1:], np.zeros((M, 1, A))], axis=1)
    # the constraints are in the loop: the same switches without them plan something else
    free = _np(eng.icem_plan(HipEngine.icem_params(noise_beta=1.0, keep_elites=K), prob["obs"], cp_[0], cp_[1], np.zeros((M, H, A)), var, n,
                             carry=torch.zeros_like(carry), carry_valid=torch.zeros_like(valid), seed=model.seed, call=1))
    first_plan = _np(eng.opt_in_plan(opt, prob["obs"], cp_[0], cp_[1], np.zeros((M, H, A)), var, n, carry=torch.zeros_like(carry),
                                     carry_valid=torch.zeros_like(valid), seed=model.seed, call=1))
    assert np.abs(first_plan - free).max() > 1e-3
    # constraint_check: the rollout of the forecast's iteration word, then the kernel; the call counter stays
    chk = model.constraint_check(prob["obs"], got, *cpa)
    assert model._call == 2
    assert sorted(chk) == ["first_violation", "returns", "violation_fraction", "violations"]
    assert chk["violations"].shape == chk["first_violation"].shape == chk["returns"].shape == (M, p) and chk["violation_fraction"].shape == (M,)
    ctxv = eng.context_forward(*cp_) if context else None
    acts = eng._t(got)[:, None].contiguous()
    rows, traj = eng.rollout_returns(prob["obs"], ctxv, acts, seed=model.seed, call=2, it=hplanner.FORECAST_IT, want_traj=True)
    r2, f2, v2 = eng.constrain_returns(traj, rows, model._opt.constraint_params, obs=prob["obs"], actions=acts)
    np.testing.assert_array_equal(_bits(chk["returns"]), _bits(_np(r2)[:, 0]))
    np.testing.assert_array_equal(chk["first_violation"], _np(f2)[:, 0])
    np.testing.assert_array_equal(chk["violations"], _np(v2)[:, 0])
    np.testing.assert_array_equal(chk["first_violation"], cref.counters(_np(traj), cons)[0][:, 0])
    np.testing.assert_array_equal(chk["violation_fraction"], (chk["violations"] > 0).mean(-1))
    wide = model.constraint_check(prob["obs"], np.stack([got, got], 1), *cpa)
    assert wide["violations"].shape == (M, 2, p) and wide["violation_fraction"].shape == (M, 2) and model._call == 2
    if context:
        with pytest.raises(ValueError, match="constraint_check: cp_obs"):
            model.constraint_check(prob["obs"], got, prob["cp_obs"][:, :-1], prob["cp_act"])
        with pytest.raises(ValueError, match="cp_obs and cp_act are required"):
            model.constraint_check(prob["obs"], got)
    with pytest.raises(ValueError, match="constraint_check: obs"):
        model.constraint_check(prob["obs"], got[:, :-1], *cpa)
    again = model.constraint_check(prob["obs"], got, *cpa)
    np.testing.assert_array_equal(_bits(again["returns"]), _bits(chk["returns"]))
    # reset_plan_carry: the next plan is a fresh model's
    fresh, _ = plan_model(context, H, **MODEL, **kw)
    fresh._call = model._call
    model.reset_plan_carry()
    np.testing.assert_array_equal(_np(model._plan_carry_valid), [0, 0])
    np.testing.assert_array_equal(model.get_action(prob["obs"], *cpa, mean, var), fresh.get_action(prob["obs"], *cpa, mean, var))
    if not context:
        # fit: a model with constraints trains as one without
        twin, _ = plan_model(False, H, **MODEL, cem_keep_elites=K, cem_noise_beta=1.0)
        rng = np.random.default_rng(2)
        o = rng.standard_normal((128, 18))
        a_, nx = rng.uniform(-1, 1, (128, 6)), o + 0.1 * rng.standard_normal((128, 18))
        for mdl in (model, twin):
            mdl.fit(o, a_, nx, epochs=1, rng=np.random.default_rng(0))
        np.testing.assert_array_equal(model.predict(o[:8], a_[:8]), twin.predict(o[:8], a_[:8]))
        return
    state = DevicePlannerState(model, M)
    c2, v2 = model._plan_carry.clone(), model._plan_carry_valid.clone()
    act = state.act(prob["obs"])
    zero = torch.zeros((M, H, A), dtype=torch.float32, device=eng.device)
    want = eng.constrained_plan(model._opt.constraint_params, None, HipEngine.icem_params(noise_beta=1.0, keep_elites=K), prob["obs"],
                                torch.zeros_like(state.hist_obs), torch.zeros_like(state.hist_act), zero, state.init_var, n, carry=c2,
                                carry_valid=v2, seed=model.seed, call=model._call)
    np.testing.assert_array_equal(_bits(_np(act)), _bits(_np(want)[:, 0]))
    np.testing.assert_array_equal(_bits(_np(model._plan_carry)), _bits(_np(c2)))


# ---------------------------------------------------------------------------------------------------------------------- 7
def a256(x):
    return (x + 255) // 256 * 256


def icem_bytes(E, m, n, C, K, num_elites, H, A, p):          # tests/test_gpu_workspace_bytes.py's restatement
    return (a256(4 * E * m * max(C, 1)) + a256(4 * m * n * H * A) + a256(4 * m * n * p) + a256(4 * m * n) + 3 * a256(4 * m * H * A)
            + a256(4 * m * max(K, 1) * H * A) + a256(4 * m) + a256(4 * m * H * A) + a256(4 * m * num_elites))


def test_workspace_bytes_and_null_constraints(hc5):
    prob, eng = hc5[True]
    H, A, p, D, E, C = 5, 6, 5, 18, 5, prob["C"]
    for m, n, K in ((1, 24, 0), (2, 24, 2), (3, 70, 8)):
        view = a256(4 * H * m * n * p * D)
        assert eng.lib.cadm_constrained_workspace_bytes(eng._ctx, m, n, K, 0) == icem_bytes(E, m, n, C, K, KE, H, A, p) + view, (m, n, K)
        assert eng.lib.cadm_constrained_workspace_bytes(eng._ctx, m, n, K, 1) == eng.lib.cadm_mppi_workspace_bytes(eng._ctx, m, n, K) + view
        assert eng.lib.cadm_icem_workspace_bytes(eng._ctx, m, n, K) == icem_bytes(E, m, n, C, K, KE, H, A, p)
    for bad in ((0, 24, 0), (2, 0, 0), (2, 24, -1)):
        assert eng.lib.cadm_constrained_workspace_bytes(eng._ctx, *bad, 0) == 0
    assert eng.lib.cadm_constrained_workspace_bytes(None, 2, 24, 0, 0) == 0
    # constraints == NULL: cadm_scored_plan, bit for bit
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    mean, var = prob["init_mean"], prob["init_var"]
    views = {slot: ws.data_ptr() for slot, (_, ws) in eng._loop_ws.items() if slot[1]}      # (the engine is shared with the tests above)
    for update, score in (("cem", None), ("mppi", HipEngine.score_params("cvar", k=2))):
        icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, return_best=True, add_mean_last=True)
        prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
        (ca, va), (cb, vb) = zero_carry(eng, M, 2, H), zero_carry(eng, M, 2, H)
        for call in (1, 2):
            want, wr = eng.scored_plan(score, prm, *args, mean, var, N, carry=ca, carry_valid=va, seed=9, call=call, want_best_return=True)
            got, gr = eng.constrained_plan(None, score, prm, *args, mean, var, N, carry=cb, carry_valid=vb, seed=9, call=call, want_best_return=True)
            np.testing.assert_array_equal(_bits(_np(got)), _bits(_np(want)))
            np.testing.assert_array_equal(_bits(_np(gr)), _bits(_np(wr)))
            np.testing.assert_array_equal(_bits(_np(ca)), _bits(_np(cb)))
    assert {slot: ws.data_ptr() for slot, (_, ws) in eng._loop_ws.items() if slot[1]} == views, "constraints=None must not allocate a trajectory view"
    assert (False, False) in eng._loop_ws and (True, False) in eng._loop_ws


def test_refusals(hop, hc5):
    """Every CADM_EINVAL / CADM_ESTATE case, through the C ABI, before any HIP call: the null pointers next to a bad argument are
    never touched and the outputs keep their sentinel."""
    prob, eng = hc5[True]
    lib, ctx, D = eng.lib, eng._ctx, 18
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=eng.device)
    out = torch.full((M * N * 5,), 123.0, dtype=torch.float32, device=eng.device)
    ibuf = torch.zeros(64, dtype=torch.int32, device=eng.device)
    P, O, I = ct.c_void_p(buf.data_ptr()), ct.c_void_p(out.data_ptr()), ct.c_void_p(ibuf.data_ptr())

    def make(n=1, mode=0, weight=1.0, dim=0, lo=-1.0, hi=1.0):
        c = _lib.ConstraintParams()
        c.n, c.mode, c.weight = n, mode, weight
        for k in range(16):
            c.dim[k], c.lo[k], c.hi[k] = 0, -1.0, 1.0
        k = max(0, min(n, 16) - 1)
        c.dim[k], c.lo[k], c.hi[k] = dim, lo, hi
        return c

    def constrain(c, cx=ctx, traj=P, obs=P, acts=P, rows=P, m=M, n=N, dst=O):
        return lib.cadm_constrain_returns(cx, None if c is None else ct.byref(c), traj, obs, acts, rows, m, n, dst, None, None, None)

    def plan(c, cx=ctx, update=0):
        prm = HipEngine.mppi_params()
        return lib.cadm_constrained_plan(cx, ct.byref(c), None, update, ct.byref(prm), P, P, P, P, P, None, None, M, N, 0, 1, P, O, None, None)

    def refused(rc, name, frag, code=-1):
        msg = lib.cadm_last_error().decode()
        assert rc == code, "%s: expected %d, got %d (%s)" % (name, code, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    nan, inf = float("nan"), float("inf")
    bad = [(make(n=0), "constraints, outside"), (make(n=17), "constraints, outside"), (make(n=-1), "constraints, outside"),
           (make(dim=-1), "reads dim -1"), (make(dim=D), "reads dim %d" % D), (make(n=3, dim=D + 5), "constraint 2 reads dim"),
           (make(lo=1.0, hi=1.0), "lo 1 >= hi 1"), (make(lo=2.0, hi=1.0), "lo 2 >= hi 1"), (make(lo=nan), "NaN bound"), (make(hi=nan), "NaN bound"),
           (make(lo=-inf, hi=inf), "both sides infinite"), (make(lo=inf, hi=inf), ">= hi"), (make(mode=2), "unknown constraint mode 2"),
           (make(mode=-1), "unknown constraint mode -1"), (make(weight=-1.0), "weight"), (make(weight=nan), "weight"), (make(weight=inf), "weight")]
    for c, frag in bad:
        refused(constrain(c), "cadm_constrain_returns", frag)
        refused(plan(c), "cadm_constrained_plan", frag)
        refused(plan(c, update=1), "cadm_constrained_plan", frag)
    ok, okt = make(), make(mode=1)
    refused(constrain(None), "cadm_constrain_returns", "is null")
    refused(constrain(ok, traj=None), "cadm_constrain_returns", "is null")
    refused(constrain(ok, rows=None), "cadm_constrain_returns", "is null")
    refused(constrain(ok, dst=None), "cadm_constrain_returns", "is null")
    refused(constrain(ok, cx=None), "cadm_constrain_returns", "is null")
    refused(constrain(okt, obs=None), "cadm_constrain_returns", "terminate mode")
    refused(constrain(okt, acts=None), "cadm_constrain_returns", "terminate mode")
    refused(constrain(ok, m=0), "cadm_constrain_returns", "m, n must be")
    refused(constrain(ok, n=0), "cadm_constrain_returns", "m, n must be")
    refused(plan(ok, update=2), "cadm_constrained_plan", "update 2")
    # a discrete ctx
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=1, H=4, seed=1)
    deng = make_engine(dprob, p=5)
    refused(constrain(ok, cx=deng._ctx), "cadm_constrain_returns", "discrete")
    refused(plan(ok, cx=deng._ctx), "cadm_constrained_plan", "continuous actions only")
    deng.close()
    # a spec ctx before cadm_set_env_spec: terminate needs the spec's reward terms, penalty does not
    spec, sprob, seng = hop
    raw = ct.c_void_p()
    assert seng.lib.cadm_ctx_create(ct.byref(seng.cfg), ct.byref(raw)) == 0
    refused(constrain(okt, cx=raw), "cadm_constrain_returns", "cadm_set_env_spec", code=-4)
    seng.lib.cadm_ctx_destroy(raw)
    # a candidate-sharded ctx (a host-supplied all-gather registered for two ranks; it is never called)
    shp = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=5, seed=3, trained_like=True)
    sheng = make_engine(shp, p=5, num_elites=KE, num_cem_iters=ITERS)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(sheng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    refused(constrain(ok, cx=sheng._ctx), "cadm_constrain_returns", "sharded")
    refused(plan(ok, cx=sheng._ctx), "cadm_constrained_plan", "sharded")
    assert lib.cadm_dist_destroy(sheng._ctx) == 0
    sheng.close()
    torch.cuda.synchronize()
    assert (_np(out) == 123.0).all()                     # no refused call wrote a return or a plan
    # the Python layer
    traj, obs, acts = synth_traj(5, 5, M, 3, 5, 18, 6)
    rows = np.zeros((M, 3, 5), np.float32)
    with pytest.raises(ValueError, match="do not agree with the engine"):
        eng.constrain_returns(traj[:4], rows, [dict(dim=0, lo=0.0)], "penalty", 1.0)
    with pytest.raises(ValueError, match="do not agree with the engine"):
        eng.constrain_returns(traj, np.ascontiguousarray(rows[:, :2]), [dict(dim=0, lo=0.0)], "penalty", 1.0)
    with pytest.raises(_lib.CadmError, match="reads dim 18"):
        eng.constrain_returns(traj, rows, [dict(dim=18, lo=0.0)], "penalty", 1.0)
    with pytest.raises(_lib.CadmError, match="terminate mode"):
        eng.constrain_returns(traj, rows, [dict(dim=0, lo=0.0)], "terminate", 1.0)
    r, f, v = eng.constrain_returns(traj, rows, [dict(dim=0, lo=0.0)], "penalty", 1.0)      # the engine works afterwards
    np.testing.assert_array_equal(_np(v), cref.counters(traj, [dict(dim=0, lo=0.0)])[1])


def test_refusals_at_construction(gpu):
    from cadm_amd.envs import make_env_spec
    cons = [dict(dim=1, lo=-1.0, hi=1.0)]
    for bad, msg in ((dict(cem_constraints=cons), "need a cem_constraint_weight"), (dict(cem_constraint_weight=1.0), "they need cem_constraints"),
                     (dict(cem_constraint_mode="terminate"), "they need cem_constraints"),
                     (dict(cem_constraints=cons, cem_constraint_weight=-1.0), "finite and >= 0"),
                     (dict(cem_constraints=cons, cem_constraint_weight=1.0, cem_constraint_mode="stop"), "'penalty' or 'terminate'"),
                     (dict(cem_constraints=[dict(dim=18, lo=0.0)], cem_constraint_weight=1.0), "observation dim 18"),
                     (dict(cem_constraints=[dict(dim=1, lo=1.0, hi=0.0)], cem_constraint_weight=1.0), "must be below"),
                     (dict(use_cem=False, cem_constraints=cons, cem_constraint_weight=1.0), "need use_cem=True")):
        for context in (False, True):
            with pytest.raises(ValueError, match=msg):
                plan_model(context, 5, **MODEL, **bad)
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        plan_model(True, 5, env=make_env_spec("cartpole"), cem_constraints=cons, cem_constraint_weight=1.0, **MODEL)
    model, prob = plan_model(True, 5, **MODEL)
    assert model._opt is None
    with pytest.raises(ValueError, match="no cem_constraints"):
        model.constraint_check(prob["obs"], np.zeros((M, 5, 6)), prob["cp_obs"], prob["cp_act"])
