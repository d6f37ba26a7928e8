"""GPU: the discount over the horizon of the opt-in planner (`cadm_set_discount`, csrc/discount.hip) -- the table, the env-return kernel
(`cadm_discount_returns`) on synthetic trajectories and at its edges, every stage behind the rollout under a table, the fused loop
against the stepwise one with every term on, a discount that reaches the plan, the class route with `plan_returns`, the engine's state
across `set_discount`, and the refusals.

Geometries: the compiled-in halfcheetah 200 x 4 kernel and tests/test_gpu_horizon.py's hopper_like declaration (the JIT module that file,
tests/test_gpu_forecast.py and tests/test_gpu_constraints.py build); the env-return kernel also on ant, slim_humanoid and pendulum at
tests/behind_rollout.py's inputs.  Numpy restatement: tests/discount_ref.py.

Bound of the env's return, derived, not measured.  The kernel forms sum = fl(disc[0] r_0), sum = fl(sum + fl(disc[t] r_t)) with r_t its
float32 step reward.  Against the float64 reference sum_t disc[t] r_t of the env's closure: a step reward is off by at most b_t =
`forecast_ref.reward_bound` (the bound tests/test_gpu_forecast.py and tests/test_gpu_constraints.py hold a step reward to), which the
weight disc[t] <= 1 does not enlarge; the product rounds by at most 2^-24 |disc[t] r_t|; and the add that takes the term in rounds by
at most 2^-24 of a partial sum, which the second 2^-24 |disc[t] r_t| of the step's share stands for.  Per step that is
b_t + 2^-23 |disc[t] r_t|, over a row at most H max_t (b_t + 2^-23 |disc[t] r_t|).  `step_out` is the float32 step reward itself and
is held to b_t.  TERMINATE rows under a discount are the same chain up to tau -- (tau + 1) max_{t <= tau} of the same term -- and one
more product and subtraction, w disc[tau] off the sum: 2^-24 |reference| is added for it, as tests/test_gpu_constraints.py adds it on a
model's own rollouts.  Everything else (PENALTY rows, the tracking cost, the reward step sum, the uncertainty and actuator costs, the
terminal terms) is compared bit for bit with the float32 chains of tests/discount_ref.py, from the device's own per-step outputs where
the stage has a GEMM in front of the sum."""
import ctypes as ct

import numpy as np
import pytest
import torch

import behind_rollout as br
import constraint_ref as cref
import discount_ref as dref
import reward_ref as rref
import value_ref as vref
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
from test_gpu_constraints import binding_bounds, coverage, iteration0_traj, plant_ends

pytestmark = pytest.mark.gpu

F = np.float32
M, N, KE, ITERS = 2, 24, 8, 3


def hopper_like():          # tests/test_gpu_horizon.py's declaration (same geometry: one JIT module serves the files that declare it)
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


class discounted:
    """`with discounted(eng, gamma) as disc:` -- the engine under a discount, cleared again behind the block (the engines are shared)"""

    def __init__(self, eng, gamma):
        self.eng, self.gamma = eng, gamma

    def __enter__(self):
        self.eng.set_discount(self.gamma)
        disc = self.eng.discount_weights()
        np.testing.assert_array_equal(_bits(disc), _bits(dref.weights(self.gamma, self.eng.H)))
        return disc

    def __exit__(self, *exc):
        self.eng.set_discount(1.0)


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


# ---------------------------------------------------------------------------------------------------------------------- 1: the table
def test_table(hop, hc8):
    for eng, H in ((hop[2], 3), (hc8[1], 8)):
        assert eng.H == H and eng.discount_weights() is None
        for gamma in (0.5, 0.99):
            eng.set_discount(gamma)
            w = eng.discount_weights()
            assert w.dtype == np.float32 and w.shape == (H + 1,) and w[0] == 1.0
            want = np.array([np.float32(np.power(np.float64(np.float32(gamma)), np.float64(t))) for t in range(H + 1)], np.float32)
            np.testing.assert_array_equal(_bits(w), _bits(want))
        eng.set_discount(1.0)
        assert eng.discount_weights() is None
        for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="not in \\(0, 1\\]"):
                eng.set_discount(bad)
            rc = eng.lib.cadm_set_discount(eng._ctx, ct.c_float(bad), None)
            assert rc == -1 and b"cadm_set_discount: the discount" in eng.lib.cadm_last_error()
        assert eng.discount_weights() is None


# ---------------------------------------------------------------------------------------------------------------------- 2: the env's return
def check_env_kernel(eng, env, terms_env, traj, obs, acts, gamma, seed, what, shows=True):
    H, m, n, p, D = traj.shape
    rows = np.random.default_rng(seed).uniform(-30, 30, (m, n, p)).astype(F)
    nan_at = (m - 1, n - 1, p - 1)
    rows[nan_at] = np.nan
    with discounted(eng, gamma) as disc:
        ref, r = dref.env_returns(env, traj, obs, acts, disc, rows=rows)
        lim = dref.env_bound(terms_env, traj, obs, acts, disc, r)
        plain = r.sum(axis=2)
        live = ~np.isnan(rows)
        ratio = (np.abs(ref - plain) / lim)[live]
        print("%s: discounted and undiscounted reference differ by more than 100 x the bound on %.0f %% of %d rows, smallest ratio %.0f"
              % (what, 100 * (ratio > 100).mean(), ratio.size, ratio.min()))
        if shows:
            assert (ratio > 100).mean() >= 0.9, "%s: the comparison does not tell a discounted return from an undiscounted one" % what
        got, steps = eng.discount_returns(traj, obs, acts, rows, want_steps=True)
        torch.cuda.synchronize()
        got, steps = _np(got), _np(steps)
        assert steps.shape == (H, m, n, p)
        with np.errstate(all="ignore"):
            b = np.moveaxis(reward_bound(terms_env, traj, obs, acts), 2, 0)
        es = np.abs(steps.astype(np.float64) - np.moveaxis(r, 2, 0))
        print("%s step_out: worst |err| / bound %.3f" % (what, (es / b).max()))
        assert (es <= b).all(), "%s step_out: worst |err| / bound %.3f" % (what, (es / b).max())
        assert np.isnan(got[nan_at]) and _bits(got)[nan_at] == _bits(rows)[nan_at], what + ": a NaN in rows_in stays that NaN"
        err = np.abs(got.astype(np.float64) - ref)[live]
        print("%s: worst |err| / bound %.3f over %d rows" % (what, (err / lim[live]).max(), err.size))
        assert (err <= lim[live]).all(), "%s: worst |err| / bound %.3f" % (what, (err / lim[live]).max())
        # run to run, inside a sub-batch, in place
        again = _np(eng.discount_returns(traj, obs, acts, rows))
        np.testing.assert_array_equal(_bits(again), _bits(got), err_msg=what + ": run to run")
        cuts = [(slice(m - 1, m), slice(None))] + ([(slice(None), slice(n - 1, n))] if n > 1 else []) + ([(slice(1, m), slice(None))] if m > 2 else [])
        for ms, ns in cuts:
            sub = _np(eng.discount_returns(np.ascontiguousarray(traj[:, ms, ns]), obs[ms], np.ascontiguousarray(acts[ms, ns]),
                                           np.ascontiguousarray(rows[ms, ns])))
            np.testing.assert_array_equal(_bits(sub), _bits(got[ms, ns]), err_msg="%s: sub-batch %r" % (what, (ms, ns)))
        io = eng._t(rows.copy())
        eng.discount_returns(traj, obs, acts, io, out=io)
        np.testing.assert_array_equal(_bits(_np(io)), _bits(got), err_msg=what + ": rows_out aliasing rows_in")
        # a NaN state at step 1 of one row: that row's return is NaN, its neighbours keep their bits
        if H >= 3:
            t = traj.copy()
            t[1, 0, 0, 0, :] = np.nan
            bad = _np(eng.discount_returns(t, obs, acts, rows))
            assert np.isnan(bad[0, 0, 0]), what + ": a NaN state did not reach its row"
            keep = np.ones((m, n, p), bool)
            keep[0, 0, 0] = False
            np.testing.assert_array_equal(_bits(bad[keep]), _bits(got[keep]), err_msg=what + ": a NaN state reached another row")
    return got


def test_env_kernel_shape_a_declared_env(hop):
    spec, prob, eng = hop
    traj, obs, acts = synth_traj(1, 3, 3, 2, 5, 11, 3)
    traj = (traj * F(0.4)).astype(F)
    check_env_kernel(eng, spec, spec, traj, obs, acts, 0.5, 11, "(a) D=11 p=5 H=3")


def test_env_kernel_shape_b_halfcheetah(hc8):
    prob, eng = hc8
    traj, obs, acts = synth_traj(2, 8, 2, 1, 20, 18, 6)
    check_env_kernel(eng, oenvs.make_env("halfcheetah"), "halfcheetah", traj, obs, acts, 0.9, 12, "(b) D=18 p=20 H=8")


def test_env_kernel_shape_c_one_particle_three_workgroups(gpu):
    """p = 1 and 135 rows: two full workgroups and one of 7 rows; step spans that start 8 bytes off a 16-byte boundary at odd steps"""
    prob = synth.make_problem(env="halfcheetah", context=True, E=1, m=1, H=3, seed=54)
    eng = make_engine(prob, p=1)
    traj, obs, acts = synth_traj(3, 3, 5, 27, 1, 18, 6)
    check_env_kernel(eng, oenvs.make_env("halfcheetah"), "halfcheetah", traj, obs, acts, 0.5, 13, "(c) D=18 p=1 H=3, 135 rows")
    eng.close()


def test_env_kernel_shape_d_declared_env_three_workgroups(hop):
    spec, prob, eng = hop
    traj, obs, acts = synth_traj(4, 3, 3, 11, 5, 11, 3)
    traj = (traj * F(0.4)).astype(F)
    check_env_kernel(eng, spec, spec, traj, obs, acts, 0.5, 14, "(d) D=11 p=5 H=3, 165 rows")


@pytest.mark.parametrize("kind", sorted(br.KINDS))
def test_env_kernel_other_kinds(gpu, kind):
    """ant, slim_humanoid and pendulum at tests/behind_rollout.py's inputs (the engines of tests/test_gpu_behind_rollout_envs.py)"""
    D, A, p, H = br.KINDS[kind][:4]
    prob = synth.make_problem(env=kind, context=True, E=5, m=3, H=H, seed=60 + sorted(br.KINDS).index(kind))
    eng = make_engine(prob, p=p)
    traj, obs, acts, _ = br.kind_inputs(kind)
    check_env_kernel(eng, oenvs.make_env(kind), kind, traj, obs, acts, 0.5, 15, "%s D=%d p=%d H=%d" % (kind, D, p, H), shows=False)
    eng.close()


def test_env_kernel_needs_a_discount(hop):
    spec, prob, eng = hop
    traj, obs, acts = synth_traj(1, 3, 3, 2, 5, 11, 3)
    with pytest.raises(_lib.CadmError, match="no discount is set"):
        eng.discount_returns(traj, obs, acts, np.zeros((3, 2, 5), F))
    with discounted(eng, 0.5):
        with pytest.raises(ValueError, match="do not agree with the engine"):
            eng.discount_returns(traj[:2], obs, acts, np.zeros((3, 2, 5), F))
        with pytest.raises(ValueError, match="obs .* actions"):
            eng.discount_returns(traj, obs[:2], acts, np.zeros((3, 2, 5), F))


# ---------------------------------------------------------------------------------------------------------------------- 3: the stages
def _value(eng, weight, seed=33):
    prm = HipEngine.value_params((16,), "relu", weight)
    eng.set_value_net(prm, vref.he_net(eng.D, (16,), seed))
    return prm


def _reward(eng, weight, seed=31):
    prm = HipEngine.reward_params("obs_act_next_obs", (16,), "tanh", weight)
    eng.set_reward_net(prm, rref.he_net(rref.input_dims("obs_act_next_obs", eng.D, eng.A), (16,), seed))
    return prm


def check_stages(eng, env, terms_env, traj, obs, acts, cons, gamma, seed, what):
    from test_gpu_critic import _simple
    import actuator_ref as aref
    import tracking_ref as tref
    H, m, n, p, D = traj.shape
    A = acts.shape[-1]
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-30, 30, (m, n, p)).astype(F)
    first, viol = cref.counters(traj, cons)
    coverage(first, H, what)
    bad = cref.violation_mask(traj, cons)
    plain_pen = _np(eng.constrain_returns(traj, rows, cons, "penalty", 4.0)[0])
    with discounted(eng, gamma) as disc:
        # PENALTY, w = 4: bit for bit, the counters unchanged
        pen, f, v = (_np(x) for x in eng.constrain_returns(traj, rows, cons, "penalty", 4.0))
        np.testing.assert_array_equal(f, first)
        np.testing.assert_array_equal(v, viol)
        np.testing.assert_array_equal(_bits(pen), _bits(dref.penalty_rows(rows, bad, 4.0, disc)), err_msg=what + ": penalty rows")
        np.testing.assert_array_equal(_bits(pen[first == H]), _bits(rows[first == H]))
        assert (pen != plain_pen)[viol > (first == 0)].all(), what + ": the penalty ignores the table"
        # TERMINATE, w = 4: within the bound of the module docstring
        ref = dref.terminate_rows(env, traj, obs, acts, rows, first, 4.0, disc)
        r = dref.env_returns(env, traj, obs, acts, disc)[1]
        lim = dref.env_bound(terms_env, traj, obs, acts, disc, r, first=first) + 2.0 ** -24 * np.abs(ref)
        ter, f, v = (_np(x) for x in eng.constrain_returns(traj, rows, cons, "terminate", 4.0, obs=obs, actions=acts))
        np.testing.assert_array_equal(f, first)
        np.testing.assert_array_equal(v, viol)
        alive = first == H
        np.testing.assert_array_equal(_bits(ter[alive]), _bits(rows[alive]), err_msg=what + ": rows without a violation")
        err = np.abs(ter.astype(np.float64) - ref)[~alive]
        print("%s terminate: worst |err| / bound %.3f over %d rows" % (what, (err / lim[~alive]).max(), err.size))
        assert (err <= lim[~alive]).all(), "%s terminate: worst |err| / bound %.3f" % (what, (err / lim[~alive]).max())
        undisc = cref.terminate_rows(env, traj, obs, acts, rows, first, 4.0)
        late = (first > 0) & (first < H)
        assert (np.abs(ref - undisc)[late] > 100 * lim[late]).mean() > 0.5, what + ": terminate does not tell the table from none"
        # tracking: rows and cost bit for bit, with and without the cut
        terms = [dict(dim=1, kind="square", w=0.7), dict(dim=D - 1, kind="abs", w=1.3), dict(dim=3, kind="huber", w=0.5, delta=0.75)]
        targets = (traj.reshape(-1, D).mean(axis=0)[[1, D - 1, 3]] + rng.standard_normal((m, H + 1, 3))).astype(F)
        targets[rng.uniform(size=targets.shape) < 0.2] = np.nan
        offset = rng.integers(-1, 2, m).astype(np.int32)
        track = HipEngine.track_params(terms)
        for fv in (None, first):
            out, cost = (_np(x) for x in eng.tracking_returns(traj, rows, track, targets, offset=offset, first=fv, want_cost=True))
            want = dref.tracking32(traj, rows, terms, targets, disc, offset, fv)
            np.testing.assert_array_equal(_bits(cost), _bits(want[1]), err_msg=what + ": tracking cost")
            np.testing.assert_array_equal(_bits(out), _bits(want[0]), err_msg=what + ": tracked rows")
            assert (cost != tref.float32_chain(traj, rows, terms, targets, offset, fv)[1]).mean() > 0.3
        # the learned reward: the step sum from the device's own step_out
        rew = _reward(eng, 1.5)
        for fv in (None, first):
            out, steps, S = (_np(x) for x in eng.reward_returns(traj, obs, acts, rows, rew, first=fv, want_steps=True))
            np.testing.assert_array_equal(_bits(S), _bits(dref.step_sum(steps, disc, fv)), err_msg=what + ": reward step sum")
            np.testing.assert_array_equal(_bits(out), _bits(rref.update(rows, S, 1.5)))
            assert (S != rref.step_sum(steps, fv))[(first > 0) if fv is not None else np.ones_like(alive)].mean() > 0.9
        # the uncertainty cost from the device's own step costs, both kernels
        unc = HipEngine.uncertainty_params("epistemic" if p > 1 else "total", 1.0, None, "std", None, obs_dim=D)
        for fv in (None, first):
            step, cost = (_np(x) for x in eng.uncertainty_cost(traj, unc, first=fv, want_steps=True))
            walk = _np(eng.uncertainty_cost(traj, unc, first=fv))
            want = dref.uncertainty_cost32(step, disc, fv)
            np.testing.assert_array_equal(_bits(cost), _bits(want), err_msg=what + ": uncertainty cost")
            np.testing.assert_array_equal(_bits(walk), _bits(want), err_msg=what + ": uncertainty cost, the walking kernel")
        # the terminal value and the terminal Q: rows + fl32(weight disc[H]) v from the device's own v_out / q_out
        val = _value(eng, 0.75)
        crt, pol, _, _ = _simple(eng, (16,), (16,), 2, "relu", "min", 0.6, seed=5)
        for fv in (None, first):
            out, vv = (_np(x) for x in eng.value_returns(traj, rows, val, first=fv, want_v=True))
            np.testing.assert_array_equal(_bits(out), _bits(dref.terminal_update(rows, vv, 0.75, disc, fv, H)), err_msg=what + ": terminal value")
            out, qq = (_np(x) for x in eng.critic_returns(traj, rows, crt, first=fv, want_q=True))
            np.testing.assert_array_equal(_bits(out), _bits(dref.terminal_update(rows, qq, 0.6, disc, fv, H)), err_msg=what + ": terminal Q")
            assert (out != vref.update(rows, qq, 0.6, fv, H))[alive if fv is not None else np.ones_like(alive)].mean() > 0.9
        # the actuator's rate cost; the sequences are untouched by the table
        seqs, dl, w, prev, prefix = aref.make_case(m, n, H, A, 1, seed=seed, nan_env=m - 1)
        act = HipEngine.actuator_params(1, dl, w, action_dim=A, horizon=H)
        y, cost = (_np(x) for x in eng.actuate_actions(eng._t(seqs).clone(), act, prev=prev, prefix=prefix, want_cost=True))
        np.testing.assert_array_equal(_bits(y), _bits(aref.actuate(seqs, 1, dl, w, prev, prefix, eng.cfg.lower_bound, eng.cfg.upper_bound)[0]))
        np.testing.assert_array_equal(_bits(cost), _bits(dref.actuator_cost32(y, w, disc, prev)), err_msg=what + ": actuator cost")
    cost1 = _np(eng.actuate_actions(eng._t(seqs).clone(), act, prev=prev, prefix=prefix, want_cost=True)[1])
    np.testing.assert_array_equal(_bits(cost1), _bits(aref.cost_f32(y, w, prev)), err_msg=what + ": actuator cost without a table")
    assert (cost < cost1)[:m - 1].all()


def test_stages_shape_a_declared_env(hop):
    spec, prob, eng = hop
    traj, obs, acts = synth_traj(1, 3, 3, 2, 5, 11, 3)
    traj = (traj * F(0.4)).astype(F)
    cons = [band(traj, 0, 1.5), band(traj, 10, 1.5, lower_only=True)]
    check_stages(eng, spec, spec, traj, obs, acts, cons, 0.5, 21, "(a) D=11 p=5 H=3")


def test_stages_shape_b_halfcheetah(hc8):
    prob, eng = hc8
    traj, obs, acts = synth_traj(2, 8, 2, 1, 20, 18, 6)
    cons = [band(traj, 1, 2.0), band(traj, 7, 2.0)]
    traj = plant_ends(traj, cons, "(b)")
    check_stages(eng, oenvs.make_env("halfcheetah"), "halfcheetah", traj, obs, acts, cons, 0.9, 22, "(b) D=18 p=20 H=8")


# ---------------------------------------------------------------------------------------------------------------------- 4: fused == stepwise
def everything(eng, prob, H, dims):
    """every term at once: TERMINATE constraints that bind, one tracking term, a reward net and a value net with one hidden layer of 16,
    an actuator rate cost and an uncertainty term"""
    cons_list = binding_bounds(iteration0_traj(eng, prob, 0.0, 4, 1), dims, H, "discounted")
    traj0 = iteration0_traj(eng, prob, 0.0, 4, 1)
    terms = [dict(dim=int(dims[0]), kind="square", w=0.3)]
    targets = np.full((M, H + 1, 1), float(traj0[..., dims[0]].mean()), F)
    return dict(cons_list=cons_list, cons=HipEngine.constraint_params(cons_list, "terminate", 4.0), terms=terms, track=HipEngine.track_params(terms),
                targets=eng._t(targets), targets_np=targets, offset=torch.zeros((M,), dtype=torch.int32, device=eng.device),
                reward=_reward(eng, 0.5), value=_value(eng, 0.75), w=np.full(eng.A, 0.25, F),
                act=HipEngine.actuator_params(0, None, 0.25, action_dim=eng.A, horizon=H),
                unc=HipEngine.uncertainty_params("epistemic", 0.3, None, "var", None, obs_dim=eng.D))


def check_fused_equals_stepwise(eng, prob, env, terms_env, dims, update, gamma, what):
    H, A, p = eng.H, eng.A, eng.p
    t = everything(eng, prob, H, dims)
    icem = dict(noise_beta=1.0 if update == "mppi" else 0.0, keep_elites=2, decay=1.0, return_best=update == "mppi", add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    obs32 = prob["obs"].astype(F)
    state = lambda: (torch.full((M, A), float("nan"), dtype=torch.float32, device=eng.device), torch.zeros((M, 0, A), dtype=torch.float32, device=eng.device))
    (pa, fa), (pb, fb) = state(), state()
    (ca, va), (cb, vb) = zero_carry(eng, M, 2, H), zero_carry(eng, M, 2, H)
    mean, var = prob["init_mean"], prob["init_var"]
    with discounted(eng, gamma) as disc:
        for call in (1, 2):
            a, ra = eng.rewarded_plan(t["reward"], t["value"], t["unc"], t["act"], pa, fa, True, t["track"], t["targets"], t["offset"], None, None,
                                      t["cons"], None, prm, *args, mean, var, N, carry=ca, carry_valid=va, seed=4, call=call, want_best_return=True)
            b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                                update=update, temperature=0.5, relative=True, constraints=t["cons"],
                                                tracking=(t["track"], t["targets"], t["offset"]), actuator=(t["act"], pb, fb),
                                                action_advance=True, uncertainty=t["unc"], value=t["value"], reward=t["reward"], **icem)
            a = _np(a)
            assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
            np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="%s: plan of call %d" % (what, call))
            np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="%s: best return of call %d" % (what, call))
            np.testing.assert_array_equal(_bits(_np(ca)), _bits(_np(cb)), err_msg="%s: carry after call %d" % (what, call))
            np.testing.assert_array_equal(_bits(_np(pa)), _bits(_np(pb)), err_msg="%s: actuator state after call %d" % (what, call))
            prev = np.full((M, A), np.nan, F) if call == 1 else prev_next
            x = info[-1]                                                           # the last iteration, stage by stage
            traj, acts = _np(x["traj"]), _np(x["actions"])
            first = cref.counters(traj, t["cons_list"])[0]
            np.testing.assert_array_equal(_np(x["first_violation"]), first)
            if call == 1:
                share = float((cref.counters(_np(info[0]["traj"]), t["cons_list"])[0] < H).mean())
                assert 0.2 <= share <= 0.8, "%s: %.2f of iteration 0's rows violate" % (what, share)
            # the env's own return: bounded
            drows = _np(x["rows_discounted"])
            ref, r = dref.env_returns(env, traj, obs32, acts, disc)
            lim = dref.env_bound(terms_env, traj, obs32, acts, disc, r)
            assert (np.abs(drows - ref) <= lim).all(), "%s: discounted rows, worst |err| / bound %.3f" % (what, (np.abs(drows - ref) / lim).max())
            np.testing.assert_array_equal(_bits(_np(x["rows_raw"])), _bits(drows))
            # TERMINATE: bounded; rows without a violation keep the discounted bits
            crow = _np(x["rows_untracked"])
            alive = first == H
            np.testing.assert_array_equal(_bits(crow[alive]), _bits(drows[alive]))
            tref_ = dref.terminate_rows(env, traj, obs32, acts, drows, first, 4.0, disc)
            tlim = dref.env_bound(terms_env, traj, obs32, acts, disc, r, first=first) + 2.0 ** -24 * np.abs(tref_)
            assert (np.abs(crow - tref_) <= tlim)[~alive].all(), "%s: terminated rows" % what
            # tracking, the reward sum, the terminal value: exact bits from the stage's own inputs
            trow, tcost = dref.tracking32(traj, crow, t["terms"], t["targets_np"], disc, np.zeros(M, np.int64), first)
            np.testing.assert_array_equal(_bits(_np(x["track_cost"])), _bits(tcost), err_msg=what + ": tracking cost")
            np.testing.assert_array_equal(_bits(_np(x["reward_rows"])), _bits(trow), err_msg=what + ": tracked rows")
            S = dref.step_sum(_np(x["reward_steps"]), disc, first)
            np.testing.assert_array_equal(_bits(_np(x["reward_sum"])), _bits(S), err_msg=what + ": reward step sum")
            rrow = rref.update(trow, S, 0.5)
            np.testing.assert_array_equal(_bits(_np(x["value_rows"])), _bits(rrow))
            vrow = dref.terminal_update(rrow, _np(x["value"]), 0.75, disc, first, H)
            np.testing.assert_array_equal(_bits(_np(x["rows"])), _bits(vrow), err_msg=what + ": rows behind the terminal value")
            # the candidate score: the particle mean, less the rate cost, less lambda times the uncertainty cost
            score = _np(eng.particle_mean(eng._t(vrow)))
            np.testing.assert_array_equal(_bits(_np(x["score"])), _bits(score))
            acost = dref.actuator_cost32(acts, t["w"], disc, prev)
            np.testing.assert_array_equal(_bits(_np(x["action_cost"])), _bits(acost), err_msg=what + ": actuator cost")
            ucost = dref.uncertainty_cost32(_np(x["unc_steps"]), disc, first)
            np.testing.assert_array_equal(_bits(_np(x["unc_cost"])), _bits(ucost), err_msg=what + ": uncertainty cost")
            cand = ((score - acost).astype(F) - (ucost * F(0.3)).astype(F)).astype(F)
            np.testing.assert_array_equal(_bits(_np(x["cand"])), _bits(cand), err_msg=what + ": cand of the last iteration")
            prev_next = a[:, 0].copy()
            mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)
    return a


@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_fused_equals_stepwise_halfcheetah(hc5, update, context):
    """`cadm_rewarded_plan` on a discounted engine == `planner.icem_plan` one launch at a time, bit for bit over two consecutive calls
    (plan, best return, carry, actuator state); the last iteration's `cand` is tests/discount_ref.py's composition of the stages."""
    prob, eng = hc5[context]
    check_fused_equals_stepwise(eng, prob, oenvs.make_env("halfcheetah"), "halfcheetah", (1, 7), update, 0.9,
                                "halfcheetah %s %s" % (update, "cadm" if context else "vanilla"))


def test_fused_equals_stepwise_declared_env(hop):
    spec, prob, eng = hop
    check_fused_equals_stepwise(eng, prob, spec, spec, (0, 3), "cem", 0.9, "hopper_like cem")


# ---------------------------------------------------------------------------------------------------------------------- 5: it reaches the plan
def test_a_discount_reaches_the_plan(hc5):
    prob, eng = hc5[True]
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    free = _np(eng.icem_plan(HipEngine.icem_params(), *args, seed=6, call=1))
    _, info1, _ = hplanner.icem_plan(eng, *args, seed=6, call=1, return_info=True)
    with discounted(eng, 0.5):
        half = _np(eng.icem_plan(HipEngine.icem_params(), *args, seed=6, call=1))
        plan, info, _ = hplanner.icem_plan(eng, *args, seed=6, call=1, return_info=True)
        np.testing.assert_array_equal(_bits(_np(plan)), _bits(half))
    assert np.isfinite(half).all() and np.abs(half - free).max() > 1e-3, "the plan ignores the discount"
    c0, c1 = _np(info[0]["cand"]), _np(info1[0]["cand"])                            # iteration 0: the same candidates, scored twice
    np.testing.assert_array_equal(_bits(_np(info[0]["actions"])), _bits(_np(info1[0]["actions"])))
    assert (c0 != c1).all()
    assert not np.array_equal(_bits(_np(info[-1]["cand"])), _bits(_np(info1[-1]["cand"])))
    again = _np(eng.icem_plan(HipEngine.icem_params(), *args, seed=6, call=1))
    np.testing.assert_array_equal(_bits(again), _bits(free), err_msg="set_discount(1.0) must restore the undiscounted bits")


MODEL = dict(hidden=(200,) * 4, n_candidates=64, n_particles=5)


@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_discount_one_is_no_discount(gpu, context):
    H, A = 5, 6
    plain, prob = plan_model(context, H, **MODEL)
    one, _ = plan_model(context, H, cem_discount=1.0, **MODEL)
    assert plain._opt is None and one._opt is None and one.engine.discount_weights() is None
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    cpa = (prob["cp_obs"], prob["cp_act"]) if context else ()
    for call in range(2):
        pa, pb = plain.get_action(prob["obs"], *cpa, mean, var), one.get_action(prob["obs"], *cpa, mean, var)
        np.testing.assert_array_equal(_bits(pa), _bits(pb))
        mean = np.concatenate([pa[:, 1:], np.zeros((M, 1, A))], axis=1)
    assert not one.engine._loop_ws


# ---------------------------------------------------------------------------------------------------------------------- 6: class route and state
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_class_route_and_state(gpu, context):
    H, A, p = 5, 6, 5
    model, prob = plan_model(context, H, cem_discount=0.9, **MODEL)
    eng, n = model.engine, MODEL["n_candidates"]
    assert model._opt is not None and model._opt.discount == float(F(0.9))
    np.testing.assert_array_equal(_bits(eng.discount_weights()), _bits(dref.weights(0.9, H)))
    cp_ = (prob["cp_obs"], prob["cp_act"]) if context else (None, None)
    cpa = cp_ if context else ()
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    got = model.get_action(prob["obs"], *cpa, mean, var)
    assert model._call == 1 and got.shape == (M, H, A) and np.isfinite(got).all() and 0 < np.abs(got).max() <= 1.0
    want = _np(eng.opt_in_plan(model._opt, prob["obs"], cp_[0], cp_[1], mean, var, n, seed=model.seed, call=1))
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert eng._loop_ws[(False, False)][1].numel() == eng.lib.cadm_constrained_workspace_bytes(eng._ctx, M, n, 0, 0)      # the trajectory view
    # plan_returns: the rollout of the forecast's iteration word, then the kernel; the call counter stays
    res = model.plan_returns(prob["obs"], got, *cpa)
    assert model._call == 1 and sorted(res) == ["returns", "step_rewards", "weights"]
    assert res["returns"].shape == (M, p) and res["step_rewards"].shape == (M, H, p) and res["weights"].shape == (H + 1,)
    ctxv = eng.context_forward(*cp_) if context else None
    acts = eng._t(got)[:, None].contiguous()
    rows, traj = eng.rollout_returns(prob["obs"], ctxv, acts, seed=model.seed, call=1, it=hplanner.FORECAST_IT, want_traj=True)
    out, steps = eng.discount_returns(traj, prob["obs"], acts, rows, want_steps=True)
    np.testing.assert_array_equal(_bits(res["returns"]), _bits(_np(out)[:, 0]))
    np.testing.assert_array_equal(_bits(res["step_rewards"]), _bits(_np(steps).transpose(1, 2, 0, 3)[:, 0]))
    np.testing.assert_array_equal(_bits(res["weights"]), _bits(dref.weights(0.9, H)))
    chain = (res["weights"][0] * res["step_rewards"][:, 0]).astype(F)
    for t in range(1, H):
        chain = (chain + (res["weights"][t] * res["step_rewards"][:, t]).astype(F)).astype(F)
    np.testing.assert_array_equal(_bits(res["returns"]), _bits(chain))
    wide = model.plan_returns(prob["obs"], np.stack([got, got], 1), *cpa)
    assert wide["returns"].shape == (M, 2, p) and wide["step_rewards"].shape == (M, 2, H, p)
    # the forecast stays undiscounted
    fc = model.forecast(prob["obs"], got, *cpa)
    assert np.abs(fc["returns"] - res["step_rewards"].sum(axis=1)).max() <= 1e-4 * np.abs(fc["returns"]).max()
    plain, _ = plan_model(context, H, **MODEL)
    with pytest.raises(ValueError, match="no cem_discount"):
        plain.plan_returns(prob["obs"], got, *cpa)
    # state: an undiscounted plan, then set_discount(0.9) and a plan == a fresh discounted engine's plan; set_discount(1.0) restores
    peng = plain.engine
    plain._push_stats()                                                            # (what a model's first get_action does)
    args = (prob["obs"], cp_[0], cp_[1], mean, var, n)
    before = _np(peng.icem_plan(HipEngine.icem_params(), *args, seed=model.seed, call=1))
    small = peng._loop_ws[(False, False)][1].numel()
    peng.set_discount(0.9)
    assert not peng._loop_ws
    after = _np(peng.icem_plan(HipEngine.icem_params(), *args, seed=model.seed, call=1))
    assert peng._loop_ws[(False, False)][1].numel() > small
    np.testing.assert_array_equal(_bits(after), _bits(got), err_msg="set_discount on a used engine against a fresh discounted engine")
    assert not np.array_equal(_bits(after), _bits(before))
    peng.set_discount(1.0)
    np.testing.assert_array_equal(_bits(_np(peng.icem_plan(HipEngine.icem_params(), *args, seed=model.seed, call=1))), _bits(before))
    assert peng._loop_ws[(False, False)][1].numel() == small


# ---------------------------------------------------------------------------------------------------------------------- 7: refusals
def test_refusals(hop, hc5):
    """CADM_ESTATE from the reference-path loops on a discounted engine, a discount on a discrete, a sharded and a spec-less ctx, the
    kwarg at construction: none of them launches anything -- the outputs keep their sentinel."""
    prob, eng = hc5[True]
    lib = eng.lib
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=eng.device)
    out = torch.full((M * N * 6,), 123.0, dtype=torch.float32, device=eng.device)
    P, O = ct.c_void_p(buf.data_ptr()), ct.c_void_p(out.data_ptr())

    def refused(rc, name, frag, code=-1):
        msg = lib.cadm_last_error().decode()
        assert rc == code, "%s: expected %d, got %d (%s)" % (name, code, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    with discounted(eng, 0.9):
        refused(lib.cadm_cem_plan(eng._ctx, P, P, P, P, P, M, N, 0, 1, P, O, None), "cadm_cem_plan", "discount", code=-4)
        refused(lib.cadm_rs_plan(eng._ctx, P, P, P, M, N, 0, 1, P, O, None, None), "cadm_rs_plan", "discount", code=-4)
        with pytest.raises(_lib.CadmError, match="discount over the horizon is set"):
            eng.cem_plan(prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    plan = eng.cem_plan(prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)      # cleared: it plans again
    assert np.isfinite(_np(plan)).all()
    refused(lib.cadm_discount_returns(eng._ctx, P, P, P, M, N, P, O, None, None), "cadm_discount_returns", "no discount is set", code=-4)
    refused(lib.cadm_discount_returns(eng._ctx, None, P, P, M, N, P, O, None, None), "cadm_discount_returns", "is null")
    refused(lib.cadm_set_discount(None, ct.c_float(0.9), None), "cadm_set_discount", "ctx is null")
    # a discrete ctx
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=1, H=4, seed=1)
    deng = make_engine(dprob, p=5)
    with pytest.raises(_lib.CadmError, match="continuous-action"):
        deng.set_discount(0.9)
    assert deng.discount_weights() is None
    deng.set_discount(1.0)
    deng.close()
    # a spec ctx before cadm_set_env_spec
    spec, sprob, seng = hop
    raw = ct.c_void_p()
    assert seng.lib.cadm_ctx_create(ct.byref(seng.cfg), ct.byref(raw)) == 0
    refused(lib.cadm_set_discount(raw, ct.c_float(0.9), None), "cadm_set_discount", "cadm_set_env_spec", code=-4)
    seng.lib.cadm_ctx_destroy(raw)
    # a candidate-sharded ctx (a host-supplied all-gather registered for two ranks; it is never called)
    shp = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=5, seed=3, trained_like=True)
    sheng = make_engine(shp, p=5, num_elites=KE, num_cem_iters=ITERS)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(sheng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    refused(lib.cadm_set_discount(sheng._ctx, ct.c_float(0.9), None), "cadm_set_discount", "sharded")
    assert lib.cadm_dist_destroy(sheng._ctx) == 0
    sheng.close()
    torch.cuda.synchronize()
    assert (_np(out) == 123.0).all() and (_np(buf) == 0).all()
    # at construction
    from cadm_amd.envs import make_env_spec
    for bad in (0.0, -1.0, 1.5, float("nan")):
        for context in (False, True):
            with pytest.raises(ValueError, match="cem_discount must be a number in"):
                plan_model(context, 5, cem_discount=bad, **MODEL)
    with pytest.raises(ValueError, match="need use_cem=True"):
        plan_model(True, 5, use_cem=False, cem_discount=0.9, **MODEL)
    with pytest.raises(ValueError, match="cem_discount needs continuous actions"):
        plan_model(True, 5, env=make_env_spec("cartpole"), cem_discount=0.9, **MODEL)
