"""GPU: the policy prior of the opt-in planner -- the kernel (`cadm_policy_eval`, csrc/policy.hip) against the numpy restatement
(tests/policy_ref.py), its independence of the batch, the proposal roll one step at a time (`cadm_policy_propose` with states_out: the
action against the restatement, the noise against Philox, the next states bit for bit against a one-step rollout of a second engine), a
non-finite start state, the fused loop (`cadm_guided_plan`) against the stepwise one, the no-op, a proposal that wins, the class route
and the refusals.

Geometries: policy_eval alone on pendulum (D = 3, A = 1), hopper_like (D = 11, A = 3), halfcheetah (D = 18, A = 6) and the widest
declarable env (D = 48, A = 24: no ctx can hold more than CADM_SPEC_MAX_A = 24 action dims, so the kernel's own bound of 64 -- one full
64-unit group -- cannot be reached through any entry point; 24 is six full tiles of four); everything that rolls out on the compiled-in
halfcheetah 200 x 4 kernel, vanilla and with context.

The kernel is held to the float64 restatement at the project's bar for fp32 kernels, `helpers.assert_close` at 1e-5, which for actions
inside [lb, ub] is tighter than 1e-5 of the action range ub - lb at every element."""
import ctypes as ct
import math

import numpy as np
import pytest
import torch

import policy_ref as pref
import value_ref as vref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import _np, assert_close, corner_spec, floored_rel, make_engine, plan_act, plan_model, zero_carry

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")
M, N, KE, ITERS = 2, 24, 8, 3
NETS = [()] + vref.ENVELOPE_NETS


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def engines(gpu):
    """name -> (problem, engine), built when first asked for.  Kernel level, never rolled out: "pend", "hopper", "wide".  Halfcheetah
    200 x 4 (the compiled-in rollout), m = 3 in the problem: "v-p5-hH" vanilla, "c-p20-hH" with context, "cd-p5-hH" with context and
    deterministic -- engines of one family share their weights, so "...-h1" is the one-step twin of every other horizon; "hc5" /
    "hc5-vanilla": tests/test_gpu_tracking.py's planner geometry (m = 2, p = 5, H = 5, 8 elites, 3 iterations)."""
    built, probs = {}, {}

    def get(name):
        if name not in built:
            if name in ("pend", "hopper", "wide"):
                from test_gpu_constraints import hopper_like
                env = {"pend": "pendulum", "hopper": hopper_like(), "wide": corner_spec("widest")}[name]
                prob = synth.make_problem(env=env, context=name != "pend", E=5, m=M, H=3, seed=52)
                built[name] = (prob, make_engine(prob, p=5))
            elif name.startswith("hc5"):
                prob = synth.make_problem(env="halfcheetah", context=name == "hc5", E=5, m=M, H=5, seed=3, trained_like=True)
                built[name] = (prob, make_engine(prob, p=5, num_elites=KE, num_cem_iters=ITERS))
            else:
                fam, p, H = name.split("-")
                if fam not in probs:
                    probs[fam] = synth.make_problem(env="halfcheetah", context=fam != "v", E=5, m=3, H=4, seed=11, trained_like=True)
                built[name] = (probs[fam], make_engine(probs[fam], p=int(p[1:]), H=int(H[1:]), deterministic=fam == "cd"))
        return built[name]
    yield get
    for n_, (_, eng) in built.items():
        assert n_ not in ("pend", "hopper", "wide") or not eng._rollout_ready, "a kernel-level engine was rolled out"
        eng.close()


def _set(eng, hidden, act="relu", squash="tanh", P=1, noise=0.0, layers=None, mean=None, std=None, seed=None):
    """register a policy on the engine: (policy_params, its layers)"""
    if layers is None:
        layers = pref.envelope_policy(eng.D, hidden, eng.A) if seed is None else pref.he_policy(eng.D, hidden, eng.A, seed, 0.5)
    prm = HipEngine.policy_params(hidden, act, squash, P, noise)
    eng.set_policy_net(prm, layers, obs_mean=mean, obs_std=std)
    return prm, layers


def _states(D, rows, seed):
    return np.random.default_rng(1000 + seed).standard_normal((rows, D)).astype(F)


# ---------------------------------------------------------------------------------------------------------------------- 1: the kernel
@pytest.mark.parametrize("squash", pref.SQUASH)
@pytest.mark.parametrize("act", pref.ACTS)
def test_kernel_against_restatement(engines, act, squash):
    """`cadm_policy_eval` against the float64 restatement for the linear policy (L = 0) and every net of value_ref.ENVELOPE_NETS widened
    to A outputs, at A = 1, 3, 6 and 24 (A4 padding at 1, 3 and 6; six full tiles at 24), on 37 rows: two full 16-row tiles and a tail
    of 5.  The nets meet the liveness condition tests/test_policy_ref.py holds them to on the same inputs, so a dead layer or a
    saturated tanh does not check nothing."""
    worst = 0.0
    for name in ("pend", "hopper", "hc5", "wide"):
        _, eng = engines(name)
        x = _states(eng.D, 37, 0)
        for hidden in NETS:
            _, layers = _set(eng, hidden, act, squash)
            share, spread, open_ = pref.liveness(x, layers, act)
            assert share >= 0.5 and spread > 1e-3 and open_ >= 0.5, "%s %r %s" % (name, hidden, act)
            ref = pref.action64(x, layers, act, squash, -1.0, 1.0)
            got = _np(eng.policy_eval(x))
            assert got.shape == (37, eng.A) and np.isfinite(got).all() and np.abs(got).max() <= 1.0
            what = "%s A=%d %r %s %s" % (name, eng.A, hidden, act, squash)
            assert np.abs(got.astype(np.float64) - ref).max() <= 1e-5 * 2.0, what      # 1e-5 of the action range
            assert_close(got, ref, what=what)
            worst = max(worst, floored_rel(got, ref) / 1e-5)
    print("\n[%s %s] worst |err| / (1e-5 of scale): %.3f" % (act, squash, worst))


def test_kernel_with_statistics_bounds_and_the_widest_net(engines):
    """obs_mean / obs_std that are not 0 / 1; action bounds that are not -1 / 1 (mid and half from the float32 bounds, the clip); and
    512 x 4, whose activation regions need the kernel's dynamic-LDS attribute raised."""
    prob, eng = engines("hc5")
    rng = np.random.default_rng(8)
    x = _states(eng.D, 37, 3)
    mean, std = rng.standard_normal(eng.D).astype(F), rng.uniform(0.3, 4.0, eng.D).astype(F)
    _, layers = _set(eng, (50, 30, 70, 18), "swish", "tanh", mean=mean, std=std)
    ref = pref.action64(x, layers, "swish", "tanh", -1.0, 1.0, mean, std)
    assert_close(_np(eng.policy_eval(x)), ref, what="with statistics")
    assert np.abs(ref - pref.action64(x, layers, "swish", "tanh", -1.0, 1.0)).max() > 1e-3, "the statistics must matter"
    _, layers = _set(eng, (512,) * 4, "relu", "tanh", seed=4)
    assert_close(_np(eng.policy_eval(x)), pref.action64(x, layers, "relu", "tanh", -1.0, 1.0), what="512 x 4")
    other = make_engine(prob, p=5, lower_bound=-0.5, upper_bound=2.0)
    for squash in pref.SQUASH:
        _, layers = _set(other, (37,) * 4, "tanh", squash, layers=pref.he_policy(other.D, (37,) * 4, other.A, 5, 2.0))
        got = _np(other.policy_eval(x))
        assert got.min() >= F(-0.5) and got.max() <= F(2.0)
        assert np.abs(got - pref.action64(x, layers, "tanh", squash, -0.5, 2.0)).max() <= 1e-5 * 2.5
        assert squash == "tanh" or ((got == F(2.0)).any() and (got == F(-0.5)).any())
    other.close()


# ---------------------------------------------------------------------------------------------------------------------- 2: batch independence
@pytest.mark.parametrize("hidden,act", [((64, 48, 200), "swish"), ((200, 200), "relu"), ((), "relu")], ids=["unequal-swish", "200x2-relu", "linear"])
def test_a_state_has_the_same_bits_in_any_batch(engines, hidden, act):
    """The same states through `policy_eval` at R = 1, 16, 17, 33, at other row positions, inside a batch large enough for two row
    tiles per workgroup, run to run -- and as the obs of `policy_propose`'s step 0 (the start state is the estimate itself; the
    one-particle engine of the next test covers the later steps): equal bits."""
    prob, eng = engines("v-p5-h1")
    _set(eng, hidden, act, "tanh", seed=21)
    x = _states(eng.D, 165, 7)
    full = _np(eng.policy_eval(x))
    assert full.shape == (165, eng.A)
    np.testing.assert_array_equal(_bits(_np(eng.policy_eval(x))), _bits(full), err_msg="run to run")
    for R in (1, 16, 17, 33):
        np.testing.assert_array_equal(_bits(_np(eng.policy_eval(x[:R]))), _bits(full[:R]), err_msg="R = %d" % R)
    np.testing.assert_array_equal(_bits(_np(eng.policy_eval(np.roll(x, 7, axis=0)))), _bits(np.roll(full, 7, axis=0)), err_msg="rows moved by 7")
    reps = 2 * 16 * 256 // 165 + 8
    big = _np(eng.policy_eval(np.concatenate([x[3:]] + [x] * reps, axis=0)))
    assert big.shape[0] > 2 * 16 * 256
    np.testing.assert_array_equal(_bits(big[:162]), _bits(full[3:]), err_msg="the two-row-tile launch, head")
    np.testing.assert_array_equal(_bits(big[-165:]), _bits(full), err_msg="the two-row-tile launch, tail")
    lead = eng.policy_eval(x.reshape(3, 55, eng.D))
    assert tuple(lead.shape) == (3, 55, eng.A)
    np.testing.assert_array_equal(_bits(_np(lead)).reshape(-1, eng.A), _bits(full))
    # the roll's own step: H = 1, every env's sequences act on obs[mi]
    for P in (1, 6, 17):
        prm = HipEngine.policy_params(hidden, act, "tanh", P, 0.0)
        seqs, states = eng.policy_propose(prm, x[:33], None, seed=1, call=2, want_states=True)
        assert tuple(seqs.shape) == (33, P, 1, eng.A) and tuple(states.shape) == (1, 33, P, eng.p, eng.D)
        np.testing.assert_array_equal(_bits(_np(seqs)[:, :, 0]), _bits(np.repeat(full[:33, None], P, axis=1)), err_msg="propose, P = %d" % P)
        np.testing.assert_array_equal(_bits(_np(states)[0]), _bits(np.broadcast_to(x[:33, None, None, :], (33, P, eng.p, eng.D))))


def test_propose_step_at_one_particle_is_policy_eval(gpu):
    """p = 1: the state estimate is the particle itself (no sum, no division), so every step of the roll has `policy_eval`'s bits on
    the states it read."""
    prob = synth.make_problem(env="halfcheetah", context=False, E=1, m=3, H=3, seed=5, trained_like=True)
    eng = make_engine(prob, p=1, deterministic=True)
    prm, _ = _set(eng, (65,), "tanh", "tanh", P=6, noise=0.0, seed=2)
    seqs, states = eng.policy_propose(prm, prob["obs"], None, seed=3, call=1, want_states=True)
    seqs, states = _np(seqs), _np(states)
    assert np.isfinite(states).all() and not np.array_equal(states[1], states[0]) and not np.array_equal(states[2], states[1])
    for t in range(3):
        np.testing.assert_array_equal(_bits(seqs[:, :, t]), _bits(_np(eng.policy_eval(states[t][:, :, 0]))), err_msg="step %d" % t)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------- 3: the roll, one step at a time
def check_roll(eng, twin, prob, prm, layers, act, squash, m, seed, call, noise, lb, ub):
    """The body of `test_one_step_at_a_time` on the first m envs of `prob`: `eng` has the net `layers` registered as `prm` describes it
    (P = prm.n_samples) and the action bounds lb, ub; `twin` is an engine with n_forwards = 1, the same weights and the same bounds.
    -> (seqs, states, worst action error / (1e-5 of the range), worst noise error / bound)."""
    H, P, rng_ = eng.H, int(prm.n_samples), float(ub) - float(lb)
    context = eng.C > 0
    obs = np.asarray(prob["obs"], F)[:m]
    ctx_vec = eng.context_forward(prob["cp_obs"][:m], prob["cp_act"][:m]) if context else None
    seqs, states = eng.policy_propose(prm, obs, ctx_vec, seed=seed, call=call, want_states=True)
    again = eng.policy_propose(prm, obs, ctx_vec, seed=seed, call=call)
    np.testing.assert_array_equal(_bits(_np(again)), _bits(_np(seqs)), err_msg="run to run, with and without states_out")
    seqs, states = _np(seqs), _np(states)
    assert seqs.shape == (m, P, H, eng.A) and states.shape == (H, m, P, eng.p, eng.D) and np.isfinite(seqs).all() and np.isfinite(states).all()
    np.testing.assert_array_equal(_bits(states[0]), _bits(np.broadcast_to(obs[:, None, None, :], states[0].shape)), err_msg="step 0 reads obs[mi]")
    worst_a = worst_z = 0.0
    for t in range(H):
        est = pref.particle_mean32(states[t])
        z = pref.xi(seed, call, m, P, t, eng.A)
        z[:, 0] = 0.0
        want, raw = pref.emulate32(est, layers, act, squash, lb, ub, xi=z, noise_std=noise, want_raw=True)
        a = seqs[:, :, t]
        err = np.abs(a.astype(np.float64) - want.astype(np.float64)).max()
        assert err <= 1e-5 * rng_, "step %d: the action is off by %.3e" % (t, err)
        worst_a = max(worst_a, err / (1e-5 * rng_))
        # sequence 0 is the policy's own action: no noise (the raw action lies inside the bounds under the tanh squash; without it, clipped)
        assert np.abs(a[:, 0].astype(np.float64) - np.clip(raw[:, 0], F(lb), F(ub))).max() <= 1e-5 * rng_
        if P > 1:
            free = (a[:, 1:] > F(lb)) & (a[:, 1:] < F(ub))
            rec = (a[:, 1:].astype(np.float64) - raw[:, 1:].astype(np.float64)) / float(F(noise))
            bound = 1e-5 * rng_ / noise + 4e-6 * np.maximum(1.0, pref.xi_radius(seed, call, m, P, t, eng.A)[:, 1:] / 2.0)
            dz = np.abs(rec - z[:, 1:])
            assert free.mean() > 0.5 and (dz[free] <= bound[free]).all(), "step %d: the noise is off by %.3e" % (t, (dz[free] / bound[free]).max())
            worst_z = max(worst_z, float((dz[free] / bound[free]).max()))
        if t + 1 < H:
            tv = twin.context_forward(prob["cp_obs"][:m], prob["cp_act"][:m]) if context else None
            _, nxt = twin.rollout_returns(obs, tv, np.ascontiguousarray(a[:, :, None, :]), obs_rows=states[t].reshape(-1, eng.D), seed=seed,
                                          call=call, it=hplanner.POLICY_IT + 2 * t, want_traj=True)
            nxt = _np(nxt)
            assert nxt.shape == (1, m, P, eng.p, eng.D)
            np.testing.assert_array_equal(_bits(states[t + 1]), _bits(nxt[0]), err_msg="the states step %d read against the one-step rollout" % (t + 1))
            assert not np.array_equal(states[t + 1], states[t])
            if not eng.deterministic and eng.p > eng.E:      # two particles of one member differ by their head noise
                assert not np.array_equal(states[t + 1][:, :, 0], states[t + 1][:, :, eng.E])
    # the rows of env 0 do not depend on m, nor a sequence's on P: the same bits wherever the row sits (row ids, hence the noise, agree)
    if m > 1:
        alone = _np(eng.policy_propose(prm, obs[:1], None if ctx_vec is None else eng.context_forward(prob["cp_obs"][:1], prob["cp_act"][:1]),
                                       seed=seed, call=call))
        np.testing.assert_array_equal(_bits(alone[0, :, 0]), _bits(seqs[0, :, 0]), err_msg="env 0 alone, step 0")
    return seqs, states, worst_a, worst_z


ROLLS = [("v-p5", 2, 1, 1), ("v-p5", 2, 1, 17), ("c-p20", 3, 3, 6), ("cd-p5", 2, 3, 6), ("v-p5", 1, 3, 6), ("c-p20", 2, 1, 17)]


@pytest.mark.parametrize("fam,H,m,P", ROLLS, ids=["%s-H%d-m%d-P%d" % r for r in ROLLS])
def test_one_step_at_a_time(engines, fam, H, m, P):
    """`policy_propose` with states_out, every step checked on its own so that nothing compounds: the action against the float32
    emulation of the particle mean of the states the step read (with the restated Philox noise), at 1e-5 of the action range; the noise
    recovered from the unclipped dims against the Philox restatement; and the states the NEXT step read, bit for bit, against a second
    engine with n_forwards = 1 and the same weights: the public `cadm_rollout_returns` from obs_rows = this step's states under the
    GPU's own action and the iteration word CADM_POLICY_IT + 2 t.  P = 17 crosses a row tile at m = 1; at m = 3, P = 6 the envs share a
    tile and step 0 must read the right obs; p = E and p = 4 E; H = 1 has no rollout; a deterministic ctx rolls the mean head.
    The recovered noise carries the action's error divided by noise_std: the bound is (1e-5 of the range) / noise_std plus the
    project's bar for a device Box-Muller draw against the oracle's (4e-6 at |z| < 2, tests/test_gpu_planner.py), scaled with the
    draw's radius sqrt(-2 ln u1) beyond 2: the error of the unit-circle factor is multiplied by it."""
    prob, eng = engines("%s-h%d" % (fam, H))
    _, twin = engines("%s-h1" % fam)
    noise, seed, call = 0.3, 5, 9
    prm, layers = _set(eng, (50, 30, 70, 18), "swish", "tanh", P=P, noise=noise)
    _, _, worst_a, worst_z = check_roll(eng, twin, prob, prm, layers, "swish", "tanh", m, seed, call, noise, -1.0, 1.0)
    print("\n[%s H=%d m=%d P=%d] worst action err / (1e-5 of range) %.3f, worst noise err / bound %.3f" % (fam, H, m, P, worst_a, worst_z))


def test_noise_against_philox(engines):
    """A policy with zero weights has the action b exactly (the accumulator is seeded with the bias and fma(0, x, b) == b), so with
    squash "none" the noise is recovered from a = float32(b + float32(noise_std * xi)) up to two roundings: the device's Box-Muller
    draws against oracle/philox.py's at the project's bar for them (4e-6 at |z| < 2, tests/test_gpu_planner.py), scaled with the draw's
    radius beyond 2.  Every sequence j >= 1, step and dim has its own draw; sequence 0 is b itself, bit for bit; noise_std = 0 draws nothing."""
    prob, eng = engines("v-p5-h2")
    A, D, m, P, noise = eng.A, eng.D, 3, 17, 0.25
    b = np.linspace(-0.3, 0.3, A).astype(F)
    layers = [(np.zeros((D, A), F), b)]
    prm, _ = _set(eng, (), "relu", "none", P=P, noise=noise, layers=layers)
    seqs = _np(eng.policy_propose(prm, np.asarray(prob["obs"], F)[:m], None, seed=77, call=4))
    np.testing.assert_array_equal(_bits(seqs[:, 0]), _bits(np.broadcast_to(b, (m, eng.H, A))), err_msg="sequence 0")
    for t in range(eng.H):
        z = pref.xi(77, 4, m, P, t, A)[:, 1:]
        a = seqs[:, 1:, t]
        free = np.abs(a) < 1.0                                   # (a draw beyond (1 - |b|) / noise_std is clipped: about one in 200)
        assert free.mean() > 0.98 and (np.abs(b + F(noise) * z)[~free] >= 1.0 - 1e-5).all()
        rec = (a.astype(np.float64) - b.astype(np.float64)) / float(F(noise))
        bound = 4e-6 * np.maximum(1.0, pref.xi_radius(77, 4, m, P, t, A)[:, 1:] / 2.0) + 2.0 ** -23 / noise
        assert (np.abs(rec - z)[free] <= bound[free]).all(), "step %d: worst %.3e" % (t, np.abs(rec - z)[free].max())
    assert len(np.unique(seqs[:, 1:])) == seqs[:, 1:].size
    quiet = HipEngine.policy_params((), "relu", "none", P, 0.0)
    np.testing.assert_array_equal(_bits(_np(eng.policy_propose(quiet, np.asarray(prob["obs"], F)[:m], None, seed=77, call=4))),
                                  _bits(np.broadcast_to(b, (m, P, eng.H, A))))


# ---------------------------------------------------------------------------------------------------------------------- 4: a non-finite start state
@pytest.mark.parametrize("poison", [NAN, math.inf])
def test_non_finite_start_state_of_one_env(engines, poison):
    """One env's obs holds a non-finite value: its sequences are the fallback clip(0, lb, ub) at every step (its particles never become
    finite again), finite, and the other envs' sequences and states -- rows of the same 16-row tile -- are bit for bit what they are
    without it."""
    prob, eng = engines("c-p20-h3")
    prm, _ = _set(eng, (5, 7), "relu", "tanh", P=6, noise=0.3)
    obs = np.asarray(prob["obs"], F)
    ctx_vec = eng.context_forward(prob["cp_obs"], prob["cp_act"])
    clean, cs = (_np(x) for x in eng.policy_propose(prm, obs, ctx_vec, seed=2, call=3, want_states=True))
    bad = obs.copy()
    bad[1, 7] = poison
    seqs, st = (_np(x) for x in eng.policy_propose(prm, bad, ctx_vec, seed=2, call=3, want_states=True))
    assert np.isfinite(seqs).all() and (seqs[1] == pref.fallback(-1.0, 1.0)).all()
    assert not np.isfinite(st[1:, 1]).all()
    for e in (0, 2):
        np.testing.assert_array_equal(_bits(seqs[e]), _bits(clean[e]), err_msg="env %d met its neighbour's poison" % e)
        np.testing.assert_array_equal(_bits(st[:, e]), _bits(cs[:, e]))
    assert (clean[1] != 0).any()
    flat = _np(eng.policy_eval(bad))
    assert (flat[1] == 0).all()
    np.testing.assert_array_equal(_bits(flat[[0, 2]]), _bits(_np(eng.policy_eval(obs))[[0, 2]]))


# ---------------------------------------------------------------------------------------------------------------------- 5: fused against stepwise
COMBOS = ["alone", "mppi-knots-actuator", "value-reward-best"]


@pytest.mark.parametrize("combo", COMBOS)
def test_fused_equals_stepwise(engines, combo):
    """`cadm_guided_plan` with device RNG == the same loop one launch at a time (`planner.icem_plan(..., policy=...)`: one
    `policy_propose`, then every iteration `icem_inject` at the slot rule), bit for bit over two consecutive calls: the plan, the best
    return, the carry (and the actuator state).  alone: CEM, keep_elites 0, vanilla; mppi-knots-actuator: MPPI, keep_elites 2,
    add_mean_last, decay 1.25, coloured noise, knots and an actuator; value-reward-best: CEM, keep_elites 2, add_mean_last, decay 1.25,
    a value and a reward net, the best sequence.  Without knots and an actuator the stepwise iterations' candidates hold the proposals
    at their slots; without the prior the plan is another."""
    from test_gpu_actuator import _params, _state
    from test_gpu_reward import _set as set_reward
    from test_gpu_value import _set as set_value
    prob, eng = engines("hc5-vanilla" if combo == "alone" else "hc5")
    H, A, P = eng.H, eng.A, 6
    pol, _ = _set(eng, (50, 30), "tanh", "tanh", P=P, noise=0.3, seed=40)
    mppi = combo == "mppi-knots-actuator"
    K = 0 if combo == "alone" else 2
    icem = dict(noise_beta=1.0 if mppi else 0.0, keep_elites=K, decay=1.25 if K else 1.0, return_best=combo == "value-reward-best",
                add_mean_last=K > 0)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if mppi else HipEngine.icem_params(**icem)
    knots = act = value = reward = None
    (pa, fa), (pb, fb) = (None, None), (None, None)
    if mppi:
        knots, act = HipEngine.knot_params(2, "linear"), _params(eng, 1, 0.4, 2.0)
        (pa, fa), (pb, fb) = _state(eng, 1, 8), _state(eng, 1, 8)
    if combo == "value-reward-best":
        value, _ = set_value(eng, (64, 48), "tanh", seed=31, weight=3.0)
        reward, _ = set_reward(eng, "obs_act_next_obs", (32,), "relu", seed=32, weight=0.5)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    (ca, va), (cb, vb) = zero_carry(eng, M, K, H), zero_carry(eng, M, K, H)
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2):
        a, ra = eng.guided_plan(pol, reward, value, None, act, pa, fa, True, None, None, None, knots, None, None, None, prm, *args, mean, var, N,
                                carry=ca, carry_valid=va, seed=4, call=call, want_best_return=True)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                            update="mppi" if mppi else "cem", temperature=0.5, relative=True, knots=knots,
                                            actuator=None if act is None else (act, pb, fb), action_advance=True, value=value, reward=reward,
                                            policy=pol, **icem)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        for x, y in ((ca, cb), (pa, pb), (fa, fb)):
            if x is not None:
                np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))
        props = _np(extra["proposals"])
        ctx_vec = eng.context_forward(prob["cp_obs"], prob["cp_act"]) if eng.C > 0 else None
        np.testing.assert_array_equal(_bits(props), _bits(_np(eng.policy_propose(pol, prob["obs"], ctx_vec, seed=4, call=call))))
        if not mppi:
            for it, x in enumerate(info):
                s = hplanner.policy_slot(K, it + 1 == ITERS, icem["add_mean_last"])
                assert s + P <= x["actions"].shape[1]
                np.testing.assert_array_equal(_bits(_np(x["actions"])[:, s:s + P]), _bits(props), err_msg="iteration %d" % it)
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)
    other = _np(eng.guided_plan(None, reward, value, None, act, pb, fb, False, None, None, None, knots, None, None, None, prm, *args, mean, var, N,
                                *zero_carry(eng, M, K, H), seed=4, call=2))
    assert not np.array_equal(_bits(other), _bits(a))
    assert (mppi, "pol", False, act is not None, False, P) in eng._loop_ws


# ---------------------------------------------------------------------------------------------------------------------- 6: the no-op
@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_no_policy_is_the_loop_underneath(engines, update):
    """policy = NULL: the plan, the best return and the carry of `cadm_rewarded_plan` on the same inputs, bit for bit, through the C
    entry itself with that loop's workspace."""
    prob, eng = engines("hc5")
    H, A = eng.H, eng.A
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    mppi, full = eng._as_mppi_params(prm)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    carry, valid = zero_carry(eng, M, 2, H)
    plan, best = eng.rewarded_plan(None, None, None, None, None, None, True, None, None, None, None, None, None, None, prm, *args, carry=carry,
                                   carry_valid=valid, seed=5, call=2, want_best_return=True)
    carry2, valid2 = zero_carry(eng, M, 2, H)
    t = [eng._t(x) for x in args[:5]]
    ws = eng._loop_workspace(mppi, M, N, 2)
    out = torch.empty((M, H, A), dtype=torch.float32, device=eng.device)
    best2 = torch.empty((M,), dtype=torch.float32, device=eng.device)
    P_ = lambda x: ct.c_void_p(x.data_ptr())
    rc = eng.lib.cadm_guided_plan(eng._ctx, None, None, None, None, None, None, None, 1, None, None, 0, None, None, None, None, None, int(mppi),
                                  ct.byref(full), *[P_(x) for x in t], P_(carry2), P_(valid2), M, N, 5, 2, P_(ws), P_(out), P_(best2), eng.stream)
    assert rc == 0, eng.lib.cadm_last_error().decode()
    for x, y in ((plan, out), (best, best2), (carry, carry2)):
        np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))


# ---------------------------------------------------------------------------------------------------------------------- 7: a proposal can win
def test_a_proposal_can_win(gpu):
    """A policy with zero weights and the bias a* (squash "none": pi == a* exactly), no noise, on a model that returns the best sequence
    and prices action rates against the applied action a*: the constant sequence a* costs exactly 0, every drawn candidate pays the rate
    weight times its squared moves, and the rate weight is 1000 times the range of the synthetic model's returns (asserted below, over
    random plans and the constant one) -- so the proposal is the best sequence of the call and the plan is a* bit for bit.  The same
    model without the prior returns a plan that moves."""
    H, A, D = 5, 6, 18
    astar = np.linspace(-0.5, 0.5, A).astype(F)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    base = dict(hidden=(200,) * 4, cem_return="best")
    probe_model, prob = plan_model(False, H, **base)
    probe = np.random.default_rng(1).uniform(-1, 1, (M, 32, H, A)).astype(F)
    probe[:, 0] = astar
    ret = probe_model.forecast(prob["obs"], probe, seed=11)["rollout_returns"].astype(np.float64).mean(axis=2)
    span = float(ret.max() - ret.min())
    assert np.isfinite(ret).all() and 0.0 < span < 1e4, "the synthetic model's returns span %.3g" % span
    w = 1000.0 * span
    plans = {}
    for name, prior in (("prior", dict(hidden_sizes=(), squash="none", n_samples=4, noise_std=0.0)), ("plain", None)):
        model, _ = plan_model(False, H, cem_action_rate_cost=w, cem_policy_prior=prior, **base)
        model.set_applied_actions(prev=np.tile(astar, (M, 1)))
        if prior is not None:
            model.set_policy([(np.zeros((D, A), F), astar)])
            np.testing.assert_array_equal(_bits(model.policy_proposals(prob["obs"])), _bits(np.broadcast_to(astar, (M, 4, H, A))))
        plans[name] = plan_act(model, prob, False, mean, var)
    np.testing.assert_array_equal(_bits(plans["prior"]), _bits(np.broadcast_to(astar, (M, H, A))))
    moves = np.abs(np.diff(plans["plain"], axis=1)).max()
    assert np.isfinite(plans["plain"]).all() and moves > 0.0, "without the prior the plan must move"
    # the drawn candidates' cheapest rate cost still outweighs the return range: what the plain plan pays, against the range
    paid = w * float((np.diff(np.concatenate([np.tile(astar, (M, 1, 1)), plans["plain"]], axis=1), axis=1) ** 2).sum(axis=(1, 2)).min())
    print("\n[a proposal can win] return span %.3g, rate weight %.3g, the plain plan pays %.3g" % (span, w, paid))
    assert paid > span


# ---------------------------------------------------------------------------------------------------------------------- 8: the class route
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_class_route(gpu, context):
    """`get_action` with a Sequential-set net agrees with the engine call and with a twin whose net was set as a list; `policy_action`
    with the restatement; `policy_proposals` shapes and bits; no net raises RuntimeError; a replaced net takes effect on the next call;
    `clear_policy` brings the RuntimeError back."""
    H, A, D = 5, 6, 18
    hidden, act = (64, 32), "swish"
    pp = dict(hidden_sizes=hidden, activation=act, n_samples=5, noise_std=0.2)
    model, prob = plan_model(context, H, hidden=(200,) * 4, cem_policy_prior=pp, cem_keep_elites=2)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    with pytest.raises(RuntimeError, match="no policy net"):
        plan_act(model, prob, context, mean, var)
    with pytest.raises(RuntimeError, match="no policy net"):
        model.policy_action(np.zeros((3, D), F))
    assert model._call == 0
    rng = np.random.default_rng(5)
    stats = (rng.standard_normal(D).astype(F), rng.uniform(0.5, 2.0, D).astype(F))
    layers = pref.he_policy(D, hidden, A, 17, 0.5)
    model.set_policy(vref.sequential(layers, act), *stats)
    plan = plan_act(model, prob, context, mean, var)
    assert np.isfinite(plan).all() and model._call == 1
    eng, opt = model.engine, model._opt
    hist = (prob["cp_obs"], prob["cp_act"]) if context else (None, None)
    carry, valid = zero_carry(eng, M, 2, H)
    direct = eng.guided_plan(opt.policy_params, None, None, None, None, None, None, True, None, None, None, None, None, None, None, opt.params,
                             prob["obs"], *hist, mean, var, model.n_candidates, carry=carry, carry_valid=valid, seed=model.seed, call=1)
    np.testing.assert_array_equal(_bits(plan), _bits(_np(direct)))
    twin, _ = plan_model(context, H, hidden=(200,) * 4, cem_policy_prior=pp, cem_keep_elites=2)
    twin.set_policy(layers, *stats)                      # the list form of the same net
    np.testing.assert_array_equal(_bits(plan_act(twin, prob, context, mean, var)), _bits(plan))
    # the policy through the class, against the restatement; the proposals
    states = (2.0 * rng.standard_normal((4, 7, D))).astype(F)
    a = model.policy_action(states)
    assert a.shape == (4, 7, A)
    assert_close(a, pref.action64(states, layers, act, "tanh", -1.0, 1.0, *stats), what="policy_action")
    hp = hist if context else ()
    props = model.policy_proposals(prob["obs"], *hp)
    assert props.shape == (M, 5, H, A) and np.isfinite(props).all() and model._call == 1
    props2, st = model.policy_proposals(prob["obs"], *hp, return_states=True)
    assert st.shape == (H, M, 5, model.n_particles, D)
    np.testing.assert_array_equal(_bits(props2), _bits(props))
    np.testing.assert_array_equal(_bits(props[:, 0, 0]), _bits(model.policy_action(np.asarray(prob["obs"], F))))
    ctx_vec = eng.context_forward(*hist) if context else None
    np.testing.assert_array_equal(_bits(props), _bits(_np(eng.policy_propose(opt.policy_params, prob["obs"], ctx_vec, seed=model.seed, call=1))))
    # a replaced net: the next call plans with it
    ws = dict(eng._loop_ws)
    other = pref.he_policy(D, hidden, A, 18, 2.0)
    model.set_policy(other, *stats)
    assert_close(model.policy_action(states), pref.action64(states, other, act, "tanh", -1.0, 1.0, *stats), what="the replaced net")
    plan2 = plan_act(model, prob, context, mean, var)
    direct2 = eng.guided_plan(opt.policy_params, None, None, None, None, None, None, True, None, None, None, None, None, None, None, opt.params,
                              prob["obs"], *hist, mean, var, model.n_candidates, carry=carry, carry_valid=valid, seed=model.seed, call=2)
    np.testing.assert_array_equal(_bits(plan2), _bits(_np(direct2)))
    assert not np.array_equal(_bits(plan2), _bits(plan))
    assert all(eng._loop_ws[k][1] is ws[k][1] for k in ws)
    model.clear_policy()
    with pytest.raises(RuntimeError, match="no policy net"):
        plan_act(model, prob, context, mean, var)
    plain, _ = plan_model(context, H, hidden=(200,) * 4, cem_noise_beta=1.0)
    for fn in (lambda: plain.set_policy(layers), lambda: plain.policy_action(states), lambda: plain.clear_policy(),
               lambda: plain.policy_proposals(prob["obs"], *hp)):
        with pytest.raises(ValueError, match="no cem_policy_prior"):
            fn()


def test_refusals_at_construction(gpu, monkeypatch):
    """`cem_policy_prior` is refused where the other `cem_*` options are: use_cem=False, a discrete env, a process group of more than
    one rank; proposals that do not fit the smallest iteration; a Sequential of other sizes or another activation than the declared one
    is refused when it is set."""
    from cadm_amd.envs import make_env_spec
    pp = dict(hidden_sizes=(16,), activation="tanh", n_samples=4)
    big = dict(hidden=(200,) * 4)
    with pytest.raises(ValueError, match="need use_cem=True"):
        plan_model(True, 5, use_cem=False, cem_policy_prior=pp, **big)
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        plan_model(True, 5, env=make_env_spec("cartpole"), cem_policy_prior=pp, **big)
    with pytest.raises(ValueError, match="hidden widths"):
        plan_model(True, 5, cem_policy_prior=dict(hidden_sizes=(0,)), **big)
    with pytest.raises(ValueError, match="candidate slots"):
        plan_model(False, 5, n_candidates=64, cem_policy_prior=dict(pp, n_samples=64), **big)
    model, _ = plan_model(False, 5, cem_policy_prior=pp, **big)
    with pytest.raises(ValueError, match="activation"):
        model.set_policy(vref.sequential(pref.he_policy(18, (16,), 6, 0), "relu"))
    with pytest.raises(ValueError, match="layer 0 is"):
        model.set_policy(vref.sequential(pref.he_policy(18, (24,), 6, 0), "tanh"))
    with pytest.raises(ValueError, match="layer 1 is"):
        model.set_policy(pref.he_policy(18, (16,), 5, 0))
    with pytest.raises(ValueError, match="obs_std"):
        model.set_policy(pref.he_policy(18, (16,), 6, 0), obs_std=np.zeros(18))
    assert not model._policy_set
    import torch.distributed as dist
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        plan_model(True, 5, process_group=object(), cem_policy_prior=pp, **big)


# ---------------------------------------------------------------------------------------------------------------------- 9: refusals, workspaces
def test_argument_checks_return_einval(engines):
    """The C entries refuse bad arguments with CADM_EINVAL (no net: CADM_ESTATE) and a message that names them and the argument, before
    any HIP call (the dummy pointers next to the bad argument are never touched); the engine plans normally afterwards."""
    prob, eng = engines("hc5")
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(8192, dtype=torch.float32, device=eng.device)
    P = ct.c_void_p(buf.data_ptr())
    mp = HipEngine.mppi_params()
    _set(eng, (32, 16), "relu", "tanh", seed=1)
    two = (ct.c_void_p * 5)(*([buf.data_ptr()] * 5))

    def V(n_hidden=2, hidden=(32, 16), activation=0, squash=1, n_samples=4, noise_std=0.0):
        v = _lib.PolicyParams()
        v.n_hidden, v.activation, v.squash, v.n_samples, v.noise_std = n_hidden, activation, squash, n_samples, noise_std
        for l, h in enumerate(hidden):
            v.hidden[l] = h
        return ct.byref(v)

    def setnet(v, c=ctx, W=two, b=two, mean=P, inv=P):
        return lib.cadm_set_policy_net(c, v, W, b, mean, inv, None)

    def propose(v, c=ctx):
        return lib.cadm_policy_propose(c, v, P, P, M, 0, 1, P, None, P, None)

    def plan(v, c=ctx, update=0, prm=ct.byref(mp), n=N):
        return lib.cadm_guided_plan(c, v, None, None, None, None, None, None, 1, None, None, 0, None, None, None, None, None, update, prm, P, P, P,
                                    P, P, None, None, M, n, 0, 1, P, P, None, None)

    def refused(rc, name, frag, code=-1):
        msg = lib.cadm_last_error().decode()
        assert rc == code, "%s: expected %d, got %d (%s)" % (name, code, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    for name, fn in (("cadm_set_policy_net", setnet), ("cadm_policy_propose", propose), ("cadm_guided_plan", plan)):
        refused(fn(V(n_hidden=5)), name, "hidden layers")
        refused(fn(V(n_hidden=-1)), name, "hidden layers")
        refused(fn(V(hidden=(32, 0))), name, "width")
        refused(fn(V(hidden=(513, 16))), name, "width")
        refused(fn(V(activation=3)), name, "activation")
        refused(fn(V(activation=-1)), name, "activation")
        refused(fn(V(squash=2)), name, "squash")
        refused(fn(V(squash=-1)), name, "squash")
        refused(fn(V(n_samples=0)), name, "n_samples")
        for bad in (NAN, math.inf, -0.5):
            refused(fn(V(noise_std=bad)), name, "noise_std")
    for name, fn in (("cadm_policy_propose", propose), ("cadm_guided_plan", plan)):
        refused(fn(V(hidden=(32, 17))), name, "registered net")
        refused(fn(V(n_hidden=1)), name, "registered net")
        refused(fn(V(activation=1)), name, "registered net")
        refused(fn(V(squash=0)), name, "registered net")
    refused(propose(None), "cadm_policy_propose", "null")
    refused(lib.cadm_policy_propose(ctx, V(), P, P, M, 0, 1, None, None, P, None), "cadm_policy_propose", "null")
    refused(lib.cadm_policy_propose(ctx, V(), P, P, M, 0, 1, P, None, None, None), "cadm_policy_propose", "null")
    refused(lib.cadm_policy_propose(ctx, V(), P, P, 0, 0, 1, P, None, P, None), "cadm_policy_propose", "m must be")
    refused(lib.cadm_policy_propose(ctx, V(), P, None, M, 0, 1, P, None, P, None), "cadm_policy_propose", "ctx_vec")
    refused(lib.cadm_policy_eval(ctx, None, 4, P, None), "cadm_policy_eval", "null")
    refused(lib.cadm_policy_eval(ctx, P, 0, P, None), "cadm_policy_eval", "R must be")
    refused(setnet(V(), W=None), "cadm_set_policy_net", "null")
    refused(setnet(V(), mean=None), "cadm_set_policy_net", "null")
    holes = (ct.c_void_p * 5)(buf.data_ptr(), None, buf.data_ptr(), None, None)
    refused(setnet(V(), b=holes), "cadm_set_policy_net", "layer 1")
    refused(plan(V(), update=2), "cadm_guided_plan", "update")
    refused(plan(V(), prm=None), "cadm_guided_plan", "bad arguments")
    # the slots: K + 1 + P beyond the smallest iteration's candidates (n = 24, 8 elites: 16 at every decay)
    refused(plan(V(n_samples=N)), "cadm_guided_plan", "do not fit")
    small = HipEngine.mppi_params(decay=2.0)
    refused(plan(V(n_samples=16), prm=ct.byref(small)), "cadm_guided_plan", "do not fit the 16")
    keep = HipEngine.mppi_params(keep_elites=3)
    refused(lib.cadm_guided_plan(ctx, V(n_samples=N - 3), None, None, None, None, None, None, 1, None, None, 0, None, None, None, None, None, 0,
                                 ct.byref(keep), P, P, P, P, P, P, P, M, N, 0, 1, P, P, None, None), "cadm_guided_plan", "do not fit")
    # no registered net
    assert lib.cadm_set_policy_net(ctx, None, None, None, None, None, None) == 0
    refused(propose(V()), "cadm_policy_propose", "no policy net", code=-4)
    refused(plan(V()), "cadm_guided_plan", "no policy net", code=-4)
    refused(lib.cadm_policy_eval(ctx, P, 4, P, None), "cadm_policy_eval", "no policy net", code=-4)
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=M, H=5, seed=1)
    deng = make_engine(dprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    refused(setnet(V(), c=deng._ctx), "cadm_set_policy_net", "continuous-action")
    refused(plan(V(), c=deng._ctx), "cadm_guided_plan", "continuous actions only")
    deng.close()
    sprob = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=5, seed=3, trained_like=True)
    seng = make_engine(sprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(seng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    refused(setnet(V(), c=seng._ctx), "cadm_set_policy_net", "sharded")
    refused(propose(V(), c=seng._ctx), "cadm_policy_propose", "sharded")
    refused(plan(V(), c=seng._ctx), "cadm_guided_plan", "sharded")
    assert lib.cadm_dist_destroy(seng._ctx) == 0
    seng.close()
    # a ctx whose planner iterations could reach the roll's iteration words
    ieng = make_engine(sprob, p=5, num_elites=KE, num_cem_iters=_lib.POLICY_IT + 1)
    assert lib.cadm_set_policy_net(ieng._ctx, V(), two, two, P, P, None) == 0
    refused(propose(V(), c=ieng._ctx), "cadm_policy_propose", "iteration words")
    ieng.close()
    assert (_np(buf) == 0).all()
    # python: shapes that do not fit the engine or the declared net
    prm, layers = _set(eng, (32, 16), "relu", "tanh", P=4, seed=1)
    with pytest.raises(ValueError, match="policy_eval: states"):
        eng.policy_eval(np.zeros((4, eng.D + 1), F))
    with pytest.raises(ValueError, match="policy_propose: obs"):
        eng.policy_propose(prm, np.zeros((M, eng.D + 1), F))
    with pytest.raises(ValueError, match="layer 2 is"):
        eng.set_policy_net(prm, pref.he_policy(eng.D, (32, 16), eng.A + 1, 0))
    args = (None,) * 14 + (HipEngine.icem_params(), prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    out = _np(eng.guided_plan(prm, *args, seed=1, call=1))
    assert np.isfinite(out).all() and np.abs(out).max() <= 1.0


def test_workspace_bytes_are_the_restated_sums(engines):
    """`cadm_policy_workspace_bytes` and `cadm_guided_workspace_bytes` against their sums restated here (csrc/policy.hip policy_carve,
    csrc/icem.hip icem_carve): every view is 4-byte words, rounded up to 256 bytes; the guided workspace is the rewarded loop's with the
    proposals and the roll's workspace behind it, and with P = 0 the rewarded loop's itself."""
    _, eng = engines("hc5")
    lib, ctx = eng.lib, eng._ctx
    E, p, H, D, A = eng.E, eng.p, eng.H, eng.D, eng.A
    a = lambda x: (x + 255) // 256 * 256

    def roll(m, P):
        return a(4 * m * P * A) + a(4 * m * P * p) + 2 * a(4 * m * P * p * D)
    for m, P in ((1, 1), (2, 6), (3, 17), (1, 24)):
        assert lib.cadm_policy_workspace_bytes(ctx, m, P) == roll(m, P), (m, P)
        for mppi in (0, 1):
            for terminate, act, unc in ((0, 0, 0), (1, 1, 1), (0, 1, 0)):
                under = lib.cadm_rewarded_workspace_bytes(ctx, m, N, 2, mppi, terminate, act, unc)
                assert lib.cadm_guided_workspace_bytes(ctx, m, N, 2, mppi, terminate, act, unc, P) == under + a(4 * m * P * H * A) + a(roll(m, P))
                assert lib.cadm_guided_workspace_bytes(ctx, m, N, 2, mppi, terminate, act, unc, 0) == under
    assert lib.cadm_policy_workspace_bytes(ctx, 0, 4) == 0 and lib.cadm_policy_workspace_bytes(ctx, 2, 0) == 0
    assert lib.cadm_policy_workspace_bytes(None, 2, 4) == 0
    assert lib.cadm_guided_workspace_bytes(ctx, 0, N, 2, 0, 0, 0, 0, 4) == 0 and lib.cadm_guided_workspace_bytes(ctx, M, N, 2, 0, 0, 0, 0, -1) == 0
