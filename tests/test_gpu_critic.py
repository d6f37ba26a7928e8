"""GPU: the terminal value from Q critics of the opt-in planner -- the fused kernel (`cadm_critic_eval` / `cadm_critic_returns`,
csrc/critic.hip) against the numpy restatement (tests/critic_ref.py), its bits in any batch and from either entry, its agreement with
the value net (csrc/value.hip) for critics that ignore their action, the row update, non-finite terminal states and the `first` cut,
the fused loop (`cadm_critic_plan`) against the stepwise one, the class route and the refusals.

Geometries: the module-scoped engines of tests/test_gpu_tracking.py -- hopper_like (D = 11, A = 3, p = 5, H = 3: K = 14 is no multiple
of 4), halfcheetah (D = 18, p = 20, H = 8 and p = 5, H = 5); synthetic trajectories from tests/behind_rollout.py; the class route on
tests/helpers.py's `plan_model`.  tests/test_gpu_critic_envelope.py runs the `check_*` bodies of this file on the other geometries.

The kernel is held to the float64 restatement at the project's bar for fp32 kernels, `helpers.assert_close` at 1e-5 of the output's
scale.  Measured on an MI355X, worst |err| / (1e-5 x max(|ref|, rms)) over q and every critic's q: relu 0.260, tanh 0.187, swish 0.467;
512 x 2 for actor and critics: 0.213."""
import ctypes as ct
import math
import os

import numpy as np
import pytest
import torch

import critic_ref as cref
import policy_ref as pref
import value_ref as vref
from cadm_amd import _lib, jit
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import _np, assert_close, floored_rel, make_engine, plan_act, plan_model, zero_carry
from test_gpu_tracking import engines      # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")
M, N, KE, ITERS = 2, 24, 8, 3


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _bounds(eng):
    return float(eng.cfg.lower_bound), float(eng.cfg.upper_bound)


def _register(eng, actor, critics, hidden, phidden, act, reduce="min", weight=1.0, mean=None, std=None):
    """register actor and critics on the engine: (critic_params, policy_params)"""
    pol = HipEngine.policy_params(phidden, actor["act"], actor.get("squash", "tanh"), 1, 0.0)
    eng.set_policy_net(pol, actor["layers"], obs_mean=actor.get("mean"), obs_std=actor.get("std"))
    crt = HipEngine.critic_params(hidden, act, len(critics), reduce, weight)
    eng.set_critic_nets(crt, critics, in_mean=mean, in_std=std)
    return crt, pol


def _simple(eng, hidden=(64, 48), phidden=(32,), C=2, act="relu", reduce="min", weight=1.0, seed=0, squash="tanh"):
    """a He-initialised actor and C critics without statistics, registered: (critic_params, policy_params, actor, critics)"""
    actor = dict(layers=pref.he_policy(eng.D, phidden, eng.A, seed, out_scale=0.5), act=act, squash=squash)
    critics = cref.he_critics(eng.D, eng.A, hidden, C, seed + 1)
    crt, pol = _register(eng, actor, critics, hidden, phidden, act, reduce, weight)
    return crt, pol, actor, critics


# ---------------------------------------------------------------------------------------------------------------------- 1: the kernel
def check_kernel_cases(eng, act, cases, rows_of, states_of, weight_eff=0.5):
    """The body of `test_kernel_against_restatement` on any engine: `cases` a list of (hidden, phidden, C, reduce, squash), `rows_of` the
    (m, n) of the launches of a case (the nets of the first serve the others), `states_of(m, n, seed)` -> (traj, its last states);
    weight_eff: what the row update multiplies q by -- the declared 0.5, or float32(0.5 disc[H]) on a ctx with a discount.  -> the worst
    |err| / (1e-5 of scale) over q and every critic's q."""
    lb, ub = _bounds(eng)
    worst, gi = 0.0, 0
    for hidden, phidden, C, reduce, squash in cases:
        gi += 1
        what = "%s %r behind %r, C = %d, %s, %s" % (act, hidden, phidden, C, reduce, squash)
        actor = crt = None
        for m, n in rows_of:
            traj, states = states_of(m, n, 30 + gi)
            if actor is None:      # (the nets of the first case serve the others)
                actor, critics, mean, std = cref.kernel_case(states, eng.A, hidden, phidden, C, act, squash, 10 + gi)
                crt, _ = _register(eng, actor, critics, hidden, phidden, act, reduce, 0.5, mean, std)
            ref, ref_each = cref.q64(states, critics, act, reduce, actor, mean=mean, std=std, lb=lb, ub=ub, want_each=True)
            q, each, a = (_np(x) for x in eng.critic_eval(states, want_each=True, want_actions=True))
            assert q.shape == (m * n * eng.p,) and each.shape == (C, m * n * eng.p) and np.isfinite(q).all(), what
            worst = max(worst, floored_rel(q, ref) / 1e-5, floored_rel(each, ref_each) / 1e-5)
            assert_close(q, ref, what=what)
            assert_close(each, ref_each, what=what + ": each")
            assert_close(a, pref.action64(states, actor["layers"], act, squash, lb, ub, actor["mean"], actor["std"]), what=what + ": action")
            np.testing.assert_array_equal(_bits(q), _bits(cref.reduce32(each, reduce)), err_msg=what + ": the reduce order")
            rows = np.random.default_rng(gi).standard_normal((m, n, eng.p)).astype(F)
            out, qo = eng.critic_returns(traj, rows, crt, want_q=True)
            np.testing.assert_array_equal(_bits(_np(qo)).reshape(-1), _bits(q), err_msg=what + ": q_out against cadm_critic_eval")
            np.testing.assert_array_equal(_bits(_np(out)), _bits(cref.update(rows, _np(qo), weight_eff)), err_msg=what)
    return worst


@pytest.mark.parametrize("act", cref.ACTS)
def test_kernel_against_restatement(engines, act):
    """`cadm_critic_eval` (q, every critic's q, the action used) on hopper_like against the float64 restatement at 1e-5 of scale: every
    critic geometry of critic_ref.KERNEL_CRITICS behind both actors, under every (C, reduce, squash), with input statistics that are not
    0 / 1 for actor and critics, at 165 rows (ten full tiles and a tail of 5) and at 15 (less than a tile).  `cadm_critic_returns`' q_out
    has the same bits, and the rows are the row update from them.  tests/test_critic_ref.py holds the same cases to the liveness
    conditions on the CPU."""
    _, eng = engines("hopper")
    cases = [(hidden, phidden) + combo for hidden in cref.KERNEL_CRITICS for phidden in cref.KERNEL_ACTORS for combo in cref.KERNEL_COMBOS]
    worst = check_kernel_cases(eng, act, cases, cref.KERNEL_ROWS, cref.kernel_states)
    print("\n[%s] worst |err| / (1e-5 of scale): %.3f" % (act, worst))


def test_kernel_at_the_widest_nets(engines):
    """512 x 2 for the actor and for two critics on halfcheetah (D = 18, A = 6, p = 20): the input tile and two regions of 16 x 512
    floats are beyond what a kernel gets without raising its dynamic-LDS attribute; 2 x 3 x 20 = 120 rows."""
    _, eng = engines("hc8")
    lb, ub = _bounds(eng)
    traj, states = cref.kernel_states(2, 3, 5, H=eng.H, p=eng.p, D=eng.D, A=eng.A)
    actor, critics, mean, std = cref.kernel_case(states, eng.A, (512, 512), (512, 512), 2, "relu", "tanh", 3)
    cref.check_live(states, critics, "relu", actor, mean, std, lb, ub, what="512 x 2")
    _register(eng, actor, critics, (512, 512), (512, 512), "relu", "min", 1.0, mean, std)
    ref = cref.q64(states, critics, "relu", "min", actor, mean=mean, std=std, lb=lb, ub=ub)
    got = _np(eng.critic_eval(states))
    print("\n[512 x 2] worst |err| / (1e-5 of scale): %.3f" % (floored_rel(got, ref) / 1e-5))
    assert_close(got, ref, what="512 x 2")


# ---------------------------------------------------------------------------------------------------------------------- 2: equal bits
def check_bits_in_any_batch(eng, states, hidden, phidden, act, C, reduce, traj=None):
    """The body of `test_a_state_has_the_same_bits_in_any_batch` for any engine and any batch `states` [R, D] (R > 16); traj [H,m,n,p,D]:
    the trajectory whose last states they are, for `critic_returns`' q_out and the call with leading dims (None: neither)."""
    R = states.shape[0]
    actor, critics, mean, std = cref.kernel_case(states, eng.A, hidden, phidden, C, act, "tanh", 21)
    crt, _ = _register(eng, actor, critics, hidden, phidden, act, reduce, 1.0, mean, std)
    full, each, a = (_np(x) for x in eng.critic_eval(states, want_each=True, want_actions=True))
    assert full.shape == (R,) and each.shape == (C, R)
    pa = _np(eng.policy_eval(states))
    np.testing.assert_array_equal(_bits(a), _bits(pa), err_msg="act_out against policy_eval")
    g, geach, ga = (_np(x) for x in eng.critic_eval(states, actions=pa, want_each=True, want_actions=True))
    np.testing.assert_array_equal(_bits(g), _bits(full), err_msg="given the actor's action")
    np.testing.assert_array_equal(_bits(geach), _bits(each))
    np.testing.assert_array_equal(_bits(ga), _bits(pa), err_msg="act_out of given actions")
    again = eng.critic_eval(states, want_each=True)
    np.testing.assert_array_equal(_bits(_np(again[0])), _bits(full), err_msg="run to run")
    np.testing.assert_array_equal(_bits(_np(again[1])), _bits(each), err_msg="run to run")
    for r in (1, 5, 16):
        q, e = eng.critic_eval(states[:r], want_each=True)
        np.testing.assert_array_equal(_bits(_np(q)), _bits(full[:r]), err_msg="R = %d" % r)
        np.testing.assert_array_equal(_bits(_np(e)), _bits(each[:, :r]), err_msg="R = %d" % r)
    q, e = eng.critic_eval(np.roll(states, 7, axis=0), want_each=True)
    np.testing.assert_array_equal(_bits(_np(q)), _bits(np.roll(full, 7)), err_msg="rows moved by 7")
    np.testing.assert_array_equal(_bits(_np(e)), _bits(np.roll(each, 7, axis=1)), err_msg="rows moved by 7")
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count      # (256 on an MI355X)
    reps = 2 * 16 * cus // R + 8
    q, e = (_np(x) for x in eng.critic_eval(np.concatenate([states[3:]] + [states] * reps, axis=0), want_each=True))
    assert q.shape[0] > 2 * 16 * cus
    np.testing.assert_array_equal(_bits(q[:R - 3]), _bits(full[3:]), err_msg="the two-row-tile launch, head")
    np.testing.assert_array_equal(_bits(q[-R:]), _bits(full), err_msg="the two-row-tile launch, tail")
    np.testing.assert_array_equal(_bits(e[:, :R - 3]), _bits(each[:, 3:]))
    np.testing.assert_array_equal(_bits(e[:, -R:]), _bits(each))
    if traj is None:
        return
    m, n = traj.shape[1:3]
    _, qo = eng.critic_returns(traj, np.zeros((m, n, eng.p), F), crt, want_q=True)
    np.testing.assert_array_equal(_bits(_np(qo)).reshape(-1), _bits(full), err_msg="critic_returns' q_out")
    lead = eng.critic_eval(states.reshape(m, n, eng.p, eng.D))
    assert tuple(lead.shape) == (m, n, eng.p)
    np.testing.assert_array_equal(_bits(_np(lead)).reshape(-1), _bits(full))


@pytest.mark.parametrize("hidden,phidden,act,C,reduce", [((64, 48, 200), (64, 48), "swish", 3, "mean"), ((200, 200), (), "relu", 2, "min"),
                                                          ((), (64, 48), "tanh", 1, "min")], ids=["unequal-swish", "200x2-relu", "linear"])
def test_a_state_has_the_same_bits_in_any_batch(engines, hidden, phidden, act, C, reduce):
    """The action used against `policy_eval`; the fused actor path against `critic_eval(states, actions=policy_eval(states))`; every
    critic's q at R = 1, 5, 16, 165, with the rows rolled by 7, inside a batch large enough for two row tiles per workgroup (more than
    2 x 16 x the CU count rows; head and tail), run to run, and from `critic_returns`' q_out: equal bits."""
    _, eng = engines("hopper")
    traj, states = cref.kernel_states(3, 11, 41)
    assert states.shape[0] == 165
    check_bits_in_any_batch(eng, states, hidden, phidden, act, C, reduce, traj)


# ---------------------------------------------------------------------------------------------------------------------- 3: against the value net
def _value_twin(D, A, hidden, act, seed):
    """(V's layers, its statistics, the critic that ignores its action, the critic's statistics)"""
    rng = np.random.default_rng(seed)
    v_layers = vref.he_net(D, hidden, seed)
    smean, sstd = rng.standard_normal(D).astype(F), rng.uniform(0.5, 2.0, D).astype(F)
    mean = np.concatenate([smean, rng.standard_normal(A).astype(F)])
    std = np.concatenate([sstd, rng.uniform(0.5, 2.0, A).astype(F)])
    return v_layers, (smean, sstd), cref.critic_from_value(v_layers, D, A), (mean, std)


@pytest.mark.parametrize("hidden,act", [((64, 48), "tanh"), ((200,), "relu"), ((), "relu")], ids=["64-48-tanh", "200-relu", "linear"])
def test_critics_that_ignore_the_action_are_the_value_net(engines, hidden, act):
    """Critics whose action rows of W_0 are zero and whose statistics on the state dims are V's: q equals `value_eval` of the V net made
    from the state rows as numbers (fma(0, x, acc) leaves every acc but -0.0 as it is: +-0 is the only licence) -- C = 1, then C = 2
    with identical nets under both reduces."""
    _, eng = engines("hopper")
    D, A = eng.D, eng.A
    v_layers, vstats, critic, (mean, std) = _value_twin(D, A, hidden, act, 17)
    eng.set_value_net(HipEngine.value_params(hidden, act, 1.0), v_layers, obs_mean=vstats[0], obs_std=vstats[1])
    states = cref.kernel_states(3, 11, 43)[1]
    v = _np(eng.value_eval(states))
    assert np.isfinite(v).all() and v.std() > 0
    actor = dict(layers=pref.he_policy(D, (32,), A, 3, out_scale=0.5), act="relu")
    for C, reduce in ((1, "min"), (1, "mean"), (2, "min"), (2, "mean")):
        _register(eng, actor, [critic] * C, hidden, (32,), act, reduce, 1.0, mean, std)
        q, each = (_np(x) for x in eng.critic_eval(states, want_each=True))
        np.testing.assert_array_equal(q, v, err_msg="C = %d, %s" % (C, reduce))
        for c in range(C):
            np.testing.assert_array_equal(each[c], v)


@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_get_action_equals_the_valued_model(gpu, update):
    """`get_action` of a `cem_terminal_q` model whose two identical critics ignore their action, against a `cem_terminal_value` model
    with the V net of their state rows, same seed: equal plans, over two calls."""
    H, A, D = 5, 6, 18
    hidden, act = (64, 32), "swish"
    v_layers, vstats, critic, (mean, std) = _value_twin(D, A, hidden, act, 19)
    kw = dict(cem_keep_elites=2, cem_update=update)
    qm, prob = plan_model(False, H, cem_terminal_q=dict(hidden_sizes=hidden, activation=act, n_critics=2, reduce="min", weight=0.8,
                                                        policy=dict(hidden_sizes=(16,), activation="tanh", squash="tanh")), **kw)
    vm, _ = plan_model(False, H, cem_terminal_value=dict(hidden_sizes=hidden, activation=act, weight=0.8), **kw)
    qm.set_policy(pref.he_policy(D, (16,), A, 2, out_scale=0.5))
    qm.set_critics([critic, critic], mean, std)
    vm.set_terminal_value(v_layers, *vstats)
    mean0, var0 = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    for call in (1, 2):
        a, b = plan_act(qm, prob, False, mean0, var0), plan_act(vm, prob, False, mean0, var0)
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b, err_msg="call %d" % call)
    plain, _ = plan_model(False, H, **kw)
    plan_act(plain, prob, False, mean0, var0)
    assert not np.array_equal(plan_act(plain, prob, False, mean0, var0), a), "the term must matter"


# ---------------------------------------------------------------------------------------------------------------------- 4: row update, non-finite states, the first cut
@pytest.mark.parametrize("weight", [1.0, -0.37, 0.0])
def test_row_update(engines, weight):
    """rows_out == float32(rows_in + float32(weight * q)) bit for bit from the kernel's own q_out; rows_out aliasing rows_in and
    q_out = NULL give the same rows_out; rows_in is not written otherwise."""
    _, eng = engines("hc5")
    crt, _, _, _ = _simple(eng, (64, 64), (32,), 2, "swish", "mean", weight, seed=5)
    traj = cref.kernel_states(3, 7, 9, H=eng.H, p=eng.p, D=eng.D, A=eng.A)[0]
    rows = (10.0 * np.random.default_rng(2).standard_normal((3, 7, eng.p))).astype(F)
    t_dev, r_dev = eng._t(traj), eng._t(rows)
    out, q = eng.critic_returns(t_dev, r_dev, crt, want_q=True)
    np.testing.assert_array_equal(_bits(_np(r_dev)), _bits(rows), err_msg="rows_in was written")
    np.testing.assert_array_equal(_bits(_np(out)), _bits(cref.update(rows, _np(q), weight)))
    np.testing.assert_array_equal(_bits(_np(eng.critic_returns(t_dev, r_dev, crt))), _bits(_np(out)), err_msg="q_out = NULL")
    alias = r_dev.clone()
    assert eng.critic_returns(t_dev, alias, crt, out=alias) is alias
    np.testing.assert_array_equal(_bits(_np(alias)), _bits(_np(out)), err_msg="rows_out aliasing rows_in")
    assert weight == 0.0 or not np.array_equal(_bits(_np(out)), _bits(rows))


def check_non_finite_and_first(eng, act, clean, dims=None, hidden=(48, 48), phidden=(32,), seed=13):
    """The body of `test_non_finite_terminal_states_and_the_first_cut` on any engine with A >= 3, p >= 3, D >= 4 and H >= 2: clean
    [H,m,n,p,D] a finite trajectory; dims: the dims the poison is planted in (None: drawn over all D); seed: of the poisoned rows and
    the cuts (`first` is drawn over 0 .. H: at a long H another seed may be needed for a poisoned row that is not cut)."""
    H, p, D = eng.H, eng.p, eng.D
    crt, _, _, _ = _simple(eng, hidden, phidden, 2, act, "min", 2.0, seed=6)
    m, n = clean.shape[1:3]
    assert clean.shape == (H, m, n, p, D)
    rows = np.random.default_rng(4).standard_normal((m, n, p)).astype(F)
    ref_out, ref_q = (_np(x) for x in eng.critic_returns(clean, rows, crt, want_q=True))
    assert np.isfinite(ref_q).all()
    rng = np.random.default_rng(seed)
    bad = clean.copy()
    bad[:-1][rng.uniform(size=bad[:-1].shape) < 0.2] = np.nan             # earlier steps: never read
    bad[0, 0, 0, 0, :] = np.inf
    hit = rng.uniform(size=(m, n, p)) < 0.2
    hit[0, 0, 0], hit[0, 0, 1], hit[m - 1, n - 1, p - 1] = True, False, True      # the first row, its neighbour, the tail tile's last row
    mi, ni, j = np.nonzero(hit)
    poison = np.array([np.nan, np.inf, -np.inf], F)[rng.integers(0, 3, mi.size)]
    bad[H - 1, mi, ni, j, rng.integers(0, D, mi.size) if dims is None else np.asarray(dims)[rng.integers(0, len(dims), mi.size)]] = poison
    out, q = (_np(x) for x in eng.critic_returns(bad, rows, crt, want_q=True))
    assert np.isnan(q[hit]).all() and np.isnan(out[hit]).all()
    np.testing.assert_array_equal(_bits(q[~hit]), _bits(ref_q[~hit]), err_msg="a row met its neighbour's poison")
    np.testing.assert_array_equal(_bits(out[~hit]), _bits(ref_out[~hit]))
    flat, each, a = (_np(x) for x in eng.critic_eval(bad[-1], want_each=True, want_actions=True))
    assert np.isnan(flat[hit]).all() and np.isnan(each[:, hit]).all()
    np.testing.assert_array_equal(_bits(flat[~hit]), _bits(ref_q[~hit]))
    assert (a[hit] == pref.fallback(*_bounds(eng))).all() and np.isfinite(a).all()      # what policy_eval gives them; no Q came of it
    # a non-finite given action
    acts = _np(eng.policy_eval(clean[-1]))
    acts[0, 0, 1, 2] = np.nan
    g = _np(eng.critic_eval(clean[-1], actions=acts))
    assert np.isnan(g[0, 0, 1]) and np.isfinite(np.delete(g.reshape(-1), 1)).all()
    # the first cut
    first = rng.integers(0, H + 1, (m, n, p)).astype(np.int32)
    first[0, 0, 0], first[0, 0, 1], first[0, 0, 2] = 0, H, H - 1
    hit[0, 0, 2] = True
    bad[H - 1, 0, 0, 2, 3] = np.nan
    cut = first < H
    assert cut[hit].any() and (~cut)[hit].any() and cut[~hit].any() and (~cut)[~hit].any()
    out, q = (_np(x) for x in eng.critic_returns(bad, rows, crt, first=first, want_q=True))
    np.testing.assert_array_equal(_bits(out[cut]), _bits(rows[cut]), err_msg="a row with first < H must keep its input bits")
    assert np.isnan(q[cut]).all()
    live = ~cut & ~hit
    np.testing.assert_array_equal(_bits(out[live]), _bits(ref_out[live]))
    np.testing.assert_array_equal(_bits(q[live]), _bits(ref_q[live]))
    assert np.isnan(out[~cut & hit]).all() and np.isnan(q[~cut & hit]).all()


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_non_finite_terminal_states_and_the_first_cut(engines, act):
    """NaN and +-inf in single dims of traj[H-1] make those rows' q and return NaN -- under relu too, whose max(NaN, 0) would hide them,
    and although the actor's fallback action is finite --, garbage in earlier steps reaches nothing, and every other row has the bits it
    has without its neighbours' poison.  With `first`, rows with first < H keep their input bits, terminal NaN or not, and read NaN in
    q_out; rows with first == H are valued."""
    _, eng = engines("hopper")
    check_non_finite_and_first(eng, act, cref.kernel_states(3, 11, 12)[0])


# ---------------------------------------------------------------------------------------------------------------------- 5: fused against stepwise
COMBOS = ["cem", "mppi", "cem-prior", "mppi-prior", "cem-terminate", "mppi-prior-terminate"]


def check_fused_equals_stepwise(prob, eng, combo, cons_dims=(1, 7), hidden=(64, 48), phidden=(32,)):
    """The body of `test_fused_equals_stepwise` on any engine whose rollout the library carries: cons_dims the dims the TERMINATE
    constraints bind (`binding_bounds` on iteration 0's trajectory); hidden, phidden: the critics' and the actor's hidden widths."""
    from test_gpu_constraints import binding_bounds, iteration0_traj
    mppi, prior, terminate = "mppi" in combo, "prior" in combo, "terminate" in combo
    H, A = eng.H, eng.A
    crt, pol1, _, _ = _simple(eng, hidden, phidden, 2, "tanh", "min", 3.0, seed=31)
    pol = HipEngine.policy_params(phidden, "tanh", "tanh", 3, 0.2) if prior else None
    K = 2
    icem = dict(noise_beta=1.0 if mppi else 0.0, keep_elites=K, decay=1.25, return_best=terminate, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if mppi else HipEngine.icem_params(**icem)
    cons = None
    if terminate:
        cons = HipEngine.constraint_params(binding_bounds(iteration0_traj(eng, prob, 0.0, 4, 1), cons_dims, H, "terminal q"), "terminate", 4.0)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    (ca, va), (cb, vb) = zero_carry(eng, M, K, H), zero_carry(eng, M, K, H)
    mean, var = prob["init_mean"], prob["init_var"]
    reach = max(abs(v) for v in _bounds(eng))      # (1.0 on every built-in kind)
    for call in (1, 2):
        a, ra = eng.critic_plan(crt, pol, None, None, None, None, None, None, True, None, None, None, None, None, cons, None, prm, *args, mean, var,
                                N, carry=ca, carry_valid=va, seed=4, call=call, want_best_return=True)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                            update="mppi" if mppi else "cem", temperature=0.5, relative=True, constraints=cons, policy=pol,
                                            critic=crt, **icem)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= reach
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ca)), _bits(_np(cb)))
        for x in info:
            q, before, rows = _np(x["q"]), _np(x["q_rows"]), _np(x["rows"])
            first = _np(x["first_violation"]) if terminate else None
            np.testing.assert_array_equal(_bits(rows), _bits(cref.update(before, q, crt.weight, first, H)))
            flat = _np(eng.critic_eval(x["traj"][-1]))
            keep = np.ones(q.shape, bool) if first is None else first >= H
            np.testing.assert_array_equal(_bits(q[keep]), _bits(flat[keep]))
            assert np.isnan(q[~keep]).all()
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)
    if terminate:
        share = float((_np(info[0]["first_violation"]) < H).mean())
        assert 0.1 <= share <= 0.9, "%.2f of the rows are cut" % share
    other = _np(eng.critic_plan(None, pol, None, None, None, None, None, None, False, None, None, None, None, None, cons, None, prm, *args, mean,
                                var, N, *zero_carry(eng, M, K, H), seed=4, call=2))
    assert not np.array_equal(_bits(other), _bits(a))
    assert (mppi, "crt", terminate, False, False, 3 if prior else 0) in eng._loop_ws


@pytest.mark.parametrize("combo", COMBOS)
def test_fused_equals_stepwise(engines, combo):
    """`cadm_critic_plan` with device RNG == the same loop one launch at a time (`planner.icem_plan(..., critic=...)`), bit for bit over
    two consecutive calls at M = 2, N = 24, 3 iterations: the plan, the best return and the carry -- CEM and MPPI, with and without a
    policy prior in the same call, with TERMINATE constraints; in every stepwise iteration the rows are the row update of the rows
    before it from the kernel's own q.  Without the term the plan is another."""
    prob, eng = engines("hc5")
    assert _bounds(eng) == (-1.0, 1.0)
    check_fused_equals_stepwise(prob, eng, combo)


@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_no_critic_is_the_loop_underneath(engines, update):
    """critic = NULL: the plan, the best return and the carry of `cadm_guided_plan` on the same inputs (with a policy prior), bit for
    bit, through the C entry itself with that loop's workspace; and the workspace of the term is the guided loop's."""
    prob, eng = engines("hc5")
    H, A = eng.H, eng.A
    _simple(eng, (16,), (32,), 1, "tanh", seed=2)
    pol = HipEngine.policy_params((32,), "tanh", "tanh", 3, 0.2)
    icem = dict(noise_beta=1.0, keep_elites=2, decay=1.25, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if update == "mppi" else HipEngine.icem_params(**icem)
    mppi, full = eng._as_mppi_params(prm)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    carry, valid = zero_carry(eng, M, 2, H)
    plan, best = eng.guided_plan(pol, None, None, None, None, None, None, True, None, None, None, None, None, None, None, prm, *args,
                                 carry=carry, carry_valid=valid, seed=5, call=2, want_best_return=True)
    carry2, valid2 = zero_carry(eng, M, 2, H)
    t = [eng._t(x) for x in args[:5]]
    ws = eng._loop_workspace(mppi, M, N, 2, pol=(False, False, False, 3))
    out = torch.empty((M, H, A), dtype=torch.float32, device=eng.device)
    best2 = torch.empty((M,), dtype=torch.float32, device=eng.device)
    P = lambda x: ct.c_void_p(x.data_ptr())
    rc = eng.lib.cadm_critic_plan(eng._ctx, None, ct.byref(pol), None, None, None, None, None, None, 1, None, None, 0, None, None, None, None, None,
                                  int(mppi), ct.byref(full), *[P(x) for x in t], P(carry2), P(valid2), M, N, 5, 2, P(ws), P(out), P(best2),
                                  eng.stream)
    assert rc == 0, eng.lib.cadm_last_error().decode()
    for x, y in ((plan, out), (best, best2), (carry, carry2)):
        np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))
    lib = eng.lib
    for terminate in (0, 1):
        for P_ in (0, 3):
            assert lib.cadm_critic_workspace_bytes(eng._ctx, M, N, 2, int(mppi), terminate, 1, 1, P_) == \
                lib.cadm_guided_workspace_bytes(eng._ctx, M, N, 2, int(mppi), terminate, 1, 1, P_)
    assert lib.cadm_critic_workspace_bytes(eng._ctx, 0, N, 2, 0, 0, 0, 0, 0) == 0


# ---------------------------------------------------------------------------------------------------------------------- 6: the class route
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_class_route(gpu, context):
    """`get_action` with Sequential-set nets agrees with the engine call and with a twin whose nets were set as lists; `q_value` and
    `plan_terminal_q` with the restatement; no critics, or no actor, raises RuntimeError; replaced critics take effect on the next call
    and build nothing; `clear_critics` brings the RuntimeError back."""
    H, A, D = 5, 6, 18
    hidden, phidden, act = (64, 32), (32,), "swish"
    tq = dict(hidden_sizes=hidden, activation=act, n_critics=2, reduce="mean", weight=0.8,
              policy=dict(hidden_sizes=phidden, activation="tanh", squash="tanh"))
    model, prob = plan_model(context, H, cem_terminal_q=tq, cem_keep_elites=2)
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    with pytest.raises(RuntimeError, match="no critics"):
        plan_act(model, prob, context, mean, var)
    rng = np.random.default_rng(5)
    pstats = (rng.standard_normal(D).astype(F), rng.uniform(0.5, 2.0, D).astype(F))
    cstats = (rng.standard_normal(D + A).astype(F), rng.uniform(0.5, 2.0, D + A).astype(F))
    actor = dict(layers=pref.he_policy(D, phidden, A, 16, out_scale=0.5), act="tanh", squash="tanh", mean=pstats[0], std=pstats[1])
    critics = cref.he_critics(D, A, hidden, 2, 17)
    model.set_critics([vref.sequential(c, act) for c in critics], *cstats)
    with pytest.raises(RuntimeError, match="no policy net"):
        plan_act(model, prob, context, mean, var)
    with pytest.raises(RuntimeError, match="no policy net"):
        model.q_value(np.zeros((3, D), F))
    assert model._call == 0
    model.set_policy(vref.sequential(actor["layers"], "tanh"), *pstats)
    plan = plan_act(model, prob, context, mean, var)
    assert np.isfinite(plan).all() and model._call == 1
    eng, opt = model.engine, model._opt
    assert opt.policy_params is None
    hist = (prob["cp_obs"], prob["cp_act"]) if context else (None, None)
    carry, valid = zero_carry(eng, M, 2, H)
    direct = eng.critic_plan(opt.critic_params, None, None, None, None, None, None, None, True, None, None, None, None, None, None, None,
                             opt.params, prob["obs"], *hist, mean, var, model.n_candidates, carry=carry, carry_valid=valid, seed=model.seed, call=1)
    np.testing.assert_array_equal(_bits(plan), _bits(_np(direct)))
    twin, _ = plan_model(context, H, cem_terminal_q=tq, cem_keep_elites=2)
    twin.set_critics(critics, *cstats)                           # the list form of the same nets
    twin.set_policy(actor["layers"], *pstats)
    np.testing.assert_array_equal(_bits(plan_act(twin, prob, context, mean, var)), _bits(plan))
    # Q through the class, against the restatement
    states = (2.0 * rng.standard_normal((4, 7, D))).astype(F)
    q, each = model.q_value(states, return_each=True)
    assert q.shape == (4, 7) and each.shape == (2, 4, 7)
    ref, ref_each = cref.q64(states, critics, act, "mean", actor, mean=cstats[0], std=cstats[1], want_each=True)
    assert_close(q, ref, what="q_value")
    assert_close(each, ref_each, what="q_value: each")
    acts = rng.uniform(-1, 1, (4, 7, A)).astype(F)
    assert_close(model.q_value(states, acts), cref.q64(states, critics, act, "mean", actions=acts, mean=cstats[0], std=cstats[1]), what="q_value at actions")
    assert_close(model.policy_action(states), pref.action64(states, actor["layers"], "tanh", "tanh", -1.0, 1.0, *pstats), what="policy_action")
    res = model.plan_terminal_q(prob["obs"], plan, *(hist if context else ()))
    assert res["q"].shape == (M, 5) and res["first"] is None and model._call == 1 and np.isfinite(res["q"]).all()
    many = model.plan_terminal_q(prob["obs"], np.repeat(plan[:, None], 3, axis=1), *(hist if context else ()))
    assert many["q"].shape == (M, 3, 5) and np.isfinite(many["q"]).all()
    np.testing.assert_array_equal(_bits(many["q"][0, 0]), _bits(res["q"][0]))      # (the noise is drawn per row: env 0's rows are where they were)
    # replaced critics: the next call plans with them, and nothing is built
    before = sorted((f, os.path.getmtime(os.path.join(jit.cache_dir(), f))) for f in os.listdir(jit.cache_dir()))
    ws = dict(eng._loop_ws)
    other = cref.he_critics(D, A, hidden, 2, 18, out_scale=30.0)
    model.set_critics(other, *cstats)
    assert_close(model.q_value(states), cref.q64(states, other, act, "mean", actor, mean=cstats[0], std=cstats[1]), what="the replaced critics")
    plan2 = plan_act(model, prob, context, mean, var)      # call 2, from call 1's carry: what `carry` / `valid` hold since the direct call above
    direct2 = eng.critic_plan(opt.critic_params, None, None, None, None, None, None, None, True, None, None, None, None, None, None, None,
                              opt.params, prob["obs"], *hist, mean, var, model.n_candidates, carry=carry, carry_valid=valid, seed=model.seed, call=2)
    np.testing.assert_array_equal(_bits(plan2), _bits(_np(direct2)))
    assert not np.array_equal(_bits(plan2), _bits(plan))
    assert sorted((f, os.path.getmtime(os.path.join(jit.cache_dir(), f))) for f in os.listdir(jit.cache_dir())) == before
    assert all(eng._loop_ws[k][1] is ws[k][1] for k in ws)
    model.clear_critics()
    with pytest.raises(RuntimeError, match="no critics"):
        plan_act(model, prob, context, mean, var)
    with pytest.raises(RuntimeError, match="no critics"):
        model.q_value(states)
    plain, _ = plan_model(context, H, cem_noise_beta=1.0)
    for fn in (lambda: plain.set_critics(critics), lambda: plain.q_value(states), lambda: plain.clear_critics()):
        with pytest.raises(ValueError, match="no cem_terminal_q"):
            fn()
    with pytest.raises(ValueError, match="no cem_policy_prior and no cem_terminal_q"):
        plain.set_policy(actor["layers"])


def test_the_actor_of_a_policy_prior_serves_the_term(gpu):
    """`cem_terminal_q` without `policy` on a model with `cem_policy_prior`: one `set_policy` serves the proposals and the term, and
    `get_action` is the engine's `critic_plan` with both."""
    H, A, D = 5, 6, 18
    pp = dict(hidden_sizes=(32,), activation="tanh", n_samples=3, noise_std=0.2)
    model, prob = plan_model(False, H, cem_terminal_q=dict(hidden_sizes=(48,), n_critics=1), cem_policy_prior=pp)
    model.set_policy(pref.he_policy(D, (32,), A, 4, out_scale=0.5))
    model.set_critics(cref.he_critics(D, A, (48,), 1, 5))
    mean, var = np.zeros((M, H, A)), np.full((M, H, A), 0.25)
    plan = plan_act(model, prob, False, mean, var)
    eng, opt = model.engine, model._opt
    direct = eng.critic_plan(opt.critic_params, opt.policy_params, None, None, None, None, None, None, True, None, None, None, None, None, None,
                             None, opt.params, prob["obs"], None, None, mean, var, model.n_candidates, seed=model.seed, call=1)
    np.testing.assert_array_equal(_bits(plan), _bits(_np(direct)))


def test_an_increasing_critic_pulls_the_plan(gpu):
    """halfcheetah, linear critics Q = c x_d (no action weights): against the plain plan, the planned trajectory's terminal mean of x_d
    (from `forecast`) moves up with +c and down with -c, in every env, on a deterministic model -- the construction of
    tests/test_gpu_value.py::test_a_linear_value_pulls_the_plan.  Cannot pass without the term."""
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
        model, _ = plan_model(False, H, cem_terminal_q=dict(hidden_sizes=(), n_critics=2, reduce="min", weight=1.0,
                                                            policy=dict(hidden_sizes=(), activation="relu", squash="tanh")), **other)
        W = np.zeros((D + A, 1), F)
        W[d, 0] = sign * c
        model.set_critics([[(W, np.zeros((1,), F))]] * 2)
        model.set_policy(pref.he_policy(D, (), A, 1, out_scale=0.5))
        plan = plan_act(model, prob, False, mean, var)
        assert np.isfinite(plan).all()
        term[name] = model.forecast(prob["obs"], plan, seed=11)["mean"][:, -1, d].astype(np.float64)
    print("\n[direction] d = %d, c = %.3g, random plans move it by %.3g; terminal mean: down %s  plain %s  up %s"
          % (d, c, moved[d], term["down"], term["plain"], term["up"]))
    assert (term["up"] > term["plain"]).all() and (term["down"] < term["plain"]).all()


# ---------------------------------------------------------------------------------------------------------------------- 7: refusals
def test_argument_checks(engines):
    """The C entries refuse bad arguments with CADM_EINVAL (no critics, or no policy net on the actor path: CADM_ESTATE) and a message
    that names them and the argument, before any HIP call (the dummy pointers next to the bad argument are never touched); the engine
    plans normally afterwards."""
    prob, eng = engines("hc5")
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(8192, dtype=torch.float32, device=eng.device)
    P = ct.c_void_p(buf.data_ptr())
    mp = HipEngine.mppi_params()
    crt0, pol0, _, _ = _simple(eng, (32, 16), (32,), 2, "relu", seed=1)
    ptrs = (ct.c_void_p * 25)(*([buf.data_ptr()] * 25))

    def Q(n_hidden=2, hidden=(32, 16), activation=0, n_critics=2, reduce=0, weight=1.0):
        v = _lib.CriticParams()
        v.n_hidden, v.activation, v.n_critics, v.reduce, v.weight = n_hidden, activation, n_critics, reduce, weight
        for l, h in enumerate(hidden):
            v.hidden[l] = h
        return ct.byref(v)

    def setnets(v, c=ctx, W=ptrs, b=ptrs, mean=P, inv=P):
        return lib.cadm_set_critic_nets(c, v, W, b, mean, inv, None)

    def returns(v, c=ctx):
        return lib.cadm_critic_returns(c, v, P, None, M, 4, P, P, None, None)

    def plan(v, c=ctx, update=0, prm=ct.byref(mp), value=None):
        return lib.cadm_critic_plan(c, v, None, None, value, None, None, None, None, 1, None, None, 0, None, None, None, None, None, update, prm,
                                    P, P, P, P, P, None, None, M, N, 0, 1, P, P, None, None)

    def refused(rc, name, frag, code=-1):
        msg = lib.cadm_last_error().decode()
        assert rc == code, "%s: expected %d, got %d (%s)" % (name, code, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg

    for name, fn in (("cadm_set_critic_nets", setnets), ("cadm_critic_returns", returns), ("cadm_critic_plan", plan)):
        refused(fn(Q(n_hidden=5)), name, "hidden layers")
        refused(fn(Q(n_hidden=-1)), name, "hidden layers")
        refused(fn(Q(hidden=(32, 0))), name, "width")
        refused(fn(Q(hidden=(513, 16))), name, "width")
        refused(fn(Q(activation=3)), name, "activation")
        refused(fn(Q(activation=-1)), name, "activation")
        refused(fn(Q(n_critics=0)), name, "critics, outside")
        refused(fn(Q(n_critics=6)), name, "critics, outside")
        refused(fn(Q(reduce=2)), name, "reduce")
        refused(fn(Q(reduce=-1)), name, "reduce")
        for bad in (NAN, math.inf, -math.inf):
            refused(fn(Q(weight=bad)), name, "weight")
    for name, fn in (("cadm_critic_returns", returns), ("cadm_critic_plan", plan)):
        refused(fn(Q(hidden=(32, 17))), name, "registered critics")
        refused(fn(Q(n_hidden=1)), name, "registered critics")
        refused(fn(Q(activation=1)), name, "registered critics")
        refused(fn(Q(n_critics=3)), name, "registered critics")
    refused(returns(None), "cadm_critic_returns", "null")
    refused(lib.cadm_critic_returns(ctx, Q(), P, None, M, 4, P, None, None, None), "cadm_critic_returns", "null")
    refused(lib.cadm_critic_returns(ctx, Q(), P, None, 0, 4, P, P, None, None), "cadm_critic_returns", "m, n must be")
    refused(lib.cadm_critic_eval(ctx, None, None, 4, P, None, None, None), "cadm_critic_eval", "null")
    refused(lib.cadm_critic_eval(ctx, P, None, 4, None, None, None, None), "cadm_critic_eval", "null")
    refused(lib.cadm_critic_eval(ctx, P, None, 0, P, None, None, None), "cadm_critic_eval", "R must be")
    refused(setnets(Q(), W=None), "cadm_set_critic_nets", "null")
    refused(setnets(Q(), mean=None), "cadm_set_critic_nets", "null")
    holes = (ct.c_void_p * 6)(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, buf.data_ptr())
    refused(setnets(Q(), b=holes), "cadm_set_critic_nets", "layer 1 of critic 1")
    refused(plan(Q(), update=2), "cadm_critic_plan", "update")
    refused(plan(Q(), prm=None), "cadm_critic_plan", "bad arguments")
    # one terminal term
    eng.set_value_net(HipEngine.value_params((8,), "relu", 1.0), vref.he_net(eng.D, (8,), 0))
    refused(plan(Q(), value=ct.byref(HipEngine.value_params((8,), "relu", 1.0))), "cadm_critic_plan", "one terminal term")
    # LDS at one row tile: 16 x (24 + 512 + 512 + 5 + 2) floats fit; nothing this ABI admits is beyond 160 KiB, so the bound is stated
    # and not reachable: the widest admitted nets are what test_kernel_at_the_widest_nets runs
    assert 16 * (192 + 512 + 512 + 7) * 4 < 160 * 1024
    # no policy net on the actor path; with given actions the critics alone will do
    assert lib.cadm_set_policy_net(ctx, None, None, None, None, None, None) == 0
    refused(returns(Q()), "cadm_critic_returns", "no policy net", code=-4)
    refused(plan(Q()), "cadm_critic_plan", "no policy net", code=-4)
    refused(lib.cadm_critic_eval(ctx, P, None, 4, P, None, None, None), "cadm_critic_eval", "no policy net", code=-4)
    q = eng.critic_eval(np.zeros((4, eng.D), F), actions=np.zeros((4, eng.A), F))
    assert np.isfinite(_np(q)).all()
    # no registered critics
    eng.set_policy_net(pol0, pref.he_policy(eng.D, (32,), eng.A, 1, out_scale=0.5))
    assert lib.cadm_set_critic_nets(ctx, None, None, None, None, None, None) == 0
    refused(returns(Q()), "cadm_critic_returns", "no critics", code=-4)
    refused(plan(Q()), "cadm_critic_plan", "no critics", code=-4)
    refused(lib.cadm_critic_eval(ctx, P, None, 4, P, None, None, None), "cadm_critic_eval", "no critics", code=-4)
    refused(lib.cadm_critic_eval(ctx, P, P, 4, P, None, None, None), "cadm_critic_eval", "no critics", code=-4)
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=M, H=5, seed=1)
    deng = make_engine(dprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    refused(setnets(Q(), c=deng._ctx), "cadm_set_critic_nets", "continuous-action")
    refused(plan(Q(), c=deng._ctx), "cadm_critic_plan", "continuous actions only")
    deng.close()
    sprob = synth.make_problem(env="halfcheetah", context=True, E=5, m=M, H=5, seed=3, trained_like=True)
    seng = make_engine(sprob, p=5, num_elites=KE, num_cem_iters=ITERS)
    fn = _lib.ALLGATHER_FN(lambda *a: 1)
    assert lib.cadm_dist_init_external(seng._ctx, 2, 0, ct.cast(fn, ct.c_void_p), None) == 0
    refused(setnets(Q(), c=seng._ctx), "cadm_set_critic_nets", "sharded")
    refused(plan(Q(), c=seng._ctx), "cadm_critic_plan", "sharded")
    assert lib.cadm_dist_destroy(seng._ctx) == 0
    seng.close()
    assert (_np(buf) == 0).all()
    # python: shapes that do not fit the engine or the declared nets
    crt, _, _, critics = _simple(eng, (32, 16), (32,), 2, "relu", seed=1)
    with pytest.raises(ValueError, match="critic_returns: traj"):
        eng.critic_returns(np.zeros((eng.H, M, 4, eng.p, eng.D + 1), F), np.zeros((M, 4, eng.p), F), crt)
    with pytest.raises(ValueError, match="critic_returns: first"):
        eng.critic_returns(np.zeros((eng.H, M, 4, eng.p, eng.D), F), np.zeros((M, 4, eng.p), F), crt, first=np.zeros((M, 4), np.int32))
    with pytest.raises(ValueError, match="critic_eval: states"):
        eng.critic_eval(np.zeros((4, eng.D + 1), F))
    with pytest.raises(ValueError, match="critic_eval: actions"):
        eng.critic_eval(np.zeros((4, eng.D), F), actions=np.zeros((4, eng.A + 1), F))
    with pytest.raises(ValueError, match="layer 1 of critic 1 is"):
        eng.set_critic_nets(crt, [critics[0], vref.he_net(eng.D + eng.A, (32, 17), 0)])
    with pytest.raises(ValueError, match="1 nets given, 2 critics declared"):
        eng.set_critic_nets(crt, critics[:1])
    with pytest.raises(ValueError, match="icem_plan: critic and value"):
        hplanner.icem_plan(eng, prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N, critic=crt,
                           value=HipEngine.value_params((8,), "relu", 1.0))
    args = (None, None, None, None, None, None, None, None, None, None, None, None, None, None, HipEngine.icem_params(), prob["obs"],
            prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"], N)
    out = _np(eng.critic_plan(crt, None, *args, seed=1, call=1))
    assert np.isfinite(out).all() and np.abs(out).max() <= 1.0


def test_refusals_at_construction(gpu, monkeypatch):
    """`cem_terminal_q` is refused where the other `cem_*` options are: use_cem=False, a discrete env, a process group of more than one
    rank; together with `cem_terminal_value`; nets of other sizes, another activation or another count than declared are refused when
    they are set."""
    from cadm_amd.envs import make_env_spec
    tq = dict(hidden_sizes=(16,), activation="tanh", policy=dict(hidden_sizes=(8,)))
    with pytest.raises(ValueError, match="need use_cem=True"):
        plan_model(True, 5, use_cem=False, cem_terminal_q=tq)
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        plan_model(True, 5, env=make_env_spec("cartpole"), cem_terminal_q=tq)
    with pytest.raises(ValueError, match="one terminal term"):
        plan_model(True, 5, cem_terminal_q=tq, cem_terminal_value=dict(hidden_sizes=(8,)))
    model, _ = plan_model(False, 5, cem_terminal_q=tq)
    good = cref.he_critics(18, 6, (16,), 2, 0)
    with pytest.raises(ValueError, match="activation"):
        model.set_critics([vref.sequential(c, "relu") for c in good])
    with pytest.raises(ValueError, match="layer 0 of critic 1 is"):
        model.set_critics([good[0], vref.he_net(24, (24,), 0)])
    with pytest.raises(ValueError, match="3 nets given"):
        model.set_critics(good + good[:1])
    with pytest.raises(ValueError, match="in_std"):
        model.set_critics(good, in_std=np.zeros(24))
    assert not model._critics_set
    import torch.distributed as dist
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        plan_model(True, 5, process_group=object(), cem_terminal_q=tq)
