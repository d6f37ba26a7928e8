"""CPU: the restatement of `imagine`'s select stage (tests/imagine_ref.py) -- the draw and its uniformity, hand-made cases of the state
machine -- and the pure parsers of `model.imagine`'s arguments and of the `imagine_policy` kwarg (cadm_amd/planner.py), with the constants
the sources and the binding must agree on.  The GPU tests hold the kernel to the restatement (tests/test_gpu_imagine.py)."""
import os
import re

import numpy as np
import pytest

import imagine_ref as iref
from cadm_amd import _lib
from cadm_amd import planner as hplanner

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---------------------------------------------------------------------------------------------------------------------- the stage's groups
def test_group_rule():
    """`imagine_ref.group` / `lds_bytes`, the restated `img_group` / `img_lds_bytes` of csrc/imagine.hip (whose constants the restatement
    carries), on the engines of tests/test_gpu_imagine_envelope.py: the budget of 12288 floats cuts the group to 7, 13, 8 and 2, the 37
    rows of the stage test fall into the groups the table names -- every one with a partial last group --, p = 255 at D = 48 fits no
    row; and the engines of tests/test_gpu_imagine.py keep the full 16."""
    src = _src("cadm_amd", "csrc", "imagine.hip")
    assert int(re.search(r"IMG_GROUP = (\d+);", src).group(1)) == iref.GROUP
    assert re.search(r"IMG_LDS_BUDGET = 48 \* 1024;", src) and iref.LDS_BUDGET == 48 * 1024
    for name, (_, D, p, G, groups) in iref.STAGE_ENGINES.items():
        assert iref.group(p, D) == G, name
        if G:
            assert iref.lds_bytes(G, p, D) <= iref.LDS_BUDGET < iref.lds_bytes(G + 1, p, D) and G < iref.GROUP
            assert [min(G, 37 - r) for r in range(0, 37, G)] == groups and sum(groups) == 37 and groups[-1] < G and iref.STAGE_AT.get(name, 100) % G != 0
    floats = lambda G, p, D: iref.lds_bytes(G, p, D) // 4
    assert (floats(7, 35, 45), floats(13, 50, 18), floats(8, 30, 48), floats(2, 125, 48)) == (11399, 11969, 11960, 12146)
    assert floats(1, 255, 48) == 12337 > 12288 == iref.LDS_BUDGET // 4
    assert 35 * 45 % 2 == 1 and sorted({(r * 35 * 45) % 4 for r in range(0, 37, 7)}) == [0, 1, 2, 3], "slim35: group starts of every alignment"
    assert 125 > 256 // 48 and 50 > 256 // 18 and 30 > 256 // 48 and 35 > 256 // 45, "p > S: the broadcast walk carries"
    for p, D in ((5, 3), (5, 11), (5, 48), (20, 18)):
        assert iref.group(p, D) == 16
    assert iref.group(685, 18) == 0 and iref.group(680, 18) == 1      # halfcheetah: the first p (a multiple of E = 5) that fits no row


# ---------------------------------------------------------------------------------------------------------------------- the draw
@pytest.mark.parametrize("p", [1, 5, 20])
def test_draw_is_in_range(p):
    """sel = (uint64(w0) * p) >> 32 lies in 0 .. p - 1 for every word, at the ends of the word range and for the words of a call"""
    assert int(iref.select(np.uint32(0xFFFFFFFF), p)) == p - 1
    assert int(iref.select(np.uint32(0), p)) == 0
    edge = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    s = iref.select(edge, p)
    assert s.dtype == np.int32 and s.min() >= 0 and s.max() <= p - 1 and (np.diff(s) >= 0).all()
    d = iref.draws(3, 2, 4, 9, 3, p)
    assert d.shape == (3, 4, 9) and d.min() >= 0 and d.max() <= p - 1
    if p > 1:
        assert len(np.unique(d)) == p


@pytest.mark.parametrize("seed,call,m,n,k,p", [(7, 0, 3, 64, 4, 5), (7, 0, 3, 64, 4, 20), (7, 1, 3, 64, 4, 5)])
def test_draw_is_uniform(seed, call, m, n, k, p):
    """Every particle's count over the N = m n k = 768 draws of a call lies within 4 sigma of N / p, sigma^2 = N (1 / p)(1 - 1 / p).  The
    restatement gives 1.66, 1.76 and 0.85 sigma at these three keys, so the condition holds for the reference alone."""
    s = iref.draws(seed, call, m, n, k, p)
    N = s.size
    assert N == 768
    counts = np.bincount(s.reshape(-1), minlength=p)
    sigma = np.sqrt(N * (1.0 / p) * (1.0 - 1.0 / p))
    worst = np.abs(counts - N / p).max() / sigma
    print("\n[seed %d call %d p %d] worst |count - N / p| = %.2f sigma" % (seed, call, p, worst))
    assert worst <= 4.0


def test_draw_depends_on_row_step_and_key():
    a = iref.words(7, 0, np.arange(64), 0)
    assert len(np.unique(a)) == 64
    assert (a != iref.words(7, 0, np.arange(64), 1)).all() and (a != iref.words(7, 1, np.arange(64), 0)).all()
    assert (a != iref.words(8, 0, np.arange(64), 0)).all()
    # the words of a batch are the words of its rows: a row's draw does not depend on m or n
    np.testing.assert_array_equal(iref.draws(7, 0, 3, 4, 2, 5).reshape(2, 12)[:, :8], iref.draws(7, 0, 2, 4, 2, 5).reshape(2, 8))


# ---------------------------------------------------------------------------------------------------------------------- the state machine
def _case():
    """k = 3 steps, three rows, p = E = 5, D = 3; the constraint: dim 0 < 1.  Row 0 lands ON the bound at t = 1; row 1's selected particle
    is NaN at t = 0; row 2 has a NaN in a particle that is not selected at t = 0."""
    rng = np.random.default_rng(0)
    k, R, p, D = 3, 3, 5, 3
    nexts = (0.1 * rng.standard_normal((k, R, p, D))).astype(F)
    rows1s = rng.standard_normal((k, R, p)).astype(F)
    sels = np.array([[1, 2, 3], [4, 0, 1], [0, 1, 2]], np.int32)
    nexts[1, 0, 4, 0] = 1.0
    nexts[0, 1, 2, 1] = np.nan
    nexts[0, 2, 0, 2] = np.nan
    state0 = (0.1 * rng.standard_normal((R, D))).astype(F)
    return state0, nexts, rows1s, sels, [dict(dim=0, hi=1.0)]


def test_state_machine_hand_made_cases():
    state0, nexts, rows1s, sels, cons = _case()
    o = iref.run_steps(state0, nexts, rows1s, sels, 5, cons)
    # row 0: terminates at t = 1 (a value equal to the bound violates), frozen afterwards
    assert o["valid"][:, 0].tolist() == [1, 1, 0] and o["done"][:, 0].tolist() == [0, 1, 0] and o["length"][0] == 2
    np.testing.assert_array_equal(o["states"][1, 0], nexts[0, 0, 1])
    np.testing.assert_array_equal(o["states"][2, 0], nexts[1, 0, 4])
    np.testing.assert_array_equal(o["states"][3, 0], o["states"][2, 0])
    assert o["rew"][1, 0] == rows1s[1, 0, 4] and o["rew"][2, 0] == 0 and o["member"][:, 0].tolist() == [1, 4, -1]
    assert o["disagreement"][2, 0] == 0 and o["disagreement"][1, 0] > 0
    # row 1: the selected particle is NaN at t = 0: no valid transition, never done, frozen at the start state
    assert o["valid"][:, 1].tolist() == [0, 0, 0] and o["done"][:, 1].tolist() == [0, 0, 0] and o["length"][1] == 0
    for t in range(1, 4):
        np.testing.assert_array_equal(o["states"][t, 1], state0[1])
    assert (o["rew"][:, 1] == 0).all() and o["member"][:, 1].tolist() == [2, -1, -1]
    assert o["disagreement"][0, 1] == np.inf and (o["disagreement"][1:, 1] == 0).all()
    # row 2: a NaN in a particle that was not selected: the row lives on, the disagreement of that step is +inf
    assert o["valid"][:, 2].tolist() == [1, 1, 1] and o["done"][:, 2].sum() == 0 and o["length"][2] == 3
    assert o["disagreement"][0, 2] == np.inf and np.isfinite(o["disagreement"][1:, 2]).all()
    np.testing.assert_array_equal(o["states"][1, 2], nexts[0, 2, 3])
    assert np.isfinite(o["states"]).all(), "nothing non-finite is ever fed back"
    assert o["alive"].tolist() == [0, 0, 1]
    # without the constraint row 0 lives on
    free = iref.run_steps(state0, nexts, rows1s, sels, 5, None)
    assert free["valid"][:, 0].tolist() == [1, 1, 1] and free["done"].sum() == 0


def test_select_step_broadcast_health_and_weights():
    rng = np.random.default_rng(1)
    R, p, D, E = 4, 20, 3, 5
    nxt = rng.standard_normal((R, p, D)).astype(F)
    rows1 = rng.standard_normal((R, p)).astype(F)
    state = rng.standard_normal((R, D)).astype(F)
    sel = np.array([0, 19, 7, 12], np.int32)
    o = iref.select_step(nxt, rows1, state, np.array([1, 1, 0, 1], np.uint8), sel, E)
    assert o["member"].tolist() == [0, 4, -1, 3]                # member = sel / (p / E); the dead row has none
    np.testing.assert_array_equal(o["bcast"], np.repeat(o["state"][:, None], p, axis=1))
    np.testing.assert_array_equal(o["state"][2], state[2])
    np.testing.assert_array_equal(o["state"][3], nxt[3, 12])
    # the disagreement is the weighted epistemic variance: against float64 at the uncertainty term's own derived bound
    import uncertainty_ref as uref
    w = np.array([0.5, 0.0, 2.0], F)
    u = iref.disagreement(nxt, E, w)
    u64, _, B, _ = uref.cost(nxt[None, :, None], E, "epistemic", w=w)
    assert (np.abs(u - u64[:, 0, 0]) <= B[:, 0, 0]).all() and (u > 0).all()
    # dims with w == 0 are not read: a NaN there changes nothing
    bad = nxt.copy()
    bad[:, 3, 1] = np.nan
    np.testing.assert_array_equal(iref.disagreement(bad, E, w), u)
    # the health test: strict on both sides, NaN and inf in a constrained dim violate, other dims are not looked at
    x = np.array([[0.0, 5.0, 0.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.5, np.inf, 0.0]], F)
    assert iref.healthy(x, [dict(dim=0, lo=-1.0, hi=1.0)]).tolist() == [True, False, False, False, True]
    assert iref.healthy(x, None).all()


# ---------------------------------------------------------------------------------------------------------------------- the parsers
KW = dict(obs_dim=18, action_dim=6, n_particles=5, policy_registered=True)


def test_imagine_args_are_parsed():
    obs = np.zeros((4, 18), F)
    a = hplanner.imagine_args(obs, horizon=3, branches=2, noise_std=0.1, **KW)
    assert a == hplanner.ImagineArgs(4, 2, 3, float(F(0.1)), None)
    a = hplanner.imagine_args(obs, horizon=np.int64(2), actions=np.zeros((4, 1, 2, 6), F), **dict(KW, policy_registered=False))
    assert (a.m, a.n, a.k, a.noise_std) == (4, 1, 2, 0.0)
    assert hplanner.imagine_args(obs, disagreement_w="delta_std", **KW).w == "delta_std"
    w = hplanner.imagine_args(obs, disagreement_w=np.arange(1, 19), **KW).w
    assert w.dtype == F and w.shape == (18,)
    hist = (np.zeros((4, 18 * 10), F), np.zeros((4, 6 * 10), F))
    assert hplanner.imagine_args(obs, *hist, context=True, history_length=10, **KW).m == 4
    import torch
    assert hplanner.imagine_args(torch.zeros((2, 18)), **KW).m == 2
    assert hplanner.imagine_args(obs, horizon=hplanner.IMAGINE_MAX_STEPS, **KW).k == (_lib.POLICY_IT - _lib.IMAGINE_IT) // 2


def test_imagine_args_refusals():
    obs = np.zeros((4, 18), F)
    acts = np.zeros((4, 2, 3, 6), F)
    no_pol = dict(KW, policy_registered=False)

    def bad(match, *a, exc=ValueError, **k):
        with pytest.raises(exc, match=match):
            hplanner.imagine_args(*a, **k)
    for v in (0, -1, 1.5, True, None):
        bad("horizon must be", obs, horizon=v, **KW)
        bad("branches must be", obs, branches=v, **KW)
    bad("neither a registered policy", obs, **no_pol)
    bad("one source of actions", obs, horizon=3, branches=2, actions=acts, **KW)
    bad(r"actions \(4, 2, 3, 6\)", obs, horizon=3, branches=1, actions=acts, **no_pol)
    bad(r"actions \(4, 2, 3, 6\)", obs, horizon=2, branches=2, actions=acts, **no_pol)
    bad(r"obs \(4, 17\)", np.zeros((4, 17), F), **KW)
    bad(r"obs \(18,\)", np.zeros((18,), F), **KW)
    bad(r"obs \(0, 18\)", np.zeros((0, 18), F), **KW)
    for poison in (np.nan, np.inf, -np.inf):
        x = obs.copy()
        x[2, 5] = poison
        bad("non-finite", x, **KW)
    bad("cp_obs and cp_act are required", obs, context=True, history_length=10, **KW)
    bad("cp_obs and cp_act are required", obs, np.zeros((4, 180), F), None, context=True, history_length=10, **KW)
    bad("cp_obs", obs, np.zeros((4, 179), F), np.zeros((4, 60), F), context=True, history_length=10, **KW)
    bad("cp_obs", obs, np.zeros((3, 180), F), np.zeros((4, 60), F), context=True, history_length=10, **KW)
    bad("no context encoder", obs, np.zeros((4, 180), F), np.zeros((4, 60), F), **KW)
    bad("discrete", obs, discrete=True, exc=NotImplementedError, **KW)
    bad("more than one rank", obs, world=2, exc=NotImplementedError, **KW)
    for v in (-0.1, np.nan, np.inf, "a", True):
        bad("noise_std", obs, noise_std=v, **KW)
    bad("noise_std perturbs the policy", obs, horizon=3, branches=2, actions=acts, noise_std=0.1, **no_pol)
    # m n p rows beyond one rollout launch's 32-bit indexing: 4 * 2^24 * 5 * 18 >= 2^31
    bad("more than one rollout launch", obs, branches=1 << 24, **KW)
    bad("iteration words", obs, horizon=hplanner.IMAGINE_MAX_STEPS + 1, **KW)
    for v in ("std", np.zeros(18), np.ones(17), -np.ones(18), np.full(18, np.nan), 2.0):
        bad("disagreement_w", obs, disagreement_w=v, **KW)


def test_imagine_policy_rules():
    """`imagine_policy` declares the actor of a model whose planner declares none: it builds the same `PolicyParams` a planner
    declaration would, is refused next to one, and is no planner option -- every cem_* kwarg at its default still means `_opt` None."""
    assert hplanner.imagine_policy_params(None) is None
    prm = hplanner.imagine_policy_params(dict(hidden_sizes=(64, 32), activation="tanh", squash="none"), None, obs_dim=18, action_dim=6)
    assert isinstance(prm, _lib.PolicyParams)
    assert (prm.n_hidden, prm.hidden[0], prm.hidden[1], prm.n_samples, prm.noise_std) == (2, 64, 32, 1, 0.0)
    assert prm.activation == _lib.VALUE_ACTS["tanh"] and prm.squash == _lib.POLICY_SQUASH["none"]
    d = hplanner.imagine_policy_params({}, None)
    assert (d.n_hidden, d.hidden[0], d.hidden[1], d.squash) == (2, 256, 256, _lib.POLICY_SQUASH["tanh"])
    assert hplanner.PlanOptions.from_kwargs() is None      # imagine_policy is not among the planner's kwargs: nothing to make it non-None
    for bad in ((64,), dict(hidden=(64,)), dict(hidden_sizes=(64,), n_samples=4), dict(hidden_sizes=(64,), noise_std=0.1)):
        with pytest.raises(ValueError, match="imagine_policy must be"):
            hplanner.imagine_policy_params(bad)
    with pytest.raises(ValueError, match="hidden widths"):
        hplanner.imagine_policy_params(dict(hidden_sizes=(0,)))
    with pytest.raises(ValueError, match="squash"):
        hplanner.imagine_policy_params(dict(squash="sigmoid"))
    with pytest.raises(NotImplementedError, match="discrete"):
        hplanner.imagine_policy_params(dict(hidden_sizes=(8,)), discrete=True)
    with pytest.raises(ValueError, match="observation dims"):
        hplanner.imagine_policy_params(dict(hidden_sizes=(8,)), obs_dim=_lib.MAX_VALUE_DIMS + 1)
    with pytest.raises(ValueError, match="action dims"):
        hplanner.imagine_policy_params(dict(hidden_sizes=(8,)), action_dim=_lib.MAX_POLICY_ACTIONS + 1)
    pp = dict(hidden_sizes=(16,), activation="tanh", n_samples=4)
    prior = hplanner.PlanOptions.from_kwargs(use_cem=True, cem_policy_prior=pp, obs_dim=18, action_dim=6, n_forwards=5)
    q = hplanner.PlanOptions.from_kwargs(use_cem=True, cem_terminal_q=dict(policy=dict(hidden_sizes=(16,))), obs_dim=18, action_dim=6, n_forwards=5)
    for opt in (prior, q):
        with pytest.raises(ValueError, match="planner-declared actor"):
            hplanner.imagine_policy_params(dict(hidden_sizes=(16,)), opt)
    # an opt-in planner without an actor takes one
    plain = hplanner.PlanOptions.from_kwargs(use_cem=True, cem_noise_beta=1.0)
    assert plain.actor_params() is None and hplanner.imagine_policy_params(dict(hidden_sizes=(16,)), plain).hidden[0] == 16


# ---------------------------------------------------------------------------------------------------------------------- the constants
def test_sources_binding_and_restatement_agree():
    common, plan_h = _src("cadm_amd", "csrc", "common.h"), _src("cadm_amd", "csrc", "planner.h")
    assert int(re.search(r"#define CADM_STREAM_IMAGINE (\d+)u", common).group(1)) == iref.STREAM_IMAGINE == _lib.STREAM_IMAGINE == 6
    assert int(re.search(r"#define CADM_STREAM_IMAGINE_ACT (\d+)u", common).group(1)) == iref.STREAM_IMAGINE_ACT == _lib.STREAM_IMAGINE_ACT
    words = sorted(int(v) for v in re.findall(r"#define CADM_STREAM_[A-Z_]+ (\d+)u", common))
    assert len(set(words)) == len(words), "two streams share a word"
    it = int(re.search(r"#define CADM_IMAGINE_IT (0x[0-9A-Fa-f]+)", plan_h).group(1), 16)
    assert it == _lib.IMAGINE_IT == iref.IMAGINE_IT == hplanner.IMAGINE_IT
    assert it % 2 == 0 and 5 < it < _lib.POLICY_IT < hplanner.FORECAST_IT < 1 << 24      # a range of its own inside the word's 24 bits
    header = _src("include", "cadm_hip.h")
    assert int(re.search(r"#define CADM_IMAGINE_VIEWS (\d+)", header).group(1)) == _lib.IMAGINE_VIEWS
    assert re.search(r"#define CADM_ABI_VERSION 2\b", header)      # the ABI version is unchanged
    assert re.search(r"^SRCS := .*\bimagine\.hip\b", _src("cadm_amd", "csrc", "Makefile"), flags=re.M)
