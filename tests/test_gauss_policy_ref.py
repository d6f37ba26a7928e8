"""CPU: the stochastic actor head's declaration and its restatement (tests/gauss_policy_ref.py) -- `planner.policy_head_params`'
refusals, `planner.imagine_args`' new ones, the float64 log-density against torch.distributions (a Normal under a TanhTransform and an
AffineTransform in float64: an independent statement of the formula), the float32 emulation inside the bars the GPU test holds the
kernel to, and the slicing `set_policy` does on a SAC actor."""
import types

import numpy as np
import pytest
import torch

import gauss_policy_ref as gref
import policy_ref as pref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd.engine import HipEngine

pytestmark = pytest.mark.filterwarnings("ignore")

F = np.float32
KW = dict(obs_dim=18, action_dim=6, n_particles=5, policy_registered=True)


# ---------------------------------------------------------------------------------------------------------------------- 1: the declaration
def test_policy_head_params_are_parsed():
    assert hplanner.policy_head_params(None) is None
    assert hplanner.policy_head_params(None, has_actor=False, discrete=True, world=4) is None      # the default touches nothing
    p = hplanner.policy_head_params(dict(kind="gaussian"), has_actor=True)
    assert isinstance(p, _lib.PolicyHeadParams)
    assert (p.kind, p.bound, p.log_std_min, p.log_std_max) == (1, 0, -5.0, 2.0)
    p = hplanner.policy_head_params(dict(log_std_bounds=(-3, 0.5), log_std_bound="tanh"), has_actor=True)
    assert (p.kind, p.bound, p.log_std_min, p.log_std_max) == (_lib.HEAD_KINDS["gaussian"], _lib.LOGSTD_BOUNDS["tanh"], -3.0, 0.5)
    assert hplanner.policy_head_params(dict(log_std_bounds=(-20.0, 10.0)), has_actor=True).log_std_max == 10.0


@pytest.mark.parametrize("head,match", [
    (dict(kind="gaussian", scale=1.0), "policy_head must be"),
    (("gaussian",), "policy_head must be"),
    (dict(kind="beta"), "kind must be"),
    (dict(kind=1), "kind must be"),
    (dict(log_std_bound="clip"), "log_std_bound must be"),
    (dict(log_std_bounds=(-5.0, float("inf"))), "finite"),
    (dict(log_std_bounds=(float("nan"), 2.0)), "finite"),
    (dict(log_std_bounds=(-5.0,)), "two finite numbers"),
    (dict(log_std_bounds="ab"), "two finite numbers"),
    (dict(log_std_bounds=(2.0, 2.0)), "lo < hi"),
    (dict(log_std_bounds=(2.0, -5.0)), "lo < hi"),
    (dict(log_std_bounds=(-5.0, 10.5)), "beyond 10"),
])
def test_policy_head_params_refusals(head, match):
    with pytest.raises(ValueError, match=match):
        hplanner.policy_head_params(head, has_actor=True)


def test_policy_head_needs_an_actor_continuous_actions_and_one_rank():
    with pytest.raises(ValueError, match="needs a declared actor"):
        hplanner.policy_head_params(dict(kind="gaussian"), has_actor=False)
    with pytest.raises(NotImplementedError, match="discrete"):
        hplanner.policy_head_params(dict(kind="gaussian"), has_actor=True, discrete=True)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        hplanner.policy_head_params(dict(kind="gaussian"), has_actor=True, world=2)


def test_imagine_args_sample():
    obs = np.zeros((4, 18), F)
    head = dict(head_declared=True, head_registered=True)
    assert hplanner.imagine_args(obs, **KW).sample is False                       # no head: today's route, whatever else
    assert hplanner.imagine_args(obs, sample=False, **KW).sample is False
    assert hplanner.imagine_args(obs, **KW, **head).sample is True                # None: a declared head and no actions
    assert hplanner.imagine_args(obs, sample=False, noise_std=0.2, **KW, **head) == hplanner.ImagineArgs(4, 1, 1, float(F(0.2)), None, False)
    assert hplanner.imagine_args(obs, sample=True, horizon=3, branches=2, **KW, **head) == hplanner.ImagineArgs(4, 2, 3, 0.0, None, True)
    acts = np.zeros((4, 1, 1, 6), F)
    given = dict(KW, policy_registered=False)
    assert hplanner.imagine_args(obs, actions=acts, **given, head_declared=True).sample is False      # None with actions: not sampled
    with pytest.raises(ValueError, match="sample=True"):
        hplanner.imagine_args(obs, actions=acts, sample=True, **given, head_declared=True)
    with pytest.raises(ValueError, match="noise_std perturbs the mode"):
        hplanner.imagine_args(obs, sample=True, noise_std=0.1, **KW, **head)
    with pytest.raises(ValueError, match="noise_std perturbs the mode"):
        hplanner.imagine_args(obs, noise_std=0.1, **KW, **head)                   # None is True here, and refuses likewise
    with pytest.raises(ValueError, match="needs a registered Gaussian head"):
        hplanner.imagine_args(obs, sample=True, **KW)
    with pytest.raises(ValueError, match="needs a registered Gaussian head"):
        hplanner.imagine_args(obs, sample=True, **KW, head_declared=True)
    with pytest.raises(ValueError, match="sample must be"):
        hplanner.imagine_args(obs, sample=1, **KW, **head)


# ---------------------------------------------------------------------------------------------------------------------- 2: the formula
def _case(A, hidden, act, lo, hi, R=64, seed=3):
    D = 7
    x = np.random.default_rng(seed).standard_normal((R, D)).astype(F)
    layers = gref.actor(D, hidden, A, act, x, lo, hi, seed=seed)
    return x, layers, gref.xi(5, 9, np.arange(R) + 11, 2, A), gref.xi_radius(5, 9, np.arange(R) + 11, 2, A)


@pytest.mark.parametrize("bound", gref.BOUNDS)
@pytest.mark.parametrize("squash", pref.SQUASH)
def test_float64_logp_against_torch_distributions(squash, bound):
    """The restatement's log-density is the density of a = affine(tanh(u)), u ~ N(mu, sig), as torch.distributions states it in float64:
    row by row through the transforms' own log-det-Jacobians at 1e-9, and dim by dim through TransformedDistribution.log_prob of the
    action itself wherever |u| < 4 (the inverse through atanh is then exact enough for 1e-9)."""
    from torch.distributions import AffineTransform, Normal, TanhTransform, TransformedDistribution
    lo, hi, lb, ub = -3.0, 0.5, -0.5, 2.0
    x, layers, e, _ = _case(6, (33, 70), "tanh", lo, hi)
    ref = gref.sample64(gref.z64(x, layers, "tanh"), e, squash, bound, lo, hi, lb, ub)
    mu = torch.as_tensor(gref.z64(x, layers, "tanh")[:, :6])
    sig, u = torch.as_tensor(ref["sig"]), torch.as_tensor(ref["u"])
    base = Normal(mu, sig)
    assert mu.dtype == torch.float64 and sig.dtype == torch.float64
    if squash == "tanh":
        mid, half = 0.5 * (ub + lb), 0.5 * (ub - lb)
        tt, at = TanhTransform(), AffineTransform(mid, half)
        y = tt(u)
        terms = base.log_prob(u) - tt.log_abs_det_jacobian(u, y) - at.log_abs_det_jacobian(y, at(y))
        direct = TransformedDistribution(base, [tt, at]).log_prob(at(y))
        near = (u.abs() < 4.0).numpy()
        assert near.mean() > 0.5
        np.testing.assert_allclose(ref["term"][near], direct.numpy()[near], rtol=0, atol=1e-9)
        np.testing.assert_allclose(ref["act"], np.clip(at(y).numpy(), lb, ub), rtol=0, atol=1e-12)
    else:
        terms = base.log_prob(u)
        np.testing.assert_allclose(ref["act"], np.clip(u.numpy(), lb, ub), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref["term"], terms.numpy(), rtol=0, atol=1e-9)
    np.testing.assert_allclose(ref["logp"], terms.sum(-1).numpy(), rtol=0, atol=1e-9)


@pytest.mark.parametrize("bound", gref.BOUNDS)
@pytest.mark.parametrize("squash", pref.SQUASH)
@pytest.mark.parametrize("A,hidden,act", [(1, (), "relu"), (6, (33, 70), "swish"), (24, (50,), "tanh")], ids=["A1-linear", "A6-33x70", "A24-50"])
def test_float32_emulation_is_inside_the_bars(A, hidden, act, squash, bound):
    """The float32 walk of the arithmetic against the float64 restatement, under the bars of `gref.bars` -- with the oracle's own draws on
    both sides, so the draw's share of the bars is slack here -- and the shares of the raw log-std the GPU test relies on."""
    lo, hi = -3.0, 0.5
    x, layers, e, r = _case(A, hidden, act, lo, hi)
    zr = gref.z64(x, layers, act)
    below, above, inside = gref.shares(zr[:, A:], lo, hi)
    assert below >= 0.1 and above >= 0.1 and inside >= 0.5, (below, above, inside)
    ref = gref.sample64(zr, e, squash, bound, lo, hi)
    got = gref.sample32(gref.z32(x, layers, act), e, squash, bound, lo, hi)
    act_bar, logp_bar = gref.bars(zr, ref, e, r, squash, bound, lo, hi)
    assert np.isfinite(got["logp"]).all() and np.isfinite(ref["logp"]).all()
    ra = np.abs(got["act"].astype(np.float64) - ref["act"]) / act_bar
    rl = np.abs(got["logp"].astype(np.float64) - ref["logp"]) / logp_bar
    print("\n[A=%d %s %s %s] worst |act err| / bar %.3f, |logp err| / bar %.3f" % (A, act, squash, bound, ra.max(), rl.max()))
    assert ra.max() <= 1.0 and rl.max() <= 1.0
    np.testing.assert_allclose(got["mode"], pref.action64(x, gref.split(layers, A)[0], act, squash), rtol=0, atol=2e-5)


def test_draws_are_their_own_stream():
    """word 8: not the proposals' noise (5) nor imagine's (7) under the same key, and a function of (seed, call, row, t) alone"""
    import imagine_ref as iref
    a = gref.xi(3, 4, np.arange(10), 1, 6)
    assert a.shape == (10, 6) and a.dtype == F and np.isfinite(a).all()
    assert not np.array_equal(a, iref.xi(3, 4, 10, 1, 6).reshape(10, 6))
    assert not np.array_equal(a, pref.xi(3, 4, 10, 1, 1, 6).reshape(10, 6))
    np.testing.assert_array_equal(gref.xi(3, 4, np.arange(5, 10), 1, 6), a[5:])
    np.testing.assert_array_equal(gref.xi(3, 4, np.arange(10), 1, 1)[:, 0], a[:, 0])      # A = 1: z0 of words (0, 1) alone
    for other in (gref.xi(4, 4, np.arange(10), 1, 6), gref.xi(3, 5, np.arange(10), 1, 6), gref.xi(3, 4, np.arange(10), 2, 6)):
        assert not np.array_equal(other, a)


# ---------------------------------------------------------------------------------------------------------------------- 3: the slicing
def test_split_gaussian_layers():
    layers = pref.he_policy(18, (16, 8), 12, 4)
    mean, W_ls, b_ls = hplanner.split_gaussian_layers(layers, 6)
    want, W_want, b_want = gref.split(layers, 6)
    assert len(mean) == 3 and mean[0] is layers[0] and mean[1] is layers[1]
    np.testing.assert_array_equal(mean[2][0], layers[2][0][:, :6])
    np.testing.assert_array_equal(mean[2][1], layers[2][1][:6])
    np.testing.assert_array_equal(W_ls, layers[2][0][:, 6:])
    np.testing.assert_array_equal(b_ls, layers[2][1][6:])
    np.testing.assert_array_equal(W_ls, W_want)
    np.testing.assert_array_equal(b_ls, b_want)
    assert mean[2][0].flags.c_contiguous and W_ls.flags.c_contiguous
    for bad in (pref.he_policy(18, (16,), 6, 4), pref.he_policy(18, (16,), 13, 4), []):
        with pytest.raises(ValueError, match="2 A = 12|no layers"):
            hplanner.split_gaussian_layers(bad, 6)


class _Recorder:
    def __init__(self):
        self.calls = []

    def set_policy_net(self, params, *given):
        self.calls.append(("net", params, given))

    def set_policy_head(self, params, *given):
        self.calls.append(("head", params, given))


def _stub(head):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as Model
    prm = HipEngine.policy_params((16,), "tanh", "tanh", 1, 0.0)
    stub = types.SimpleNamespace(_opt=None, _imagine_policy=prm, _policy_head=head, _policy_set=False, _head_set=False,
                                 action_space_dims=6, engine=_Recorder(), _actor_params=lambda: prm)
    return Model, stub, prm


def test_set_policy_hands_on_the_hand_sliced_net():
    """`set_policy` on a model with a head: the mean columns go through the existing registration, unchanged in every other respect,
    the log-std columns through `set_policy_head`; a torch module as SAC code has it gives the same arrays; without a head the call is
    today's; `clear_policy` clears both flags."""
    head = hplanner.policy_head_params(dict(kind="gaussian", log_std_bound="tanh"), has_actor=True)
    Model, stub, prm = _stub(head)
    layers = pref.he_policy(18, (16,), 12, 4)
    mean = np.arange(18, dtype=F)
    Model.set_policy(stub, layers, obs_mean=mean)
    (k0, p0, g0), (k1, p1, g1) = stub.engine.calls
    assert (k0, k1) == ("net", "head") and p0 is prm and p1 is head and stub._policy_set and stub._head_set
    want, W_want, b_want = gref.split(layers, 6)
    got_layers, got_mean, got_std = g0
    assert got_mean is mean and got_std is None and len(got_layers) == 2
    for (w, b), (w2, b2) in zip(got_layers, want):
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(b, b2)
    np.testing.assert_array_equal(g1[0], W_want)
    np.testing.assert_array_equal(g1[1], b_want)
    # the module SAC code holds: Linear.weight is [out, in], chunk(2, -1) of its output is (mean, log-std)
    net = torch.nn.Sequential(torch.nn.Linear(18, 16), torch.nn.Tanh(), torch.nn.Linear(16, 12))
    with torch.no_grad():
        net[0].weight.copy_(torch.as_tensor(layers[0][0].T)); net[0].bias.copy_(torch.as_tensor(layers[0][1]))
        net[2].weight.copy_(torch.as_tensor(layers[1][0].T)); net[2].bias.copy_(torch.as_tensor(layers[1][1]))
    stub.engine.calls.clear()
    Model.set_policy(stub, net)
    np.testing.assert_array_equal(stub.engine.calls[0][2][0][1][0], want[1][0])
    np.testing.assert_array_equal(stub.engine.calls[1][2][0], W_want)
    x = torch.randn(5, 18)
    mu, _ = net(x).chunk(2, -1)
    np.testing.assert_allclose(mu.detach().numpy(), np.tanh(x.numpy() @ want[0][0] + want[0][1]) @ want[1][0] + want[1][1], atol=1e-5)
    with pytest.raises(ValueError, match="not the declared one"):
        Model.set_policy(stub, torch.nn.Sequential(torch.nn.Linear(18, 16), torch.nn.ReLU(), torch.nn.Linear(16, 12)))
    with pytest.raises(ValueError, match="2 A = 12"):
        Model.set_policy(stub, pref.he_policy(18, (16,), 6, 4))
    Model.clear_policy(stub)
    assert stub.engine.calls[-1][:2] == ("net", None) and not stub._policy_set and not stub._head_set
    # no head: the one existing call, given what the caller gave
    Model, plain, prm = _stub(None)
    six = pref.he_policy(18, (16,), 6, 4)
    Model.set_policy(plain, six)
    assert plain.engine.calls == [("net", prm, (six, None, None))]
