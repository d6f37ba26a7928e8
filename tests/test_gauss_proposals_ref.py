"""CPU: proposals of the policy prior drawn from the actor's Gaussian head -- the parsing of `cem_policy_prior`'s `proposals` / `std_scale`
and every refusal (pure functions, no GPU), the float32 restatement of a sampled proposal step against the float64 one under the bar
the GPU test holds the kernel to (tests/gauss_proposals_ref.py), the shares of the raw log-std that exercise both clamp branches and the
interior, the CPU half of the bitwise anchor (a zero log-std layer: the head route is the noise route), and the C header's declaration."""
import os
import re

import numpy as np
import pytest

import gauss_policy_ref as gref
import gauss_proposals_ref as gp
import policy_ref as pref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd.engine import HipEngine
from cadm_amd.planner import PlanOptions

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = dict(hidden_sizes=(16,), activation="tanh", n_samples=4)


def _opt(**prior):
    return PlanOptions.from_kwargs(use_cem=True, cem_policy_prior=dict(NET, **prior), obs_dim=18, action_dim=6)


# ---------------------------------------------------------------------------------------------------------------------- parsing, refusals
def test_new_keys_are_parsed():
    opt = _opt()
    assert (opt.proposals, opt.std_scale) == ("noise", 1.0) and opt.policy == ((16,), "tanh", "tanh", 4, 0.0)
    assert hplanner.policy_proposals_setting(opt) == ("noise", 1.0)
    opt = _opt(proposals="head", std_scale=0.5)
    assert (opt.proposals, opt.std_scale) == ("head", 0.5) and len(opt.policy) == 5 and opt.policy_params.noise_std == 0.0
    assert hplanner.policy_proposals_setting(opt, head_declared=True) == ("head", 0.5)
    assert _opt(proposals="head", std_scale=0).std_scale == 0.0
    assert _opt(proposals="head", std_scale=np.float32(0.1)).std_scale == float(F(0.1))      # what the library is handed
    assert _opt(proposals="noise", noise_std=0.3, std_scale=1).policy[4] == float(F(0.3))
    # a model without a prior sets nothing; the fields sit in front of the ones existing tests count from the end
    assert hplanner.policy_proposals_setting(None) is None
    assert hplanner.policy_proposals_setting(PlanOptions.from_kwargs(use_cem=True, cem_noise_beta=1.0)) is None
    assert PlanOptions(*range(18)).proposals == "noise" and PlanOptions(*range(18)).std_scale == 1.0
    assert HipEngine.policy_proposals_args() == (_lib.PROPOSALS["noise"], 1.0)
    assert HipEngine.policy_proposals_args("head", 2) == (_lib.PROPOSALS["head"], 2.0)


@pytest.mark.parametrize("prior,match", [
    (dict(proposals="mode"), "proposals must be"),
    (dict(proposals=1), "proposals must be"),
    (dict(proposals=None), "proposals must be"),
    (dict(proposals="head", noise_std=0.3), "one source"),
    (dict(std_scale=0.5), "std_scale"),
    (dict(proposals="noise", std_scale=2.0), "std_scale"),
    (dict(proposals="head", std_scale=-0.1), "std_scale must be a finite number >= 0"),
    (dict(proposals="head", std_scale=float("nan")), "std_scale must be a finite number >= 0"),
    (dict(proposals="head", std_scale=float("inf")), "std_scale must be a finite number >= 0"),
    (dict(proposals="head", std_scale=True), "std_scale must be a finite number >= 0"),
    (dict(proposals="head", std_scale="1"), "std_scale must be a finite number >= 0"),
    (dict(proposals="head", scale=1.0), "cem_policy_prior must be dict"),
])
def test_refusals(prior, match):
    with pytest.raises(ValueError, match=match):
        _opt(**prior)


def test_head_proposals_need_a_declared_head():
    opt = _opt(proposals="head")
    with pytest.raises(ValueError, match="declare policy_head"):
        hplanner.policy_proposals_setting(opt, head_declared=False)
    with pytest.raises(ValueError, match="declare policy_head"):
        hplanner.policy_proposals_setting(opt)
    assert hplanner.policy_proposals_setting(_opt(), head_declared=False) == ("noise", 1.0)      # the noise route needs none


def test_header_declares_the_call_and_the_binding_types_it():
    src = open(os.path.join(ROOT, "include", "cadm_hip.h")).read()
    assert re.search(r"int cadm_set_policy_proposals\(cadm_ctx\* ctx, int32_t source, float std_scale\);", src)
    for name, v in _lib.PROPOSALS.items():
        assert re.search(r"#define CADM_PROPOSE_%s %d\b" % (name.upper(), v), src)
    assert re.search(r"#define CADM_ABI_VERSION 2\b", src)      # the ABI version is unchanged: no struct changed its layout
    assert "cadm_set_policy_proposals" in _lib.SIGNATURES


# ---------------------------------------------------------------------------------------------------------------------- the restatement
def _case(name, D, A, t=1):
    est = pref.particle_mean32(gp.states(gp.M, gp.P, gp.NP, D, seed=A))
    layers = gref.actor(D, gp.HIDDEN, A, gp.ACT, est.reshape(-1, D), gp.LO, gp.HI, seed=A)
    return est, layers


@pytest.mark.parametrize("std_scale", [1.0, 0.5, 2.0])
@pytest.mark.parametrize("bound", gref.BOUNDS)
@pytest.mark.parametrize("squash", pref.SQUASH)
@pytest.mark.parametrize("name,D,A", gp.SHAPES)
def test_float32_restatement_is_inside_the_bar(name, D, A, squash, bound, std_scale):
    """The float32 walk against the float64 restatement under `gp.bar`, on the shapes, the net, the bounds and the draws the GPU test
    uses, with the oracle's own draws on both sides (the draw's share of the bar is slack here): the reference alone leaves room."""
    est, layers = _case(name, D, A)
    worst = 0.0
    for t in range(gp.H):
        xi, r = gp.draws(gp.SEED, gp.CALL, gp.M, gp.P, t, A, std_scale)
        ref = gp.step64(est, layers, gp.ACT, squash, bound, gp.LO, gp.HI, xi, std_scale)
        got = gp.step32(est, layers, gp.ACT, squash, bound, gp.LO, gp.HI, xi, std_scale)
        assert got.dtype == F and got.shape == (gp.M, gp.P, A) and np.abs(got).max() <= 1.0
        ratio = np.abs(got.astype(np.float64) - ref["act"]) / gp.bar(ref, xi, r, squash, bound, gp.LO, gp.HI)
        worst = max(worst, float(ratio.max()))
        assert (ref["sig"][:, 0] == 0).all() and (ref["sig"][:, 1:] > 0).all()
        if squash == "none":
            assert not np.array_equal(got[:, 1], got[:, 0])
    print("\n[%s %s %s x%g] worst |float32 - float64| / bar %.3f" % (name, squash, bound, std_scale, worst))
    assert worst <= 1.0, "the reference itself takes %.2f of the bar" % worst


@pytest.mark.parametrize("name,D,A", gp.SHAPES)
def test_log_std_shares(name, D, A):
    """With `gref.actor`'s calibrated log-std columns a share of the raw l lies below lo, a share above hi and a share strictly inside:
    both clamp branches and the interior are exercised"""
    est, layers = _case(name, D, A)
    l = gref.z64(est, layers, gp.ACT)[..., A:]
    below, above, inside = gref.shares(l, gp.LO, gp.HI)
    assert below >= 0.1 and above >= 0.1 and inside >= 0.4, (below, above, inside)


def test_std_scale_zero_and_sequence_zero_draw_nothing():
    name, D, A = gp.SHAPES[1]
    est, layers = _case(name, D, A)
    mean_layers, _, _ = gref.split(layers, A)
    xi, r = gp.draws(gp.SEED, gp.CALL, gp.M, gp.P, 2, A, 0.0)
    assert not xi.any() and not r.any()
    quiet = gp.step32(est, layers, gp.ACT, "tanh", "clamp", gp.LO, gp.HI, xi, 0.0)
    mode = pref.emulate32(est, mean_layers, gp.ACT, "tanh")
    np.testing.assert_array_equal(quiet.view(np.uint32), mode.view(np.uint32))
    xi, _ = gp.draws(gp.SEED, gp.CALL, gp.M, gp.P, 2, A, 1.0)
    loud = gp.step32(est, layers, gp.ACT, "tanh", "clamp", gp.LO, gp.HI, xi, 1.0)
    np.testing.assert_array_equal(loud[:, 0].view(np.uint32), mode[:, 0].view(np.uint32))
    assert (loud[:, 1:] != mode[:, 1:]).all()


def test_a_poisoned_estimate_takes_the_fallback():
    name, D, A = gp.SHAPES[1]
    est, layers = _case(name, D, A)
    bad = est.copy()
    bad[1, 2, 5] = np.nan
    xi, r = gp.draws(gp.SEED, gp.CALL, gp.M, gp.P, 1, A)
    clean = gp.step32(est, layers, gp.ACT, "tanh", "tanh", gp.LO, gp.HI, xi, 1.0)
    got = gp.step32(bad, layers, gp.ACT, "tanh", "tanh", gp.LO, gp.HI, xi, 1.0)
    assert (got[1, 2] == pref.fallback(-1.0, 1.0)).all() and (gp.step64(bad, layers, gp.ACT, "tanh", "tanh", gp.LO, gp.HI, xi, 1.0)["act"][1, 2] == 0).all()
    keep = np.ones((gp.M, gp.P), bool)
    keep[1, 2] = False
    np.testing.assert_array_equal(got[keep].view(np.uint32), clean[keep].view(np.uint32))


@pytest.mark.parametrize("s", [0.3, 1.0, 1.7])
@pytest.mark.parametrize("name,D,A", gp.SHAPES)
def test_anchor_zero_log_std_layer_is_the_noise_route(name, D, A, s):
    """W_ls = 0, b_ls = 0, lo < 0 < hi: l = 0, ls = 0, sig = exp(0) = 1, std_scale * sig = std_scale, so for squash "none" the restated
    head route equals the restated noise route at noise_std = std_scale, bit for bit -- the CPU half of the GPU test's anchor."""
    layers = gp.anchor_layers(D, gp.HIDDEN, A, seed=3)
    mean_layers, W_ls, b_ls = gref.split(layers, A)
    assert not W_ls.any() and not b_ls.any() and gp.LO < 0.0 < gp.HI and np.exp(F(0)) == F(1)
    est = pref.particle_mean32(gp.states(gp.M, gp.P, gp.NP, D, seed=A))
    assert not gref.z32(est, layers, gp.ACT)[..., A:].any()
    for t in range(gp.H):
        xi, _ = gp.draws(gp.SEED, gp.CALL, gp.M, gp.P, t, A, s)
        head = gp.step32(est, layers, gp.ACT, "none", "clamp", gp.LO, gp.HI, xi, s)      # (the tanh bound maps l = 0 to the midpoint, not to 0)
        noise = gp.noise32(est, mean_layers, gp.ACT, "none", xi, s)
        np.testing.assert_array_equal(head.view(np.uint32), noise.view(np.uint32), err_msg="step %d" % t)
        assert not np.array_equal(head[:, 1], head[:, 0])
