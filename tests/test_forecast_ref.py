"""CPU: the float64 restatement of the plan forecast (tests/forecast_ref.py) against a brute-force loop, the variance identity
total = epistemic + aleatoric, and the divergence rule."""
import numpy as np
import pytest

from cadm_amd.env_spec import restate
from forecast_ref import brute_force, diverged_step, forecast_ref, reward_terms, step_rewards
from oracle import envs as oenvs

STATE_KEYS = ("mean", "member_mean", "var_total", "var_epistemic", "var_aleatoric", "lo", "hi")


def _traj(seed, H, m, n, p, D):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((H, m, n, p, D)) * rng.uniform(0.5, 3.0, D) + rng.standard_normal(D)).astype(np.float32)


@pytest.mark.parametrize("H,m,n,p,D,E,k", [(3, 2, 2, 6, 5, 3, 1), (2, 1, 3, 4, 3, 1, 2), (2, 2, 1, 5, 4, 5, 5), (2, 1, 1, 1, 3, 1, 1)])
def test_restatement_matches_brute_force(H, m, n, p, D, E, k):
    traj = _traj(H + p, H, m, n, p, D)
    ref = forecast_ref(traj, np.zeros((m, D), np.float32), np.zeros((m, n, H, 1), np.float32), E, k)
    loop = brute_force(traj, E, k)
    for key in STATE_KEYS:
        np.testing.assert_allclose(ref[key], loop[key], rtol=1e-12, atol=1e-12, err_msg=key)
    assert (ref["diverged_step"] == H).all()


def test_variance_identity_in_float64():
    traj = _traj(1, 4, 2, 3, 20, 18)
    ref = forecast_ref(traj, np.zeros((2, 18), np.float32), np.zeros((2, 3, 4, 1), np.float32), 5)
    np.testing.assert_allclose(ref["var_total"], ref["var_epistemic"] + ref["var_aleatoric"], rtol=1e-12)
    assert (ref["var_epistemic"] > 0).all() and (ref["var_aleatoric"] > 0).all()
    # one member: nothing to disagree about; one particle per member: no spread inside a member
    one = forecast_ref(traj, np.zeros((2, 18), np.float32), np.zeros((2, 3, 4, 1), np.float32), 1)
    assert (one["var_epistemic"] == 0).all() and np.allclose(one["var_aleatoric"], one["var_total"], rtol=1e-12)
    each = forecast_ref(traj, np.zeros((2, 18), np.float32), np.zeros((2, 3, 4, 1), np.float32), 20)
    assert (each["var_aleatoric"] == 0).all() and np.allclose(each["var_epistemic"], each["var_total"], rtol=1e-12)


def test_diverged_step_rule():
    H, m, n, p, D = 4, 2, 2, 5, 3
    traj = _traj(2, H, m, n, p, D)
    traj[1, 0, 1, 3, 2] = np.inf
    traj[3, 0, 1, 0, 0] = np.nan          # a later one in the same sequence: the first counts
    traj[2, 1, 0, 4, 1] = np.nan
    obs = np.zeros((m, D), np.float32)
    acts = np.zeros((m, n, H, 1), np.float32)
    rew = np.ones((m, n, H, p), np.float32)
    ref = forecast_ref(traj, obs, acts, 5, rewards=rew)
    np.testing.assert_array_equal(diverged_step(traj), [[H, 1], [2, H]])
    np.testing.assert_array_equal(ref["diverged_step"], [[H, 1], [2, H]])
    clean = forecast_ref(_traj(2, H, m, n, p, D), obs, acts, 5, rewards=rew)
    for key in ("mean", "var_total", "var_epistemic", "var_aleatoric", "lo", "hi", "reward_mean", "reward_var"):
        assert np.isnan(ref[key][0, 1, 1:]).all() and np.isnan(ref[key][1, 0, 2:]).all(), key
        np.testing.assert_array_equal(ref[key][0, 1, :1], clean[key][0, 1, :1], err_msg=key)
        np.testing.assert_array_equal(ref[key][1, 0, :2], clean[key][1, 0, :2], err_msg=key)
        np.testing.assert_array_equal(ref[key][0, 0], clean[key][0, 0], err_msg=key)
        np.testing.assert_array_equal(ref[key][1, 1], clean[key][1, 1], err_msg=key)
    assert np.isnan(ref["member_mean"][:, 0, 1, 1:]).all() and np.isnan(ref["reward_member"][:, 1, 0, 2:]).all()
    assert np.isnan(ref["returns"][0, 1]).all() and np.isnan(ref["returns"][1, 0]).all()
    np.testing.assert_array_equal(ref["returns"][0, 0], np.full(p, float(H)))
    np.testing.assert_array_equal(ref["member_mean"][:, 0, 1, :1], clean["member_mean"][:, 0, 1, :1])


def test_rewards_use_pre_and_post_step_states():
    """halfcheetah reads dim 0 of the PRE-step state: obs at step 0, the previous step's value after; the term accounting agrees."""
    H, m, n, p = 3, 2, 1, 4
    traj = _traj(3, H, m, n, p, 18)
    rng = np.random.default_rng(4)
    obs = rng.standard_normal((m, 18)).astype(np.float32)
    acts = rng.uniform(-1, 1, (m, n, H, 6)).astype(np.float32)
    r = step_rewards(oenvs.make_env("halfcheetah"), traj, obs, acts)
    ctrl = np.float32(0.1) * np.sum(np.square(acts), axis=-1)
    np.testing.assert_array_equal(r[:, :, 0], np.broadcast_to(obs[:, None, None, 0] - ctrl[:, :, 0, None], (m, n, p)))
    np.testing.assert_array_equal(r[:, :, 2], traj[1, :, :, :, 0] - ctrl[:, :, 2, None])
    T, S = reward_terms("halfcheetah", traj, obs, acts)
    assert T == 2 and S.shape == (m, n, H, p) and (S >= np.abs(r) - 1e-6).all()
    np.testing.assert_array_equal(step_rewards(restate("halfcheetah"), traj, obs, acts), r)
