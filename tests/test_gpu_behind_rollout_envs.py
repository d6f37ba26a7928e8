"""GPU: the kernels behind the rollout -- the forecast's statistics (csrc/forecast.hip) and the constraints (csrc/constrain.hip) --
on ant, slim_humanoid and pendulum: the three instantiations of `step_reward<ENV>` (csrc/step_reward.h) that do what halfcheetah's
does not.  Ant adds a survive bonus; slim_humanoid reads two dim pairs, pair 11 (obs[22]) and pair 0 (obs[1] inside (1, 2)), and its
D = 45 is odd, the last pair has no second element; pendulum has atan2f, fmodf with a floor-mod fix-up, and a torque clip.

Shapes, seeds and the adjustments that make those terms bite: tests/behind_rollout.py.  The checks are the ones
tests/test_gpu_forecast.py and tests/test_gpu_constraints.py define (imported, not restated), with the step-reward bound of
tests/forecast_ref.py `reward_bound`.  The composite's last assertion -- the forecast's returns against the rollout's own returns --
ties step_reward<ENV> to the reward the rollout kernels computed, per kind.

Measured on an MI355X, worst |err| / bound:
                                               ant     slim_humanoid   pendulum
    terminate rows (constraint kernel)         0.370   0.106           0.284
    per-particle step rewards                  0.110   0.126           0.171
      of them bit-equal to the float32 closure 1046 of 1050, 419 of 450, 548 of 675
    reward_mean / reward_member                0.300 / 0.623   0.183 / 0.476   0.072 / 0.171
    reward_var / returns                       0.008 / 0.073   0.005 / 0.062   0.016 / 0.057
    state mean / member_mean                   0.169 / 0.195   0.120 / 0.148   0.210 / 0.000
    state variances, the variance identity     0.020, 0.013    0.013, 0.009    0.042, 0.000
    composite: mean / member_mean vs oracle    0.015 / 0.034   0.013 / 0.032   0.019 / 0.052
    composite: returns vs rollout_returns      0.000           0.088           0.049
Pendulum stays within its bound: the assumed 2 ulp of the device's atan2f are not exceeded on these inputs (its step rewards use
0.171 of a bound whose larger part is the angle term)."""
import numpy as np
import pytest

import behind_rollout as br
from cadm_amd import synth
from helpers import make_engine, oracle_problem
from oracle import envs as oenvs
from test_gpu_constraints import check_kernel
from test_gpu_forecast import _np, check_composite, check_order_stats, check_rewards, check_state_stats

pytestmark = pytest.mark.gpu

KINDS = sorted(br.KINDS)


@pytest.fixture(scope="module")
def engines(gpu):
    """kind -> (problem, engine): context, E = 5, m = 3, the table's p and H; built when first asked for, one per kind."""
    built = {}

    def get(kind):
        if kind not in built:
            D, A, p, H = br.KINDS[kind][:4]
            prob = synth.make_problem(env=kind, context=True, E=5, m=3, H=H, seed=60 + KINDS.index(kind))
            assert (prob["D"], prob["A"]) == (D, A)
            built[kind] = (prob, make_engine(prob, p=p))
        return built[kind]
    yield get
    for _, eng in built.values():
        eng.close()


@pytest.fixture(scope="module")
def inputs():
    """kind -> (traj, obs, actions, constraints), computed once and shared; no test may have written to them"""
    made, kept = {}, {}

    def get(kind):
        if kind not in made:
            made[kind] = br.kind_inputs(kind)
            kept[kind] = [a.copy() for a in made[kind][:3]]
        return made[kind]
    yield get
    for kind, arrays in kept.items():
        for a, b in zip(made[kind][:3], arrays):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: a shared input was written to" % kind


@pytest.mark.parametrize("kind", KINDS)
def test_constraint_kernel(engines, inputs, kind):
    """Counters and penalty rows bit for bit, terminate rows within (tau + 1) max b, run to run, sub-batch, in place."""
    prob, eng = engines(kind)
    traj, obs, acts, cons = inputs(kind)
    H, m, n, p, D = traj.shape
    assert (eng.H, eng.p, eng.D) == (H, p, D)
    check_kernel(eng, oenvs.make_env(kind), kind, traj, obs, acts, cons, 40 + KINDS.index(kind), "%s D=%d p=%d H=%d, %d rows" % (kind, D, p, H, m * n * p))


@pytest.mark.parametrize("kind", KINDS)
def test_forecast_state_and_order_statistics(engines, inputs, kind):
    prob, eng = engines(kind)
    traj, obs, acts, _ = inputs(kind)
    got = _np(eng.forecast_stats(traj, obs, acts))
    check_state_stats(got, traj, 5, "%s E=5" % kind)
    check_order_stats(eng, traj, obs, acts, 5, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_forecast_rewards(engines, inputs, kind):
    """The kernel's per-particle step rewards (read through E = p) within `reward_bound` of the env's closure; their statistics at E = 5."""
    prob, eng = engines(kind)
    traj, obs, acts, _ = inputs(kind)
    if kind == "slim_humanoid":
        assert 0.2 <= br.alive_share(traj, obs) <= 0.8
    if kind == "pendulum":
        assert (np.abs(acts) > 2.0).mean() > 0.1
    check_rewards(eng, oenvs.make_env(kind), kind, traj, obs, acts, 5, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_composite(engines, kind):
    """cadm_plan_forecast (m = 3, n = 2, injected noise) against the oracle's trajectory, and its returns against the rollout's own."""
    prob, eng = engines(kind)
    check_composite(eng, prob, oracle_problem(prob, np.float32), oenvs.make_env(kind), kind, 70 + KINDS.index(kind), kind)
