"""The caller's per-env bookkeeping around get_action pinned to the reference's own `Sampler`:
tests/golden/sampler_golden.npz records what /root/reference/cadm/samplers/sampler.py's `obtain_samples`, run unchanged on a
toy env and a recording policy (tests/golden/make_sampler_golden.py), FED the policy at every step -- warm-start mean,
init_var, history windows -- together with the plans, actions, next observations and dones of that run.  The oracle's
restatement (oracle/caller.py) and the host-side `CEMWarmStart` must reproduce that stream; the device kernels replay it in
tests/test_gpu_caller.py."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "sampler_golden.npz"))
CASES = sorted({k.split("/")[0] for k in GOLD.files})


def stream(case):
    g = lambda k: GOLD[case + "/" + k]
    n_env, L, H, D, A, Hh, sd = (int(x) for x in g("meta"))
    return dict(n_env=n_env, L=L, H=H, D=D, A=A, Hh=Hh, state_diff=bool(sd), T=g("obses").shape[0], **{
        k: g(k) for k in ("obses", "init_mean", "init_var", "cp_obs", "cp_act", "plans", "actions", "next_obses", "dones")})


@pytest.mark.parametrize("case", CASES)
def test_oracle_caller_reproduces_the_reference_sampler(case):
    from cadm_amd.policies.mpc_controller import CEMWarmStart
    from oracle.caller import SamplerState
    s = stream(case)
    ref = SamplerState(s["n_env"], s["H"], s["D"], s["A"], s["Hh"], s["state_diff"])
    warm = CEMWarmStart(s["n_env"], s["H"], s["A"])
    assert s["dones"].any() and (~s["dones"]).any() and s["T"] > s["Hh"] + 1          # episode ends and the shift path both occur
    for t in range(s["T"]):
        np.testing.assert_array_equal(ref.prev_sol, s["init_mean"][t])
        np.testing.assert_array_equal(ref.init_var, s["init_var"][t])
        np.testing.assert_array_equal(ref.history_state, s["cp_obs"][t])
        np.testing.assert_array_equal(ref.history_act, s["cp_act"][t])
        np.testing.assert_array_equal(warm.prev_sol, s["init_mean"][t])
        np.testing.assert_array_equal(warm.init_var, s["init_var"][t])
        act = ref.after_plan(s["plans"][t])
        np.testing.assert_array_equal(act, s["actions"][t])
        np.testing.assert_array_equal(warm.step(s["plans"][t]), s["actions"][t])
        ref.after_step(s["obses"][t], act, s["next_obses"][t], s["dones"][t])
        for i in np.flatnonzero(s["dones"][t]):
            warm.reset(i)
        if t + 1 < s["T"]:       # the executor hands the NEXT policy call the reset observation of a finished env
            np.testing.assert_array_equal(s["obses"][t + 1], s["next_obses"][t])
