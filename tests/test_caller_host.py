"""The host side of caller.DevicePlannerState on a model without a history window (vanilla PE-TS), without a GPU: the reference
resets the CEM warm start of a finished env with or without a context (/root/reference/cadm/samplers/sampler.py:193-195), and for a
vanilla model nothing on the device does it -- `cadm_history_update` refuses a model without a history window -- so `observe` has
to.  The stand-in engine lives on the CPU and its library raises when reached."""
import numpy as np
import pytest
import torch

from cadm_amd.caller import DevicePlannerState
from cadm_amd.engine import HipEngine

M, H, A, D = 3, 4, 2, 5


class _Lib:
    def cadm_history_update(self, *a):
        raise AssertionError("cadm_history_update reached for a model without a history window")

    def cadm_warm_start_shift(self, *a):
        raise AssertionError("cadm_warm_start_shift reached by observe / reset")


class _Engine:
    device, C, Hh, H, A, D, discrete, stream = torch.device("cpu"), 0, 0, H, A, D, False, None
    _t = HipEngine._t

    def __init__(self):
        self.lib, self._ctx = _Lib(), None

    def _check(self, rc, what=""):
        assert rc == 0, what


class _Model:
    state_diff, use_cem, _opt = False, True, None

    def __init__(self):
        self.engine, self.carry_resets = _Engine(), []

    def reset_plan_carry(self, mask=None):
        self.carry_resets.append(None if mask is None else np.asarray(mask).copy())


def _state():
    model = _Model()
    state = DevicePlannerState(model, M)
    assert not state.context and tuple(state.prev_sol.shape) == (M, H, A)
    sol = torch.arange(1, M * H * A + 1, dtype=torch.float32).reshape(M, H, A)      # no zero anywhere: a reset row is told from a kept one
    state.prev_sol.copy_(sol)
    return model, state, sol.numpy().copy()


@pytest.mark.parametrize("as_type", ["list", "bool", "int32_tensor", "bool_tensor"])
def test_vanilla_observe_resets_the_finished_envs_warm_start(as_type):
    model, state, sol = _state()
    done = {"list": [1, 0, 1], "bool": np.array([True, False, True]), "int32_tensor": torch.tensor([1, 0, 1], dtype=torch.int32),
            "bool_tensor": torch.tensor([True, False, True])}[as_type]
    z = np.zeros((M, D), np.float32)
    state.observe(z, np.zeros((M, A), np.float32), z, done=done)
    got = state.prev_sol.numpy()
    np.testing.assert_array_equal(got[[0, 2]], np.zeros((2, H, A), np.float32))
    np.testing.assert_array_equal(got[1], sol[1])
    np.testing.assert_array_equal(state.init_var.numpy(), np.full((M, H, A), 0.25, np.float32))
    assert len(model.carry_resets) == 1 and np.asarray(model.carry_resets[0]).astype(bool).tolist() == [True, False, True]


def test_vanilla_observe_without_done_resets_nothing():
    model, state, sol = _state()
    z = np.zeros((M, D), np.float32)
    state.observe(z, np.zeros((M, A), np.float32), z)
    state.observe(z, np.zeros((M, A), np.float32), z, done=None)
    state.observe(z, np.zeros((M, A), np.float32), z, done=np.zeros(M, bool))
    np.testing.assert_array_equal(state.prev_sol.numpy(), sol)
    assert len(model.carry_resets) == 1 and not model.carry_resets[0].any()      # only the call that was given a mask


def test_vanilla_observe_refuses_a_mask_of_another_length():
    _, state, sol = _state()
    z = np.zeros((M, D), np.float32)
    with pytest.raises(ValueError, match="done has 2 entries for 3 envs"):
        state.observe(z, np.zeros((M, A), np.float32), z, done=[1, 0])
    np.testing.assert_array_equal(state.prev_sol.numpy(), sol)


def test_reset_clears_everything_and_discrete_actions_are_refused():
    model, state, _ = _state()
    state.reset()
    assert not state.prev_sol.any() and model.carry_resets == [None]
    model.engine.discrete = True
    with pytest.raises(NotImplementedError, match="discrete actions"):
        DevicePlannerState(model, M)
