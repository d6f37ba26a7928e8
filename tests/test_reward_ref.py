"""CPU: the learned reward of the opt-in planner -- the restatements of tests/reward_ref.py against each other (the float32 emulation of
the kernel's chain against float64, the vectorised step sum against plain loops, the gather from the three sources), the struct and the
signatures against the header, the library's exports, the options, and the host-side refusals of `set_reward_net`.  The kernel itself:
tests/test_gpu_reward.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import reward_ref as rref
import value_ref as vref
from behind_rollout import synth_traj
from cadm_amd import _lib
from cadm_amd.engine import HipEngine
from cadm_amd.planner import PlanOptions
from helpers import assert_close, floored_rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ("cadm_set_reward_net", "cadm_reward_eval", "cadm_reward_returns", "cadm_rewarded_workspace_bytes", "cadm_rewarded_plan")


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------- the restatements
CHAINS = [("next_obs", (), "relu"), ("obs_act", (48,), "tanh"), ("obs_act_next_obs", (128, 128), "relu"), ("obs_act_next_obs", (256, 256), "swish"),
          ("obs_act", (64, 48, 200), "tanh"), ("next_obs", (512,) * 4, "relu")]


@pytest.mark.parametrize("inputs,hidden,act", CHAINS, ids=["%s-%s-%s" % (i, "x".join(map(str, h)) or "linear", a) for i, h, a in CHAINS])
def test_float32_chain_against_float64(inputs, hidden, act):
    """The kernel's chain in float32 stays within 1e-5 of the output's scale of the float64 restatement on He-initialised nets, on inputs
    gathered from a synthetic trajectory, with statistics that are not 0 and 1."""
    H, m, n, p, D, A = 4, 2, 3, 5, 18, 6
    traj, obs, actions = synth_traj(5, H, m, n, p, D, A)
    x = rref.gather_inputs(traj, obs, actions, inputs)
    K = rref.input_dims(inputs, D, A)
    assert x.shape == (H, m, n, p, K)
    rng = np.random.default_rng(len(hidden))
    mean, std = x.reshape(-1, K).mean(axis=0).astype(F), rng.uniform(0.5, 3.0, K).astype(F)
    layers = rref.he_net(K, hidden, seed=3)
    ref = rref.reward64(x, layers, act, mean, std)
    emu = rref.emulate32(x, layers, act, mean, std)
    assert emu.dtype == F and emu.shape == (H, m, n, p) and np.isfinite(ref).all()
    assert_close(emu, ref, what="%s %r %s" % (inputs, hidden, act))
    print("\n[%s %r %s] float32 chain against float64: %.2e of scale" % (inputs, hidden, act, floored_rel(emu, ref)))


ENVELOPE = [(e, i, h, a) for e in ("pend", "slim", "wide") for i in rref.INPUTS for h in vref.ENVELOPE_NETS for a in vref.ACTS] + \
    [("ant", i, (130, 66), a) for i in rref.INPUTS for a in vref.ACTS]


@pytest.mark.parametrize("name,inputs,hidden,act", ENVELOPE, ids=["%s-%s-%s-%s" % (e, i, "x".join(map(str, h)), a) for e, i, h, a in ENVELOPE])
def test_float32_chain_at_the_envelope_shapes(name, inputs, hidden, act):
    """The nets tests/test_gpu_terms_envelope.py registers (widths off the multiples of 4 and 64, four hidden layers) on its inputs
    (K = 3, 4, 7 on pendulum; 45, 62, 107 on slim_humanoid; 48, 72, 120 at the envelope's corner; 28, 36, 64 on ant with (130, 66); 3 x 11 candidates): the
    float32 chain stays within the GPU test's bar of the float64 restatement, and the nets meet that file's liveness condition."""
    import behind_rollout as br
    _, D, A = br.TERM_ENGINES[name][:3]
    x = rref.gather_inputs(*br.term_traj(name, 3, 11, 91), inputs)
    K = rref.input_dims(inputs, D, A)
    layers = vref.envelope_net(K, hidden)
    share, spread = vref.liveness(x, layers, act)
    assert share >= 0.5 and spread > 1e-3, "%s %s %r %s: live share %.2f, output spread %.2e" % (name, inputs, hidden, act, share, spread)
    ref = rref.reward64(x, layers, act)
    emu = rref.emulate32(x, layers, act)
    assert emu.dtype == F and np.isfinite(ref).all()
    assert_close(emu, ref, what="%s %s %r %s" % (name, inputs, hidden, act))
    print("\n[%s %s %r %s] float32 chain against float64: %.2e of scale, live share %.2f" % (name, inputs, hidden, act, floored_rel(emu, ref), share))


@pytest.mark.parametrize("inputs", rref.INPUTS)
def test_gather_places_every_source(inputs):
    """With inputs whose every element is unique, every element of the gathered input is the one the definition names: obs[mi] for the
    s_t of step 0, traj[t-1] for the later ones, actions[mi,ni,t] for every particle, traj[t] for s_{t+1}."""
    H, m, n, p, D, A = 3, 2, 3, 2, 4, 3
    traj = np.arange(H * m * n * p * D, dtype=F).reshape(H, m, n, p, D)
    obs = (10000 + np.arange(m * D, dtype=F)).reshape(m, D)
    actions = (20000 + np.arange(m * n * H * A, dtype=F)).reshape(m, n, H, A)
    assert len(set(traj.ravel()) | set(obs.ravel()) | set(actions.ravel())) == traj.size + obs.size + actions.size
    x = rref.gather_inputs(traj, obs, actions, inputs)
    assert x.shape == (H, m, n, p, rref.input_dims(inputs, D, A)) and x.dtype == F
    for t in range(H):
        for mi in range(m):
            for ni in range(n):
                for j in range(p):
                    prev = obs[mi] if t == 0 else traj[t - 1, mi, ni, j]
                    want = {"next_obs": [traj[t, mi, ni, j]], "obs_act": [prev, actions[mi, ni, t]],
                            "obs_act_next_obs": [prev, actions[mi, ni, t], traj[t, mi, ni, j]]}[inputs]
                    np.testing.assert_array_equal(x[t, mi, ni, j], np.concatenate(want))


@pytest.mark.parametrize("inputs", rref.INPUTS)
def test_vectorised_sum_equals_plain_loops_bitwise(inputs):
    """`gather_inputs` + `emulate32` + `step_sum` + `update` give the bits of the plain loops, with and without `first`, and `first` cuts
    what the definition says: the violating step still pays."""
    H, m, n, p, D, A = 5, 2, 3, 4, 11, 3
    traj, obs, actions = synth_traj(9, H, m, n, p, D, A)
    rng = np.random.default_rng(1)
    rows = (10.0 * rng.standard_normal((m, n, p))).astype(F)
    K = rref.input_dims(inputs, D, A)
    layers = rref.he_net(K, (24, 12), 2)
    mean, std = rng.standard_normal(K).astype(F), rng.uniform(0.5, 2.0, K).astype(F)
    r = rref.emulate32(rref.gather_inputs(traj, obs, actions, inputs), layers, "tanh", mean, std)
    first = rng.integers(0, H + 1, (m, n, p)).astype(np.int32)
    first.reshape(-1)[:4] = (0, H - 1, H, 2)
    for f in (None, first):
        S = rref.step_sum(r, f)
        out = rref.update(rows, S, -0.37)
        bout, bS, bsteps = rref.brute_force(traj, obs, actions, rows, layers, "tanh", inputs, -0.37, mean, std, f)
        np.testing.assert_array_equal(bits(out), bits(bout))
        np.testing.assert_array_equal(bits(S), bits(bS))
        np.testing.assert_array_equal(bits(rref.masked_steps(r, f)), bits(bsteps))
    q = (0, 0, 0)      # first = 0: exactly step 0 counts
    assert rref.step_sum(r, first)[q] == F(F(0) + r[(0,) + q])
    q = (0, 0, 1)      # first = H - 1 and first = H: every step
    assert bits(rref.step_sum(r, first))[q] == bits(rref.step_sum(r))[q] and bits(rref.step_sum(r, first))[0, 0, 2] == bits(rref.step_sum(r))[0, 0, 2]


def test_non_finite_inputs_and_the_update():
    """A non-finite value anywhere in a counted step's input makes R, S and the row NaN, relu or not; in a step that is not counted it
    changes nothing; the update is one float32 multiply and one float32 add."""
    H, m, n, p, D, A = 4, 1, 2, 3, 11, 3
    traj, obs, actions = synth_traj(3, H, m, n, p, D, A)
    layers = rref.he_net(rref.input_dims("obs_act", D, A), (16,), 1)
    clean = rref.emulate32(rref.gather_inputs(traj, obs, actions, "obs_act"), layers, "relu")
    bad = traj.copy()
    bad[1, 0, 1, 2, 5] = np.nan                      # s_2 of row (0, 1, 2): the input of step 2 under "obs_act"
    for fn in (rref.reward64, rref.emulate32):
        r = fn(rref.gather_inputs(bad, obs, actions, "obs_act"), layers, "relu")
        assert np.isnan(r[2, 0, 1, 2]) and np.isnan(r).sum() == 1
    r = rref.emulate32(rref.gather_inputs(bad, obs, actions, "obs_act"), layers, "relu")
    keep = np.ones(r.shape, bool)
    keep[2, 0, 1, 2] = False
    np.testing.assert_array_equal(bits(r)[keep], bits(clean)[keep])
    assert np.isnan(rref.step_sum(r)[0, 1, 2]) and np.isnan(rref.step_sum(r)).sum() == 1
    first = np.full((m, n, p), H, np.int32)
    first[0, 1, 2] = 1                               # step 2 is not counted: the NaN is never summed
    np.testing.assert_array_equal(bits(rref.step_sum(r, first)), bits(rref.step_sum(clean, first)))
    rows, S = np.array([1.0, -2.5, 3.0e7], F), np.array([0.3, np.nan, 1.0], F)
    out = rref.update(rows, S, 0.7)
    assert out[0] == F(F(1.0) + F(F(0.7) * F(0.3))) and np.isnan(out[1]) and out[2] == F(F(3.0e7) + F(0.7))
    assert rref.step_sum(np.array([[-0.0]], F))[0].view(np.uint32) == 0      # (0 + -0.0) is +0.0


# ---------------------------------------------------------------------------------------------------------------------- the header
def test_struct_and_signatures_match_the_header():
    src = open(os.path.join(ROOT, "include", "cadm_hip.h")).read()
    consts = {k: int(re.search(r"#define %s (\d+)" % k, src).group(1)) for k in
              ("CADM_MAX_REWARD_DIMS", "CADM_REWARD_NEXT_OBS", "CADM_REWARD_OBS_ACT", "CADM_REWARD_OBS_ACT_NEXT_OBS")}
    assert consts["CADM_MAX_REWARD_DIMS"] == _lib.MAX_REWARD_DIMS == 256
    assert _lib.REWARD_INPUTS == {"next_obs": consts["CADM_REWARD_NEXT_OBS"], "obs_act": consts["CADM_REWARD_OBS_ACT"],
                                  "obs_act_next_obs": consts["CADM_REWARD_OBS_ACT_NEXT_OBS"]}
    assert tuple(_lib.REWARD_INPUTS) == rref.INPUTS
    body = re.search(r"typedef struct cadm_reward_params \{(.*?)\} cadm_reward_params;", src, flags=re.S).group(1)
    fields = re.findall(r"\b(int32_t|float)\s+(\w+)(\[CADM_MAX_VALUE_LAYERS\])?;", body)
    want = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [(n, want[t] * 4 if arr else want[t]) for t, n, arr in fields] == [(n, t) for n, t in _lib.RewardParams._fields_]
    assert [n for n, _ in _lib.RewardParams._fields_] == ["n_hidden", "hidden", "activation", "inputs", "weight"]
    assert ctypes.sizeof(_lib.RewardParams) == (1 + 4 + 1 + 1 + 1) * 4
    assert re.search(r"#define CADM_ABI_VERSION 2\b", src)      # the ABI version is unchanged
    kinds = {"cadm_ctx*": ctypes.c_void_p, "void*": ctypes.c_void_p, "float*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p, "int": ctypes.c_int,
             "uint32_t": ctypes.c_uint32, "float**": ctypes.POINTER(ctypes.c_void_p)}
    structs = {"cadm_reward_params*": "RewardParams", "cadm_value_params*": "ValueParams", "cadm_uncertainty_params*": "UncertaintyParams",
               "cadm_actuator_params*": "ActuatorParams", "cadm_track_params*": "TrackParams", "cadm_knot_params*": "KnotParams",
               "cadm_constraint_params*": "ConstraintParams", "cadm_score_params*": "ScoreParams", "cadm_mppi_params*": "MppiParams"}
    for name in NEW_SYMBOLS + ("cadm_reward_workspace_bytes",):
        ret, args = re.search(r"^(int|size_t) %s\((.*?)\);" % name, src, flags=re.S | re.M).groups()
        got = []
        for a in args.split(","):
            typ = re.sub(r"\bconst\b", "", a).strip().rsplit(" ", 1)[0].replace(" ", "")
            got.append(kinds[typ] if typ in kinds else ctypes.POINTER(getattr(_lib, structs[typ])))
        res, sig = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t), name
        assert len(sig) == len(got) and all(x is y for x, y in zip(sig, got)), name
    # the loop entry is cadm_valued_plan's arguments behind the reward's one; the workspace query takes the same switches
    assert _lib.SIGNATURES["cadm_rewarded_plan"][1][2:] == _lib.SIGNATURES["cadm_valued_plan"][1][1:]
    assert _lib.SIGNATURES["cadm_rewarded_workspace_bytes"][1] == _lib.SIGNATURES["cadm_valued_workspace_bytes"][1]


def test_library_exports_the_new_symbols_without_a_gpu():
    """The built library exports the five new entry points (and the workspace query of cadm_reward_returns), loads without a GPU, and
    their argument checks answer before any HIP call."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS + ("cadm_reward_workspace_bytes",):
        assert hasattr(raw, name), "libcadm_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    assert lib.cadm_rewarded_workspace_bytes(None, 1, 1, 0, 0, 0, 0, 0) == 0 and lib.cadm_reward_workspace_bytes(None, 1, 1) == 0
    assert lib.cadm_set_reward_net(None, None, None, None, None, None, None) == -1 and b"ctx is null" in lib.cadm_last_error()
    assert lib.cadm_reward_eval(None, None, 1, None, None) == -1


# ---------------------------------------------------------------------------------------------------------------------- the options
def test_plan_options_accept_and_refuse():
    """`cem_reward_net` alone takes the opt-in route and is folded into the struct the library reads; every default still gives None; the
    new fields keep the places that existing tests pin; what is refused is refused without an engine."""
    assert PlanOptions.from_kwargs() is None
    assert PlanOptions.from_kwargs(cem_reward_net=None) is None
    assert PlanOptions.from_kwargs(use_cem=True, cem_reward_net=None) is None
    assert PlanOptions._fields[-3:] == ("tracking", "track_params", "target_advance")
    assert PlanOptions._fields[-9:-3] == ("reward", "reward_params", "value", "value_params", "uncertainty", "uncertainty_params")
    assert PlanOptions(*range(18)).reward_params is None and PlanOptions(*range(18)).reward is None
    opt = PlanOptions.from_kwargs(cem_noise_beta=1.0, use_cem=True)
    assert opt.reward is None and opt.reward_params is None
    opt = PlanOptions.from_kwargs(use_cem=True, obs_dim=18, action_dim=6,
                                  cem_reward_net=dict(inputs="obs_act", hidden_sizes=(128, 128), activation="relu", weight=1.0))
    rp = opt.reward_params
    assert isinstance(rp, _lib.RewardParams)
    assert (rp.n_hidden, list(rp.hidden), rp.activation, rp.inputs, rp.weight) == (2, [128, 128, 0, 0], 0, _lib.REWARD_INPUTS["obs_act"], 1.0)
    assert opt.reward == ("obs_act", (128, 128), "relu", 1.0) and opt.update == "cem" and opt.value_params is None and opt.track_params is None
    opt = PlanOptions.from_kwargs(use_cem=True, cem_reward_net=dict(inputs="next_obs", hidden_sizes=[np.int64(7)], activation="swish", weight=-0.5))
    assert opt.reward == ("next_obs", (7,), "swish", -0.5) and opt.reward_params.activation == _lib.VALUE_ACTS["swish"]
    opt = PlanOptions.from_kwargs(use_cem=True, cem_reward_net={})
    assert opt.reward == ("obs_act_next_obs", (), "relu", 1.0) and opt.reward_params.n_hidden == 0
    both = PlanOptions.from_kwargs(use_cem=True, cem_reward_net=dict(hidden_sizes=(8,)), cem_terminal_value=dict(hidden_sizes=(9,)))
    assert both.reward[1] == (8,) and both.value[0] == (9,)
    with pytest.raises(ValueError, match="need use_cem=True"):
        PlanOptions.from_kwargs(cem_reward_net=dict(hidden_sizes=(8,)))
    for bad, frag in ((dict(hidden_sizes=(8,) * 5), "at most 4"), (dict(hidden_sizes=(0,)), "hidden widths"), (dict(hidden_sizes=(513,)), "hidden widths"),
                      (dict(hidden_sizes=(8.5,)), "hidden widths"), (dict(hidden_sizes=(True,)), "hidden widths"), (dict(activation="gelu"), "activation"),
                      (dict(activation=3), "activation"), (dict(weight=math.nan), "finite"), (dict(weight=math.inf), "finite"),
                      (dict(weight="a"), "finite"), (dict(inputs="obs"), "reward inputs"), (dict(inputs=3), "reward inputs"),
                      (dict(inputs=True), "reward inputs"), (dict(widths=(8,)), "must be dict"), ([8, 8], "must be dict")):
        with pytest.raises(ValueError, match=frag):
            PlanOptions.from_kwargs(use_cem=True, cem_reward_net=bad)
    # K = 2 D + A beyond 256, and just inside it
    with pytest.raises(ValueError, match="up to 256"):
        PlanOptions.from_kwargs(use_cem=True, obs_dim=126, action_dim=5, cem_reward_net={})
    assert PlanOptions.from_kwargs(use_cem=True, obs_dim=125, action_dim=6, cem_reward_net={}) is not None
    assert PlanOptions.from_kwargs(use_cem=True, obs_dim=126, action_dim=5, cem_reward_net=dict(inputs="obs_act")) is not None
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        PlanOptions.from_kwargs(use_cem=True, discrete=True, cem_reward_net={})

    class _Group:
        pass
    import torch.distributed as dist
    real = dist.get_world_size
    dist.get_world_size = lambda group=None: 2
    try:
        with pytest.raises(NotImplementedError, match="process group"):
            PlanOptions.from_kwargs(use_cem=True, process_group=_Group(), cem_reward_net={})
    finally:
        dist.get_world_size = real


class _Engine:
    """what `HipEngine.set_reward_net` reads before it touches the library"""
    D, A = 18, 6
    value_weights = staticmethod(HipEngine.value_weights)
    _host = staticmethod(HipEngine._host)


def test_host_side_refusals_of_set_reward_net():
    """The shared import checks a reward net against ITS input dims (K = D + A here): shapes, the declared sizes and activation,
    finiteness and std > 0 are refused on the host, before any library call (the stand-in engine has no library to call)."""
    import value_ref as vref
    prm = HipEngine.reward_params("obs_act", (24, 12), "tanh", 1.0)
    good = rref.he_net(24, (24, 12), 5)
    call = lambda weights, **kw: HipEngine.set_reward_net(_Engine(), prm, weights, **kw)
    cases = [
        (rref.he_net(24, (24,), 5), {}, "2 layers given"),
        (rref.he_net(18, (24, 12), 5), {}, "layer 0 is"),
        (rref.he_net(42, (24, 12), 5), {}, "layer 0 is"),
        ([(np.where(W == W[0, 0], np.nan, W), b) for W, b in good], {}, "not finite"),
        (vref.sequential(good, "relu"), {}, "activation"),
        (good, dict(in_std=np.zeros(24)), "in_std must be finite and > 0"),
        (good, dict(in_std=np.ones(18)), r"expected \[24\]"),
        (good, dict(in_mean=np.full(24, np.nan)), "in_mean must be finite"),
    ]
    for weights, kw, frag in cases:
        with pytest.raises(ValueError, match=frag):
            call(weights, **kw)
    with pytest.raises(AttributeError):      # everything in order: the stand-in is asked for its library
        call(good)
