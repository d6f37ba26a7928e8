"""CPU: the terminal value of the opt-in planner -- the float32 emulation of the kernel's chain against the float64 restatement
(tests/value_ref.py), the struct and the five signatures against the header, the options, the Sequential import and the host-side
refusals of `set_terminal_value`.  The kernel itself: tests/test_gpu_value.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import value_ref as vref
from cadm_amd import _lib
from cadm_amd.engine import HipEngine
from cadm_amd.planner import PlanOptions
from helpers import assert_close, floored_rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---------------------------------------------------------------------------------------------------------------------- the restatement
CHAINS = [((), "relu"), ((48,), "tanh"), ((256, 256), "relu"), ((200, 200), "swish"), ((64, 48, 200), "tanh"), ((512,) * 3, "swish"),
          ((512,) * 4, "relu")]


@pytest.mark.parametrize("hidden,act", CHAINS, ids=["%s-%s" % ("x".join(map(str, h)) or "linear", a) for h, a in CHAINS])
def test_float32_chain_against_float64(hidden, act):
    """The kernel's chain in float32 (bias-seeded accumulators, one fma per k, ascending) stays within 1e-5 of the output's scale of the
    float64 restatement on He-initialised nets: the bar the GPU test holds the kernel to leaves room for the format."""
    D = 18
    rng = np.random.default_rng(len(hidden))
    states = (rng.standard_normal((37, D)) * rng.uniform(0.5, 3.0, D) + rng.standard_normal(D)).astype(F)
    mean, std = rng.standard_normal(D).astype(F), rng.uniform(0.5, 3.0, D).astype(F)
    layers = vref.he_net(D, hidden, seed=3)
    ref = vref.value(states, layers, act, mean, std)
    emu = vref.emulate32(states, layers, act, mean, std)
    assert emu.dtype == F and np.isfinite(ref).all()
    assert_close(emu, ref, what="%r %s" % (hidden, act))
    print("\n[%r %s] float32 chain against float64: %.2e of scale" % (hidden, act, floored_rel(emu, ref)))


ENVELOPE = [(e, h, a) for e in ("pend", "slim", "wide") for h in vref.ENVELOPE_NETS for a in vref.ACTS] + [("ant", (130, 66), a) for a in vref.ACTS]


@pytest.mark.parametrize("name,hidden,act", ENVELOPE, ids=["%s-%s-%s" % (e, "x".join(map(str, h)), a) for e, h, a in ENVELOPE])
def test_float32_chain_at_the_envelope_shapes(name, hidden, act):
    """The nets tests/test_gpu_terms_envelope.py registers (widths off the multiples of 4 and 64, four hidden layers) on its inputs
    (D = 3, 45, 48, and 28 with (130, 66); 3 x 11 candidates): the float32 chain stays within the GPU test's bar of the float64 restatement, and the nets meet
    that file's liveness condition -- every hidden layer has a row with at least half of its units non-zero, and the output's standard
    deviation over the rows is above 1e-3 of its largest magnitude."""
    import behind_rollout as br
    D = br.TERM_ENGINES[name][1]
    states = br.term_traj(name, 3, 11, 91)[0][-1].reshape(-1, D)
    layers = vref.envelope_net(D, hidden)
    share, spread = vref.liveness(states, layers, act)
    assert share >= 0.5 and spread > 1e-3, "%s %r %s: live share %.2f, output spread %.2e" % (name, hidden, act, share, spread)
    ref = vref.value(states, layers, act)
    emu = vref.emulate32(states, layers, act)
    assert emu.dtype == F and np.isfinite(ref).all()
    assert_close(emu, ref, what="%s %r %s" % (name, hidden, act))
    print("\n[%s %r %s] float32 chain against float64: %.2e of scale, live share %.2f" % (name, hidden, act, floored_rel(emu, ref), share))


def test_non_finite_states_and_the_update():
    """A non-finite value anywhere in a state makes V NaN in both statements, relu or not, and nothing else; the row update is one float32
    multiply and one float32 add, and a row with first < H keeps its bits."""
    D = 11
    layers = vref.he_net(D, (16,), 1)
    states = np.random.default_rng(0).standard_normal((6, D)).astype(F)
    clean = vref.emulate32(states, layers, "relu")
    bad = states.copy()
    bad[1, 3], bad[4, 10], bad[5, 0] = np.nan, np.inf, -np.inf
    for fn in (vref.value, vref.emulate32):
        v = fn(bad, layers, "relu")
        assert np.isnan(v[[1, 4, 5]]).all() and np.isfinite(v[[0, 2, 3]]).all()
    np.testing.assert_array_equal(vref.emulate32(bad, layers, "relu")[[0, 2, 3]].view(np.uint32), clean[[0, 2, 3]].view(np.uint32))
    rows = np.array([1.0, -2.5, 3.0e7, 0.1], F)
    v = np.array([0.3, np.nan, 1.0, 7.0], F)
    out = vref.update(rows, v, 0.7, first=np.array([5, 5, 5, 2]), H=5)
    assert out[0] == F(F(1.0) + F(F(0.7) * F(0.3))) and np.isnan(out[1]) and out[2] == F(F(3.0e7) + F(0.7)) and out[3] == rows[3]
    assert vref.inv_std(np.array([3.0], F))[0] == F(1.0 / 3.0)


# ---------------------------------------------------------------------------------------------------------------------- the header
def test_struct_and_signatures_match_the_header():
    src = open(os.path.join(ROOT, "include", "cadm_hip.h")).read()
    consts = {k: int(re.search(r"#define %s (\d+)" % k, src).group(1)) for k in
              ("CADM_MAX_VALUE_LAYERS", "CADM_MAX_VALUE_WIDTH", "CADM_MAX_VALUE_DIMS", "CADM_VALUE_RELU", "CADM_VALUE_TANH", "CADM_VALUE_SWISH")}
    assert (consts["CADM_MAX_VALUE_LAYERS"], consts["CADM_MAX_VALUE_WIDTH"], consts["CADM_MAX_VALUE_DIMS"]) == \
        (_lib.MAX_VALUE_LAYERS, _lib.MAX_VALUE_WIDTH, _lib.MAX_VALUE_DIMS) == (4, 512, 128)
    assert _lib.VALUE_ACTS == {"relu": consts["CADM_VALUE_RELU"], "tanh": consts["CADM_VALUE_TANH"], "swish": consts["CADM_VALUE_SWISH"]}
    body = re.search(r"typedef struct cadm_value_params \{(.*?)\} cadm_value_params;", src, flags=re.S).group(1)
    fields = re.findall(r"\b(int32_t|float)\s+(\w+)(\[CADM_MAX_VALUE_LAYERS\])?;", body)
    want = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [(n, want[t] * 4 if arr else want[t]) for t, n, arr in fields] == [(n, t) for n, t in _lib.ValueParams._fields_]
    assert [n for n, _ in _lib.ValueParams._fields_] == ["n_hidden", "hidden", "activation", "weight"]
    assert ctypes.sizeof(_lib.ValueParams) == (1 + 4 + 1 + 1) * 4
    assert re.search(r"#define CADM_ABI_VERSION 2\b", src)
    kinds = {"cadm_ctx*": ctypes.c_void_p, "void*": ctypes.c_void_p, "float*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p, "int": ctypes.c_int,
             "uint32_t": ctypes.c_uint32, "float**": ctypes.POINTER(ctypes.c_void_p)}
    structs = {"cadm_value_params*": "ValueParams", "cadm_uncertainty_params*": "UncertaintyParams", "cadm_actuator_params*": "ActuatorParams",
               "cadm_track_params*": "TrackParams", "cadm_knot_params*": "KnotParams", "cadm_constraint_params*": "ConstraintParams",
               "cadm_score_params*": "ScoreParams", "cadm_mppi_params*": "MppiParams"}
    for name in ("cadm_set_value_net", "cadm_value_eval", "cadm_value_returns", "cadm_valued_workspace_bytes", "cadm_valued_plan"):
        ret, args = re.search(r"^(int|size_t) %s\((.*?)\);" % name, src, flags=re.S | re.M).groups()
        got = []
        for a in args.split(","):
            typ = re.sub(r"\bconst\b", "", a).strip().rsplit(" ", 1)[0].replace(" ", "")
            got.append(kinds[typ] if typ in kinds else ctypes.POINTER(getattr(_lib, structs[typ])))
        res, sig = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t), name
        assert len(sig) == len(got) and all(x is y for x, y in zip(sig, got)), name
    # the loop entry is cadm_uncertain_plan's arguments behind the value's one; the workspace query takes one switch more
    assert _lib.SIGNATURES["cadm_valued_plan"][1][2:] == _lib.SIGNATURES["cadm_uncertain_plan"][1][1:]
    assert _lib.SIGNATURES["cadm_valued_workspace_bytes"][1][:-1] == _lib.SIGNATURES["cadm_uncertain_workspace_bytes"][1]


# ---------------------------------------------------------------------------------------------------------------------- the options
def test_plan_options_accept_and_refuse():
    """`cem_terminal_value` alone takes the opt-in route and is folded into the struct the library reads; every default still gives None;
    the new fields sit in front of the uncertainty and tracking ones, whose places existing tests pin; what is refused is refused
    without an engine."""
    assert PlanOptions.from_kwargs() is None
    assert PlanOptions.from_kwargs(cem_terminal_value=None) is None
    assert PlanOptions.from_kwargs(use_cem=True, cem_terminal_value=None) is None
    assert PlanOptions._fields[-3:] == ("tracking", "track_params", "target_advance")
    assert PlanOptions._fields[-7:-3] == ("value", "value_params", "uncertainty", "uncertainty_params")
    assert PlanOptions(*range(18)).value_params is None and PlanOptions(*range(18)).value is None
    opt = PlanOptions.from_kwargs(cem_noise_beta=1.0, use_cem=True)
    assert opt.value is None and opt.value_params is None
    opt = PlanOptions.from_kwargs(use_cem=True, obs_dim=18, cem_terminal_value=dict(hidden_sizes=(256, 256), activation="relu", weight=1.0))
    vp = opt.value_params
    assert isinstance(vp, _lib.ValueParams) and (vp.n_hidden, list(vp.hidden), vp.activation, vp.weight) == (2, [256, 256, 0, 0], 0, 1.0)
    assert opt.value == ((256, 256), "relu", 1.0) and opt.update == "cem" and opt.uncertainty_params is None and opt.track_params is None
    opt = PlanOptions.from_kwargs(use_cem=True, cem_terminal_value=dict(hidden_sizes=[np.int64(7)], activation="swish", weight=-0.5))
    assert opt.value == ((7,), "swish", -0.5) and opt.value_params.activation == _lib.VALUE_ACTS["swish"]
    opt = PlanOptions.from_kwargs(use_cem=True, cem_terminal_value={})
    assert opt.value == ((), "relu", 1.0) and opt.value_params.n_hidden == 0
    with pytest.raises(ValueError, match="need use_cem=True"):
        PlanOptions.from_kwargs(cem_terminal_value=dict(hidden_sizes=(8,)))
    for bad, frag in ((dict(hidden_sizes=(8,) * 5), "at most 4"), (dict(hidden_sizes=(0,)), "hidden widths"), (dict(hidden_sizes=(513,)), "hidden widths"),
                      (dict(hidden_sizes=(8.5,)), "hidden widths"), (dict(hidden_sizes=(True,)), "hidden widths"), (dict(activation="gelu"), "activation"),
                      (dict(activation=3), "activation"), (dict(weight=math.nan), "finite"), (dict(weight=math.inf), "finite"),
                      (dict(weight="a"), "finite"), (dict(widths=(8,)), "must be dict"), ([8, 8], "must be dict")):
        with pytest.raises(ValueError, match=frag):
            PlanOptions.from_kwargs(use_cem=True, cem_terminal_value=bad)
    with pytest.raises(ValueError, match="up to 128"):
        PlanOptions.from_kwargs(use_cem=True, obs_dim=129, cem_terminal_value={})
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        PlanOptions.from_kwargs(use_cem=True, discrete=True, cem_terminal_value={})
    with pytest.raises(TypeError):
        PlanOptions.from_kwargs(*([0.0, 0, 1.0, "mean", False, "cem", 1.0, False, "mean", None, True, False, None, 20, None, "penalty", None] + [{}]))


# ---------------------------------------------------------------------------------------------------------------------- the import
@pytest.mark.parametrize("act", vref.ACTS)
def test_sequential_import_equals_the_list_form(act):
    """A torch.nn.Sequential of Linear and ReLU / Tanh / SiLU modules gives the list form's arrays bit for bit (Linear.weight transposed)
    and names its activation; torch's own forward agrees with the restatement."""
    layers = vref.he_net(18, (24, 12), 5)
    seq = vref.sequential(layers, act)
    got, name = HipEngine.value_weights(seq)
    assert name == act and len(got) == 3
    for (W, b), (W2, b2) in zip(layers, got):
        assert W2.dtype == F and W2.flags["C_CONTIGUOUS"] and W2.shape == W.shape
        np.testing.assert_array_equal(W2.view(np.uint32), W.view(np.uint32))
        np.testing.assert_array_equal(b2.view(np.uint32), b.view(np.uint32))
    same, none = HipEngine.value_weights([(torch.from_numpy(W), b.astype(np.float64)) for W, b in layers])
    assert none is None and all((x[0] == y[0]).all() and (x[1] == y[1]).all() for x, y in zip(same, layers))
    states = np.random.default_rng(2).standard_normal((9, 18)).astype(F)
    with torch.no_grad():
        fwd = seq(torch.from_numpy(states)).numpy()[:, 0]
    assert_close(fwd, vref.value(states, layers, act), what="torch forward")
    linear, name = HipEngine.value_weights(torch.nn.Sequential(torch.nn.Linear(18, 1)))
    assert name is None and linear[0][0].shape == (18, 1)


class _Engine:
    """what `HipEngine.set_value_net` reads before it touches the library"""
    D = 18
    value_weights = staticmethod(HipEngine.value_weights)
    _host = staticmethod(HipEngine._host)


def test_host_side_refusals_of_set_value_net():
    """Shapes, the declared sizes and activation, finiteness and std > 0 are refused on the host, before any library call (the stand-in
    engine has no library to call)."""
    prm = HipEngine.value_params((24, 12), "tanh", 1.0)
    good = vref.he_net(18, (24, 12), 5)
    call = lambda weights, **kw: HipEngine.set_value_net(_Engine(), prm, weights, **kw)
    cases = [
        (vref.he_net(18, (24,), 5), {}, "2 layers given"),
        (vref.he_net(18, (24, 13), 5), {}, "layer 1 is"),
        (vref.he_net(17, (24, 12), 5), {}, "layer 0 is"),
        ([(W, b[:-1]) for W, b in good], {}, r"expected \[in,out\] and \[out\]"),
        ([(W.T, b) for W, b in good], {}, "expected|layer 0 is"),
        ([(np.where(W == W[0, 0], np.nan, W), b) for W, b in good], {}, "not finite"),
        ([(W, np.where(b == b[0], np.inf, b)) for W, b in good], {}, "not finite"),
        (vref.sequential(good, "relu"), {}, "activation"),
        (torch.nn.Sequential(torch.nn.Linear(18, 24), torch.nn.Sigmoid(), torch.nn.Linear(24, 1)), {}, "ReLU, Tanh or SiLU"),
        (torch.nn.Sequential(torch.nn.Linear(18, 24), torch.nn.Tanh()), {}, "ends with a Linear"),
        (torch.nn.Sequential(torch.nn.Linear(18, 24), torch.nn.Tanh(), torch.nn.Linear(24, 12), torch.nn.ReLU(), torch.nn.Linear(12, 1)), {},
         "one activation"),
        (torch.nn.Linear(18, 1), {}, "Sequential"),
        (7, {}, "list of"),
        (good, dict(obs_std=np.zeros(18)), "obs_std must be finite and > 0"),
        (good, dict(obs_std=-np.ones(18)), "obs_std must be finite and > 0"),
        (good, dict(obs_std=np.full(18, np.inf)), "obs_std must be finite and > 0"),
        (good, dict(obs_std=np.ones(17)), r"expected \[18\]"),
        (good, dict(obs_mean=np.full(18, np.nan)), "obs_mean must be finite"),
        (good, dict(obs_mean=np.zeros((2, 18))), r"expected \[18\]"),
    ]
    for weights, kw, frag in cases:
        with pytest.raises(ValueError, match=frag):
            call(weights, **kw)
    with pytest.raises(AttributeError):      # everything in order: the stand-in is asked for its library
        call(good)
