"""GPU: the four caller-supplied nets of the opt-in planner (value, reward, policy, critics) share one host path (csrc/mlp_chain.h:
description checks, registration, launch).  What sharing puts at risk is one net's registration disturbing another's, and a refusal
arriving in another order; the kernels' own parity is held by the four nets' own tests.

Geometry: the module-scoped engines of tests/test_gpu_tracking.py, halfcheetah without context (D = 18, A = 6, p = 5, H = 5): the smallest
built-in env they offer.  Everything is compared bit for bit (`torch.equal`): registration moves weights, it computes nothing."""
import ctypes as ct

import pytest
import torch

import critic_ref as cref
import policy_ref as pref
import reward_ref as rref
import value_ref as vref
from cadm_amd import _lib
from cadm_amd.engine import HipEngine
from helpers import make_engine
from test_gpu_tracking import ITERS, KE, engines      # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

NETS = ("value", "reward", "policy", "critic")
SMALL, BIG = (8,), (24, 24)      # BIG packs into more floats than SMALL's allocation holds: a replacement by it frees and allocates
SETTER = {"value": "set_value_net", "reward": "set_reward_net", "policy": "set_policy_net", "critic": "set_critic_nets"}
EINVAL = -1                      # include/cadm_hip.h CADM_EINVAL


def _nets(eng, hidden, seed):
    """name -> the arguments of its setter: a He-initialised net of `hidden` per kind, two critics"""
    D, A = eng.D, eng.A
    return {"value": (HipEngine.value_params(hidden, "relu", 1.0), vref.he_net(D, hidden, seed)),
            "reward": (HipEngine.reward_params("obs_act_next_obs", hidden, "relu", 1.0), rref.he_net(2 * D + A, hidden, seed + 1)),
            "policy": (HipEngine.policy_params(hidden, "relu", "tanh", 1, 0.0), pref.he_policy(D, hidden, A, seed + 2, out_scale=0.5)),
            "critic": (HipEngine.critic_params(hidden, "relu", 2, "min", 1.0), cref.he_critics(D, A, hidden, 2, seed + 3))}


def _set(eng, name, args):
    getattr(eng, SETTER[name])(*args)


def _inputs(eng, rows):
    """states [rows, D], concatenated reward inputs [rows, 2 D + A] and actions [rows, A] on the device.  The critics are evaluated at
    GIVEN actions, so that what they return does not depend on the policy net this test replaces ("critic_pi" is the other launch)."""
    g = torch.Generator().manual_seed(rows)
    states = torch.randn((rows, eng.D), generator=g)
    x = torch.randn((rows, 2 * eng.D + eng.A), generator=g)
    acts = torch.rand((rows, eng.A), generator=g) * 2.0 - 1.0
    return eng._t(states), eng._t(x), eng._t(acts)


def _eval(eng, name, inp):
    states, x, acts = inp
    if name == "value":
        return (eng.value_eval(states),)
    if name == "reward":
        return (eng.reward_eval(x),)
    if name == "policy":
        return (eng.policy_eval(states),)
    if name == "critic":
        return eng.critic_eval(states, actions=acts, want_each=True)
    return eng.critic_eval(states, want_each=True, want_actions=True)      # "critic_pi": the registered policy net acts


def _pi_holds(eng, changed, inputs, record, what):
    """The critics at the ACTOR's action (the launch that reads the policy net's registration from critic.hip) return the recorded
    bits while neither the policy net nor the critics are the ones replaced or cleared."""
    if changed in ("policy", "critic"):
        return
    for i, inp in enumerate(inputs):
        assert _same(_eval(eng, "critic_pi", inp), record["critic_pi"][i]), "%s: critics at the actor's action at %d rows" % (what, inp[0].shape[0])


def _same(got, want):
    return len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def small(engines):
    """(engine, the four SMALL nets registered on it, inputs at the two row counts, name -> [their evaluations at either count], the
    critics' at the actor's action among them as "critic_pi").  17 rows: one full tile plus one row; 16 * 2 * CUs + 17: the launchers
    take two row tiles."""
    _, eng = engines("hc5-vanilla")
    nets = _nets(eng, SMALL, 100)
    for name in NETS:
        _set(eng, name, nets[name])
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    inputs = [_inputs(eng, 17), _inputs(eng, 16 * 2 * cus + 17)]
    record = {name: [_eval(eng, name, inp) for inp in inputs] for name in NETS + ("critic_pi",)}
    for name in record:
        assert all(torch.isfinite(t).all() for res in record[name] for t in res), name
    return eng, nets, inputs, record


def test_one_registration_leaves_the_others_alone(engines, small):
    """Replacing a net by a larger one (free and allocate), by the first one again (the allocation it now has) and clearing it: the
    other three nets return the recorded bits at both row counts, and the replaced one what the same net returns on a fresh engine."""
    eng, nets, inputs, record = small
    prob, _ = engines("hc5-vanilla")
    big = _nets(eng, BIG, 200)
    fresh_eng = make_engine(prob, p=5, num_elites=KE, num_cem_iters=ITERS)
    try:
        for name in NETS:
            _set(fresh_eng, name, big[name])
        fresh = {name: [_eval(fresh_eng, name, inp) for inp in inputs] for name in NETS}
    finally:
        fresh_eng.close()

    def check(changed, want_changed, what):
        for name in NETS:
            want = want_changed if name == changed else record[name]
            for i, inp in enumerate(inputs):
                assert _same(_eval(eng, name, inp), want[i]), "%s: %s at %d rows" % (what, name, inp[0].shape[0])
        _pi_holds(eng, None if want_changed is record[changed] else changed, inputs, record, what)

    for name in NETS:
        _set(eng, name, big[name])
        assert not _same(fresh[name][0], record[name][0]), name      # (the two nets can be told apart)
        check(name, fresh[name], "%s replaced by %r" % (name, BIG))
        _set(eng, name, nets[name])
        check(name, record[name], "%s back to %r" % (name, SMALL))
        _set(eng, name, (None,))
        with pytest.raises(_lib.CadmError, match="no .*registered"):
            _eval(eng, name, inputs[0])
        for other in NETS:
            if other != name:
                for i, inp in enumerate(inputs):
                    assert _same(_eval(eng, other, inp), record[other][i]), "%s cleared: %s" % (name, other)
        _pi_holds(eng, name, inputs, record, "%s cleared" % name)
        _set(eng, name, nets[name])
        check(name, record[name], "%s registered again" % name)


NAN = float("nan")
# (net, the fields of its raw parameter struct -- two of them break a rule each --, what cadm_last_error() must hold: the FIRST of the two
# refusals in the order of the net's check)
REFUSALS = [
    ("value", dict(n_hidden=5, activation=9), "5 hidden layers, outside"),
    ("value", dict(hidden=(0,), weight=NAN), "has width 0"),
    ("value", dict(activation=9, weight=NAN), "unknown value activation 9"),
    ("reward", dict(inputs=7, weight=NAN), "unknown reward inputs 7"),
    ("reward", dict(activation=9, inputs=7), "unknown reward activation 9"),
    ("policy", dict(squash=5, n_samples=0), "unknown policy squash 5"),
    ("policy", dict(n_samples=0, noise_std=-1.0), "n_samples must be"),
    ("critic", dict(n_critics=0, reduce=9), "0 critics, outside"),
    ("critic", dict(reduce=9, weight=NAN), "unknown critic reduce 9"),
]
RAW = {"value": (_lib.ValueParams, dict(weight=1.0)),
       "reward": (_lib.RewardParams, dict(inputs=2, weight=1.0)),
       "policy": (_lib.PolicyParams, dict(squash=1, n_samples=1, noise_std=0.0)),
       "critic": (_lib.CriticParams, dict(n_critics=2, reduce=0, weight=1.0))}


@pytest.mark.parametrize("name,fields,frag", REFUSALS, ids=["%s-%s" % (n, "+".join(f)) for n, f, _ in REFUSALS])
def test_the_first_refusal_is_the_checks_first(small, name, fields, frag):
    """A raw parameter struct that breaks two rules, passed straight to the library (the Python constructors would refuse first):
    CADM_EINVAL, the message of the rule that comes first in the net's check, before any HIP call (the dummy pointers are never
    touched), and the net registered before still returns its bits."""
    eng, _, inputs, record = small
    cls, base = RAW[name]
    f = dict(n_hidden=1, hidden=(8,), activation=0)
    f.update(base)
    f.update(fields)
    prm = cls()
    prm.n_hidden = f.pop("n_hidden")
    for l, h in enumerate(f.pop("hidden")):
        prm.hidden[l] = h
    for k, v in f.items():
        setattr(prm, k, v)
    buf = torch.zeros((16,), dtype=torch.float32, device=eng.device)
    P = ct.c_void_p(buf.data_ptr())
    ptrs = (ct.c_void_p * 10)(*([buf.data_ptr()] * 10))
    entry = "cadm_" + SETTER[name]
    rc = getattr(eng.lib, entry)(eng._ctx, ct.byref(prm), ptrs, ptrs, P, P, None)
    msg = eng.lib.cadm_last_error().decode()
    assert rc == EINVAL, "%s: expected %d, got %d (%s)" % (entry, EINVAL, rc, msg)
    assert msg.startswith(entry + ":") and frag in msg, msg
    assert _same(_eval(eng, name, inputs[0]), record[name][0]), "%s after the refusal" % name
